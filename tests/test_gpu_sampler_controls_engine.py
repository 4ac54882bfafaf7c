"""The sampler controls inside the decode engine (a tiny quantised Llama through `optimize_transformers`): logit bias,
presence / frequency penalty and min_p in the chaining tail of the prompt pass, eager steps, the one-step graph and the
graph of 8 chained steps. A seeded sampled run is replayed step by step from the saved logits through
tests/sampler_controls_reference.py with the numpy Philox uniform of each position (acceptance rule and tolerance of
tests/test_gpu_sampler_kernel.py) and must not depend on the launch mode or the burst size; greedy runs are the
reference's argmax of bit-equal fp32 scores, token for token."""
import copy

import numpy as np
import pytest
import torch

from tests import sampler_controls_reference as C
from tests import sampler_reference as R

pytestmark = pytest.mark.gpu

PROMPT = [5, 9, 33, 2, 71, 9, 9]
# The tiny model's best logits lie within ~0.3 of each other: a low temperature and a high min_p make the cut bite.
# 8 candidates and top_p 0.85: the nucleus boundary (tail mass 0.15) falls between the last candidate's tail (~0.08) and
# the last two's (~0.18), so a step whose boundary lies within the 100-margin band of it (3.8e-4) is about a 1 % event
SAMPLED = dict(do_sample=True, temperature=0.3, top_k=8, top_p=0.85, repetition_penalty=1.1)
CONTROLS = dict(presence_penalty=0.3, frequency_penalty=0.2, min_p=0.6,
                logit_bias={17: float("-inf"), 40: 1.0, 200: -0.5, 9: 0.25, 319: 0.5})
N_NEW = 32


@pytest.fixture(scope="module")
def qmodel():
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, RtnConfig
    from tests.test_gpu_api import _tiny_llama

    fp = _tiny_llama()
    fp.generation_config.eos_token_id = None
    q = AutoModelForCausalLM.from_pretrained(copy.deepcopy(fp), quantization_config=RtnConfig(
        bits=4, group_size=32, compute_dtype="fp32", scale_dtype="fp32"), device_map="cuda")
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers

    optimize_transformers(q, max_ctx=256)
    return q


def _native(eng, n_new, burst=16, launch="graph", **kw):
    eng.launch = launch
    eng.captured = False
    eng.set_sampler(**kw)
    try:
        out = sum(eng.iter_generate(PROMPT, n_new, burst=burst), [])
        return out, eng.token_counts().cpu().numpy().copy() if eng.controls_installed else None
    finally:
        eng.clear_sampler()


def _rows(eng, n_new, **kw):
    """burst = 1: the logits every token was chosen from are still in engine.logits when the burst is read"""
    eng.launch = "graph"
    eng.captured = False
    eng.set_sampler(**kw)
    tokens, rows = [], []
    try:
        for new in eng.iter_generate(PROMPT, n_new, burst=1):
            rows.append(eng.logits.cpu().numpy().copy())
            tokens += new
    finally:
        eng.clear_sampler()
    return tokens, rows


def test_seeded_run_with_all_controls_step_by_step_and_across_launch_modes(qmodel):
    eng = qmodel.woq_engine
    vocab, seed, n = eng.cfg.vocab, 0x5EED0123456789, len(PROMPT)
    tokens, rows = _rows(eng, N_NEW, seed=seed, **SAMPLED, **CONTROLS)
    assert len(tokens) == N_NEW and not eng.controls_installed and not eng.sampler_installed
    history, counts, needed_tol, cut_by_min_p = list(PROMPT), np.zeros(vocab, np.int64), 0, 0
    for i, (t, lg) in enumerate(zip(tokens, rows)):
        s = C.scores_f32(lg, history, counts, SAMPLED["repetition_penalty"], SAMPLED["temperature"], True,
                         CONTROLS["presence_penalty"], CONTROLS["frequency_penalty"], CONTROLS["logit_bias"])
        ref = C.choose(s, SAMPLED["top_k"], SAMPLED["top_p"], CONTROLS["min_p"])
        cut_by_min_p += ref.n_kept < R.choose(s, SAMPLED["top_k"], SAMPLED["top_p"]).n_kept
        tol = 8 * ref.n_kept * R.TWO_M24
        u = R.uniform_at(seed, n - 1 + i)  # the position the step fed (the prompt pass fed n - 1)
        assert ref.accepts(t, u, tol), (i, t, u, ref.pick(u))
        if (ref.needs_tolerance(u, tol) or ref.boundary_margin < 100 * 8 * ref.n_candidates * R.TWO_M24
                or ref.min_p_units < 100):
            needed_tol += 1
        else:
            assert t == ref.pick(u), (i, t, u, ref.pick(u))
        history.append(t)
        counts[t] += 1
    print("draws that needed the tolerance: %d, steps cut by min_p: %d of %d" % (needed_tol, cut_by_min_p, N_NEW))
    assert needed_tol <= 2, needed_tol
    assert cut_by_min_p >= N_NEW // 4 and len(set(tokens)) > 4 and 17 not in tokens
    # every launch mode, every burst size: the same tokens, and the count table = the histogram of the generated tokens
    for launch, burst in (("eager", 16), ("graph", 5), ("graph", 16)):
        again, table = _native(eng, N_NEW, burst=burst, launch=launch, seed=seed, **SAMPLED, **CONTROLS)
        assert again == tokens, (launch, burst)
        assert np.array_equal(table, np.bincount(tokens, minlength=vocab)), (launch, burst)
    assert eng.status() == 0


def test_changing_penalty_and_bias_mid_run_keeps_the_graph(qmodel):
    eng = qmodel.woq_engine
    seed = 77
    tokens, _ = _native(eng, N_NEW, burst=8, seed=seed, **SAMPLED, **CONTROLS)
    eng.launch = "graph"
    eng.captured = False
    eng.set_sampler(seed=seed, **SAMPLED, **CONTROLS)
    try:
        out = []
        for new in eng.iter_generate(PROMPT, N_NEW, burst=8):
            out += new
            if len(out) == 17:
                assert eng.captured
                banned = {int(t): float("-inf") for t in set(tokens[17:])}  # whatever came next may not come now
                eng.set_sampler(seed=seed, **SAMPLED, **dict(CONTROLS, frequency_penalty=1.5, logit_bias=banned))
                assert eng.captured and eng.controls_installed  # values live in device memory: the graph stays
    finally:
        eng.clear_sampler()
    assert out[:17] == tokens[:17] and not set(out[17:]) & set(tokens[17:])
    assert eng.status() == 0 and not eng.captured


def test_greedy_with_frequency_penalty_is_the_reference_argmax_and_the_torch_path(qmodel):
    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler, generate_sampled

    eng = qmodel.woq_engine
    vocab = eng.cfg.vocab
    plain = eng.generate(PROMPT, N_NEW)
    kw = dict(do_sample=False, frequency_penalty=2.0, presence_penalty=0.5, logit_bias={plain[0]: -1.0})
    tokens, rows = _rows(eng, N_NEW, **kw)
    history, counts = list(PROMPT), np.zeros(vocab, np.int64)
    for i, (t, lg) in enumerate(zip(tokens, rows)):
        s = C.adjusted_f32(lg, history, counts, 1.0, 0.5, 2.0, kw["logit_bias"])
        assert t == int(np.flatnonzero(s == np.nanmax(s))[0]), i  # bit-equal scores: the same argmax, lowest id on ties
        history.append(t)
        counts[t] += 1
    assert tokens != plain and np.bincount(tokens).max() <= np.bincount(plain).max()
    assert _native(eng, N_NEW, launch="eager", **kw)[0] == tokens
    assert _native(eng, N_NEW, burst=5, **kw)[0] == tokens
    # the torch restatement: the same logits kernels, the same IEEE operations
    assert generate_sampled(eng, PROMPT, N_NEW, DeviceSampler(**kw)) == tokens
    assert eng.status() == 0


def test_neutral_controls_are_the_existing_sampler_path(qmodel):
    eng = qmodel.woq_engine
    plain = dict(do_sample=True, temperature=0.9, top_k=8, top_p=0.95, repetition_penalty=1.1)
    want, table = _native(eng, N_NEW, seed=9, **plain)
    assert table is None
    eng.set_sampler(seed=9, **plain, presence_penalty=0.0, frequency_penalty=None, min_p=0.0, logit_bias={})
    try:
        assert eng.sampler_installed and not eng.controls_installed
        got = sum(eng.iter_generate(PROMPT, N_NEW), [])
    finally:
        eng.clear_sampler()
    assert got == want
    # installed, then made neutral again: the controls go (and the graph with them)
    eng.set_sampler(seed=9, **plain, min_p=0.2)
    try:
        assert eng.controls_installed
        eng.set_sampler(seed=9, **plain)
        assert not eng.controls_installed and not eng.captured
        assert sum(eng.iter_generate(PROMPT, N_NEW), []) == want
    finally:
        eng.clear_sampler()
    # a min_p that cuts nothing and a bias of +0.0 leave the choice alone too (the pre-pass path, same fp32 scores)
    got, _ = _native(eng, N_NEW, seed=9, **plain, min_p=1e-30, logit_bias={3: 0.0})
    assert got == want
    assert eng.native_sampler_supports(**plain, min_p=0.1, logit_bias={0: -1.0}, presence_penalty=-2.0)
    assert eng.native_sampler_supports(do_sample=True, top_k=0, top_p=1.0, min_p=0.1)
    assert not eng.native_sampler_supports(do_sample=False, min_p=0.1)
    assert not eng.native_sampler_supports(**plain, logit_bias={eng.cfg.vocab: 1.0})
    assert not eng.native_sampler_supports(**plain, logit_bias={1: float("inf")})
    assert not eng.native_sampler_supports(**plain, frequency_penalty=float("nan"))
    assert not eng.native_sampler_supports(**plain, min_p=1.5)
    assert not eng.native_sampler_supports(do_sample=True, top_k=0, top_p=0.9, min_p=0.1)
    with pytest.raises(RuntimeError, match="QBits"):
        eng.set_sampler(do_sample=False, min_p=0.1)
    eng.clear_sampler()
    assert eng.status() == 0


def test_model_generate_maps_min_p_and_sequence_bias_onto_the_native_sampler(qmodel):
    from intel_extension_for_transformers_amd.runtime.engine import iter_sampled_auto

    eng = qmodel.woq_engine
    ids = torch.tensor([PROMPT], device="cuda")
    count = eng.native_sampled_requests
    torch.manual_seed(11)
    a = qmodel.generate(ids, max_new_tokens=24, min_p=0.1, do_sample=True, top_k=0)
    torch.manual_seed(11)
    b = qmodel.generate(ids, max_new_tokens=24, min_p=0.1, do_sample=True, top_k=0)
    assert eng.native_sampled_requests == count + 2 and torch.equal(a, b) and a.shape == (1, len(PROMPT) + 24)
    greedy = qmodel.generate(ids, max_new_tokens=24)[0, len(PROMPT):].tolist()
    t = greedy[0]
    for kw in (dict(sequence_bias={(t,): float("-inf")}), dict(suppress_tokens=[t])):
        out = qmodel.generate(ids, max_new_tokens=24, **kw)[0, len(PROMPT):].tolist()
        assert t not in out and len(out) == 24
    assert eng.native_sampled_requests == count + 4 and not eng.sampler_installed and not eng.controls_installed
    # a seed makes a sampled request reproducible whatever torch's generator holds
    runs = [sum(iter_sampled_auto(eng, PROMPT, 16, do_sample=True, temperature=0.9, top_k=8, frequency_penalty=0.5,
                                  seed=1234), []) for _ in range(2)]
    assert runs[0] == runs[1] and eng.native_sampled_requests == count + 6
    assert eng.status() == 0


def test_controls_need_an_installed_sampler_and_one_gpu(qmodel):
    import ctypes

    from intel_extension_for_transformers_amd import _lib as L
    from intel_extension_for_transformers_amd.runtime.engine import WoqDecoderEngine

    eng = qmodel.woq_engine
    assert not eng.sampler_installed
    ctl, ids, vals = L.sampler_controls(presence_penalty=0.5)
    assert L.lib().woq_engine_set_sampler_controls(eng._h, ctypes.byref(ctl), ids, vals) != 0
    assert L.lib().woq_last_error().decode().startswith("QBits:") and "sampler installed" in L.lib().woq_last_error().decode()
    # switching an installed sampler to greedy while min_p is set is refused on that entry point too
    eng.set_sampler(do_sample=True, top_k=8, min_p=0.2)
    try:
        with pytest.raises(RuntimeError, match="QBits: min_p"):
            eng.set_sampler(do_sample=False, min_p=0.2)
    finally:
        eng.clear_sampler()
    # refused controls leave no sampler behind: the next greedy request is the plain one
    before = eng.generate(PROMPT, 8)
    with pytest.raises(RuntimeError, match="QBits"):
        eng.set_sampler(do_sample=False, min_p=0.1)
    assert not eng.sampler_installed and not eng.controls_installed
    with pytest.raises(RuntimeError, match="QBits"):
        eng.set_sampler(do_sample=True, top_k=8, logit_bias={eng.cfg.vocab: 1.0})
    assert not eng.sampler_installed and eng.generate(PROMPT, 8) == before
    # a tensor-parallel rank's engine: the head is vocab-sharded
    tp = WoqDecoderEngine(hidden=256, inter=512, heads=4, kv_heads=4, head_dim=64, layers=1, vocab=320, max_ctx=64,
                          tp_rank=0, tp_size=2)
    assert L.lib().woq_engine_set_sampler_controls(tp._h, ctypes.byref(ctl), ids, vals) != 0
    assert "one GPU" in L.lib().woq_last_error().decode()
    assert not tp.native_sampler_supports(do_sample=False, presence_penalty=0.5)
    assert eng.status() == 0
