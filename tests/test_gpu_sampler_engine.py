"""The native sampler inside the decode engine (tiny Llama through `optimize_transformers`): the chaining tail of the
prompt pass, eager steps, the one-step graph and the graph of 8 chained steps picks its token with csrc/woq_sample.hip.
Deterministic settings are held token for token to the torch path (`iter_sampled` + `DeviceSampler`: same logits kernels,
same IEEE penalty); a seeded sampled run is checked step by step against tests/sampler_reference.py with the numpy Philox
uniform of each position (acceptance rule and tolerance of tests/test_gpu_sampler_kernel.py), and must not depend on the
launch mode, the burst size or a parameter change without recapture. One table test pins which setter calls drop a
captured graph: those that change (sampler, controls, guide, logprobs), and no others."""
import copy

import numpy as np
import pytest
import torch

from tests import sampler_reference as R

pytestmark = pytest.mark.gpu

PROMPT = [5, 9, 33, 2, 71, 9, 9]
SAMPLED = dict(do_sample=True, temperature=0.9, top_k=8, top_p=0.95, repetition_penalty=1.1)


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
        return sum(eng.iter_generate(PROMPT, n_new, burst=burst), [])
    finally:
        eng.clear_sampler()


def test_deterministic_settings_equal_the_torch_sampler_path(qmodel):
    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler, generate_sampled

    eng = qmodel.woq_engine
    before = eng.generate(PROMPT, 24)
    want = generate_sampled(eng, PROMPT, 24, DeviceSampler(do_sample=False, repetition_penalty=1.3))
    assert _native(eng, 24, do_sample=False, repetition_penalty=1.3) == want
    assert _native(eng, 24, launch="eager", do_sample=False, repetition_penalty=1.3) == want
    assert _native(eng, 24, do_sample=True, top_k=1, temperature=0.7, repetition_penalty=1.3, seed=5) == want
    assert want != before  # the penalty matters on this prompt, so the comparison says something
    # with the sampler removed the greedy path is the untouched one
    assert not eng.sampler_installed and eng.generate(PROMPT, 24) == before
    assert eng.status() == 0


def test_chunked_prompt_marks_only_prompt_and_generated_ids(qmodel):
    """A prompt longer than `chunk` goes through several prompt passes; only the last one's tail may pick (and mark) a
    token: the history stays the distinct ids of prompt + generated, and the tokens stay the torch path's."""
    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler, generate_sampled

    eng = qmodel.woq_engine
    want = generate_sampled(eng, PROMPT, 24, DeviceSampler(do_sample=False, repetition_penalty=1.3), chunk=3)
    assert want == generate_sampled(eng, PROMPT, 24, DeviceSampler(do_sample=False, repetition_penalty=1.3))
    for launch in ("graph", "eager"):
        eng.launch = launch
        eng.captured = False
        eng.set_sampler(do_sample=False, repetition_penalty=1.3)
        try:
            got = sum(eng.iter_generate(PROMPT, 24, chunk=3), [])
            bits = eng.seen_bits().cpu().numpy().view(np.uint32)
        finally:
            eng.clear_sampler()
        assert got == want, launch
        expect = np.zeros_like(bits)
        for t in set(PROMPT + got):
            expect[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
        assert np.array_equal(bits, expect), launch
    eng.launch = "graph"
    # a sampled request too: the bit set is prompt + generated, whatever the chunking
    eng.set_sampler(seed=7, **SAMPLED)
    try:
        got = sum(eng.iter_generate(PROMPT, 24, chunk=2), [])
        bits = eng.seen_bits().cpu().numpy().view(np.uint32)
    finally:
        eng.clear_sampler()
    expect = np.zeros_like(bits)
    for t in set(PROMPT + got):
        expect[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    assert np.array_equal(bits, expect)
    assert eng.status() == 0


def test_native_sampler_supports_mirrors_the_native_checks(qmodel):
    eng = qmodel.woq_engine
    assert eng.native_sampler_supports(do_sample=True, temperature=0.1, top_k=40, top_p=0.75, repetition_penalty=1.1)
    assert not eng.native_sampler_supports(do_sample=True, temperature=float("inf"), top_k=40)
    assert not eng.native_sampler_supports(do_sample=True, temperature=float("nan"), top_k=40)
    assert not eng.native_sampler_supports(do_sample=False, repetition_penalty=0.0)
    assert not eng.native_sampler_supports(do_sample=True, top_k=40, repetition_penalty=-1.0)


def test_seeded_sampled_run_step_by_step_and_across_launch_modes(qmodel):
    eng = qmodel.woq_engine
    seed, n_new, n = 0x5EED0123456789, 48, len(PROMPT)
    # burst = 1: the logits every token was drawn from are still in engine.logits when the burst is read
    eng.launch = "graph"
    eng.captured = False
    eng.set_sampler(seed=seed, **SAMPLED)
    tokens, rows = [], []
    try:
        for new in eng.iter_generate(PROMPT, n_new, burst=1):
            rows.append(eng.logits.cpu().numpy().copy())
            tokens += new
    finally:
        eng.clear_sampler()
    assert len(tokens) == n_new and eng.native_sampled_requests >= 1
    history, needed_tol = list(PROMPT), 0
    for i, (t, lg) in enumerate(zip(tokens, rows)):
        s = R.scores_f32(lg, history, SAMPLED["repetition_penalty"], SAMPLED["temperature"], True)
        ref = R.choose(s, SAMPLED["top_k"], SAMPLED["top_p"])
        tol = 8 * ref.n_kept * R.TWO_M24
        u = R.uniform_at(seed, n - 1 + i)  # the position the step fed (the prompt pass fed n - 1)
        assert ref.accepts(t, u, tol), (i, t, u, ref.pick(u))
        if ref.needs_tolerance(u, tol) or ref.boundary_margin < 100 * 8 * ref.n_candidates * R.TWO_M24:
            needed_tol += 1
        else:
            assert t == ref.pick(u), (i, t, u, ref.pick(u))
        history.append(t)
    assert needed_tol <= 2, needed_tol
    assert len(set(tokens)) > 8  # a sampled run, not a greedy one in disguise
    # the seen bit set == prompt + generated ids
    eng.set_sampler(seed=seed, **SAMPLED)
    try:
        again = sum(eng.iter_generate(PROMPT, n_new, burst=16), [])
        bits = eng.seen_bits().cpu().numpy().view(np.uint32)
    finally:
        eng.clear_sampler()
    assert again == tokens  # graph, bursts of 16 (8-step graphs + single steps)
    want = np.zeros_like(bits)
    for t in set(PROMPT + tokens):
        want[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    assert np.array_equal(bits, want)
    assert _native(eng, n_new, burst=16, launch="eager", seed=seed, **SAMPLED) == tokens
    assert _native(eng, n_new, burst=5, launch="graph", seed=seed, **SAMPLED) == tokens
    # a temperature change half way, without a new capture: identical up to the change
    eng.launch = "graph"
    eng.captured = False
    eng.set_sampler(seed=seed, **SAMPLED)
    try:
        out = []
        for new in eng.iter_generate(PROMPT, n_new, burst=8):
            out += new
            if len(out) == 25:
                assert eng.captured
                eng.set_sampler(seed=seed, **dict(SAMPLED, temperature=5.0, top_k=200, top_p=1.0))
                assert eng.captured  # parameters live in device memory: the graph stays
    finally:
        eng.clear_sampler()
    assert out[:25] == tokens[:25] and out != tokens
    assert eng.status() == 0 and not eng.captured


# the reachable tails as (sampler, controls, guide, logprobs): what a captured graph holds of the tail
TAILS = [(s, c, g, lp) for s, c, g in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)) for lp in (0, 1)]


def _permissive_guide(vocab, flip):
    """two states, nothing banned: every id moves to the other state (`flip`) or stays"""
    from intel_extension_for_transformers_amd.runtime.guide import TokenGuide

    table = np.empty((2, vocab), np.uint16)
    table[0], table[1] = (1, 0) if flip else (0, 1)
    return TokenGuide(table)


def _set_tail(eng, tail, variant=0):
    """the engine into `tail` through the public setters alone; `variant` changes every installed value, no flag"""
    s, c, g, lp = tail
    if s:
        eng.set_sampler(do_sample=True, temperature=0.9 + variant, top_k=8, seed=3 + variant,
                        **(dict(presence_penalty=0.5 + variant, logit_bias={7: -1.0 - variant}) if c else {}))
        if g:
            eng.set_guide(_permissive_guide(eng.cfg.vocab, flip=bool(variant)))
        elif eng.guide_installed:
            eng.clear_guide()
    else:
        eng.clear_sampler()
    eng.set_logprobs(bool(lp))
    assert (eng.sampler_installed, eng.controls_installed, eng.guide_installed, eng.logprobs_on) == tuple(map(bool, tail))


def _replay_one(eng):
    """woq_engine_replay(h, 1, stream) itself: (return code, message)"""
    from intel_extension_for_transformers_amd import _lib as L

    rc = L.lib().woq_engine_replay(eng._h, 1, L.stream_ptr())
    return rc, (L.lib().woq_last_error().decode() if rc else "")


def test_a_captured_graph_survives_a_setter_iff_the_tail_stays(qmodel):
    """Every ordered pair (A, B) of the ten tails: capture under A, move to B through the setters (other values where
    both have the same thing installed), replay. The graph is still there iff A == B; otherwise the replay is refused
    with a message (no fault). `eng.captured` says the same throughout. All 100 pairs are walked: on the two-layer model
    a capture is well under a millisecond and the whole table takes about 0.1 s on an MI355X."""
    eng = qmodel.woq_engine
    eng.launch = "graph"
    eng.prefill(PROMPT, greedy=True)
    try:
        for a in TAILS:
            for b in TAILS:
                _set_tail(eng, a)
                eng.pos.fill_(len(PROMPT))
                eng.capture()
                _set_tail(eng, b, variant=1)
                rc, why = _replay_one(eng)
                assert eng.captured == (a == b), (a, b)
                if a == b:
                    assert rc == 0, (a, b, why)
                else:
                    assert rc != 0 and "engine graph not captured" in why, (a, b, rc, why)
        # what the setters document to keep the graph, one by one
        _set_tail(eng, (1, 1, 1, 0))
        eng.capture()
        for keep in (lambda: eng.set_sampler(do_sample=True, temperature=5.0, top_k=200, presence_penalty=0.5),  # sampler
                     lambda: eng.set_sampler(do_sample=True, temperature=5.0, top_k=200, min_p=0.1),  # the controls' values
                     lambda: eng.set_guide(_permissive_guide(eng.cfg.vocab, flip=True)),  # another guide
                     lambda: eng.guide_reset(1)):
            keep()
            assert eng.captured and _replay_one(eng) == (0, "")
        # removing the controls under an installed guide runs the same kernels and still drops the graph
        eng.set_sampler(do_sample=True, temperature=5.0, top_k=200)
        assert not eng.captured and eng.guide_installed and _replay_one(eng)[0] != 0
        torch.cuda.synchronize()
    finally:
        eng.clear_sampler()
        eng.set_logprobs(False)
    assert eng.status() == 0 and not eng.captured


def test_model_generate_uses_the_native_sampler_and_falls_back(qmodel):
    eng = qmodel.woq_engine
    ids = torch.tensor([PROMPT], device="cuda")
    count = eng.native_sampled_requests
    torch.manual_seed(11)
    a = qmodel.generate(ids, max_new_tokens=24, **SAMPLED)
    torch.manual_seed(11)
    b = qmodel.generate(ids, max_new_tokens=24, **SAMPLED)
    assert eng.native_sampled_requests == count + 2 and not eng.sampler_installed
    assert torch.equal(a, b) and a.shape == (1, len(PROMPT) + 24)
    c = qmodel.generate(ids, max_new_tokens=24, **SAMPLED)  # another seed from the generator
    assert not torch.equal(a, c)
    first = int(a[0, len(PROMPT)])
    torch.manual_seed(11)
    short = qmodel.generate(ids, max_new_tokens=24, eos_token_id=first, **SAMPLED)
    assert short.shape[1] == len(PROMPT) + 1

    class Collect:
        def __init__(self):
            self.items, self.ended = [], False

        def put(self, v):
            self.items.append(v.reshape(-1).tolist())

        def end(self):
            self.ended = True

    st = Collect()
    torch.manual_seed(11)
    qmodel.generate(ids, max_new_tokens=6, streamer=st, **SAMPLED)
    assert st.ended and st.items[0] == PROMPT and sum(st.items[1:], []) == a[0, len(PROMPT):len(PROMPT) + 6].tolist()
    # what the native sampler does not cover still works, on the torch sampler
    count = eng.native_sampled_requests
    assert not eng.native_sampler_supports(do_sample=True, top_k=0, top_p=0.9)
    assert not eng.native_sampler_supports(do_sample=True, top_k=2000)
    for kw in (dict(top_k=0, top_p=0.9), dict(top_k=2000)):
        out = qmodel.generate(ids, max_new_tokens=8, do_sample=True, temperature=0.8, **kw)
        assert out.shape == (1, len(PROMPT) + 8)
    assert eng.native_sampled_requests == count
    with pytest.raises(RuntimeError, match="QBits"):
        eng.set_sampler(do_sample=True, top_k=0, top_p=0.9)
    assert eng.status() == 0


def test_chatbot_default_request_streams_what_predict_returns(tmp_path):
    from intel_extension_for_transformers_amd.neural_chat import GenerationConfig, PipelineConfig, build_chatbot
    from intel_extension_for_transformers_amd.transformers import RtnConfig
    from tests.test_gpu_api import _tiny_llama, _tiny_tokenizer

    d = tmp_path / "tiny-llama-chat"
    fp = _tiny_llama()
    fp.generation_config.eos_token_id = None
    fp.save_pretrained(str(d))
    _tiny_tokenizer(d, fp.config.vocab_size)
    bot = build_chatbot(PipelineConfig(model_name_or_path=str(d), device="cuda",
                                       optimization_config=RtnConfig(bits=4, group_size=128, scale_dtype="fp16")))
    cfg = GenerationConfig(max_new_tokens=12)  # the default request: sampling + repetition penalty
    assert cfg.do_sample and cfg.top_k == 40
    count = bot.engine.native_sampled_requests
    torch.manual_seed(3)
    text = bot.predict("w5 w17 w200 w3 w77", config=cfg)
    torch.manual_seed(3)
    pieces = list(bot.predict_stream("w5 w17 w200 w3 w77", config=cfg)[0])
    assert "".join(pieces) == text and len(text.split()) >= 1
    assert bot.engine.native_sampled_requests == count + 2 and not bot.engine.sampler_installed
