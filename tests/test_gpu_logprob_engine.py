"""The log-probability record inside the decode engine (tiny Llama through `optimize_transformers`, max_ctx 256, a prompt
of 7 ids, 24 new tokens): after the pick of the prompt pass's tail, of eager steps, of the one-step graph and of the graph
of 8 chained steps, csrc/woq_logprob.hip writes row p of three device logs. The record describes the raw logits whatever
picked the token; tokens do not change; launch mode, burst size and prompt chunking do not change a bit of it.

Values are held to float64 (tests/logprob_reference.py) within tol = 4 x the largest deviation of the fp32 restatement of
the kernel's summation order from float64 on the logits of this file's own steps (computed from the reference alone)."""
import copy

import numpy as np
import pytest
import torch

from tests import logprob_reference as R

pytestmark = pytest.mark.gpu

PROMPT = [5, 9, 33, 2, 71, 9, 9]
N_NEW = 24
ROW0 = len(PROMPT) - 1  # the first generated token's row
PENALTY = dict(do_sample=False, repetition_penalty=1.3)
SAMPLED = dict(do_sample=True, temperature=0.9, top_k=8, top_p=0.95, repetition_penalty=1.1, seed=7)
SENTINEL = -5.0


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


def _mark_logs(eng):
    """every row of the three logs <- a value no record holds, so that what a run wrote is what it wrote"""
    eng.set_logprobs(True)
    eng.clear_logprobs()
    chosen, top_id, top_lp = eng.logprob_log()
    chosen.fill_(SENTINEL), top_id.fill_(int(SENTINEL)), top_lp.fill_(SENTINEL)


def _raw_rows(eng, rows=slice(ROW0, ROW0 + N_NEW)):
    """the logs' bits [rows, 1 + 20 + 20] int32 on the host"""
    chosen, top_id, top_lp = eng.logprob_log()
    return torch.cat([chosen[rows, None].view(torch.int32), top_id[rows], top_lp[rows].view(torch.int32)], 1).cpu()


def _run(eng, launch="graph", burst=16, sampler=None, chunk=2048, n_top=20):
    eng.launch = launch
    eng.captured = False
    _mark_logs(eng)
    toks, lps, top = eng.generate(PROMPT, N_NEW, burst=burst, sampler=sampler, chunk=chunk, logprobs=n_top)
    assert not eng.logprobs_on and not eng.sampler_installed
    return toks, lps, top, _raw_rows(eng)


@pytest.fixture(scope="module")
def stepped(qmodel):
    """Burst 1 by hand, greedy and with the penalty sampler: after each chaining step its logits, token and record.
    -> {name: (tokens, logits [24, vocab] fp32, raw rows)} and the file's tolerance."""
    eng = qmodel.woq_engine
    eng.launch = "eager"
    out = {}
    for name, sampler in (("greedy", None), ("penalty", PENALTY)):
        _mark_logs(eng)
        eng.set_logprobs(True)
        if sampler is not None:
            eng.set_sampler(**sampler)
            eng.mark_seen(PROMPT, clear=True)
        try:
            eng.prefill(PROMPT, greedy=True)
            toks, logits = [int(eng.token.item())], [eng.logits.cpu().numpy().copy()]
            for _ in range(N_NEW - 1):
                eng.step(greedy=True)
                toks.append(int(eng.token.item()))
                logits.append(eng.logits.cpu().numpy().copy())
            assert int(eng.pos.item()) == len(PROMPT) + N_NEW - 1
            assert eng.token_log()[ROW0 + 1:ROW0 + N_NEW].tolist() == toks[1:]
        finally:
            eng.clear_sampler()
            eng.clear_logprobs()
        out[name] = (toks, np.stack(logits), _raw_rows(eng))
    dev = max(R.deviation(lg, t) for toks, logits, _ in out.values() for lg, t in zip(logits, toks))
    assert 0 < dev < 1e-4
    print("largest deviation of the fp32 restatement from float64 on these steps: %.3e" % dev)
    return out, 4 * dev


def _unpack(raw):
    raw = raw.numpy()
    return raw[:, 0].copy().view(np.float32), raw[:, 1:1 + R.TOP], raw[:, 1 + R.TOP:].copy().view(np.float32)


def _check_against_f64(raw, logits, toks, tol, what):
    chosen, top_id, top_lp = _unpack(raw)
    worst = 0.0
    for j, (lg, t) in enumerate(zip(logits, toks)):
        c64, id64, lp64 = R.record_f64(lg, t)
        assert (top_id[j] == id64).all(), (what, j)
        listed = id64 >= 0
        assert np.isneginf(top_lp[j][~listed]).all(), (what, j)
        worst = max(worst, abs(float(chosen[j]) - c64), float(np.abs(top_lp[j][listed] - lp64[listed]).max()))
        # chosen is the record's own value at the token
        at = np.flatnonzero(id64 == t)
        if len(at):
            assert chosen[j] == top_lp[j][at[0]], (what, j)
    print("%s: max |record - float64| = %.3e (tol %.3e)" % (what, worst, tol))
    assert worst <= tol, what


def test_each_step_matches_the_float64_reference_of_its_logits(qmodel, stepped):
    out, tol = stepped
    for name, (toks, logits, raw) in out.items():
        _check_against_f64(raw, logits, toks, tol, name)


def test_greedy_records_lead_with_the_token_and_penalised_ones_describe_raw_logits(qmodel, stepped):
    out, _ = stepped
    toks, logits, raw = out["greedy"]
    assert (_unpack(raw)[1][:, 0] == np.array(toks)).all()
    ptoks, plogits, praw = out["penalty"]
    first = _unpack(praw)[1][:, 0]
    assert (first == plogits.argmax(1)).all()        # the raw distribution's best id ...
    assert (first != np.array(ptoks)).any()          # ... which the penalty overrules on this prompt at least once
    assert ptoks != toks


def test_tokens_do_not_change_with_recording(qmodel):
    eng = qmodel.woq_engine
    eng.launch = "graph"
    eng.captured = False
    greedy = eng.generate(PROMPT, N_NEW)
    sampled = eng.generate(PROMPT, N_NEW, sampler=SAMPLED)
    assert _run(eng)[0] == greedy
    assert _run(eng, sampler=SAMPLED)[0] == sampled
    assert sampled != greedy
    assert eng.generate(PROMPT, N_NEW) == greedy and eng.status() == 0


@pytest.mark.parametrize("sampler", [None, PENALTY], ids=["greedy", "penalty"])
def test_launch_mode_and_burst_size_do_not_change_a_bit(qmodel, stepped, sampler):
    eng = qmodel.woq_engine
    toks, _, want = stepped[0]["greedy" if sampler is None else "penalty"]
    for launch in ("graph", "eager"):
        for burst in (1, 5, 16):  # 16 = two replays of the 8-step graph, 5 and the tail of 23 = its remainder
            got_toks, lps, top, raw = _run(eng, launch=launch, burst=burst, sampler=sampler)
            assert got_toks == toks, (launch, burst)
            assert torch.equal(raw, want), (launch, burst)
            # what generate returns is the logs' content
            chosen, top_id, top_lp = _unpack(raw)
            assert np.array_equal(np.array(lps, dtype=np.float32), chosen)
            assert [[i for i, _ in row] for row in top] == top_id.tolist()
            assert np.array_equal(np.array([[v for _, v in row] for row in top], dtype=np.float32), top_lp)
    eng.launch = "graph"


def test_first_token_has_a_record_and_prompt_chunks_do_not_matter(qmodel, stepped):
    eng = qmodel.woq_engine
    toks, lps, top, raw = _run(eng, n_top=3)
    assert len(toks) == len(lps) == len(top) == N_NEW and all(len(t) == 3 for t in top)
    assert torch.equal(raw[0], stepped[0]["greedy"][2][0]) and top[0][0][0] == toks[0]
    ctoks, clps, ctop, craw = _run(eng, chunk=3, n_top=3)
    assert ctoks == toks and torch.equal(craw, raw)
    # only the last chunk's tail left a record: the rows of the earlier chunks' last positions are untouched
    assert (_raw_rows(eng, slice(0, ROW0))[:, 1:1 + R.TOP] == int(SENTINEL)).all()


def test_torch_fallback_agrees_with_the_native_records(qmodel, stepped):
    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler, iter_sampled

    eng = qmodel.woq_engine
    tol = stepped[1]
    bursts = list(iter_sampled(eng, PROMPT, N_NEW, DeviceSampler(**PENALTY), logprobs=5))
    ftoks, flps, ftop = (sum((b[i] for b in bursts), []) for i in range(3))
    toks, lps, top, _ = _run(eng, sampler=PENALTY, n_top=5)
    assert ftoks == toks == stepped[0]["penalty"][0]
    assert [[i for i, _ in row] for row in ftop] == [[i for i, _ in row] for row in top]
    err = max(float(np.abs(np.array(flps) - np.array(lps)).max()),
              float(np.abs(np.array([[v for _, v in r] for r in ftop]) - np.array([[v for _, v in r] for r in top])).max()))
    print("torch fallback vs native records: %.3e (tol %.3e)" % (err, tol))
    assert err <= tol


def test_cleanup_restores_the_plain_step_and_leaves_other_rows_alone(qmodel):
    eng = qmodel.woq_engine
    eng.launch = "graph"
    eng.captured = False
    before = eng.generate(PROMPT, N_NEW)
    _run(eng)
    beyond = _raw_rows(eng, slice(ROW0 + N_NEW, eng.cfg.max_ctx + 1))
    assert (beyond[:, 1:1 + R.TOP] == int(SENTINEL)).all()
    assert (beyond[:, 0].numpy().copy().view(np.float32) == SENTINEL).all()
    assert (_raw_rows(eng, slice(0, ROW0))[:, 1:1 + R.TOP] == int(SENTINEL)).all()
    eng.set_logprobs(True)
    assert eng.captured is False
    eng.clear_logprobs()
    assert eng.generate(PROMPT, N_NEW) == before and eng.status() == 0
    with pytest.raises(ValueError):
        eng.generate(PROMPT, 2, logprobs=21)
