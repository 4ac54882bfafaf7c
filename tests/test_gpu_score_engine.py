"""Scoring a given text inside the decode engine (tiny Llama of tests/test_gpu_logprob_engine.py, max_ctx 256, a prompt
of 40 fixed ids): `woq_engine_prefill_scored` writes one row of the three log-probability logs per prompt position,
`score` / `perplexity` read them back.

Each written row is held to tests/score_reference.py's float64 record of the residual-stream rows the prompt pass itself
left (`woq_engine_prefill_rows_ptr`), the model's final norm and its lm_head, within the reference's own tolerance.
Rows the call does not own keep a sentinel; the last row of a greedy call and everything else a prompt pass leaves behind
(KV cache, logits, token) are bit-identical to plain `prefill`."""
import copy
import math

import numpy as np
import pytest
import torch

from tests import logprob_reference as R
from tests import score_reference as S

pytestmark = pytest.mark.gpu

PROMPT = [5, 9, 33, 2, 71, 9, 9, 140, 3, 250, 17, 64, 8, 301, 77, 12, 5, 199, 42, 6,
          88, 230, 11, 9, 154, 31, 2, 270, 19, 101, 55, 7, 213, 90, 4, 166, 23, 315, 60, 129]
N = len(PROMPT)
SENTINEL = -5.0


@pytest.fixture(scope="module")
def qmodel():
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, RtnConfig
    from tests.test_gpu_api import _tiny_llama

    fp = _tiny_llama()
    fp.generation_config.eos_token_id = None
    q = AutoModelForCausalLM.from_pretrained(copy.deepcopy(fp), quantization_config=RtnConfig(
        bits=4, group_size=32, compute_dtype="fp32", scale_dtype="fp32"), device_map="cuda")
    optimize_transformers(q, max_ctx=256)
    return q


def _mark_logs(eng):
    eng.set_logprobs(True)
    eng.clear_logprobs()
    chosen, top_id, top_lp = eng.logprob_log()
    chosen.fill_(SENTINEL), top_id.fill_(int(SENTINEL)), top_lp.fill_(SENTINEL)


def _raw_rows(eng, rows):
    chosen, top_id, top_lp = eng.logprob_log()
    return torch.cat([chosen[rows, None].view(torch.int32), top_id[rows], top_lp[rows].view(torch.int32)], 1).cpu()


def _unpack(raw):
    raw = raw.numpy()
    return raw[:, 0].copy().view(np.float32), raw[:, 1:1 + R.TOP], raw[:, 1 + R.TOP:].copy().view(np.float32)


def _untouched(eng, rows):
    chosen, top_id, top_lp = _unpack(_raw_rows(eng, rows))
    return (chosen == SENTINEL).all() and (top_id == int(SENTINEL)).all() and (top_lp == SENTINEL).all()


def _check_chunk(eng, start, T, targets, n_rows):
    """log rows start .. start + n_rows - 1 against score_f64 of the hidden rows the prompt pass left"""
    head = eng.head_tensors
    x = eng.prefill_rows(T)[:n_rows].cpu().numpy()
    norm_w, W = head["norm"].detach().cpu().numpy(), head["lm_head"].detach().cpu()
    tg = np.asarray(targets[:n_rows], dtype=np.int32)
    c64, id64, lp64 = S.score_f64(x, norm_w, eng.cfg.rms_eps, W, tg)
    tol = S.tolerance(x, norm_w, eng.cfg.rms_eps, W, tg)
    logits = S.logits_f64(x, norm_w, eng.cfg.rms_eps, W)
    chosen, top_id, top_lp = _unpack(_raw_rows(eng, slice(start, start + n_rows)))
    worst, loose = 0.0, 0
    for r in range(n_rows):
        if np.isnan(c64[r]):
            assert np.isnan(chosen[r])
        else:
            worst = max(worst, abs(float(chosen[r]) - c64[r]))
        if S.min_top_gap(logits[r]) > 2 * tol:
            assert (top_id[r] == id64[r]).all(), (start, r)
            worst = max(worst, float(np.abs(top_lp[r] - lp64[r]).max()))
        else:  # near-ties among the top 21: the same ids up to the tied ones, each value that of its id
            loose += 1
            lp_all = logits[r].astype(np.float64) - (logits[r, id64[r, 0]] - lp64[r, 0])
            assert len(set(top_id[r].tolist()) ^ set(id64[r].tolist())) <= 2, (start, r)
            worst = max(worst, float(np.abs(top_lp[r] - lp_all[top_id[r]]).max()))
    print("rows %d..%d: max |engine - float64| = %.3e (tol %.3e), %d rows compared by id"
          % (start, start + n_rows - 1, worst, tol, loose))
    assert 0 < tol < 1e-3 and worst <= tol


@pytest.mark.parametrize("chunk", [N, 16], ids=["one_chunk", "chunks_of_16"])
def test_scored_rows_match_the_reference_of_the_rows_the_prompt_pass_left(qmodel, chunk):
    eng = qmodel.woq_engine
    _mark_logs(eng)
    targets = PROMPT[1:] + [-1]
    for s0 in range(0, N, chunk):
        T = min(chunk, N - s0)
        eng.prefill_scored(PROMPT[s0:s0 + T], targets[s0:s0 + T], start_pos=s0, greedy=False)
        _check_chunk(eng, s0, T, targets[s0:s0 + T], T)
        assert _untouched(eng, slice(s0 + T, eng.cfg.max_ctx + 1))  # nothing beyond the rows written so far
    # the last row's target is outside the vocabulary: chosen NaN, its top 20 written
    chosen, top_id, _ = _unpack(_raw_rows(eng, slice(N - 1, N)))
    assert np.isnan(chosen[0]) and (top_id[0] >= 0).all()
    assert not eng.logprobs_on and eng.status() == 0


def test_greedy_leaves_the_last_row_to_the_tail(qmodel):
    eng = qmodel.woq_engine
    targets = PROMPT[1:] + [-1]
    # recording off: the tail writes nothing, row N - 1 keeps the sentinel
    _mark_logs(eng)
    eng.prefill_scored(PROMPT, targets, greedy=True)
    _check_chunk(eng, 0, N, targets, N - 1)
    assert _untouched(eng, slice(N - 1, eng.cfg.max_ctx + 1))
    # recording on: row N - 1 and the token are what plain prefill writes; KV cache and logits as well
    _mark_logs(eng)
    eng.set_logprobs(True)
    try:
        eng.kv_cache("k").zero_(), eng.kv_cache("v").zero_()
        plain_logits = eng.prefill(PROMPT, greedy=True).clone()
        plain = (_raw_rows(eng, slice(N - 1, N)), int(eng.token.item()), int(eng.pos.item()),
                 eng.kv_cache("k").clone(), eng.kv_cache("v").clone(), eng.logits.clone())
        assert _untouched(eng, slice(0, N - 1))
        _mark_logs(eng)
        eng.kv_cache("k").zero_(), eng.kv_cache("v").zero_()
        eng.set_logprobs(True)
        scored_logits = eng.prefill_scored(PROMPT, targets, greedy=True).clone()
        assert torch.equal(_raw_rows(eng, slice(N - 1, N)), plain[0])
        assert (int(eng.token.item()), int(eng.pos.item())) == plain[1:3]
        assert torch.equal(eng.kv_cache("k"), plain[3]) and torch.equal(eng.kv_cache("v"), plain[4])
        assert torch.equal(eng.logits, plain[5]) and torch.equal(scored_logits, plain_logits)
        assert not _untouched(eng, slice(0, N - 1)) and _untouched(eng, slice(N, eng.cfg.max_ctx + 1))
    finally:
        eng.clear_logprobs()


def test_score_and_perplexity_return_the_log_rows(qmodel):
    eng = qmodel.woq_engine
    eng.launch = "graph"
    eng.captured = False
    before = eng.generate(PROMPT, 8, logprobs=5)
    _mark_logs(eng)
    lps, top = eng.score(PROMPT, logprobs=3)
    assert not eng.logprobs_on and not eng.sampler_installed
    chosen, top_id, top_lp = _unpack(_raw_rows(eng, slice(0, N - 1)))
    assert len(lps) == len(top) == N - 1 and all(len(t) == 3 for t in top)
    assert np.array_equal(np.array(lps, dtype=np.float32), chosen) and np.isfinite(chosen).all()
    assert [[i for i, _ in row] for row in top] == top_id[:, :3].tolist()
    assert np.array_equal(np.array([[v for _, v in row] for row in top], dtype=np.float32), top_lp[:, :3])
    assert _untouched(eng, slice(N, eng.cfg.max_ctx + 1))
    clps, _ = eng.score(PROMPT, chunk=16)  # chunked: again the log rows
    assert np.array_equal(np.array(clps, dtype=np.float32), _unpack(_raw_rows(eng, slice(0, N - 1)))[0])
    lps, _ = eng.score(PROMPT)
    assert eng.perplexity(PROMPT) == math.exp(-math.fsum(lps) / (N - 1))
    # the flags survive in the other state too
    eng.set_logprobs(True)
    eng.set_sampler(do_sample=False, repetition_penalty=1.3)
    try:
        assert eng.score(PROMPT)[0] == lps
        assert eng.logprobs_on and eng.sampler_installed
    finally:
        eng.clear_sampler()
        eng.clear_logprobs()
    assert eng.generate(PROMPT, 8, logprobs=5) == before and eng.status() == 0


def test_errors(qmodel):
    from intel_extension_for_transformers_amd.runtime.engine import WoqDecoderEngine

    eng = qmodel.woq_engine
    with pytest.raises(RuntimeError, match="QBits:"):
        eng.score([5])
    with pytest.raises(RuntimeError, match="QBits:"):
        eng.score([5] * (eng.cfg.max_ctx + 1))
    with pytest.raises(ValueError):
        eng.score(PROMPT, logprobs=21)
    # an engine that never allocated its logs refuses prefill_scored (before anything else is looked at)
    c = eng.cfg
    fresh = WoqDecoderEngine(c.hidden, c.inter, c.heads, c.kv_heads, c.head_dim, c.layers, c.vocab, max_ctx=c.max_ctx)
    head = eng.head_tensors
    fresh.set_head(head["embed"], head["norm"], head["lm_head"])
    with pytest.raises(RuntimeError, match="QBits: no log-probability log"):
        fresh.prefill_scored([5, 9], [9, -1])
