"""H2O eviction inside the decode engine, on the tiny model of the streaming tests (heads 4, kv heads 2: G = 2)."""
import numpy as np
import pytest

from intel_extension_for_transformers_amd.runtime.engine import H2OConfig, StreamingConfig
from tests import h2o_reference as H
from tests import kv_shift_reference as KR
from tests.test_gpu_engine import _tiny

pytestmark = pytest.mark.gpu
PROMPT = [7, 300, 12, 45, 99, 3]
CTX, KEEP, DISCARD = 32, 4, 14


@pytest.fixture(scope="module")
def tiny():
    e, oracle, cfg = _tiny(128, False, "fp16", seed=3, max_ctx=CTX)
    e.launch = "eager"
    return e, oracle, cfg


@pytest.fixture(scope="module")
def eng(tiny):
    return tiny[0]


def _run(e, k):
    """the prompt pass and k logits-only steps feeding the device's own argmax -> (tokens, logits of every step)"""
    e.clear_status()
    tokens, logits = [int(e.prefill(PROMPT, greedy=False)[0].argmax())], []
    for i in range(k):
        e.token.fill_(tokens[-1])
        e.pos.fill_(len(PROMPT) + i)
        e.step(greedy=False)
        logits.append(e.logits.cpu().numpy().copy())
        tokens.append(int(logits[-1].argmax()))
    return tokens, logits


def test_scores_do_not_change_the_step_and_sum_to_the_queries_seen(eng):
    k, G = 9, 2
    eng.set_fuse_attn(False)  # the separate-launch form, which an engine with H2O runs
    want = _run(eng, k)
    eng.set_h2o(True)
    eng.h2o_reset()
    got = _run(eng, k)
    total = eng.h2o_scores().sum(-1).cpu().numpy()
    eng.set_h2o(False)
    eng.set_fuse_attn(True)
    assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
    n = len(PROMPT) + k  # every query's probabilities sum to 1: G per query, fp32 summation error of n terms each
    print("score sums", total.tolist(), "expected", G * n)
    assert np.abs(total - G * n).max() <= G * n * n * 2.0 ** -23


def test_scores_are_the_oracles_attention_summed_over_queries_and_group(tiny):
    """The wiring (q un-rotated with its bias, the layer's score rows, the K row appended before the launch, every prompt
    chunk counted): the prompt in two chunks and 8 steps against the fp32 CPU oracle, whose attention calls are wrapped to
    add up their float64 probabilities (tests/h2o_reference.py). Bound: the engine's q and K lie within the prompt pass's
    1e-2 of the oracle's (the smoke bound; steps are tighter), so a logit is off by at most d = 2e-2 * max|logit| and a
    probability by the factor exp(2 d)."""
    eng, oracle, cfg = tiny
    layers = cfg["layers"]
    eng.clear_status()
    eng.set_h2o(True)
    eng.h2o_reset()
    oracle.reset()
    with H.ScoreBook(layers, cfg["heads"], cfg["kv_heads"], cfg["head_dim"], CTX) as book:
        eng.prefill(PROMPT[:4], start_pos=0, greedy=False)
        tok = int(eng.prefill(PROMPT[4:], start_pos=4, greedy=False)[0].argmax())
        oracle.forward_prompt(PROMPT[:4], 0)
        oracle.forward_prompt(PROMPT[4:], 4)
        for p in range(len(PROMPT), len(PROMPT) + 8):
            eng.token.fill_(tok)
            eng.pos.fill_(p)
            eng.step(greedy=False)
            oracle.forward_token(tok, p)
            tok = int(eng.logits.argmax())
    want = book.score
    got = eng.h2o_scores().cpu().numpy().astype(np.float64)
    eng.set_h2o(False)
    oracle.reset()
    n = len(PROMPT) + 8
    d = 2e-2 * book.logit
    rel = np.abs(got[..., :n] - want[..., :n]) / want[..., :n]
    print("largest logit %.3f, bound %.3e, worst relative score error %.3e, score spread %.2f .. %.2f"
          % (book.logit, np.expm1(2 * d), rel.max(), want[..., :n].min(), want[..., :n].max()))
    assert book.calls == layers * 10 and eng.status() == 0
    assert (rel <= np.expm1(2 * d)).all() and not got[..., n:].any()


def test_graphs_follow_h2o_being_switched_on_and_off(eng):
    """plain, H2O, H2O, plain back to back in graph mode: every request captures what it runs and equals its eager twin"""
    cfg = H2OConfig(CTX, KEEP, 7, recent=5)
    eng.launch = "eager"
    plain, h2o = eng.generate(PROMPT, 20), eng.generate(PROMPT, 50, streaming=cfg)
    eng.launch = "graph"
    try:
        assert eng.generate(PROMPT, 20) == plain
        assert eng.generate(PROMPT, 50, streaming=cfg) == h2o and not eng.captured
        assert eng.generate(PROMPT, 50, streaming=cfg) == h2o
        assert eng.generate(PROMPT, 20) == plain and eng.captured and eng.status() == 0
    finally:
        eng.launch = "eager"


def test_recent_that_leaves_only_the_oldest_rows_is_the_rolling_cache(eng):
    n_new = 60
    want = eng.generate(PROMPT, n_new, streaming=StreamingConfig(CTX, KEEP, DISCARD))
    got = eng.generate(PROMPT, n_new, streaming=H2OConfig(CTX, KEEP, DISCARD, recent=CTX - KEEP - DISCARD))
    assert got == want and eng.status() == 0 and not eng.h2o_installed
    caches = []
    eng.set_fuse_attn(False)  # one launch form for both runs
    for h2o in (False, True):  # the first eviction alone, on the same cache bytes
        eng.set_h2o(h2o)
        _run(eng, CTX - len(PROMPT))
        if h2o:
            eng.h2o_evict(KEEP, DISCARD, CTX - KEEP - DISCARD, CTX, move_pos=False)
        else:
            eng.kv_shift(KEEP, DISCARD, CTX, move_pos=False)
        caches.append([KR.bits_of(eng.kv_cache(w)[0])[:, :CTX - DISCARD] for w in "kv"])
    eng.set_h2o(False)
    eng.set_fuse_attn(True)
    assert np.array_equal(caches[0][0], caches[1][0]) and np.array_equal(caches[0][1], caches[1][1])


def test_general_recent_is_one_stream_in_every_launch_mode(eng, recent=5):
    cfg = H2OConfig(CTX, KEEP, 7, recent=recent)
    outs = []
    for launch, burst in [("graph", 16), ("graph", 5), ("eager", 16), ("eager", 5)]:
        eng.launch = launch
        outs.append(eng.generate(PROMPT, 70, burst=burst, streaming=cfg))
    eng.launch = "eager"
    assert all(o == outs[0] for o in outs) and len(outs[0]) == 70 and eng.status() == 0 and eng.discarded() == 0
    eng.set_h2o(True)
    eng.h2o_reset()
    _run(eng, CTX - len(PROMPT))
    v0 = KR.bits_of(eng.kv_cache("v")[0])
    eng.pos.fill_(CTX)
    eng.h2o_evict(KEEP, 7, recent, CTX)
    v1 = KR.bits_of(eng.kv_cache("v")[0])
    assert int(eng.pos.item()) == CTX - 7 and eng.discarded() == 7
    eng.set_discarded(0)
    eng.set_h2o(False)
    assert np.array_equal(v1[:, :KEEP], v0[:, :KEEP])                             # the sinks
    assert np.array_equal(v1[:, CTX - 7 - recent:CTX - 7], v0[:, CTX - recent:])  # the newest rows: every head's tail


def test_h2o_refuses_what_it_cannot_serve():
    e = _tiny(128, False, "fp16", seed=3, max_ctx=CTX, window=8)[0]
    with pytest.raises(RuntimeError, match="QBits:.*sliding window"):
        e.set_h2o(True)
    e = _tiny(128, False, "fp16", seed=3, max_ctx=CTX, max_batch=2)[0]
    with pytest.raises(RuntimeError, match="QBits:.*one sequence"):
        e.set_h2o(True)
    with pytest.raises(RuntimeError, match="QBits:"):
        e.h2o_evict(KEEP, 7, 5, CTX)  # not installed
