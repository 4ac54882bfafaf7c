"""The request drivers of runtime/request.py over a scripted engine that records its calls (no GPU): the chained driver
(`iter_generate`, `generate`) and the host-fed one (`iter_sampled`), and the pieces they share — the request scope, the
prompt pass, the `logprobs` check, the records and the eos cut."""
import re
from types import SimpleNamespace

import pytest
import torch

from intel_extension_for_transformers_amd.runtime import request
from intel_extension_for_transformers_amd.runtime.engine import WoqDecoderEngine
from intel_extension_for_transformers_amd.runtime.streaming import StreamingConfig, plan_steps, plan_stream

VOCAB, MAX_CTX, TOP = 50, 32, 20
PROMPT = [3, 1, 4, 1, 5, 9]
BURSTS = (1, 5, 7, 16)
# (max_new_tokens, streaming): the rolling cache (n_discard = (32 - 4) // 2 = 14), and the same shapes inside the cache
SHAPES = ((100, StreamingConfig(ctx_size=32, n_keep=4)), (20, None))
N_SHIFTS = 6  # of the rolling request: 99 steps from position 6, the cache is full after 26 of them, then after every 14
LOGITS = torch.randn(100, VOCAB, generator=torch.Generator().manual_seed(5))  # row i: the logits the i-th new token is picked from
SCRIPT = LOGITS.argmax(1).tolist()                                            # ... and the token itself


def _lp(i):
    """what the scripted engine records for the i-th new token: chosen, top ids, top log-probabilities"""
    return -0.25 * i, [(SCRIPT[i] + j) % VOCAB for j in range(TOP)], [-0.25 * i - j for j in range(TOP)]


class ScriptedEngine:
    """What the drivers use of a WoqDecoderEngine, on CPU tensors. The chaining tail (`prefill(greedy=True)`, `replay`)
    emits SCRIPT; `prefill(greedy=False)` and `step` leave LOGITS rows in `logits`. Every call lands in `calls`."""
    device = "cpu"
    _request_geometry = WoqDecoderEngine._request_geometry
    _check_shiftable = WoqDecoderEngine._check_shiftable

    def __init__(self, fail_after=None):
        self.cfg = SimpleNamespace(max_ctx=MAX_CTX, vocab=VOCAB)
        self.token, self.pos = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        self.logits = torch.zeros(VOCAB)
        self._log = torch.full((MAX_CTX + 1,), -1, dtype=torch.int32)
        self._lps = (torch.zeros(MAX_CTX + 1), torch.zeros(MAX_CTX + 1, TOP, dtype=torch.int32), torch.zeros(MAX_CTX + 1, TOP))
        self.sampler_installed = self.controls_installed = self.guide_installed = self.logprobs_on = False
        self.native_sampled_requests = 0
        self.calls, self.shifts = [], []
        self._i = 0  # new tokens emitted so far
        self._fail_after = fail_after  # replay / step calls that succeed before one raises

    def _emit(self, row):
        """the chaining tail: pick SCRIPT's next token, record it in row `row` of the logs"""
        self.token.fill_(SCRIPT[self._i])
        for log, value in zip(self._lps, _lp(self._i)):
            log[row] = torch.tensor(value)
        self._i += 1

    def _maybe_fail(self):
        if self._fail_after is not None:
            if self._fail_after == 0:
                raise RuntimeError("scripted failure")
            self._fail_after -= 1

    def prefill(self, tokens, start_pos=0, greedy=True):
        self.calls.append(("prefill", len(tokens), start_pos, greedy))
        self.pos.fill_(start_pos + len(tokens))
        self._i = 0
        self.logits.copy_(LOGITS[0])
        if greedy:
            self._emit(start_pos + len(tokens) - 1)

    def replay(self, k):
        self.calls.append(("burst", int(self.pos), k))
        self._maybe_fail()
        for _ in range(k):
            p = int(self.pos)
            assert p < MAX_CTX  # a step feeds a position inside the cache
            self._emit(p)
            self._log[p] = self.token[0]
            self.pos += 1

    def step(self, greedy=True):
        self.calls.append(("step", int(self.pos)))
        self._maybe_fail()
        assert not greedy and int(self.pos) < MAX_CTX
        self._i += 1
        self.logits.copy_(LOGITS[self._i])

    def kv_shift(self, n_keep, n_discard, n_cached, seq=0, move_pos=True):
        self.calls.append(("shift", n_cached))
        self.shifts.append((n_keep, n_discard, n_cached, move_pos))
        if move_pos:
            assert n_cached == int(self.pos)
            self.pos -= n_discard

    def set_logprobs(self, on=True):
        self.calls.append(("logprobs", on))
        self.logprobs_on = on

    def token_log(self):
        return self._log

    def logprob_log(self):
        return self._lps

    def __getattr__(self, name):  # the calls that only need recording
        if name in ("prepare_decode", "tune_attn_for", "set_discarded", "mark_seen", "mark_counts"):
            return lambda *a, **kw: self.calls.append((name,) + a + tuple(kw.values()))
        raise AttributeError(name)

    def plan(self):
        """the shifts and bursts / steps it ran, in `plan_stream`'s / `plan_steps`' form"""
        return [c for c in self.calls if c[0] in ("shift", "burst", "step")]

    def count(self, name):
        return sum(c[0] == name for c in self.calls)


def _argmax(logits, history, generated):
    return logits.argmax().reshape(1)


def _geometry(n_new, streaming):
    return (None, 0, 0) if streaming is None else streaming.resolve(MAX_CTX, len(PROMPT))


def _drivers(**kw):
    """both iterators over a fresh engine each, same request"""
    return [(e, f(e)) for e, f in ((ScriptedEngine(), lambda e: request.iter_generate(e, PROMPT, **kw)),
                                   (ScriptedEngine(), lambda e: request.iter_sampled(e, PROMPT, sampler=_argmax, **kw)))]


@pytest.mark.parametrize("burst", BURSTS)
@pytest.mark.parametrize("n_new,streaming", SHAPES)
def test_generate_is_the_concatenation_of_the_iterators_bursts_and_follows_the_plan(burst, n_new, streaming):
    a, b = ScriptedEngine(), ScriptedEngine()
    out = request.generate(a, PROMPT, n_new, burst=burst, streaming=streaming)
    bursts = list(request.iter_generate(b, PROMPT, n_new, burst=burst, streaming=streaming))
    assert out == sum(bursts, []) == SCRIPT[:n_new]
    assert a.calls == b.calls
    ctx, n_keep, n_discard = _geometry(n_new, streaming)
    plan = list(plan_stream(len(PROMPT), n_new, ctx, n_keep, n_discard, burst))
    assert b.plan() == plan  # ("burst", device position, k) and ("shift", n_cached), in order
    assert [len(x) for x in bursts] == [1] + [ev[2] for ev in plan if ev[0] == "burst"]
    assert b.shifts == [(n_keep, n_discard, ev[1], True) for ev in plan if ev[0] == "shift"]
    assert len(b.shifts) == (0 if streaming is None else N_SHIFTS)
    if streaming is None:
        assert b.count("set_discarded") == 0
    assert ("tune_attn_for", min(MAX_CTX, len(PROMPT) + n_new)) in b.calls


@pytest.mark.parametrize("burst", BURSTS)
@pytest.mark.parametrize("n_new,streaming", SHAPES)
def test_host_fed_driver_steps_once_per_token_and_sets_the_position_after_a_shift(burst, n_new, streaming):
    eng = ScriptedEngine()
    bursts = list(request.iter_sampled(eng, PROMPT, n_new, _argmax, burst=burst, streaming=streaming))
    assert sum(bursts, []) == SCRIPT[:n_new]
    assert [len(x) for x in bursts] == [min(burst, n_new - m) for m in range(0, n_new, burst)]
    if streaming is None:
        assert request.generate_sampled(ScriptedEngine(), PROMPT, n_new, _argmax, burst=burst) == SCRIPT[:n_new]
    assert eng.count("step") == n_new - 1 and eng.count("burst") == 0
    ctx, n_keep, n_discard = _geometry(n_new, streaming)
    # every step at the plan's cache position: the one after a shift at n_cached - n_discard, set by the host
    assert eng.plan() == list(plan_steps(plan_stream(len(PROMPT), n_new, ctx, n_keep, n_discard, burst)))
    for i, c in enumerate(eng.calls):
        if c[0] == "shift":
            assert eng.calls[i + 1] == ("step", c[1] - n_discard)
    assert eng.shifts == [(n_keep, n_discard, MAX_CTX, False)] * (0 if streaming is None else N_SHIFTS)
    assert all(c[3] is False for c in eng.calls if c[0] == "prefill")
    assert eng.count("set_discarded") == (0 if streaming is None else 2)


@pytest.mark.parametrize("n_new,streaming", SHAPES)
def test_records_of_both_drivers(n_new, streaming):
    n_top = 3
    toks, lps, top = request.generate(ScriptedEngine(), PROMPT, n_new, burst=7, logprobs=n_top, streaming=streaming)
    assert toks == SCRIPT[:n_new]
    for i in range(n_new):
        chosen, ids, vals = _lp(i)
        assert lps[i] == chosen and top[i] == list(zip(ids[:n_top], vals[:n_top]))
    eng = ScriptedEngine()
    got = list(request.iter_sampled(eng, PROMPT, n_new, _argmax, burst=7, logprobs=n_top, streaming=streaming))
    toks, lps, top = (sum((b[i] for b in got), []) for i in range(3))
    assert toks == SCRIPT[:n_new] and not eng.count("logprobs")
    for i in range(n_new):  # log_softmax / topk of the logits the token was picked from
        lsm = torch.log_softmax(LOGITS[i], -1)
        best = torch.topk(LOGITS[i], n_top).indices
        assert lps[i] == pytest.approx(float(lsm[SCRIPT[i]]), rel=1e-6)
        assert [t[0] for t in top[i]] == best.tolist()
        assert [t[1] for t in top[i]] == pytest.approx(lsm[best].tolist(), rel=1e-6)


def test_recording_is_on_for_the_call_and_back_afterwards():
    eng = ScriptedEngine()
    list(request.iter_generate(eng, PROMPT, 4, logprobs=0))
    assert [c for c in eng.calls if c[0] == "logprobs"] == [("logprobs", True), ("logprobs", False)]


@pytest.mark.parametrize("streaming", [s for _, s in SHAPES])
def test_eos_is_kept_stops_the_request_and_launches_no_further_burst(streaming):
    burst = 5
    # an id whose first occurrence lies inside a burst of either driver (the chained bursts hold new tokens 1-5, 6-10, ...,
    # the host-fed ones 0-4, 5-9, ...), with more tokens asked for
    first = next(i for i in range(7, 15) if SCRIPT[i] not in SCRIPT[:i] and i % burst in (2, 3))
    (chained, a), (host_fed, b) = _drivers(max_new_tokens=20, burst=burst, eos=[SCRIPT[first]], streaming=streaming)
    a, b = list(a), list(b)
    assert sum(a, []) == sum(b, []) == SCRIPT[:first + 1]
    # the bursts up to the one that holds the eos, whose steps past it ran and are dropped; nothing after it
    assert len(a) == 1 + -(-first // burst) and chained.count("burst") == -(-first // burst)
    assert len(b) == first // burst + 1 and host_fed.count("step") == burst * (first // burst + 1) - 1
    # the prompt pass's token is the eos (one token per burst: the host-fed driver's first burst is that token alone)
    for eng, it in _drivers(max_new_tokens=20, burst=1, eos=[SCRIPT[0]], streaming=streaming):
        assert list(it) == [[SCRIPT[0]]]
        assert not eng.plan() and not eng.count("prepare_decode")


def test_prepare_decode_only_when_more_than_one_token_is_asked_for():
    for n_new in (0, 1, 2, 20):
        eng = ScriptedEngine()
        assert request.generate(eng, PROMPT, n_new) == SCRIPT[:n_new]
        assert eng.count("prepare_decode") == (1 if n_new > 1 else 0)
        assert eng.count("burst") == (1 if n_new > 1 else 0) + (1 if n_new > 17 else 0)


def test_no_new_tokens_launches_the_prompt_pass_and_yields_nothing():
    for eng, it in _drivers(max_new_tokens=0):
        assert list(it) == []
        assert [c[0] for c in eng.calls] == ["prefill", "tune_attn_for"]


def test_which_chunks_end_on_the_chaining_tail():
    prompt = PROMPT[:5]

    def flags(eng, **kw):
        list(request.iter_generate(eng, prompt, 4, chunk=2, **kw))
        chunks = [c for c in eng.calls if c[0] == "prefill"]
        assert [c[1:3] for c in chunks] == [(2, 0), (2, 2), (1, 4)]
        return [c[3] for c in chunks]

    assert flags(ScriptedEngine()) == [True, True, True]
    assert flags(ScriptedEngine(), logprobs=2) == [False, False, True]
    sampled = ScriptedEngine()
    sampled.sampler_installed = True
    assert flags(sampled) == [False, False, True]
    assert sampled.calls[0] == ("mark_seen", prompt, True) and sampled.native_sampled_requests == 1
    eng = ScriptedEngine()
    list(request.iter_sampled(eng, prompt, 4, _argmax, chunk=2))
    assert [c[3] for c in eng.calls if c[0] == "prefill"] == [False, False, False]


def _discarded(eng):
    return [i for i, c in enumerate(eng.calls) if c == ("set_discarded", 0)]


@pytest.mark.parametrize("driver", (0, 1))
def test_a_streaming_request_zeroes_the_dropped_count_on_entry_and_however_it_ends(driver):
    kw = dict(max_new_tokens=100, burst=5, streaming=SHAPES[0][1])
    eng, it = _drivers(**kw)[driver]  # exhausted
    list(it)
    assert _discarded(eng) == [0, len(eng.calls) - 1] and eng.count("set_discarded") == 2
    eng, it = _drivers(**kw)[driver]  # closed after its first burst
    next(it)
    assert _discarded(eng) == [0]
    it.close()
    assert _discarded(eng) == [0, len(eng.calls) - 1]
    eng, it = _drivers(**kw)[driver]  # a launch raises
    eng._fail_after = 3
    with pytest.raises(RuntimeError, match="scripted failure"):
        list(it)
    assert _discarded(eng) == [0, len(eng.calls) - 1] and eng.calls[-2][0] in ("burst", "step")


@pytest.mark.parametrize("logprobs", (21, -1))
def test_a_logprobs_count_out_of_range_raises_before_anything_is_launched(logprobs):
    for streaming in (None, SHAPES[0][1]):
        for eng, it in _drivers(max_new_tokens=4, logprobs=logprobs, streaming=streaming):
            with pytest.raises(ValueError, match=re.escape("`logprobs` is a count of alternatives in [0, 20]")):
                list(it)
            assert eng.calls == []


def test_a_request_beyond_the_cache_without_streaming_raises_before_anything_is_launched():
    for eng, it in _drivers(max_new_tokens=100):
        with pytest.raises(RuntimeError, match=re.escape("prompt (6) + max_new_tokens (100) exceeds the engine's max_ctx (32)")):
            list(it)
        assert eng.calls == []
