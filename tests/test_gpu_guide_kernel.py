"""The token tail with a token guide (csrc/woq_sample.hip: `score_adjust_kernel<true>` + `sample_kernel<true>` +
`guide_advance_kernel`) alone, through `woq_probe_guide`, against tests/guide_reference.py on top of
tests/sampler_controls_reference.py.

* The adjusted scores are compared BIT FOR BIT (uint32 views) with the reference: steps 1-4 of the controls' contract,
  then -inf where the state's row bans the id. The token and the state after the advance are equal.
* Greedy picks are the reference's argmax over the masked scores, lowest id on ties.
* Sampled picks follow the acceptance rule of tests/test_gpu_sampler_kernel.py for candidate lists: token t is accepted
  iff u lies in [C_(t-1) - tol, C_t + tol] of the reference's float64 CDF, tol = 8 * n_kept * 2^-24, and a draw that is
  not within tol of a CDF boundary must equal the float64 pick.

Vocabularies 1, 255, 256, 257, 32000 and 128256: the edges of the 256-thread pre-pass. States: tables of 1 and 3 states,
the last state of a 65535-state table, and state 40000 of a 128256-id table, whose row starts beyond 2^32 elements.
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import guide_reference as G
from tests import sampler_controls_reference as C
from tests import sampler_reference as R

pytestmark = pytest.mark.gpu

VOCABS = (1, 255, 256, 257, 32000, 128256)
NEG_INF = float("-inf")
SAMPLED = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.9)
ALL_ON = dict(repetition_penalty=1.3, presence_penalty=0.7, frequency_penalty=0.35)
NEUTRAL = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)


def _seen_words(vocab, ids):
    w = np.zeros((vocab + 31) // 32, dtype=np.uint32)
    ids = np.asarray(ids, dtype=np.int64)
    np.bitwise_or.at(w, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return w


def _inputs(vocab, seed, controls_on):
    """logits = 4 * randn with a NaN, a -inf and a -0.0 among them where the vocabulary has room; with `controls_on`
    about a tenth of the ids seen, a tenth counted (1..40 times) and up to 300 bias entries (-inf, +-0.0, random); the
    last id is seen, counted and biased."""
    rng = np.random.default_rng(seed)
    logits = (4 * rng.standard_normal(vocab)).astype(np.float32)
    ids = rng.permutation(vocab)
    if vocab >= 255:
        logits[ids[0]], logits[ids[1]], logits[ids[2]] = np.nan, NEG_INF, -0.0
    counts = np.zeros(vocab, dtype=np.uint32)
    if not controls_on:
        return logits, np.zeros(0, np.int64), counts, None
    n = max(1, vocab // 10)
    seen = np.unique(np.concatenate([ids[:n], [vocab - 1]]))
    counted = np.unique(np.concatenate([ids[n // 2:n // 2 + n], [vocab - 1]]))
    counts[counted] = rng.integers(1, 41, counted.size).astype(np.uint32)
    biased = np.unique(np.concatenate([ids[:min(299, vocab // 2)], [vocab - 1]]))
    vals = (3 * rng.standard_normal(biased.size)).astype(np.float32)
    vals[:4] = [7.5, NEG_INF, 0.0, -0.0][:min(4, vals.size)]
    return logits, seen, counts, {int(i): float(v) for i, v in zip(biased, vals)}


def _run(logits, seen, counts, cfg, controls, table, state, us=(0.0,), advance_state=-1):
    """one probe call per uniform, each on its own copy of the bit set and the counts; `table` a device tensor ->
    tokens, adjusted scores of the first call, states after the advance, status words"""
    dev, n, vocab = "cuda", len(us), logits.size
    lg = torch.from_numpy(logits).to(dev)
    words = torch.from_numpy(_seen_words(vocab, seen).view(np.int32)).to(dev).repeat(n, 1).contiguous()
    cnt = torch.from_numpy(counts.view(np.int32)).to(dev).repeat(n, 1).contiguous()
    u = torch.tensor(list(us), dtype=torch.float32, device=dev)
    tok = torch.full((n,), -1, dtype=torch.int32, device=dev)
    out_state = torch.full((n,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    adj = torch.zeros(vocab, dtype=torch.float32, device=dev)
    p = torch.zeros(1, dtype=torch.int32, device=dev)
    for j in range(n):
        L.probe_guide(lg, words[j], cnt[j], cfg, controls, table, state, p, tok[j:j + 1], adj, out_state[j:j + 1],
                      advance_state=advance_state, u=u[j:j + 1], status=status[j:j + 1])
    torch.cuda.synchronize()
    return tok.cpu().numpy(), adj.cpu().numpy(), out_state.cpu().numpy(), status.cpu().numpy()


def _device_table(t):
    return torch.from_numpy(t.view(np.int16)).cuda()


def _check_greedy(logits, seen, counts, bias, pk, table_dev, row, next_of, state):
    """greedy probe at `state` whose row is `row` (numpy uint16 [vocab]); next_of(token) = the expected next state"""
    cfg = L.sampler_config(do_sample=False, repetition_penalty=pk["repetition_penalty"])
    ctl = L.sampler_controls(pk["presence_penalty"], pk["frequency_penalty"], 0.0, bias)
    want = G.masked_f32(C.adjusted_f32(logits, seen, counts, pk["repetition_penalty"], pk["presence_penalty"],
                                       pk["frequency_penalty"], bias), row)
    tokens, adj, states, status = _run(logits, seen, counts, cfg, ctl, table_dev, state)
    assert np.array_equal(np.isnan(adj), np.isnan(want))
    assert C.same_bits(adj, want), np.flatnonzero(adj.view(np.uint32) != want.view(np.uint32))[:8]
    best = int(np.flatnonzero(want == np.nanmax(want))[0])
    assert row[best] != G.BANNED  # the inputs leave a finite allowed score
    assert tokens.tolist() == [best] and states.tolist() == [next_of(best)] and not status.any()
    return want


def _sampled_reference(logits, seen, counts, bias, pk, row):
    """-> (masked adjusted scores, the float64 choice over them, whether the nucleus boundary is 100 tolerances away
    from every candidate: the condition tests/test_gpu_sampler_controls_kernel.py puts on its inputs)"""
    want = G.masked_f32(C.adjusted_f32(logits, seen, counts, pk["repetition_penalty"], pk["presence_penalty"],
                                       pk["frequency_penalty"], bias), row)
    ref = C.choose(R.scores_f32(want, [], 1.0, SAMPLED["temperature"], True), SAMPLED["top_k"], SAMPLED["top_p"], 0.0)
    return want, ref, ref.boundary_margin >= 100 * 8 * ref.n_candidates * R.TWO_M24


def _case(vocab, seed, controls_on, pk, row):
    """inputs, chosen on the reference alone (a seed search), with a finite allowed score and a far nucleus boundary"""
    for attempt in range(50):
        logits, seen, counts, bias = _inputs(vocab, seed + 7919 * attempt, controls_on)
        first = int(np.flatnonzero(row != G.BANNED)[0])
        logits[first] = logits[first] if np.isfinite(logits[first]) else 0.25
        if bias and bias.get(first) == NEG_INF:
            bias[first] = 1.0
        if _sampled_reference(logits, seen, counts, bias, pk, row)[2]:
            return logits, seen, counts, bias
    raise AssertionError("no input with the nucleus boundary 100 tolerances away from every candidate")


def _check_sampled(logits, seen, counts, bias, pk, table_dev, row, next_of, state, seed):
    cfg = L.sampler_config(seed=3, repetition_penalty=pk["repetition_penalty"], **SAMPLED)
    ctl = L.sampler_controls(pk["presence_penalty"], pk["frequency_penalty"], 0.0, bias)
    want, ref, far = _sampled_reference(logits, seen, counts, bias, pk, row)
    assert far
    tol = 8 * ref.n_kept * R.TWO_M24
    rng = np.random.default_rng(seed)
    us = [0.0, 1.0 - R.TWO_M24] + [float(rng.integers(0, 1 << 24)) * R.TWO_M24 for _ in range(14)]
    tokens, adj, states, status = _run(logits, seen, counts, cfg, ctl, table_dev, state, us)
    assert C.same_bits(adj, want) and not status.any()
    for u, t, st in zip(us, tokens, states):
        assert row[t] != G.BANNED, (u, int(t))
        assert ref.accepts(int(t), u, tol), (u, int(t), ref.pick(u))
        if not ref.needs_tolerance(u, tol):
            assert int(t) == ref.pick(u), (u, int(t), ref.pick(u))
        assert int(st) == next_of(int(t))


@pytest.mark.parametrize("n_states", (1, 3))
@pytest.mark.parametrize("vocab", VOCABS)
def test_masked_scores_token_and_next_state_match_the_reference(vocab, n_states):
    rng = np.random.default_rng(1000 * n_states + vocab)
    table = G.random_table(rng, n_states, vocab)
    table_dev = _device_table(table)
    state = n_states - 1
    for name, pk in (("all_on", ALL_ON), ("neutral", NEUTRAL)):
        logits, seen, counts, bias = _case(vocab, vocab + n_states + len(name), name == "all_on", pk, table[state])
        next_of = lambda t: int(table[state, t])  # noqa: E731
        _check_greedy(logits, seen, counts, bias, pk, table_dev, table[state], next_of, state)
        _check_sampled(logits, seen, counts, bias, pk, table_dev, table[state], next_of, state, seed=vocab)


def test_banned_best_logit_banned_positive_bias_and_a_single_allowed_id():
    vocab = 32000
    rng = np.random.default_rng(7)
    logits = rng.standard_normal(vocab).astype(np.float32)
    a, b, c, d = sorted(int(i) for i in rng.choice(vocab, 4, replace=False))
    logits[a], logits[b], logits[c] = 9.0, 9.0, 12.0  # c the raw argmax; a and b tie behind it
    table = np.zeros((3, vocab), np.uint16)
    table[0, :] = 1
    table[0, c] = G.BANNED  # state 0 bans the largest logit
    table[0, d] = G.BANNED  # ... and an id that a bias of +50 would make the winner
    table[1, :] = G.BANNED
    table[1, d] = 2         # state 1 allows exactly one id
    table[2, :] = 0
    table_dev = _device_table(table)
    zero = np.zeros(vocab, np.uint32)
    none = np.zeros(0, np.int64)
    greedy = L.sampler_config(do_sample=False)
    want = G.masked_f32(C.adjusted_f32(logits, none, zero, 1.0, 0.0, 0.0, {d: 50.0}), table[0])
    tokens, adj, states, status = _run(logits, none, zero, greedy, L.sampler_controls(0.0, 0.0, 0.0, {d: 50.0}), table_dev, 0)
    assert C.same_bits(adj, want) and adj[c] == NEG_INF and adj[d] == NEG_INF
    assert tokens.tolist() == [a] and states.tolist() == [1] and not status.any()
    # one candidate: greedy and every draw take it (the reference's one-candidate case)
    want = G.masked_f32(logits, table[1])
    ref = C.choose(R.scores_f32(want, [], 1.0, SAMPLED["temperature"], True), SAMPLED["top_k"], SAMPLED["top_p"], 0.0)
    assert ref.n_kept == 1 and ref.pick(0.5) == d
    tokens, adj, states, status = _run(logits, none, zero, greedy, L.sampler_controls(), table_dev, 1)
    assert C.same_bits(adj, want) and tokens.tolist() == [d] and states.tolist() == [2] and not status.any()
    tokens, adj, states, status = _run(logits, none, zero, L.sampler_config(seed=1, **SAMPLED), L.sampler_controls(),
                                       table_dev, 1, us=(0.0, 0.37, 1.0 - R.TWO_M24))
    assert C.same_bits(adj, want) and tokens.tolist() == [d] * 3 and states.tolist() == [2] * 3 and not status.any()
    # whole-vocabulary sampling over one allowed id
    whole = L.sampler_config(seed=1, do_sample=True, temperature=0.8, top_k=0, top_p=1.0)
    tokens, _adj, states, status = _run(logits, none, zero, whole, L.sampler_controls(), table_dev, 1, us=(0.0, 0.99))
    assert tokens.tolist() == [d] * 2 and states.tolist() == [2] * 2 and not status.any()


def test_a_pick_the_advances_row_bans_keeps_the_state_and_raises_status_bit_4():
    """The mask comes from state 0, the advance is handed state 1, whose row bans the pick: only the probe can do that."""
    vocab = 257
    logits = np.linspace(-1.0, 1.0, vocab).astype(np.float32)  # the argmax is the last id
    table = np.zeros((2, vocab), np.uint16)
    table[0, :] = 1
    table[1, :] = 0
    table[1, vocab - 1] = G.BANNED
    zero, none = np.zeros(vocab, np.uint32), np.zeros(0, np.int64)
    tokens, _adj, states, status = _run(logits, none, zero, L.sampler_config(do_sample=False), L.sampler_controls(),
                                       _device_table(table), 0, advance_state=1)
    assert tokens.tolist() == [vocab - 1]
    assert (states.tolist(), status.tolist()) == ([1], [L.STATUS_GUIDE_BANNED_PICK])
    assert G.advance(table, 1, vocab - 1) == (1, 16)
    # the same probe with an allowed pick: the advance starts from the state it is handed
    table[1, vocab - 1] = 0
    tokens, _adj, states, status = _run(logits, none, zero, L.sampler_config(do_sample=False), L.sampler_controls(),
                                       _device_table(table), 0, advance_state=1)
    assert (tokens.tolist(), states.tolist(), status.tolist()) == ([vocab - 1], [0], [0])


def _sparse_table_case(vocab, n_states, state, seed):
    """a table from an uninitialised allocation in which only row `state` is written"""
    rng = np.random.default_rng(seed)
    row = rng.integers(0, n_states, vocab).astype(np.uint16)
    row[rng.random(vocab) < 0.5] = G.BANNED
    row[0] = n_states - 1
    table_dev = torch.empty((n_states, vocab), dtype=torch.int16, device="cuda")
    table_dev[state] = torch.from_numpy(row.view(np.int16)).cuda()
    logits, seen, counts, bias = _case(vocab, seed, True, ALL_ON, row)
    next_of = lambda t: int(row[t])  # noqa: E731
    _check_greedy(logits, seen, counts, bias, ALL_ON, table_dev, row, next_of, state)
    _check_sampled(logits, seen, counts, bias, ALL_ON, table_dev, row, next_of, state, seed=seed)


def test_last_state_of_a_65535_state_table():
    _sparse_table_case(257, 65535, 65534, seed=11)


def test_row_offset_beyond_2_to_the_32_elements():
    vocab, state = 128256, 40000
    assert state * vocab > 1 << 32
    free, _total = torch.cuda.mem_get_info()
    if free < 12 * (1 << 30):
        pytest.skip("needs 12 GB of free device memory for the table")
    _sparse_table_case(vocab, state + 1, state, seed=13)


def test_refused_probe_arguments_launch_nothing():
    vocab = 300
    lg = torch.zeros(vocab, device="cuda")
    words = torch.zeros((vocab + 31) // 32, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(vocab, dtype=torch.int32, device="cuda")
    tok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    adj = torch.full((vocab,), 123.0, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    table = torch.zeros((2, vocab), dtype=torch.int16, device="cuda")
    for state, adv in ((2, -1), (-1, -1), (0, 2)):
        with pytest.raises(RuntimeError, match="QBits:"):
            L.probe_guide(lg, words, cnt, L.sampler_config(), L.sampler_controls(), table, state, pos, tok, adj, st,
                          advance_state=adv)
    torch.cuda.synchronize()
    assert tok.tolist() == [-1] and st.tolist() == [-1] and bool((adj == 123.0).all())
