"""The token tail with sampler controls (csrc/woq_sample.hip: `score_adjust_kernel` + `sample_kernel<true>`) alone, through
`woq_probe_sample_controls`, against tests/sampler_controls_reference.py.

* The pre-pass's adjusted scores (bias, repetition / frequency / presence penalty) are compared BIT FOR BIT with the numpy
  float32 restatement; the counts after a launch are the counts before plus one on the picked id; the picked id's seen
  bit is set and no other.
* Greedy picks are the reference's argmax, lowest id on ties.
* Sampled picks follow the acceptance rule of tests/test_gpu_sampler_kernel.py: token t is accepted iff u lies in
  [C_(t-1) - tol, C_t + tol] of the reference's float64 CDF, and every draw that is not within tol of a CDF boundary must
  equal the float64 pick. Candidate lists: tol = 8 * n_kept * 2^-24. Whole vocabulary: tol = 4 x the largest drift of the
  fp32 block-wise CDF (sampler_reference.hierarchical_cdf_f32) of the MASKED weights (0 below min_p) against float64 —
  that file's derivation with the weights the kernel sums here. Draws are chosen on the reference alone so that at most
  1 % need the tolerance.
* The min_p cut: a candidate is near when |exp(d) - min_p| <= (|d| + 4) * 2^-24 * min_p (sampler_controls_reference.
  min_p_nearness). Inputs are chosen on the reference alone (a seed search) so that no candidate lies within 100 x that
  margin; then the number of ids the kernel drew from (the probe's kept_out) must equal the reference's exactly.

Vocabularies: 1000 (fewer ids than the sampling workgroup has threads, a partial last seen word), 32000, 50257 (no
multiple of 32, 64, 256 or 1024: the pre-pass's last workgroup and the bit set's tail).
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import sampler_controls_reference as C
from tests import sampler_reference as R

pytestmark = pytest.mark.gpu

VOCABS = (1000, 32000, 50257)
N_DRAWS = 256
NEG_INF = float("-inf")


def _seen_words(vocab, ids):
    w = np.zeros((vocab + 31) // 32, dtype=np.uint32)
    ids = np.asarray(ids, dtype=np.int64)
    np.bitwise_or.at(w, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return w


def _inputs(vocab, seed, special=True):
    """logits = 4 * randn (with `special`: a few NaN, -inf and -0.0 among them); ~150 seen ids; counts in 1..40 on ~200
    ids; 300 bias entries: -inf, +0.0, -0.0 and random values, on seen ids, counted ids, -0.0 logits and at random; the
    last id of the vocabulary is seen, counted and biased."""
    rng = np.random.default_rng(seed)
    logits = (4 * rng.standard_normal(vocab)).astype(np.float32)
    ids = rng.permutation(vocab - 1)
    seen = np.concatenate([ids[:150], [vocab - 1]])
    counted = np.concatenate([ids[100:300], [vocab - 1]])  # 50 of them seen too
    counts = np.zeros(vocab, dtype=np.uint32)
    counts[counted] = rng.integers(1, 41, counted.size).astype(np.uint32)
    counts[counted[:3]] = 40
    biased = np.concatenate([ids[140:160], ids[290:310], ids[400:659], [vocab - 1]])
    assert biased.size == 300 and np.unique(biased).size == 300
    vals = (3 * rng.standard_normal(300)).astype(np.float32)
    vals[:4] = [NEG_INF, 0.0, -0.0, NEG_INF]      # on seen ids
    vals[20:24] = [NEG_INF, 0.0, -0.0, 7.5]       # on counted ids
    vals[40:46] = [NEG_INF, 0.0, -0.0, 0.0, -0.0, NEG_INF]
    if special:
        logits[ids[700:706]] = np.nan
        logits[ids[706:720]] = NEG_INF
        logits[ids[720:724]] = -0.0               # no bias entry: must stay -0.0
        logits[biased[41:43]] = -0.0              # -0.0 + (+0.0) = +0.0, -0.0 + (-0.0) = -0.0
        logits[biased[43]] = np.nan
        logits[biased[44]] = NEG_INF
    bias = {int(i): float(v) for i, v in zip(biased, vals)}
    return logits, seen, counts, bias


def _run(logits, words, counts, cfg, controls, us, pos=0):
    """one probe call per uniform, each on its own copy of the bit set and the counts -> tokens, bit sets, counts,
    adjusted scores, kept counts, status"""
    dev, n, vocab = "cuda", len(us), logits.size
    lg = torch.from_numpy(logits).to(dev)
    seen = torch.from_numpy(words.view(np.int32)).to(dev).repeat(n, 1).contiguous()
    cnt = torch.from_numpy(counts.view(np.int32)).to(dev).repeat(n, 1).contiguous()
    u = torch.tensor(us, dtype=torch.float32, device=dev)
    tok = torch.full((n,), -1, dtype=torch.int32, device=dev)
    kept = torch.full((n,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    adj = torch.zeros(n, vocab, dtype=torch.float32, device=dev)
    p = torch.tensor([pos], dtype=torch.int32, device=dev)
    for j in range(n):
        L.probe_sample_controls(lg, seen[j], cnt[j], cfg, controls, p, tok[j:j + 1], adj[j], u=u[j:j + 1],
                                status=status[j:j + 1], kept_out=kept[j:j + 1])
    torch.cuda.synchronize()
    return (tok.cpu().numpy(), seen.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32), adj.cpu().numpy(),
            kept.cpu().numpy(), status.cpu().numpy())


def _check_side_effects(tokens, seen_after, words, counts_after, counts):
    for j, t in enumerate(tokens):
        want = words.copy()
        want[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
        assert np.array_equal(seen_after[j], want), (j, t)
        cw = counts.copy()
        cw[t] += 1
        assert np.array_equal(counts_after[j], cw), (j, t)


def _uniforms(seed, near):
    """N_DRAWS uniforms on the kernel's grid: 0, 1 - 2^-24, the rest random multiples of 2^-24, at most 1 % of them
    within tol of a CDF boundary (chosen on the reference alone, as tests/test_gpu_sampler_kernel.py does)."""
    rng = np.random.default_rng(seed)
    us = [0.0, 1.0 - R.TWO_M24]
    budget = N_DRAWS // 100 - sum(bool(near(u)) for u in us)
    while len(us) < N_DRAWS:
        u = float(rng.integers(0, 1 << 24)) * R.TWO_M24
        if near(u):
            if budget <= 0:
                continue
            budget -= 1
        us.append(u)
    return np.array(us)


PENALTIES = {
    "positive": dict(repetition_penalty=1.3, presence_penalty=0.7, frequency_penalty=0.35),
    "negative": dict(repetition_penalty=0.8, presence_penalty=-1.25, frequency_penalty=-0.15),
    "no_repetition": dict(repetition_penalty=1.0, presence_penalty=2.0, frequency_penalty=2.0),
}


@pytest.mark.parametrize("vocab", VOCABS)
def test_adjusted_scores_are_bit_equal_and_greedy_picks_the_reference_argmax(vocab):
    for pi, (name, pk) in enumerate(PENALTIES.items()):
        logits, seen, counts, bias = _inputs(vocab, seed=vocab + pi)
        words = _seen_words(vocab, seen)
        cfg = L.sampler_config(do_sample=False, repetition_penalty=pk["repetition_penalty"])
        ctl = L.sampler_controls(pk["presence_penalty"], pk["frequency_penalty"], 0.0, bias)
        want = C.adjusted_f32(logits, seen, counts, pk["repetition_penalty"], pk["presence_penalty"],
                              pk["frequency_penalty"], bias)
        tokens, seen_after, counts_after, adj, _kept, status = _run(logits, words, counts, cfg, ctl, [0.0])
        assert C.same_bits(adj[0], want), (name, vocab, np.flatnonzero(adj[0].view(np.uint32) != want.view(np.uint32))[:8])
        # the sentinel: -0.0 without an entry stays -0.0
        zero_ids = [i for i in np.flatnonzero((logits == 0) & np.signbit(logits)) if int(i) not in bias
                    and counts[i] == 0 and i not in set(seen.tolist())]
        assert zero_ids and all(np.signbit(adj[0][i]) for i in zero_ids)
        assert not status.any()
        best = int(np.flatnonzero(want == np.nanmax(want))[0])
        assert tokens.tolist() == [best], (name, vocab)
        _check_side_effects(tokens, seen_after, words, counts_after, counts)
        # the same scores with sampling on: the pre-pass does not depend on the draw's settings
        cfg = L.sampler_config(do_sample=True, temperature=0.7, top_k=5, top_p=1.0,
                               repetition_penalty=pk["repetition_penalty"])
        _t, _s, _c, adj, _k, status = _run(logits, words, counts, cfg, ctl, [0.5])
        assert C.same_bits(adj[0], want) and not status.any()


@pytest.mark.parametrize("vocab", VOCABS)
def test_greedy_winner_changed_by_penalties_banned_by_bias_and_lowest_id_on_ties(vocab):
    rng = np.random.default_rng(vocab)
    logits = rng.standard_normal(vocab).astype(np.float32)
    a, b, c = sorted(int(i) for i in rng.choice(vocab, 3, replace=False))
    logits[a], logits[b], logits[c] = 9.0, 9.0, 12.0  # c is the raw argmax; a and b tie behind it
    cfg = L.sampler_config(do_sample=False)
    words = _seen_words(vocab, [])
    # the frequency penalty takes the winner down: generated 4 times at 1.0 -> 8.0 < 9.0
    counts = np.zeros(vocab, dtype=np.uint32)
    counts[c] = 4
    want = C.adjusted_f32(logits, [], counts, 1.0, 0.0, 1.0, None)
    assert int(np.argmax(logits)) == c and int(np.flatnonzero(want == want.max())[0]) == a
    tokens, seen_after, counts_after, adj, _k, status = _run(logits, words, counts, cfg,
                                                             L.sampler_controls(0.0, 1.0, 0.0, None), [0.0])
    assert tokens.tolist() == [a] and C.same_bits(adj[0], want) and not status.any()
    _check_side_effects(tokens, seen_after, words, counts_after, counts)
    # a -inf bias bans the raw argmax; of the two tied ids the lower wins
    zero = np.zeros(vocab, dtype=np.uint32)
    want = C.adjusted_f32(logits, [], zero, 1.0, 0.0, 0.0, {c: NEG_INF})
    tokens, seen_after, counts_after, adj, _k, status = _run(logits, words, zero, cfg,
                                                             L.sampler_controls(0.0, 0.0, 0.0, {c: NEG_INF}), [0.0])
    assert tokens.tolist() == [a] and C.same_bits(adj[0], want) and adj[0][c] == NEG_INF and not status.any()
    _check_side_effects(tokens, seen_after, words, counts_after, zero)
    # a positive bias makes a new winner
    d = (a + 1) % vocab if (a + 1) % vocab not in (b, c) else (a + 2) % vocab
    tokens = _run(logits, words, zero, cfg, L.sampler_controls(0.0, 0.0, 0.0, {d: 50.0}), [0.0])[0]
    assert tokens.tolist() == [d]


SAMPLED = {
    "k40_p0.9": dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.9, repetition_penalty=1.1),
    "whole_vocab": dict(do_sample=True, temperature=0.8, top_k=0, top_p=1.0, repetition_penalty=1.1),
}
CONTROLS = dict(presence_penalty=0.4, frequency_penalty=0.1)


def _sampled_case(vocab, name, min_p, with_bias):
    """inputs (a seed search on the reference alone) whose min_p cut and nucleus boundary are both far from any
    candidate -> logits, seen, counts, bias, scores, reference choice"""
    kw = SAMPLED[name]
    for attempt in range(50):
        logits, seen, counts, bias = _inputs(vocab, seed=7919 * attempt + vocab + int(1000 * min_p) + len(name),
                                             special=with_bias)
        bias = bias if with_bias else None
        s = C.scores_f32(logits, seen, counts, kw["repetition_penalty"], kw["temperature"], True,
                         CONTROLS["presence_penalty"], CONTROLS["frequency_penalty"], bias)
        ref = C.choose(s, kw["top_k"], kw["top_p"], min_p)
        far_cut = ref.min_p_units >= 100.0
        far_nucleus = kw["top_k"] <= 0 or ref.boundary_margin >= 100 * 8 * ref.n_candidates * R.TWO_M24
        if far_cut and far_nucleus:
            return logits, seen, counts, bias, s, ref
    raise AssertionError("no input with every candidate 100 margins away from the cuts")


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("min_p", (0.0, 0.05, 0.5, 1.0))
@pytest.mark.parametrize("name", list(SAMPLED))
def test_sampled_picks_and_the_min_p_cut(name, min_p, vocab):
    kw = SAMPLED[name]
    with_bias = min_p in (0.0, 0.05)  # 300 bias entries, NaN and -inf logits on two of the four cuts
    logits, seen, counts, bias, s, ref = _sampled_case(vocab, name, min_p, with_bias)
    assert ref.min_p_units >= 100.0
    words = _seen_words(vocab, seen)
    cfg = L.sampler_config(seed=3, **kw)
    ctl = L.sampler_controls(CONTROLS["presence_penalty"], CONTROLS["frequency_penalty"], min_p, bias)
    if kw["top_k"] > 0:
        tol = 8 * ref.n_kept * R.TWO_M24
    else:
        d = s[ref.ids].astype(np.float64) - float(np.max(s[ref.ids]))
        w32 = np.where(d == 0.0, 1.0, np.exp(d))
        w32 = np.where(w32 >= float(np.float32(min_p)), w32, 0.0).astype(np.float32)
        c32 = R.hierarchical_cdf_f32(w32).astype(np.float64)
        drift = float(np.max(np.abs(c32 / c32[-1] - ref.cdf)))
        tol = 4 * drift
        print("whole vocabulary %d min_p %g: ids with mass %d, fp32 CDF drift %.3e, tol %.3e" %
              (vocab, min_p, ref.n_mass, drift, tol))
        assert 0 <= tol < 1e-5
    us = _uniforms(vocab + int(100 * min_p), near=lambda u: ref.needs_tolerance(u, tol))
    tokens, seen_after, counts_after, adj, kept, status = _run(logits, words, counts, cfg, ctl, us)
    assert not status.any(), status[status != 0][:4]
    want = C.adjusted_f32(logits, seen, counts, kw["repetition_penalty"], CONTROLS["presence_penalty"],
                          CONTROLS["frequency_penalty"], bias)
    assert C.same_bits(adj[0], want) and C.same_bits(adj[-1], want)
    _check_side_effects(tokens, seen_after, words, counts_after, counts)
    if min_p > 0.0:  # the cut itself: the drawn-from set has exactly the reference's size
        assert (kept == ref.n_mass).all(), (name, min_p, vocab, sorted(set(kept.tolist())), ref.n_mass)
    elif kw["top_k"] > 0:
        assert (kept == ref.n_kept).all(), (name, vocab, sorted(set(kept.tolist())), ref.n_kept)
    assert sum(ref.needs_tolerance(u, tol) for u in us) <= N_DRAWS // 100
    exact = 0
    for u, t in zip(us, tokens):
        assert ref.accepts(int(t), u, tol), (name, min_p, vocab, u, int(t), ref.pick(u))
        if not ref.needs_tolerance(u, tol):
            assert int(t) == ref.pick(u), (name, min_p, vocab, u, int(t), ref.pick(u))
            exact += 1
    print("%s min_p %g vocab %d: candidates %d, kept %d, min_p distance %.3g margins, distinct picks %d, exact %d / %d" %
          (name, min_p, vocab, ref.n_candidates, ref.n_mass, ref.min_p_units, len(set(tokens.tolist())), exact, N_DRAWS))
    if min_p == 1.0:  # only scores equal to the best survive
        assert ref.n_mass == 1 and len(set(tokens.tolist())) == 1


def test_refused_configurations_launch_nothing():
    vocab = 2000
    logits, seen, counts, _bias = _inputs(vocab, seed=1)
    lg = torch.from_numpy(logits).cuda()
    words = torch.from_numpy(_seen_words(vocab, seen).view(np.int32)).cuda()
    cnt = torch.from_numpy(counts.view(np.int32)).cuda()
    tok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    adj = torch.full((vocab,), 123.0, dtype=torch.float32, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    sampled = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.9)
    nan, inf = float("nan"), float("inf")
    refused = [
        (sampled, dict(logit_bias={vocab: 1.0})),
        (sampled, dict(logit_bias={-1: 1.0})),
        (sampled, dict(min_p=1.5)),
        (sampled, dict(min_p=-0.1)),
        (sampled, dict(min_p=nan)),
        (dict(do_sample=False), dict(min_p=0.1)),
        (sampled, dict(presence_penalty=inf)),
        (sampled, dict(frequency_penalty=nan)),
        (sampled, dict(logit_bias={3: inf})),
        (sampled, dict(logit_bias={3: nan})),
        (dict(do_sample=True, top_k=0, top_p=0.9), dict(min_p=0.1)),   # a nucleus over the whole vocabulary: as before
        (dict(do_sample=True, top_k=2000), dict(presence_penalty=0.5)),
    ]
    for kw, ck in refused:
        with pytest.raises(RuntimeError, match="QBits:"):
            L.probe_sample_controls(lg, words, cnt, L.sampler_config(**kw), L.sampler_controls(**ck), pos, tok, adj)
    # duplicate ids and more than 1024 entries cannot be written as a dict: build the arrays by hand
    import ctypes

    def raw(ids, vals):
        n = len(ids)
        return (L.SamplerControls(n_bias=n), (ctypes.c_int32 * n)(*ids), (ctypes.c_float * n)(*vals))

    for controls in (raw([5, 9, 5], [1.0, 2.0, 3.0]), raw(list(range(1025)), [0.5] * 1025)):
        with pytest.raises(RuntimeError, match="QBits:"):
            L.probe_sample_controls(lg, words, cnt, L.sampler_config(**sampled), controls, pos, tok, adj)
    torch.cuda.synchronize()
    assert tok.tolist() == [-1] and bool((adj == 123.0).all())
    assert np.array_equal(cnt.cpu().numpy().view(np.uint32), counts)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), _seen_words(vocab, seen))
