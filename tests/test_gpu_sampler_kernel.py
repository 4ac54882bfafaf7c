"""`sample_kernel` (csrc/woq_sample.hip) alone, through `woq_probe_sample`, against tests/sampler_reference.py.

Scores: the reference applies the kernel's two IEEE single operations in numpy, so the top-k kept set is pure comparisons
and must match exactly; ordering, nucleus and CDF run in float64. Every setting gets 256 explicit uniforms per input
(0, 1 - 2^-24, the rest random multiples of 2^-24). Token t is accepted iff u lies in [C_(t-1) - tol, C_t + tol] of the
reference's normalised CDF.

* candidate-list settings: tol = 8 * n_kept * 2^-24 (n fp32 additions of terms <= 1 plus ~2 ulp per expf, doubled for the
  normalisation), n_kept = the candidates the nucleus leaves.
* whole vocabulary (top_k = 0, top_p = 1, T = 0.8): tol = 4 x the largest drift of an fp32 block-wise restatement of the
  CDF (sampler_reference.hierarchical_cdf_f32) against float64 on this file's own inputs, x 4 because the kernel's
  summation order differs. Measured on these inputs (CPU, numpy): drift 3.9e-7 .. 7.9e-7 over the six inputs, tol 1.6e-6 .. 3.2e-6;
  the test recomputes both and prints them.

Draws are chosen on the reference alone (`_uniforms`) so that the second precondition holds even where CDF boundaries
lie dense. Preconditions, asserted on the reference alone: the nucleus boundary is at least 100 * (8 * n_candidates * 2^-24) away
from 1 - top_p; at most 1 % of a case's draws lie within tol of a CDF boundary — every other draw must equal the float64
pick exactly. After each call: the picked token's bit is set, no other bit changed, status 0.
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import sampler_reference as R

pytestmark = pytest.mark.gpu

N_DRAWS = 256
VOCABS = (32000, 50257, 128256)
SETTINGS = {
    "neuralchat_default": dict(do_sample=True, temperature=0.1, top_k=40, top_p=0.75, repetition_penalty=1.1),
    "t0.9_k8_p0.95": dict(do_sample=True, temperature=0.9, top_k=8, top_p=0.95, repetition_penalty=1.1),
    "k1": dict(do_sample=True, temperature=0.7, top_k=1, top_p=1.0, repetition_penalty=1.3),
    # top_p = 1: with 1024 candidates no nucleus boundary can keep 100 * tol = 0.05 of distance from its neighbours
    "k1024": dict(do_sample=True, temperature=1.5, top_k=1024, top_p=1.0, repetition_penalty=1.1),
    "penalty_argmax": dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.3),
    "whole_vocab": dict(do_sample=True, temperature=0.8, top_k=0, top_p=1.0, repetition_penalty=1.1),
}


def _inputs(vocab, kw, variant, seed):
    """logits = 4 * randn; seen ids among the largest (positive) and the smallest finite (negative) logits and at random;
    variant "neginf": a tenth of the entries -inf; "tie": a 3-way tie at the k-th value among unseen ids (ranks
    k .. k + 2: two more candidates survive; for k = 1024 ranks k - 2 .. k, the candidate list is exactly full)."""
    rng = np.random.default_rng(seed)
    logits = (4 * rng.standard_normal(vocab)).astype(np.float32)
    if variant == "neginf":
        logits[rng.choice(vocab, vocab // 10, replace=False)] = -np.inf
    rank = np.argsort(-logits, kind="stable")
    finite = rank[np.isfinite(logits[rank])]
    seen = np.unique(np.concatenate([finite[[0, 2, 5, 11]], finite[-4:], rng.choice(vocab, 200, replace=False)]))
    assert (logits[seen] > 0).any() and (logits[seen] < 0).any()
    if variant == "tie":
        k = max(kw["top_k"], 1)
        a = k - 1 if k < 1024 else k - 3  # rank (0-based) of the first of the three tied scores
        order = np.argsort(-R.scores_f32(logits, seen, kw["repetition_penalty"], kw["temperature"], kw["do_sample"]),
                           kind="stable")
        seen = seen[seen != order[a]]  # the tied scores belong to unseen ids: equal logits, equal scores
        more = [int(i) for i in order[a + 3:a + 400] if i not in seen][:2]
        logits[more] = logits[order[a]]
        top = np.sort(R.scores_f32(logits, seen, kw["repetition_penalty"], kw["temperature"], kw["do_sample"]))[::-1]
        assert top[a] == top[a + 1] == top[a + 2] > top[a + 3] and (a == 0 or top[a - 1] > top[a])
    return logits, seen


def _seen_words(vocab, ids):
    w = np.zeros((vocab + 31) // 32, dtype=np.uint32)
    ids = np.asarray(ids, dtype=np.int64)  # an empty list would otherwise become float64
    np.bitwise_or.at(w, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return w


def _uniforms(seed, near=None):
    """256 uniforms on the kernel's own grid (multiples of 2^-24): 0, 1 - 2^-24, the rest random. `near(u)` (the
    reference's "within tol of a CDF boundary"): draws are chosen, on the reference alone, so that at most 1 % of them
    need the tolerance — where boundaries lie dense (the whole vocabulary, long candidate tails) a random set would not."""
    rng = np.random.default_rng(seed)
    us = [0.0, 1.0 - R.TWO_M24]
    budget = N_DRAWS // 100 - (sum(bool(near(u)) for u in us) if near else 0)
    while len(us) < N_DRAWS:
        u = float(rng.integers(0, 1 << 24)) * R.TWO_M24
        if near is not None and near(u):
            if budget <= 0:
                continue
            budget -= 1
        us.append(u)
    return np.array(us)


def _run(logits, seen_words, cfg, us, pos=0):
    """one probe call per uniform, all asynchronous, each on its own copy of the bit set -> tokens, bit sets, status"""
    dev = "cuda"
    lg = torch.from_numpy(logits).to(dev)
    n = len(us)
    seen = torch.from_numpy(seen_words.view(np.int32)).to(dev).repeat(n, 1).contiguous()
    u = torch.tensor(us, dtype=torch.float32, device=dev)
    tok = torch.full((n,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    p = torch.tensor([pos], dtype=torch.int32, device=dev)
    for j in range(n):
        L.probe_sample(lg, seen[j], cfg, p, tok[j:j + 1], u=u[j:j + 1], status=status[j:j + 1])
    torch.cuda.synchronize()
    return tok.cpu().numpy(), seen.cpu().numpy().view(np.uint32), status.cpu().numpy()


def _check_bits(tokens, seen_after, seen_before):
    for j, t in enumerate(tokens):
        want = seen_before.copy()
        want[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
        assert np.array_equal(seen_after[j], want), (j, t)


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("name", list(SETTINGS))
def test_token_choice_against_float64_reference(name, vocab):
    kw = SETTINGS[name]
    variants = ("plain", "neginf") if name == "whole_vocab" else ("plain", "neginf", "tie")
    cfg = L.sampler_config(seed=99, **kw)
    for vi, variant in enumerate(variants):
        logits, seen_ids = _inputs(vocab, kw, variant, seed=1000 * vi + vocab % 997 + len(name))
        words = _seen_words(vocab, seen_ids)
        s = R.scores_f32(logits, seen_ids, kw["repetition_penalty"], kw["temperature"], kw["do_sample"])
        if not kw["do_sample"]:
            us = _uniforms(vocab + vi)
            tokens, seen_after, status = _run(logits, words, cfg, us)
            assert not status.any(), (name, vocab, variant, status[status != 0][:4])
            _check_bits(tokens, seen_after, words)
            best = int(np.flatnonzero(s == np.nanmax(s))[0])  # lowest id on ties
            assert (tokens == best).all(), (name, vocab, variant)
            continue
        ref = R.choose(s, kw["top_k"], kw["top_p"])
        if kw["top_k"] > 0:
            tol = 8 * ref.n_kept * R.TWO_M24
            assert ref.boundary_margin >= 100 * 8 * ref.n_candidates * R.TWO_M24, (name, vocab, variant, ref.boundary_margin)
            if variant == "tie":
                assert ref.n_candidates == (kw["top_k"] + 2 if kw["top_k"] < 1024 else 1024)
        else:
            w32 = np.exp(s[ref.ids].astype(np.float64) - float(np.max(s[ref.ids]))).astype(np.float32)
            c32 = R.hierarchical_cdf_f32(w32).astype(np.float64)
            drift = float(np.max(np.abs(c32 / c32[-1] - ref.cdf)))
            tol = 4 * drift
            print("whole vocabulary %d %s: fp32 CDF drift %.3e, tol %.3e" % (vocab, variant, drift, tol))
            assert 0 < tol < 1e-5
        us = _uniforms(vocab + vi, near=lambda u: ref.needs_tolerance(u, tol))
        tokens, seen_after, status = _run(logits, words, cfg, us)
        assert not status.any(), (name, vocab, variant, status[status != 0][:4])
        _check_bits(tokens, seen_after, words)
        near = sum(ref.needs_tolerance(u, tol) for u in us)
        assert near <= N_DRAWS // 100, (name, vocab, variant, near)
        exact = 0
        for u, t in zip(us, tokens):
            assert ref.accepts(int(t), u, tol), (name, vocab, variant, u, int(t), ref.pick(u))
            if not ref.needs_tolerance(u, tol):
                assert int(t) == ref.pick(u), (name, vocab, variant, u, int(t), ref.pick(u))
                exact += 1
        print("%s vocab %d %s: candidates %d, kept %d, distinct picks %d, exact %d / %d" %
              (name, vocab, variant, ref.n_candidates, ref.n_kept, len(set(tokens.tolist())), exact, N_DRAWS))


def test_philox_words_match_the_numpy_restatement():
    """(seed, position) spread, position 0 and max_ctx - 1 of a 2048-context engine included; without an explicit u the
    pick is the reference's at u = (x0 >> 8) * 2^-24."""
    vocab, kw = 32000, SETTINGS["t0.9_k8_p0.95"]
    logits, seen_ids = _inputs(vocab, kw, "plain", seed=5)
    words = _seen_words(vocab, seen_ids)
    ref = R.choose(R.scores_f32(logits, seen_ids, kw["repetition_penalty"], kw["temperature"], True), kw["top_k"], kw["top_p"])
    lg = torch.from_numpy(logits).cuda()
    tol = 8 * ref.n_kept * R.TWO_M24
    for seed in (0, 1, 0xFFFFFFFF, 0x123456789ABCDEF0, (1 << 63) - 1):
        cfg = L.sampler_config(seed=seed, **kw)
        for pos in (0, 1, 7, 1000, 2047, 131071):
            seen = torch.from_numpy(words.view(np.int32)).cuda()
            out = torch.zeros(4, dtype=torch.int32, device="cuda")
            tok = torch.zeros(1, dtype=torch.int32, device="cuda")
            L.probe_sample(lg, seen, cfg, torch.tensor([pos], dtype=torch.int32, device="cuda"), tok, philox_out=out)
            got = [int(x) & 0xFFFFFFFF for x in out.cpu().tolist()]
            assert got == R.philox4x32_10((pos, 0, 0, 0), (seed & 0xFFFFFFFF, seed >> 32)), (seed, pos)
            u = R.uniform_at(seed, pos)
            assert ref.accepts(int(tok.item()), u, tol) and (ref.needs_tolerance(u, tol) or int(tok.item()) == ref.pick(u))


def test_all_nan_row_and_candidate_overflow():
    """every logit NaN: token 0 and status bit 4 (sampling and argmax alike); more than 1024 scores tied at the k-th
    value: the 1024 lowest ids among the tied are the candidates, status bit 8."""
    vocab = 32000
    nan = np.full(vocab, np.nan, dtype=np.float32)
    words = _seen_words(vocab, [3, 70])
    for name in ("neuralchat_default", "penalty_argmax", "whole_vocab"):
        tokens, seen_after, status = _run(nan, words, L.sampler_config(seed=1, **SETTINGS[name]), [0.0, 0.5])
        assert (tokens == 0).all() and (status == 4).all(), (name, tokens, status)
        _check_bits(tokens, seen_after, words)
    rng = np.random.default_rng(3)
    logits = (4 * rng.standard_normal(vocab)).astype(np.float32)
    tied = np.sort(rng.choice(vocab, 2000, replace=False))
    logits[tied] = 30.0
    kw = dict(do_sample=True, temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0)
    us = _uniforms(11)
    tokens, seen_after, status = _run(logits, _seen_words(vocab, []), L.sampler_config(seed=1, **kw), us)
    assert (status == 8).all()
    ref = R.choose(R.scores_f32(logits, [], 1.0, 1.0, True), 5, 1.0)
    assert ref.n_kept == 1024 and np.array_equal(ref.ids, tied[:1024])
    tol = 8 * 1024 * R.TWO_M24
    for u, t in zip(us, tokens):
        assert ref.accepts(int(t), u, tol), (u, int(t), ref.pick(u))
    _check_bits(tokens, seen_after, _seen_words(vocab, []))


def test_fewer_than_k_finite_scores_and_the_end_of_the_unit_interval():
    """Fewer than k finite scores: the -inf entries tie at the k-th value but weigh exactly 0 — the draw is over the
    finite ones and the status stays 0 (no truncation happened that a caller could notice). Whole vocabulary with an
    explicit u = 1.0 (above what Philox can give): u * Z is not exceeded anywhere, the pick is the last id with mass."""
    vocab = 32000
    rng = np.random.default_rng(17)
    logits = np.full(vocab, -np.inf, dtype=np.float32)
    finite = np.sort(rng.choice(vocab, 10, replace=False))
    logits[finite] = rng.standard_normal(10).astype(np.float32)
    kw = dict(do_sample=True, temperature=1.0, top_k=40, top_p=1.0, repetition_penalty=1.0)
    ref = R.choose(R.scores_f32(logits, [], 1.0, 1.0, True), 40, 1.0)
    tol = 8 * ref.n_kept * R.TWO_M24
    us = _uniforms(23, near=lambda u: ref.needs_tolerance(u, tol))
    words = _seen_words(vocab, [])
    tokens, seen_after, status = _run(logits, words, L.sampler_config(seed=1, **kw), us)
    assert not status.any(), status[status != 0][:4]
    assert set(tokens.tolist()) <= set(finite.tolist()) and len(set(tokens.tolist())) > 3
    for u, t in zip(us, tokens):
        assert ref.accepts(int(t), u, tol), (u, int(t), ref.pick(u))
    _check_bits(tokens, seen_after, words)

    logits = rng.standard_normal(vocab).astype(np.float32)
    logits[-100:] = -np.inf
    tokens, seen_after, status = _run(logits, words, L.sampler_config(seed=1, **SETTINGS["whole_vocab"]), [1.0])
    assert tokens.tolist() == [vocab - 101] and not status.any()
    _check_bits(tokens, seen_after, words)
