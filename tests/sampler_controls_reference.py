"""Reference for the sampler controls of csrc/woq_sample.hip (logit bias, presence / frequency penalty, min_p), shared by
tests/test_sampler_controls_cpu.py and the GPU sampler-controls tests. It extends tests/sampler_reference.py by import.

The adjusted score of id i is built from IEEE single operations, each rounded on its own, in the kernel's order:
  1. s = l + b[i] for ids with a bias entry (finite or -inf);
  2. the repetition penalty over the seen ids (sampler_reference.scores_f32);
  3. for ids generated c[i] > 0 times: s = s - (freq * float(c[i]));
  4. then s = s - pres;
  5. when sampling, s = s / T.
numpy float32 arithmetic does exactly that, so the kernel's adjusted-score buffer must equal `adjusted_f32` bit for bit.
`choose` adds the min_p cut (HF MinPLogitsWarper, min_tokens_to_keep 1, after top-k and top-p) to the float64 choice.
"""
import numpy as np

from tests import sampler_reference as R

TWO_M24 = R.TWO_M24


def adjusted_f32(logits, seen_ids, counts, penalty, presence=0.0, frequency=0.0, bias=None):
    """steps 1-4: fp32 scores before the temperature. `counts` [vocab] non-negative integers, `bias` {id: value}."""
    s = np.asarray(logits, dtype=np.float32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if bias:
            ids = np.array(list(bias), dtype=np.int64)
            s[ids] = s[ids] + np.array([bias[int(i)] for i in ids], dtype=np.float32)
        s = R.scores_f32(s, seen_ids, penalty, 1.0, False)
        c = np.asarray(counts)
        hit = c > 0
        step = (np.float32(frequency) * c[hit].astype(np.float32)).astype(np.float32)
        s[hit] = (s[hit] - step).astype(np.float32)
        s[hit] = (s[hit] - np.float32(presence)).astype(np.float32)
    return s


def scores_f32(logits, seen_ids, counts, penalty, temperature, do_sample, presence=0.0, frequency=0.0, bias=None):
    """steps 1-5: what the choice runs over"""
    s = adjusted_f32(logits, seen_ids, counts, penalty, presence, frequency, bias)
    return R.scores_f32(s, [], 1.0, temperature, do_sample)


def same_bits(a, b):
    """bit equality of two fp32 arrays, except that any NaN equals any NaN (payloads are not part of the contract)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(both_nan | (a.view(np.uint32) == b.view(np.uint32))))


def min_p_nearness(d, min_p):
    """|exp(d) - min_p| in units of the cut's fp32 margin (|d| + 4) * 2^-24 * min_p, d = s_i - s_0 in float64: half an
    ulp of the fp32 subtraction is |d| * 2^-24 relative in e^d, plus about 2 ulp of expf, doubled. d == 0 is exact in
    the kernel (equal scores weigh 1.0 without an expf, and 1.0 >= min_p always), so it is never near."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        units = np.abs(np.exp(d) - min_p) / ((np.abs(d) + 4.0) * TWO_M24 * min_p)
    return np.where(d == 0.0, np.inf, np.where(np.isfinite(d), units, np.inf))


def choose(scores, top_k, top_p, min_p=0.0, max_candidates=1024):
    """sampler_reference.choose followed by the min_p cut: a candidate stays iff exp(s_i - s_max) >= min_p (fp32 value of
    min_p). Candidate lists: the kept set is the first min(m_top_p, m_min_p) sorted candidates. Whole vocabulary
    (top_k = 0, top_p = 1): ids stay in id order, a dropped id weighs 0. The result carries `min_p_units`: the smallest
    `min_p_nearness` over every candidate (inf without min_p), and `n_mass`: ids with a non-zero weight."""
    base = R.choose(scores, top_k, top_p, max_candidates)
    s = np.asarray(scores, dtype=np.float32)
    mp = float(np.float32(min_p))
    if mp <= 0.0:
        base.min_p_units = np.inf
        base.n_mass = int(np.count_nonzero(np.diff(np.concatenate([[0.0], base.cdf])) > 0))
        return base
    if top_k <= 0:
        sv = s[base.ids].astype(np.float64)
        d = sv - float(np.max(sv))
        with np.errstate(over="ignore"):
            w = np.where(d == 0.0, 1.0, np.exp(d))
        w = np.where(w >= mp, w, 0.0)
        c = np.cumsum(w)
        out = R.Choice(base.ids, c / c[-1], base.n_candidates, base.boundary_margin)
        out.min_p_units, out.n_mass = float(np.min(min_p_nearness(d, mp))), int(np.count_nonzero(w))
        return out
    full = R.choose(scores, top_k, 1.0, max_candidates)  # every candidate, sorted
    sv = s[full.ids].astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.where(sv == sv[0], 0.0, sv - sv[0])
        w = np.where(d == 0.0, 1.0, np.exp(d))
    below = np.nonzero(~(w >= mp))[0]
    m = min(base.n_kept, int(below[0]) if below.size else len(w))
    c = np.cumsum(w[:m])
    out = R.Choice(full.ids[:m], c / c[-1], base.n_candidates, base.boundary_margin)
    out.min_p_units, out.n_mass = float(np.min(min_p_nearness(d, mp))), m
    return out
