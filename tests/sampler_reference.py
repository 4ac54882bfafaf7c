"""Reference for the native sampler (csrc/woq_sample.hip), shared by tests/test_sampler_cpu.py and the GPU sampler tests:
a numpy restatement of Philox4x32-10 and a float64 restatement of the token choice.

The scores are computed with the SAME two IEEE single operations the kernel and torch apply (`s < 0 ? s * pen : s / pen`
over the seen ids, then `/ T` when sampling), so the top-k kept set is pure comparisons of identical fp32 values and must
match exactly; ordering, the nucleus and the CDF then run in float64.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
TWO_M24 = 2.0 ** -24


def philox4x32_10(counter, key):
    """counter (c0, c1, c2, c3), key (k0, k1) as Python ints -> the four output words."""
    c0, c1, c2, c3 = [int(c) & MASK for c in counter]
    k0, k1 = [int(k) & MASK for k in key]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [c0, c1, c2, c3]


def uniform_at(seed, pos):
    """The sampler's uniform for (64-bit seed, position): (x0 >> 8) * 2^-24."""
    x0 = philox4x32_10((pos, 0, 0, 0), (seed & MASK, (seed >> 32) & MASK))[0]
    return (x0 >> 8) * TWO_M24


def scores_f32(logits, seen_ids, penalty, temperature, do_sample):
    """fp32 penalised (and, when sampling, temperature-scaled) scores: the kernel's two IEEE single operations."""
    s = np.asarray(logits, dtype=np.float32).copy()
    ids = np.unique(np.asarray(seen_ids, dtype=np.int64))
    pen = np.float32(penalty)
    if ids.size and float(pen) != 1.0:
        with np.errstate(invalid="ignore"):
            v = s[ids]
            s[ids] = np.where(v < 0, v * pen, v / pen).astype(np.float32)
    if do_sample:
        with np.errstate(invalid="ignore"):
            s = (s / np.float32(temperature)).astype(np.float32)
    return s


class Choice:
    """ids in draw order, their normalised float64 CDF, and what the acceptance rule needs."""

    def __init__(self, ids, cdf, n_candidates, boundary_margin):
        self.ids, self.cdf, self.n_candidates, self.boundary_margin = ids, cdf, n_candidates, boundary_margin

    @property
    def n_kept(self):
        return len(self.ids)

    def pick(self, u):
        """first kept candidate whose inclusive sum exceeds u (the last one if rounding leaves none)"""
        j = int(np.searchsorted(self.cdf, u, side="right"))
        return int(self.ids[min(j, len(self.ids) - 1)])

    def accepts(self, token, u, tol):
        """token t is accepted iff u lies in [C_(t-1) - tol, C_t + tol]"""
        hit = np.nonzero(self.ids == token)[0]
        if hit.size == 0:
            return False
        j = int(hit[0])
        lo = self.cdf[j - 1] if j > 0 else 0.0
        return lo - tol <= u <= self.cdf[j] + tol

    def needs_tolerance(self, u, tol):
        """u within tol of an interior CDF boundary: the fp32 kernel may legitimately land on either side"""
        return bool(np.any(np.abs(self.cdf[:-1] - u) <= tol))


def choose(scores, top_k, top_p, max_candidates=1024):
    """float64 reference over fp32 `scores` (sampling): top-k with ties kept (the lowest ids among the tied when more
    than `max_candidates` survive), order (score descending, id ascending), nucleus with min_tokens_to_keep 1.
    top_k = 0: the whole vocabulary in id order (top_p must be 1)."""
    s = np.asarray(scores, dtype=np.float32)
    valid = ~np.isnan(s)
    if top_k <= 0:
        assert top_p >= 1.0
        ids = np.nonzero(valid)[0]
        w = np.exp(s[ids].astype(np.float64) - float(np.max(s[ids])))
        c = np.cumsum(w)
        return Choice(ids, c / c[-1], len(ids), np.inf)
    vs = s[valid]
    k = min(int(top_k), vs.size)
    kth = np.partition(vs, vs.size - k)[vs.size - k]
    above = np.nonzero(valid & (s > kth))[0]
    tied = np.nonzero(valid & (s == kth))[0]
    tied = tied[:max(0, max_candidates - above.size)]
    cand = np.concatenate([above, tied])
    order = np.lexsort((cand, -s[cand].astype(np.float64)))
    ids = cand[order]
    sv = s[ids].astype(np.float64)
    with np.errstate(invalid="ignore"):
        w = np.where(sv == sv[0], 1.0, np.exp(sv - sv[0]))
    c = np.cumsum(w)
    z = c[-1]
    m, margin = len(ids), np.inf
    if top_p < 1.0:
        thr = 1.0 - float(np.float32(top_p))
        tail = (z - np.concatenate([[0.0], c[:-1]])) / z  # mass of candidates i.. (ascending cumulative of HF's sort)
        drop = tail <= thr
        drop[0] = False
        m = int(np.argmax(drop)) if drop.any() else len(ids)
        margin = float(np.min(np.abs(tail[1:] - thr))) if len(ids) > 1 else np.inf
    return Choice(ids[:m], c[:m] / c[m - 1], len(ids), margin)


def kept_set(scores, top_k, top_p):
    """ids the processed scores leave finite (what DeviceSampler.processed keeps)"""
    return set(int(i) for i in choose(scores, top_k, top_p, max_candidates=1 << 30).ids)


def hierarchical_cdf_f32(w):
    """fp32 restatement of a pairwise-style CDF: inclusive sums inside blocks of 64 (tree order inside a block is below
    what this models: sequential fp32 here), block totals accumulated in fp32 — the shape of the kernel's whole-vocabulary
    walk. Used only to size that case's tolerance from the test's own inputs."""
    w = np.asarray(w, dtype=np.float32)
    pad = (-len(w)) % 64
    blocks = np.concatenate([w, np.zeros(pad, np.float32)]).reshape(-1, 64)
    inner = np.cumsum(blocks, axis=1, dtype=np.float32)
    base = np.concatenate([[np.float32(0)], np.cumsum(inner[:-1, -1], dtype=np.float32)]).astype(np.float32)
    return (inner + base[:, None]).astype(np.float32).reshape(-1)[:len(w)]
