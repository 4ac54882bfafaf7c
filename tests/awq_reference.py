"""AWQ (Lin et al. 2023, as in llm-awq / AutoAWQ) with the linear-output objective, stated in numpy float64 and
independent of the package: what `qbits.awq_scale_delta` / `qbits.awq_clip_search` (csrc/woq_awq.hip) and
`quantization/awq.py` have to compute. Q is `quant_reference.quantize`'s integer rule (bits in {2, 3, 4, 8}, sym or asym).

Working layout: W [K, N], row k = input feature k (Linear.weight.T). The loss is the squared output error of the linears,
so the activations X [T, K] enter only through

    H = X^T X / T      and      a = mean_t |x_t|  [K]

auto_scale, one absorb group (linears W_1 .. W_m sharing X):
    r_i = i / 20, i = 0 .. 19;  s = clamp(a^r_i, min=1e-4);  s /= sqrt(max(s) min(s))
    loss_i = sum_m tr(D^T H D),  D = diag(1 / s) Q(diag(s) W_m) - W_m;  the first minimum wins (i = 0: s = 1, plain RTN)

auto_clip, one linear whose input was scaled by s: H' = diag(1 / s) H diag(1 / s); per column n and group g of `group`
rows, c_j = 1 - j / 20, j = 0 .. 9:
    sym   the group clamped to +-c max|w|;   asym   to [c min(min w, 0), c max(max w, 0)]
    e_j = d^T G_g d,  d = Q(clamped) - w (against the unclipped w),  G_g = the group's diagonal block of H'
    the first minimum wins; the weight is clamped accordingly (j = 0 clamps nothing: plain RTN)
"""
import numpy as np

try:
    from . import quant_reference as Q
except ImportError:  # imported as a top-level module
    import quant_reference as Q

WNAME = {4: "int4_clip", 8: "int8", 3: "int3_clip", 2: "int2_clip"}
N_GRID = 20
N_CLIP = 10


def stats(X):
    """X [T, K] -> (H = X^T X / T, a = mean |x|)"""
    X = np.asarray(X, np.float64)
    return X.T @ X / X.shape[0], np.abs(X).mean(0)


def loss_from_h(D, H):
    """tr(D^T H D)"""
    D = np.asarray(D, np.float64)
    return float((D * (np.asarray(H, np.float64) @ D)).sum())


def loss_from_x(D, X):
    """||X D||_F^2 / T: the same number from the activations themselves"""
    X = np.asarray(X, np.float64)
    return float(((X @ np.asarray(D, np.float64)) ** 2).sum() / X.shape[0])


def scale_of(a, i, n_grid=N_GRID):
    """candidate i of the scale search"""
    s = np.maximum(np.asarray(a, np.float64) ** (i / n_grid), 1e-4)
    return s / np.sqrt(s.max() * s.min())


def scale_delta(W, s, group, bits, asym):
    """-> dict(D = diag(1 / s) Q(diag(s) W) - W, code [K, N], x [K, N] = the value rounded to give the code (before
    rounding; asym: without the zero point), back = D + W, qs [G, N] = the quantiser's scales)"""
    W = np.asarray(W, np.float64)
    s = np.asarray(s, np.float64)[:, None]
    r = Q.quantize(W * s, group, WNAME[bits], asym)
    g, _ = Q.group_of(W.shape[0], group)
    x = (W * s) / np.repeat(r["s"], g, axis=0)[:W.shape[0]]
    back = r["deq"] / s
    return dict(D=back - W, code=r["code"], x=x, back=back, qs=r["s"])


def auto_scale(Ws, H, a, group, bits, asym, n_grid=N_GRID):
    """the scale search of one absorb group -> dict(best, s [K], losses [n_grid])"""
    losses = np.array([sum(loss_from_h(scale_delta(W, scale_of(a, i, n_grid), group, bits, asym)["D"], H) for W in Ws)
                       for i in range(n_grid)])
    best = int(losses.argmin())  # the first minimum
    return dict(best=best, s=scale_of(a, best, n_grid), losses=losses)


def h_scaled(H, s):
    """the Gram matrix of the scaled input x / s"""
    s = np.asarray(s, np.float64)
    return np.asarray(H, np.float64) / np.outer(s, s)


def clamp_of(W, group, asym, c):
    """-> (lo [K, N], hi [K, N]): candidate c's bounds of every element's group"""
    W = np.asarray(W, np.float64)
    K = W.shape[0]
    g, G = Q.group_of(K, group)
    lo, hi = np.empty_like(W), np.empty_like(W)
    for gi in range(G):
        rows = slice(gi * g, min(K, (gi + 1) * g))
        v = W[rows]
        if asym:
            lo[rows], hi[rows] = c * np.minimum(v.min(0), 0.0), c * np.maximum(v.max(0), 0.0)
        else:
            m = c * np.abs(v).max(0)
            lo[rows], hi[rows] = -m, m
    return lo, hi


def clip_search(W, Hs, group, bits, asym, n_grid=N_GRID, n_cand=N_CLIP):
    """the clip search of one linear under Hs (= H' where the input was scaled) -> dict(best [G, N], losses
    [n_cand, G, N], w_out [K, N], and per candidate and cell what an fp32 evaluation may differ by:
      fp32_bound [n_cand, G, N]  with delta_i = 8 2^-24 (|w_i| + |d_i|) (the bound, the scale, the dequantised product
                                 and the subtraction are at most seven fp32 roundings of numbers no larger than
                                 |w_i| + |d_i|) and the quadratic form's own rounding (rows + 2) 2^-24 sum |d_i G_ik d_k|:
                                 sum_ik |G_ik| (delta_i |d_k| + |d_i| delta_k) + (rows + 2) 2^-24 sum_ik |d_i G_ik d_k|
      near_tie [n_cand, G, N]    a value of the cell (or its asym zero point) lies within Q.FP32_SLOP-relative of a
                                 rounding tie, so an fp32 evaluation may take the other code)"""
    W = np.asarray(W, np.float64)
    Hs = np.asarray(Hs, np.float64)
    K, N = W.shape
    g, G = Q.group_of(K, group)
    losses, bound = np.empty((n_cand, G, N)), np.empty((n_cand, G, N))
    near = np.zeros((n_cand, G, N), bool)
    clamped = []
    for j in range(n_cand):
        lo, hi = clamp_of(W, group, asym, 1.0 - j / n_grid)
        cl = np.clip(W, lo, hi)
        clamped.append(cl)
        r = Q.quantize(cl, group, WNAME[bits], asym)
        d = r["deq"] - W
        x = cl / np.repeat(r["s"], g, axis=0)[:K]
        tie = np.abs(np.abs(x - np.floor(x)) - 0.5) <= Q.FP32_SLOP * np.maximum(1.0, np.abs(x))
        delta = 8 * 2.0 ** -24 * (np.abs(W) + np.abs(d))
        for gi in range(G):
            rows = slice(gi * g, min(K, (gi + 1) * g))
            blk, dg, ag = Hs[rows, rows], d[rows], np.abs(d[rows])
            losses[j, gi] = (dg * (blk @ dg)).sum(0)
            ab = np.abs(blk)
            bound[j, gi] = ((delta[rows] * (ab @ ag)).sum(0) + (ag * (ab @ delta[rows])).sum(0)
                            + (dg.shape[0] + 2) * 2.0 ** -24 * (ag * (ab @ ag)).sum(0))
            near[j, gi] = tie[rows].any(0)
        if asym:
            zt = r["zt"]
            near[j] |= np.abs(np.abs(zt - np.floor(zt)) - 0.5) <= Q.FP32_SLOP * np.maximum(1.0, np.abs(zt))
    best = losses.argmin(0)  # the first minimum
    pick = np.repeat(best, g, axis=0)[:K]
    w_out = np.choose(pick, clamped)
    return dict(best=best, losses=losses, w_out=w_out, fp32_bound=bound, near_tie=near)


def runner_up_gap(losses):
    """[...] relative distance of the second-best candidate from the best, per cell (losses [n_cand, ...])"""
    srt = np.sort(losses, axis=0)
    return (srt[1] - srt[0]) / np.where(srt[0] == 0, 1.0, srt[0])


# ---- inputs ---------------------------------------------------------------------------------------------------------
def salient(K, N, seed=0, tokens=512, n_salient=6, boost=16.0):
    """(w fp32 [K, N] Gaussian, X fp32 [tokens, K]): X as `gptq_reference.correlated` builds it (eight common factors
    plus noise of its own per feature) with `n_salient` channels multiplied by `boost`: the channels whose weights AWQ
    protects by scaling them up."""
    rng = np.random.default_rng(seed)
    load = rng.standard_normal((8, K))
    X = rng.standard_normal((tokens, 8)) @ load + 0.5 * rng.standard_normal((tokens, K))
    X[:, rng.choice(K, size=n_salient, replace=False)] *= boost
    w = (0.05 * rng.standard_normal((K, N))).astype(np.float32)
    return w, X.astype(np.float32)
