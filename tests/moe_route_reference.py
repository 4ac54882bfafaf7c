"""Float64 statement of the router `qbits.moe_route` (csrc/woq_moe_route.hip) computes, with per-element tolerances. Pure numpy.

R0: xn = x / sqrt(mean(x^2) + eps) * norm_w (xn = x without norm_w); logit = xn @ W.T; p = softmax(logit); idx = the top_k
largest p, descending, equal p: the lower id first; w = p[idx], divided by its own sum when renorm.

Bands (U = 2^-24), roundings counted from the kernel source:
  xn     n_norm U |xn|: the sum of squares is 4 ceil(H / 256) fmaf of a lane + 6 butterfly adds, then / H, + eps, sqrt and
         1 / (4), then the two products of (x * inv) * norm_w (2). Without norm_w xn is x: no band.
  logit  (n_dot + n_norm) U (|xn| @ |W|.T). T = 1: 4 ceil(H / 256) fmaf of a lane + 6 butterfly adds. T > 1: a wave runs
         4 ceil(H / 64) v_mfma_f32_16x16x4_f32, each a chain of four fused multiply-adds (4), + 3 adds over the waves.
  p      p (2 max_e dlogit + (|logit - max|_max + E + 8) U): the subtraction, expf (<= 2 ulp, twice: numerator and sum), the
         ascending sum of E positive terms, the division.
  w      without renorm p's band; with it w (2 max_j relp_j + (k + 1) U).
Tolerance = 4 x band, the project's factor. margin = the row's gap between its k-th and (k + 1)-th largest logit."""
import numpy as np

U = 2.0 ** -24


def n_norm(H):
    return 4 * -(-H // 256) + 6 + 4 + 2


def n_dot(H, T):
    return 4 * -(-H // 256) + 6 if T == 1 else 4 * 4 * -(-H // 64) + 3


def reference(x, W, top_k, renorm, norm_w=None, eps=0.0):
    """x fp32 [T, H], W [E, H] (the values the device holds) -> dict of float64 results, tolerances, band and margin"""
    T, H = x.shape
    E = W.shape[0]
    x64, W64 = x.astype(np.float64), W.astype(np.float64)
    xn = x64 if norm_w is None else x64 / np.sqrt((x64 ** 2).mean(1, keepdims=True) + eps) * norm_w.astype(np.float64)
    logit = xn @ W64.T
    nn = 0 if norm_w is None else n_norm(H)
    band = (n_dot(H, T) + nn) * U * (np.abs(xn) @ np.abs(W64).T)
    z = logit - logit.max(1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    idx = np.argsort(-p, axis=1, kind="stable")[:, :top_k]  # stable: equal p keep ascending ids
    srt = -np.sort(-logit, axis=1)
    margin = srt[:, top_k - 1] - srt[:, top_k] if top_k < E else np.full(T, np.inf)
    relp = 2 * band.max(1, keepdims=True) + (np.abs(z).max(1, keepdims=True) + E + 8) * U
    w = np.take_along_axis(p, idx, 1)
    tol_w = 4 * w * relp
    if renorm:
        w = w / w.sum(1, keepdims=True)
        tol_w = 4 * w * (2 * relp + (top_k + 1) * U)
    return {"xn": xn, "tol_xn": 4 * nn * U * np.abs(xn), "idx": idx, "w": w, "tol_w": tol_w, "band": band.max(1),
            "margin": margin}
