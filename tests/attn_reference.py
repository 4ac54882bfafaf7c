"""float64 reference of the engine's attention kernels (tests/test_gpu_attention_kernels.py), written from HF semantics
as DESIGN §5 and oracle.LlamaOracle define them:

* RoPE in the rotate_half form, with the exact fp32 cos / sin tables the kernel is handed;
* query position p sees cache positions [max(0, p + 1 - window), p] (window 0: no lower edge);
* query head h reads kv head h // (heads // kv_heads);
* softmax(q . k / sqrt(head_dim)) . v in float64.

The reference attends over the cache AS STORED: the caller hands it the rows read back from the device and widened
exactly, so cache-dtype rounding is checked once (the append tests) and not folded into every attention bound.
Storage rounding (`round_to`) is round-to-nearest-even with the kernels' saturation (woq_hip.h: fp16 at +-65504, e4m3
at +-448; bf16 keeps fp32's range).
"""
import numpy as np

# (mantissa bits, smallest normal exponent, largest finite value)
FORMATS = {"fp16": (10, -14, 65504.0), "bf16": (7, -126, 3.3895313892515355e38), "fp8": (3, -6, 448.0)}


def round_to(x, fmt):
    """x (float64) rounded to nearest-even in `fmt`, saturated at the format's largest finite value."""
    m, emin, big = FORMATS[fmt]
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(x)))
    e = np.where(np.isfinite(e), np.maximum(e, emin), emin)
    quantum = np.exp2(e - m)
    return np.clip(np.round(x / quantum) * quantum, -big, big)


def rotate(x, cos, sin):
    """rotate_half RoPE of x [..., D] with cos / sin [..., D / 2] (broadcast), float64."""
    x = np.asarray(x, dtype=np.float64)
    h = x.shape[-1] // 2
    a, b = x[..., :h], x[..., h:]
    c, s = np.asarray(cos, dtype=np.float64), np.asarray(sin, dtype=np.float64)
    return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)


def unrotate(x, cos, sin):
    """the inverse of `rotate` (float64): the un-rotated vector whose rotation is x"""
    x = np.asarray(x, dtype=np.float64)
    h = x.shape[-1] // 2
    a, b = x[..., :h], x[..., h:]
    c, s = np.asarray(cos, dtype=np.float64), np.asarray(sin, dtype=np.float64)
    return np.concatenate([a * c + b * s, b * c - a * s], axis=-1)


def rotate_error(x, cos, sin):
    """a bound on |fp32 rotation - float64 rotation| per element: two fp32 products and one fp32 sum (or one product and
    one fma), each off by at most half an ulp (2^-24 relative) of a term no larger than |a c| + |b s| (first half) or
    |b c| + |a s| (second half)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    h = x.shape[-1] // 2
    a, b = x[..., :h], x[..., h:]
    c, s = np.abs(np.asarray(cos, dtype=np.float64)), np.abs(np.asarray(sin, dtype=np.float64))
    return 3 * 2.0 ** -24 * np.concatenate([a * c + b * s, b * c + a * s], axis=-1)


def stored_bounds(ref, err, fmt):
    """the two values a rotation computed to within `err` of `ref` may be stored as: rounding is monotone, so the stored
    value lies in [round(ref - err), round(ref + err)] — that is round(ref) itself except at rounding ties, where it
    is one of the two neighbours (one ulp of storage)"""
    return round_to(ref - err, fmt), round_to(ref + err, fmt)


def attend(q, K, V, positions, window, targets=None, block=256):
    """q [R, D] at query positions `positions` [R] over cache rows K, V [N, D] (row t = position t), float64. Returns
    out [R, D], max |v| over each query's visible rows [R] and, with `targets` [R], the softmax weight of each query's
    target position (0 where it is not visible). Rows go in blocks, each over the columns its queries can see."""
    q = np.asarray(q, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    positions = np.asarray(positions)
    R_, D = q.shape
    vrow = np.abs(V).max(axis=1)
    out, vmax, wt = np.empty((R_, D)), np.empty(R_), np.zeros(R_)
    for b0 in range(0, R_, block):
        p = positions[b0:b0 + block, None]
        lo = np.maximum(0, p + 1 - window) if window > 0 else np.zeros_like(p)
        c0, c1 = int(lo.min()), int(p.max()) + 1
        t = np.arange(c0, c1)[None, :]
        vis = (t <= p) & (t >= lo)
        s = np.where(vis, (q[b0:b0 + block] @ K[c0:c1].T) / np.sqrt(D), -np.inf)
        s -= s.max(axis=1, keepdims=True)
        w = np.exp(s)
        w /= w.sum(axis=1, keepdims=True)
        out[b0:b0 + block] = w @ V[c0:c1]
        vmax[b0:b0 + block] = np.where(vis, vrow[None, c0:c1], 0.0).max(axis=1)
        if targets is not None:
            tg = np.asarray(targets[b0:b0 + block]) - c0
            ok = (tg >= 0) & (tg < c1 - c0)
            wt[b0:b0 + block] = np.where(ok, w[np.arange(len(tg)), np.clip(tg, 0, c1 - c0 - 1)], 0.0)
    return out, vmax, wt
