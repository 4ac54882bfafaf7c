"""The backward of the weight-only linear with respect to its activations, stated in float64: what
`qbits.woq_linear_backward` (csrc/woq_linear_bwd.hip) has to compute. Pure numpy.

  forward   y[m][n]  = sum_j x[m][shuffle[j]] w[j][n]          w[j][n] = (code - z) s  |  table[code] s
  backward  dX[m][shuffle[j]] = sum_n dY[m][n] w[j][n]          S[m][shuffle[j]] = sum_n |dY[m][n] w[j][n]|

w is indexed by BLOB row j (shuffle = identity without act-order; with it, convert_idx of the raw GPTQ g_idx: position
j of the group-sorted order holds original channel shuffle[j]). The weights start from the codes, scales and zero points
`tests/quant_reference.py` produces from its input families; the scales are rounded to fp32, the type they are handed
to the device in, so w is exact in float64. Nothing here is taken from an implementation's output.

The kernel's bound (`bound`): |got - dX| <= 2^-9 S + 2^-22 N max_n|dY[m][n]| max|w|. Two operands rounded to 11 bits
give 2^-10, doubled for the relative-scale product (w enters as fp16((q - zp) fp16(s 2^-E))); the second term covers
elements the per-tensor relative scale pushes under fp16's normal range, plus fp32 accumulation.
"""
import functools

import numpy as np

from tests import quant_reference as qr

REL = 2.0 ** -9
ABS = 2.0 ** -22


def convert_idx(g_idx, group):
    """raw GPTQ g_idx (group of every input channel) -> shuffle (oracle/woq_oracle.c orc_convert_idx): a stable sort"""
    g_idx = np.asarray(g_idx, np.int64)
    K = g_idx.shape[0]
    ret = np.zeros(K, np.int32)
    counter = {}
    for i in range(K):
        g = int(g_idx[i])
        ret[g * group + counter.get(g, 0)] = i
        counter[g] = counter.get(g, 0) + 1
    return ret


@functools.lru_cache(maxsize=None)
def weight(K, N, group, wname, asym=False, act_order=False, seed=0):
    """-> dict: q int8 [K, N] / s fp32 [G, N] / z int8 [G, N] | None in the domain `qbits.repack_quantized_weight`
    takes (signed nibbles and zero points for 4 bits, signed bytes for int8, table indices for the table types),
    g_idx int32 [K] raw | None, shuffle int64 [K] | None, W [K, N] float64 in blob-row order. Read-only."""
    w, _, _ = qr.families(K, N, group, wname, asym=asym, seed=seed)
    d = qr.quantize(w, group, wname, asym=asym)
    g, G = qr.group_of(K, group)
    s32 = d["s"].astype(np.float32)
    code = d["code"]
    rows = np.minimum(np.arange(K) // g, G - 1)
    if qr.kind(wname) == "int":
        off = 2 ** (qr.INT_BITS[wname] - 1)
        if asym:
            q, z = (code - off).astype(np.int8), (d["z"] - off).astype(np.int8)
            W = (code - d["z"][rows]).astype(np.float64) * s32.astype(np.float64)[rows]
        else:
            q, z = code.astype(np.int8), None
            W = code.astype(np.float64) * s32.astype(np.float64)[rows]
    else:
        q, z = code.astype(np.int8), None
        W = qr.TABLES[wname][code] * s32.astype(np.float64)[rows]
    g_idx = shuffle = None
    if act_order:
        rng = np.random.default_rng(seed + 1)
        g_idx = rng.permutation(np.arange(K, dtype=np.int32) // g).astype(np.int32)
        shuffle = convert_idx(g_idx, g).astype(np.int64)
    out = dict(q=q, s=s32, z=z, g_idx=g_idx, shuffle=shuffle, W=W)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def uniform_weight(K, N, group, asym, seed=0):
    """int4 codes, scales and zero points drawn directly, every scale within a factor of 16 of the largest: no
    dequantised element is subnormal relative to it (the one-hot test). Same dict as `weight`."""
    rng = np.random.default_rng(seed)
    g, G = qr.group_of(K, group)
    q = rng.integers(-8, 8, (K, N)).astype(np.int8)
    s32 = (0.01 * 2.0 ** rng.uniform(-4, 0, (G, N))).astype(np.float32)
    z = rng.integers(-8, 8, (G, N)).astype(np.int8) if asym else None
    rows = np.minimum(np.arange(K) // g, G - 1)
    W = (q.astype(np.float64) - (z[rows] if asym else 0)) * s32.astype(np.float64)[rows]
    return dict(q=q, s=s32, z=z, g_idx=None, shuffle=None, W=W)


def gradient(M, N, seed=0, span=30):
    """dY fp32 [M, N]: N(0, 1) rows times 2^e, e stepping through -span .. span over the rows (gradients span far more
    than fp16's exponent range across rows), with a few exact zeros"""
    rng = np.random.default_rng(seed)
    e = np.round(np.linspace(-span, span, M)) if M > 1 else np.zeros(1)
    dY = rng.standard_normal((M, N)) * 2.0 ** rng.permutation(e)[:, None]
    dY[rng.random((M, N)) < 0.02] = 0.0
    return dY.astype(np.float32)


def forward(x, W, shuffle=None):
    x = np.asarray(x, np.float64)
    return (x[:, shuffle] if shuffle is not None else x) @ W


def backward(dY, W, shuffle=None):
    """-> (dX [M, K], S [M, K]) in float64, columns in the caller's (un-shuffled) order"""
    dY = np.asarray(dY, np.float64)
    g = dY @ W.T
    S = np.abs(dY) @ np.abs(W).T
    if shuffle is None:
        return g, S
    dX, Ss = np.empty_like(g), np.empty_like(S)
    dX[:, shuffle], Ss[:, shuffle] = g, S
    return dX, Ss


def bound(dY, W, S):
    """[M, K] tolerances of the kernel"""
    dY = np.asarray(dY, np.float64)
    return REL * S + ABS * dY.shape[1] * np.abs(dY).max(1, keepdims=True) * np.abs(W).max()
