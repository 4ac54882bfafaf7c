"""Reference for the unmerged LoRA adapters of the decode engine (csrc/woq_lora.hip): numpy, float64.

A targeted projection computes y = x W_deq (+ bias) + s (x A^T) B^T with A [r, K], B [n, r], s = lora_alpha / r. A fused
projection has PARTS in blob column order: q | k | v concatenated along N, gate / up interleaved per 16-column tile as
`runtime.fuse_gate_up` lays the blob out (`fuse_cols` restates it), one part for o_proj and down_proj. A part is
(A, B, s), or (None, n_cols, 0.0) when the target carries no adapter.

`delta`      the decode step's vector d[n] = base_bias[n] + s_p sum_j B_p[n'][j] t_p[j], t_p[j] = inv sum_k A_p[j][k] x[k].
`xq_input`   the vector an XQ consumer really reads: decode(encode(fl32(y))) (tests/xq_reference.py), and the RMSNorm factor
             from the K / 16 partial sums of squares.
`shrink` / `expand` / `silu_pairs`  the prompt pass's rows: T[m][j] = inv_m sum_k A[j][k] g_k X[m][k] over the stacked rows
             of the parts, D[m][n] = s_p sum_j T[m][roff_p + j] B_p[n'][j], and SiLU(gate) * up over interleaved tiles.

Tolerance (`delta` / `expand` return it per element beside the value). It is derived from the arithmetic, not measured:
an fp32 sum of n terms in ANY order is within n 2^-24 sum|terms| of the exact sum to first order; the two-stage sum
chains K products (into t) and r products (into d), and multiplies by inv and by s once each, so
    tol[n] = (K + r + 2) 2^-24  sum_j |s B[n][j]|  sum_k |inv A[j][k] x[k]|.
What lies outside that sum is added where it occurs, one rounding each: the fp32 addition onto a stored value (the static
bias of the decode step; the fp32 / fp16 rows of the prompt pass) costs 2^-24 of the result, and a result stored as fp16
half an fp16 ulp (`half_ulp16`). The SiLU * mul of the gate/up mode passes the gate's and the up's tolerances on through
its partial derivatives (|SiLU'| <= 1.1) and adds the fp32 epilogue's own roundings (`silu_pairs`).
"""
import numpy as np

from tests import xq_reference as X

F32 = np.float32
U = 2.0 ** -24  # half an fp32 ulp of 1: the relative error of one fp32 rounding


def fuse_cols(gate, up):
    """[..., I] x 2 -> [..., 2 I], 16-column tiles interleaved gate, up, gate, up, ... (runtime.fuse_gate_up)"""
    lead, inter = gate.shape[:-1], gate.shape[-1]
    assert inter % 16 == 0 and up.shape == gate.shape
    g = gate.reshape(*lead, inter // 16, 1, 16)
    u = up.reshape(*lead, inter // 16, 1, 16)
    return np.concatenate([g, u], axis=-2).reshape(*lead, 2 * inter)


def part_cols(part):
    return int(part[1]) if part[0] is None else int(part[1].shape[0])


def part_rank(part):
    return 0 if part[0] is None else int(part[0].shape[0])


def _assemble(cols, interleave):
    """per-part [..., n_p] arrays -> [..., N] in blob column order"""
    if interleave:
        assert len(cols) == 2
        return fuse_cols(cols[0], cols[1])
    return np.concatenate(cols, axis=-1)


def _two_stage(x64, inv, part, K):
    """x64 [..., K], inv [...] or scalar -> (s (x A^T) B^T inv, tolerance) [..., n] for one part"""
    n = part_cols(part)
    lead = x64.shape[:-1]
    if part[0] is None:
        return np.zeros(lead + (n,)), np.zeros(lead + (n,))
    A, B, s = np.asarray(part[0], F32).astype(np.float64), np.asarray(part[1], F32).astype(np.float64), float(F32(part[2]))
    r = A.shape[0]
    assert A.shape == (r, K) and B.shape == (n, r)
    inv = np.asarray(inv, np.float64)[..., None]
    t = (x64 @ A.T) * inv
    t_abs = (np.abs(x64) @ np.abs(A).T) * np.abs(inv)
    return s * (t @ B.T), (K + r + 2) * U * (t_abs @ np.abs(s * B).T)


def delta(x, parts, base_bias=None, inv=1.0, interleave=False):
    """x [K] (float64, or fp32 taken exactly) -> (d float64 [N], tol float64 [N])"""
    x64 = np.asarray(x, np.float64)
    K = x64.shape[0]
    vals, tols = zip(*(_two_stage(x64, inv, p, K) for p in parts))
    d, tol = _assemble(list(vals), interleave), _assemble(list(tols), interleave)
    if base_bias is not None:
        d = d + np.asarray(base_bias, F32).astype(np.float64)
        tol = tol + U * np.abs(d)  # the one fp32 addition of the static bias
    return d, tol


def xq_input(y, ssq_of=None, eps=0.0):
    """y fp32 [K] (what the producer converts: x times the consumer's norm weight) -> (decoded float64 [K], inv): the
    values an XQ consumer reads, and 1 / sqrt(sum(ssq) / K + eps) over the float64 block sums of squares of `ssq_of`
    (the raw x; None = no norm, inv 1)."""
    limbs, u, _ = X.encode(np.asarray(y, F32))
    dec = X.decode(limbs, u)
    if ssq_of is None:
        return dec, 1.0
    return dec, 1.0 / np.sqrt(X.block_ssq(ssq_of).sum() / len(dec) + float(eps))


def rms_inv_rows(Xr, eps):
    x64 = np.asarray(Xr).astype(np.float64)
    return 1.0 / np.sqrt((x64 * x64).mean(axis=-1) + float(eps))


def shrink(Xr, a_parts, norm_w=None, eps=0.0):
    """Xr [M, K] fp32 / fp16 (taken exactly), a_parts = the parts' A [r_p, K] -> (T float64 [M, R_tot], tol [M, R_tot]);
    tol = (K + 2) 2^-24 sum_k |inv A g X| (K products, the product with g and the one with inv)"""
    x64 = np.asarray(Xr).astype(np.float64)
    K = x64.shape[1]
    inv = np.ones(x64.shape[0])
    if norm_w is not None:
        inv = rms_inv_rows(Xr, eps)
        x64 = x64 * np.asarray(norm_w, F32).astype(np.float64)
    A = np.concatenate([np.asarray(a, F32).astype(np.float64) for a in a_parts], axis=0)
    return (x64 @ A.T) * inv[:, None], (K + 2) * U * (np.abs(x64) @ np.abs(A).T) * inv[:, None]


def expand(Xr, parts, norm_w=None, eps=0.0, interleave=False):
    """the rows' adapter term from the rows themselves: Xr [M, K] -> (D float64 [M, N], tol [M, N]), blob column order"""
    x64 = np.asarray(Xr).astype(np.float64)
    K = x64.shape[1]
    inv = np.ones(x64.shape[0])
    if norm_w is not None:
        inv = rms_inv_rows(Xr, eps)
        x64 = x64 * np.asarray(norm_w, F32).astype(np.float64)
    vals, tols = zip(*(_two_stage(x64, inv, p, K) for p in parts))
    return _assemble(list(vals), interleave), _assemble(list(tols), interleave)


def half_ulp16(v):
    """half an fp16 ulp at magnitude |v| (normal range: 2^(e - 11) for |v| in [2^e, 2^(e + 1)); 2^-25 below 2^-14)"""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.ldexp(0.5, (e - 10).astype(np.int64))


def _silu(g):
    return g / (1.0 + np.exp(-g))


def silu_pairs(gu, tol_gu):
    """gu [M, 2 I] float64 in blob column order (gate tile, up tile, ...) with per-element tolerance -> (SiLU(gate) * up
    [M, I], its tolerance): |d/dgate| = |SiLU'(g)| |u| <= 1.1 |u|, |d/dup| = |SiLU(g)|, plus the fp32 epilogue (the two
    additions, the exponential of an argument rounded once — relative |g| 2^-24 — within 2 ulp, the division and the product:
    under 8 (1 + |g|) 2^-24 of the result)"""
    M = gu.shape[0]
    g, u = gu.reshape(M, -1, 2, 16)[:, :, 0, :].reshape(M, -1), gu.reshape(M, -1, 2, 16)[:, :, 1, :].reshape(M, -1)
    tg = tol_gu.reshape(M, -1, 2, 16)[:, :, 0, :].reshape(M, -1)
    tu = tol_gu.reshape(M, -1, 2, 16)[:, :, 1, :].reshape(M, -1)
    out = _silu(g) * u
    tol = 1.1 * np.abs(u) * tg + np.abs(_silu(g)) * tu + tg * tu + 8 * (1 + np.abs(g)) * U * np.abs(out)
    return out, tol
