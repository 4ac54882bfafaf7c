"""Float64 statement of the routed expert block `qbits.moe_forward` (csrc/woq_moe.hip) computes, with a per-element
tolerance. Pure numpy.

R0: out[t] = sum_j w[t, j] * (SiLU(x_t Wg_e) * (x_t Wu_e)) Wd_e, e = idx[t, j], j ascending, a slot whose id lies outside
[0, E) contributing zero; Wg | Wu = the two column halves of expert e's dequantised gate/up blob [H, 2I], Wd its down blob
[I, H] (`woq_dequantize_packed_weight`, oracle-checked elsewhere).

Tolerance 4 (A + B), derived as tests/gemv_f32_reference.py::terms derives its own:
  B = max |R1 - R0|, R1 = R0 with the activation replaced by the kernels' fixed point at both products: per row and per
      1024-k chunk round(fl32(v) 2^(21 - e)) 2^(e - 21), e = the frexp exponent of the chunk's largest |v| — applied to x
      and to the intermediate h (`gemv_f32_reference.convert` with the chunks as its slices).
  A = the fp32 rounding band, n_ops 2^-24 over sum |x| |w|, carried through the block: gate and up each carry
      A_g = n(H) U (|x| |Wg|); through SiLU * mul (exp, add, divide, multiply: 4 more) as that file's `band` does,
      A_h = (|SiLU'(g)| + A_g / 2) A_g |u| + |SiLU(g)| A_u + A_g A_u + 4 U |h|; the down product carries it on,
      A_y = A_h |Wd| + n(I) U (|h| |Wd|); the k-term sum A = sum_j |w_j| A_y_j + (k + 1) U sum_j |w_j| |y_j|.
      n(K) counts the longest chain of fp32 roundings behind one product output, from the kernel source: a wave owns 2 tiles
      of each 1024-k chunk; per tile and scale block (1 for scale_mode 0, 4 for scale_mode 1) limb_combine (3 conversions
      + 2 fma = 5, charged 6 as that file does), the zero-point term (a second limb_combine, a product, an fma: 7), the
      product scale * unsc (1) and the fma into the running sum (1); then the sum over the 4 waves (4).
A 16-bit output adds half a unit in its last place of |R0| (one rounding), outside the factor 4.
"""
import numpy as np

from tests.gemv_f32_reference import _silu_d, convert
from tests.xq_reference import _silu

U = 2.0 ** -24
CHUNK = 1024


def n_ops(K, smode, asym):
    chunks = (K + CHUNK - 1) // CHUNK
    return 2 * chunks * (4 if smode == 1 else 1) * (6 + (7 if asym else 0) + 2) + 4


def _chunks(K):
    return [(k0, min(k0 + CHUNK, K)) for k0 in range(0, K, CHUNK)]


def block(x, idx, w, Wgu, Wdn, quant, fixed_point):
    """-> (out [T, H], A [T, H]) in float64; quant = (smode, asym) of the blobs"""
    T, H = x.shape
    E, inter = len(Wgu), Wdn[0].shape[0]
    x64 = x.astype(np.float64)
    xc = convert(x, _chunks(H)) if fixed_point else x64
    out, A = np.zeros((T, H)), np.zeros((T, H))
    n_h, n_i = n_ops(H, *quant), n_ops(inter, *quant)
    for t in range(T):
        mag_sum = np.zeros(H)
        for j in range(idx.shape[1]):
            e = int(idx[t, j])
            if not 0 <= e < E:
                continue
            g, u = xc[t] @ Wgu[e][:, :inter], xc[t] @ Wgu[e][:, inter:]
            h = _silu(g) * u
            a_g = n_h * U * (np.abs(x64[t]) @ np.abs(Wgu[e][:, :inter]))
            a_u = n_h * U * (np.abs(x64[t]) @ np.abs(Wgu[e][:, inter:]))
            a_h = (np.abs(_silu_d(g)) + 0.5 * a_g) * a_g * np.abs(u) + np.abs(_silu(g)) * a_u + a_g * a_u + 4 * U * np.abs(h)
            hc = convert(h[None].astype(np.float32), _chunks(inter))[0] if fixed_point else h
            y = hc @ Wdn[e]
            a_y = a_h @ np.abs(Wdn[e]) + n_i * U * (np.abs(h) @ np.abs(Wdn[e]))
            out[t] += float(w[t, j]) * y
            A[t] += abs(float(w[t, j])) * a_y
            mag_sum += abs(float(w[t, j])) * np.abs(y)
        A[t] += (idx.shape[1] + 1) * U * mag_sum
    return out, A


def reference(x, idx, w, Wgu, Wdn, quant, out_bits=24):
    """x fp32 [T, H], idx int [T, k], w fp32 [T, k], Wgu E x [H, 2I], Wdn E x [I, H] float64 -> (R0, tol, B)"""
    r0, A = block(x, idx, w, Wgu, Wdn, quant, False)
    r1, _ = block(x, idx, w, Wgu, Wdn, quant, True)
    B = float(np.abs(r1 - r0).max())
    tol = 4 * (A + B) + (0.0 if out_bits == 24 else 2.0 ** -out_bits * np.abs(r0))
    return r0, tol, B
