"""Float64 statement of the routed expert block in its prompt form (`qbits.moe_forward(form="prompt")`,
csrc/woq_moe_prompt.hip), with a per-element tolerance that is derived, not measured. Pure numpy.

R0 is `tests/moe_reference.block(..., fixed_point=False)[0]`: the same definition as the grouped form.

Tolerance, per product y = x W over K: T(K) = (2^-9 + n(K) U) (|x| @ |W|), the bound of tests/woq_backward_reference.py:
  2^-9   both operands enter one fp16 product: the activation rounded once to 11 bits (2^-11) after an exact power-of-two
         scaling per row and 128-k tile; the weight as fp16((q - zp) fp16(s 2^-E)), two roundings (2^-10; scale_mode 0
         keeps the exact integer q - zp and applies s in fp32, which is tighter). 2^-11 + 2^-10 < 2^-9.
  n(K)   the longest chain of fp32 roundings behind one output, from the kernel source: per 128-k tile four MFMAs of 32 k
         accumulate in fp32, charged one rounding per k (128), then the factor row * column (1) and the fma into the
         running sum (1): n(K) = 130 ceil(K / 128). U = 2^-24.
It is carried through the block exactly as `moe_reference.block` carries its A: gate and up each carry A_g = T(H);
through SiLU * mul A_h = (|SiLU'(g)| + A_g / 2) A_g |u| + |SiLU(g)| A_u + A_g A_u + 4 U |h|; the down product
A_y = A_h |Wd| + T(I) of h; the k-term sum A = sum_j |w_j| A_y_j + (k + 1) U sum_j |w_j| |y_j|. A 16-bit output adds half a
unit in its last place of |R0|. No factor is fitted to what the kernel returns.
"""
import numpy as np

from tests import moe_reference as MR
from tests.gemv_f32_reference import _silu_d
from tests.xq_reference import _silu

U = 2.0 ** -24
REL = 2.0 ** -9


def coeff(K):
    return REL + 130 * ((K + 127) // 128) * U


def reference(x, idx, w, Wgu, Wdn, out_bits=24):
    """x fp32 [T, H], idx int [T, k], w fp32 [T, k], Wgu E x [H, 2I], Wdn E x [I, H] float64 -> (R0, tol)"""
    T, H = x.shape
    E, inter = len(Wgu), Wdn[0].shape[0]
    r0 = MR.block(x, idx, w, Wgu, Wdn, (0, False), False)[0]
    x64 = x.astype(np.float64)
    c_h, c_i = coeff(H), coeff(inter)
    absgu, absdn = [np.abs(m) for m in Wgu], [np.abs(m) for m in Wdn]
    A = np.zeros((T, H))
    for t in range(T):
        mag_sum = np.zeros(H)
        for j in range(idx.shape[1]):
            e = int(idx[t, j])
            if not 0 <= e < E:
                continue
            gu, a_gu = x64[t] @ Wgu[e], c_h * (np.abs(x64[t]) @ absgu[e])
            g, u, a_g, a_u = gu[:inter], gu[inter:], a_gu[:inter], a_gu[inter:]
            h = _silu(g) * u
            a_h = (np.abs(_silu_d(g)) + 0.5 * a_g) * a_g * np.abs(u) + np.abs(_silu(g)) * a_u + a_g * a_u + 4 * U * np.abs(h)
            a_y = a_h @ absdn[e] + c_i * (np.abs(h) @ absdn[e])
            A[t] += abs(float(w[t, j])) * a_y
            mag_sum += abs(float(w[t, j])) * np.abs(h @ Wdn[e])
        A[t] += (idx.shape[1] + 1) * U * mag_sum
    return r0, A + (0.0 if out_bits == 24 else 2.0 ** -out_bits * np.abs(r0))
