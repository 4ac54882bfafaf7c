"""Float64 statement of the backward of the routed expert block (`qbits.moe_backward`, csrc/woq_moe_bwd.hip) and a
per-element tolerance that is derived, not measured.

`reference`: the block (tests/moe_reference.py's definition) written in torch float64 on the CPU over the dequantised
weights and differentiated by `torch.autograd`; no derivative is written out by hand.

`bound`: the kernel's error carried along the chain, every term from the kernel source. d = dh', s = SiLU, s' = SiLU'.
  a_g, a_u   the recomputed g and u come from the prompt form's product: moe_prompt_reference.coeff(H) (|x| @ |Wgu|).
  a_d        product 1 is the dense backward's tile (woq_bwd_tile.h) per block: woq_backward_reference.bound, i.e.
             2^-9 (|dOut| @ |Wd|^T) (two operand roundings to fp16, one of them doubled by the relative scale) +
             2^-22 n max|dOut_t| max|Wd| with n = planes H, the fp32 chain (both nibble planes of int8 in one chain) and
             max|Wd| over ALL experts: 2^E is one power of two per blob kind.
  a_h        moe_prompt_reference's: (|s'| + a_g / 2) a_g |u| + |s| a_u + a_g a_u + 4 U |h| (expf, divide, two products).
  dw         sum_i (|d| + a_d)(|h| + a_h) - |d| |h|, plus the fp32 sum: a thread's 8 ceil(I / 2048) fmas, the six
             butterfly steps and two adds of moe_bwd_act_kernel: n_dw U sum |d h|.
  a_s'       |s''| <= 1/2, so a_g / 2, plus (|g| + 4) U for s' = sg (1 + g (1 - sg)) in fp32 (the difference 1 - sg is
             absolute-exact to U and is multiplied by g).
  a_dg       |w| ((|d| + a_d)(|u| + a_u)(|s'| + a_s') - |d| |u| |s'|) + 4 U |dg| (three products by w, u, s').
  a_du       |w| ((|d| + a_d)(|s| + a_s) - |d| |s|) + 3 U |du|, a_s = (|s'| + a_g / 2) a_g + 3 U |s|.
  a_dx       product 2 on the fp16 image of [dg | du] (its rounding is one of the two operand roundings of 2^-9):
             (1 + 2^-9) (a_dgu @ |Wgu|^T) + 2^-9 (|dgu| @ |Wgu|^T) + 2^-22 planes 2 I max(|dgu| + a_dgu) max|Wgu|.
  dX         sum_j a_dx + (k + 1) U sum_j |dx_j|; a 16-bit output adds half a unit in its last place of |dX|.
No factor is fitted to what the kernel returns.
"""
import numpy as np
import torch

from tests import moe_prompt_reference as PR
from tests import woq_backward_reference as BR
from tests.gemv_f32_reference import _silu_d
from tests.xq_reference import _silu

U = 2.0 ** -24


def reference(x, idx, w, dout, Wgu, Wdn):
    """x, dout [T, H], idx int [T, k], w [T, k], Wgu E x [H, 2I], Wdn E x [I, H] float64 -> (dX [T, H], dw [T, k])"""
    E, inter = len(Wgu), Wdn[0].shape[0]
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    wt = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
    out = torch.zeros_like(xt)
    for e in range(E):
        tok, pos = np.nonzero(idx == e)
        if tok.size == 0:
            continue
        gu = xt[tok] @ torch.from_numpy(Wgu[e])
        y = (torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]) @ torch.from_numpy(Wdn[e])
        out = out.index_add(0, torch.from_numpy(tok), y * wt[tok, pos][:, None])
    (out * torch.tensor(np.asarray(dout, np.float64))).sum().backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()  # noqa: E731
    return zero(xt), zero(wt)


def bound(x, idx, w, dout, Wgu, Wdn, dX, planes=1, out_bits=24):
    """-> (tolerance of dX [T, H], tolerance of dw [T, k]); dX = the reference's, for the output rounding"""
    T, H = x.shape
    E, inter, k = len(Wgu), Wdn[0].shape[0], idx.shape[1]
    x64, d64, w64 = (np.asarray(a, np.float64) for a in (x, dout, w))
    max_dn, max_gu = max(np.abs(m).max() for m in Wdn), max(np.abs(m).max() for m in Wgu)
    n_dw = 8 * ((inter + 2047) // 2048) + 8
    bx, mag, bw = np.zeros((T, H)), np.zeros((T, H)), np.zeros((T, k))
    for e in range(E):
        tok, pos = np.nonzero(idx == e)
        if tok.size == 0:
            continue
        agu, adn = np.abs(Wgu[e]), np.abs(Wdn[e])
        gu, a_gu = x64[tok] @ Wgu[e], PR.coeff(H) * (np.abs(x64[tok]) @ agu)
        g, u, a_g, a_u = gu[:, :inter], gu[:, inter:], a_gu[:, :inter], a_gu[:, inter:]
        s, sd, au = _silu(g), np.abs(_silu_d(g)), np.abs(u)
        h = s * u
        a_h = (sd + 0.5 * a_g) * a_g * au + np.abs(s) * a_u + a_g * a_u + 4 * U * np.abs(h)
        go = d64[tok]
        d = go @ Wdn[e].T
        a_d = BR.REL * (np.abs(go) @ adn.T) + BR.ABS * planes * H * np.abs(go).max(1, keepdims=True) * max_dn
        ad = np.abs(d)
        bw[tok, pos] = ((ad + a_d) * (np.abs(h) + a_h) - ad * np.abs(h)).sum(1) + n_dw * U * (ad * np.abs(h)).sum(1)
        ws = np.abs(w64[tok, pos])[:, None]
        a_sd = 0.5 * a_g + (np.abs(g) + 4) * U
        a_s = (sd + 0.5 * a_g) * a_g + 3 * U * np.abs(s)
        dg, du = ws * ad * au * sd, ws * ad * np.abs(s)
        a_dg = ws * ((ad + a_d) * (au + a_u) * (sd + a_sd) - ad * au * sd) + 4 * U * dg
        a_du = ws * ((ad + a_d) * (np.abs(s) + a_s) - ad * np.abs(s)) + 3 * U * du
        dgu, a_dgu = np.concatenate([dg, du], 1), np.concatenate([a_dg, a_du], 1)
        a_dx = ((1 + BR.REL) * (a_dgu @ agu.T) + BR.REL * (dgu @ agu.T)
                + BR.ABS * planes * 2 * inter * (dgu + a_dgu).max(1, keepdims=True) * max_gu)
        np.add.at(bx, tok, a_dx)
        np.add.at(mag, tok, dgu @ agu.T)  # >= |dx|
    return bx + (k + 1) * U * mag + (0.0 if out_bits == 24 else 2.0 ** -out_bits * np.abs(dX)), bw
