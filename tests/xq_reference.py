"""Reference for the XQ activation format (csrc/woq_xq.h), the batch-1 GEMV over it (csrc/woq_gemv_xqs.h, launched from
csrc/woq_gemv_xq.hip) and the dense lm_head (csrc/woq_ops.hip lm_head_kernel): numpy, float64.

`encode` / `decode`: a bit-exact model of `xq_emit16` for finite inputs. Block b = values [16 b, 16 b + 16); e_b = the
frexp exponent of the block's largest magnitude (max|y| in [2^(e-1), 2^e)), clamped to [-100, 100], 0 for an all-zero
block; v = rint(y * 2^(21 - e)) (exact in float64; ties to even, like the kernel's fp32 add of 1.5 * 2^23), so
|v| <= 2^21 and |decode - y| <= 2^(e - 22) <= max|y| * 2^-21; v = s0 + 2^8 s1 + 2^16 s2 with s0, s1 in [-128, 127] and
s2 in [-32, 32]; u = 2^(e - 25); sx = fl32(sum of the block's v); decode = v * u * 16.

`gemv_f64`: the specification of one projection. `tolerance_terms` -> (A, B), from the reference alone:
  R0 = gemv_f64 on the exact fp32 input (times the input norm weight in float64): what the projection should return;
  R1 = gemv_f64 on decode(encode(fl32(x * g))): what the kernel is fed;
  A  = max|gemv_f32 - R1|: `gemv_f32` restates the kernel's own arithmetic — exact integer sums per 16-k block (per
       digit plane for the table types, whose tables are the kernel's integer ones), fp32 recombination, fp32 products
       with u and the scale, fp32 accumulation over a wave's tiles in K order, the lane quarters, the waves and the
       chained launches added in the kernel's order, then the fp32 epilogue;
  B  = max|R1 - R0|.
A test allows 4 x (A + B) against R0 and 4 x A against R1; the 4 is the margin the project gives its fp32 restatements
(tests/score_reference.py).

`geometry`: the launch shape `xq_geometry` / `xq_k_plan` (csrc/woq_gemv_xq.hip) pick, restated so that a test can say
which form its K selects.

lm_head: `lm_head_f64` (tests/score_reference.py's norm and weights), tolerance 4 x A with A from `lm_head_f32`, an all-fp32
restatement in the kernel's order.
"""
import numpy as np

from oracle import woq_oracle as orc
from tests import score_reference as S

F32 = np.float32


# ---- the format ---------------------------------------------------------------------------------------------------
def block_exponents(y):
    """e_b of every 16-value block of the fp32 vector y"""
    a = np.abs(np.asarray(y, F32).astype(np.float64)).reshape(-1, 16).max(axis=1)
    _, e = np.frexp(a)
    return np.where(a > 0, np.clip(e, -100, 100), 0).astype(np.int64)


def fixed_point(y):
    """-> (v int64 [nb, 16], e int64 [nb])"""
    y64 = np.asarray(y, F32).astype(np.float64).reshape(-1, 16)
    assert np.isfinite(y64).all(), "only finite inputs are specified"
    e = block_exponents(y)
    return np.rint(y64 * np.ldexp(1.0, 21 - e)[:, None]).astype(np.int64), e


def _digit(v):
    """low balanced base-256 digit of v (the low byte, sign-extended) and what is left"""
    s = ((v + 128) & 255) - 128
    return s, (v - s) >> 8


def encode(y):
    """fp32 [16 nb] -> (limbs int8 [nb, 3, 16], u fp32 [nb], sx fp32 [nb])"""
    v, e = fixed_point(y)
    s0, v1 = _digit(v)
    s1, s2 = _digit(v1)
    limbs = np.stack([s0, s1, s2], axis=1).astype(np.int8)
    return limbs, np.ldexp(1.0, e - 25).astype(F32), v.sum(axis=1).astype(F32)


def limb_values(limbs):
    lm = np.asarray(limbs).astype(np.int64)
    return lm[:, 0] + 256 * lm[:, 1] + 65536 * lm[:, 2]


def decode(limbs, u):
    """-> float64 [16 nb]"""
    return (limb_values(limbs) * (np.asarray(u, F32).astype(np.float64) * 16.0)[:, None]).reshape(-1)


def block_ssq(x):
    """float64 sums of squares of the 16-value blocks of fp32 x"""
    x64 = np.asarray(x, F32).astype(np.float64).reshape(-1, 16)
    return (x64 * x64).sum(axis=1)


SSQ_REL = 8 * 2.0 ** -24  # 16 fp32 squares and a 4-level fp32 butterfly against the float64 sum


# ---- geometry ------------------------------------------------------------------------------------------------------
def _one_launch(tiles_k, cb, smode, ndig):
    tpw = 8 if (tiles_k > 16 and cb == 1) else 4
    wide = cb == 2 and ndig == 3
    if wide and tiles_k > 32 and smode == 0:
        tpw = 8
    nw = (tiles_k + tpw - 1) // tpw
    return nw, tpw, 1 <= nw <= (8 if (cb * tpw > 8 or wide) else 16)


def geometry(K, epi=0, smode=0, ndig=0):
    """-> list of chained launches (first tile, tiles, waves, tiles per wave template, [tiles of each wave]); [] = refused"""
    tiles_k, cb = K // 128, 2 if epi == 1 else 1
    chunks = 0
    if _one_launch(tiles_k, cb, smode, ndig)[2]:
        chunks = 1
    elif epi == 0:
        for s in range(2, 9):
            if _one_launch((tiles_k + s - 1) // s, cb, smode, ndig)[2]:
                chunks = s
                break
    if chunks == 0:
        return []
    per, out = (tiles_k + chunks - 1) // chunks, []
    for c in range(chunks):
        begin = c * per
        count = min(per, tiles_k - begin)
        if count <= 0:
            break
        nw, tpw, ok = _one_launch(count, cb, smode, ndig)
        assert ok
        base, rem = divmod(count, nw)
        out.append((begin, count, nw, tpw, [base + (1 if w < rem else 0) for w in range(nw)]))
    return out


# ---- the projection ------------------------------------------------------------------------------------------------
def rms_inv(x, eps):
    x64 = np.asarray(x, F32).astype(np.float64)
    return 1.0 / np.sqrt((x64 * x64).mean() + float(eps))


def _silu(g):
    return g / (1.0 + np.exp(-g))


def gemv_f64(x, W_deq64, inv=1.0, bias=None, residual=None, epi=0):
    """x [K] (float64, or fp32 taken exactly), W_deq64 [K, N]; epi 1: columns interleaved in 16-column tiles gate, up,
    gate, up, ... (runtime.fuse_gate_up), result [N / 2] = SiLU(gate) * up"""
    y = (np.asarray(x, np.float64) @ W_deq64) * inv
    if bias is not None:
        y = y + np.asarray(bias, F32).astype(np.float64)
    if epi == 1:
        y = y.reshape(-1, 2, 16)
        y = (_silu(y[:, 0, :]) * y[:, 1, :]).reshape(-1)
    if residual is not None:
        y = y + np.asarray(residual, F32).astype(np.float64)
    return y


TABLE_SCALE = {(orc.W_NF4, 3): 4194304.0, (orc.W_NF4, 2): 32512.0, (orc.W_FP4_E2M1, 1): 2.0, (orc.W_FP4_E2M1_BNB, 2): 192.0}


def table_planes(wtype, ndig):
    """-> (int64 [ndig, 16] balanced digits of rint(table * S), 16 / S): the kernel's digit planes (lut_args_for)"""
    S_ = TABLE_SCALE[(wtype, ndig)]
    v = np.rint(orc.LUTS[wtype].astype(np.float64) * S_).astype(np.int64)
    planes = []
    for _ in range(ndig):
        d, v = _digit(v)
        planes.append(d)
    assert (v == 0).all()
    return np.stack(planes), F32(16.0 / S_)


def _fma(a, b, c):
    """fp32 fused multiply-add (the product of two fp32 values is exact in float64)"""
    return (a.astype(np.float64) * np.asarray(b, F32).astype(np.float64) + c.astype(np.float64)).astype(F32)


def _combine(d):
    """digit_combine: d [3, ...] exact digit sums -> fp32"""
    return ((d[2] * 65536.0).astype(F32).astype(np.float64) + (d[0] + 256.0 * d[1]).astype(F32).astype(np.float64)).astype(F32)


def gemv_f32(y, codes, scales_kn, zp_kn, launches, smode, inv32=F32(1), bias=None, residual=None, epi=0,
             table=None):
    """The kernel's arithmetic restated. y fp32 [K]: the vector that is converted; codes int64 [K, N]: signed int4 values,
    or table codes 0..15 with table = (planes, wmul); scales_kn fp32 [K, N] (each k's group scale as stored, widened);
    zp_kn int64 [K, N] or None; launches = geometry(...). -> fp32 [N] (epi 1: [N / 2])"""
    limbs, u, sx = encode(y)
    K, N = codes.shape
    lm = limbs.astype(np.float64)                                    # [nb, 3, 16]
    cb = codes.reshape(K // 16, 16, N)
    if table is None:
        planes_b = [16.0 * cb.astype(np.float64)]
        wmul = None
    else:
        planes_b = [p[cb].astype(np.float64) for p in table[0]]
        wmul = table[1]
    # f[b, n]: the recombined fp32 sum of block b against column n
    f = None
    for pb in reversed(planes_b):  # most significant plane first
        fj = _combine(np.einsum("bpk,bkn->pbn", lm, pb))
        f = fj if f is None else _fma(f, F32(256), fj)
    sc = scales_kn.reshape(K // 16, 16, N)[:, 0, :].astype(F32)       # one scale per block (groups are multiples of 32)
    if zp_kn is not None:
        z16 = (-16.0 * zp_kn.reshape(K // 16, 16, N)[:, 0, :]).astype(F32)
        f = _fma(z16, sx[:, None], f)
    ub = u[:, None]
    out = np.zeros(N, F32)
    for li, (begin, count, nw, tpw, per_wave) in enumerate(launches):
        acc = np.zeros(N, F32)
        t0 = begin
        for cnt in per_wave:
            tot = np.zeros((4, N), F32)  # one running sum per lane quarter
            for t in range(t0, t0 + cnt):
                b0, b1 = 8 * t + np.arange(4), 8 * t + 4 + np.arange(4)
                if smode == 0:
                    tot = _fma(sc[b0], _fma(f[b0], ub[b0], (f[b1] * ub[b1]).astype(F32)), tot)
                else:
                    tot = _fma((sc[b0] * ub[b0]).astype(F32), f[b0], _fma((sc[b1] * ub[b1]).astype(F32), f[b1], tot))
            if wmul is not None:
                tot = (tot * wmul).astype(F32)
            acc = (acc + ((tot[0] + tot[2]).astype(F32) + (tot[1] + tot[3]).astype(F32)).astype(F32)).astype(F32)
            t0 += cnt
        v = (acc * inv32).astype(F32) if li == 0 else acc
        if li == 0 and bias is not None:
            v = (v + np.asarray(bias, F32)).astype(F32)
        if epi == 1:
            v = v.reshape(-1, 2, 16)
            g, up = v[:, 0, :], v[:, 1, :]
            v = ((g / (F32(1) + np.exp(-g, dtype=F32))).astype(F32) * up).astype(F32).reshape(-1)
        if li == 0:
            out = v if residual is None else (v + np.asarray(residual, F32)).astype(F32)
        else:
            out = (v + out).astype(F32)
    return out


def inv_f32(x, eps):
    """the kernel's RMSNorm factor from fp32 block sums"""
    x = np.asarray(x, F32)
    ss = (x * x).reshape(-1, 16).sum(axis=1, dtype=F32).sum(dtype=F32)
    return (F32(1) / np.sqrt(ss / F32(x.size) + F32(eps), dtype=F32)).astype(F32)


def tolerance_terms(x, g, eps, W_deq64, restate, bias=None, residual=None, epi=0):
    """-> (R0, R1, A, B). g = the input norm weight or None (then no norm factor either); restate(y, inv32) -> gemv_f32"""
    x = np.asarray(x, F32)
    if g is None:
        y32, x_exact, inv, inv32 = x, x.astype(np.float64), 1.0, F32(1)
    else:
        g = np.asarray(g, F32)
        y32, x_exact = (x * g).astype(F32), x.astype(np.float64) * g.astype(np.float64)
        inv, inv32 = rms_inv(x, eps), inv_f32(x, eps)
    r0 = gemv_f64(x_exact, W_deq64, inv, bias, residual, epi)
    lm, u, _ = encode(y32)
    r1 = gemv_f64(decode(lm, u), W_deq64, inv, bias, residual, epi)
    a = float(np.abs(restate(y32, inv32).astype(np.float64) - r1).max())
    return r0, r1, a, float(np.abs(r1 - r0).max())


# ---- lm_head ---------------------------------------------------------------------------------------------------------
def lm_head_f64(hidden, norm_w, eps, W):
    """-> float64 logits [vocab]"""
    w64, _ = S.weights_f64(W)
    with np.errstate(invalid="ignore"):
        return (S.norm_f64(np.asarray(hidden, F32)[None, :], norm_w, eps) @ w64.T)[0]


def _butterfly(v):
    """wave_sum: xor-shuffle adds over the last axis (64 lanes), fp32"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(F32)
    return v[..., 0]


def lm_head_f32(hidden, norm_w, eps, W):
    """lm_head_kernel's arithmetic restated in fp32: thread t sums x^2 over t, t + 256, ... by fma, a butterfly per wave,
    the four waves in order; xn = x * inv * w; lane l of a row's wave runs one fma chain over the 8 elements at
    8 l + 512 s, then the butterfly"""
    w64, _ = S.weights_f64(W)
    x, nw = np.asarray(hidden, F32), np.asarray(norm_w, F32)
    H = x.size
    xp = np.zeros((H + 255) // 256 * 256, F32)
    xp[:H] = x
    ss = np.zeros(256, F32)
    for row in xp.reshape(-1, 256):
        ss = _fma(row, row, ss)
    part = _butterfly(ss.reshape(4, 64))
    tot = ((part[0] + part[1]).astype(F32) + part[2]).astype(F32) + part[3]
    inv = (F32(1) / np.sqrt(F32(tot) / F32(H) + F32(eps), dtype=F32)).astype(F32)
    xn = ((x * inv).astype(F32) * nw).astype(F32)
    Hp = (H + 511) // 512 * 512
    wp = np.zeros((w64.shape[0], Hp), F32)
    wp[:, :H] = w64.astype(F32)
    xnp = np.zeros(Hp, F32)
    xnp[:H] = xn
    wp, xnp = wp.reshape(-1, Hp // 512, 64, 8), xnp.reshape(Hp // 512, 64, 8)
    acc = np.zeros((w64.shape[0], 64), F32)
    for s_ in range(Hp // 512):
        for j in range(8):  # (lanes past the row's end add exact zeros)
            acc = _fma(wp[:, s_, :, j], xnp[s_, :, j], acc)
    return _butterfly(acc)


def lm_head_tolerance_terms(hidden, norm_w, eps, W):
    """A: the largest deviation of `lm_head_f32` from float64"""
    return float(np.abs(lm_head_f32(hidden, norm_w, eps, W).astype(np.float64) - lm_head_f64(hidden, norm_w, eps, W)).max())
