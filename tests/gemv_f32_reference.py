"""Reference for the fp32-activation decode GEMVs with their fused epilogues (csrc/woq_gemv_i8.hip gemv_tile_kernel,
csrc/woq_gemv.hip gemv_generic_kernel, csrc/woq_gemv_fp8.hip gemv_fp8_kernel + silu_mul_tiles_kernel), as
`woq_probe_gemv_f32` runs them: numpy, float64. Shared by tests/test_gemv_f32_reference_cpu.py (no GPU: the geometry the
case list claims, and what the tolerance band would catch) and tests/test_gpu_f32_gemv_kernel.py.

The operation (R0), per activation row: with y_k = x_k g_k (g = the RMSNorm weight, 1 without a norm) taken at
k' = shuffle[k] under act-order, inv = rsqrt(mean_k(x_k^2) + eps) (1 without a norm; the mean is over K, not Kpad),
    out_n = inv * sum_k y_k' W_deq[k, n] + bias_n + residual_n,
and for epi 1 SiLU(gate) * up over the interleaved 16-column tiles (gate tile, up tile, gate tile, ...) before the
residual. W_deq is the oracle's dequantisation of the blob.

R1 = the same in float64 with y replaced by what the matrix-core kernels convert it to: per wave slice (the K range one
wave owns, from the launch geometry restated below) round(fl32(y) * 2^(21 - e)) * 2^(e - 21), e = the frexp exponent of
the slice's largest |fl32(y)| clamped to [-100, 100] (0 for an all-zero slice). The tile kernel carries that integer as
three int8 limbs, the fp8 kernel as six base-16 digits: the same 22-bit integer. Everything after the conversion is exact
integer arithmetic inside a tile (fp8: exact products), so R1 needs no model of the matrix core. B = max|R1 - R0|; the
generic kernel multiplies in fp32, B = 0.

Tolerance of the tile and generic kernels: |out - R0| <= 4 (A + B), A = n_ops * 2^-24 * mag per output,
mag = |inv| (|y| . |W_deq|) + |bias| + |residual|, for epi 1 propagated through SiLU * mul in float64 (|d out| <=
(|SiLU'(gate)| + A_gate / 2) A_gate |up| + |SiLU(gate)| A_up + A_gate A_up, SiLU'' <= 1 / 2). n_ops = an upper bound of
the longest chain of fp32 roundings behind one output, counted from the kernel sources (`n_ops_tile`, `n_ops_generic`);
it charges every wave the launch's full TPW tiles although balanced slices may hold one fewer, charges operations that
happen to be exact (the add of a zero zero-point term, conversions of small integers), and adds parallel branches
serially:
  tile kernel, per 128-k tile and 64-k half (per-128 / per-column scales: one "half" per tile, the two MFMAs accumulate in
    int32): per digit plane limb_combine = 3 int -> float conversions + 2 fma, + 1 fma by 256 between planes (6 per
    plane); zero points: a second limb_combine (5), the product with -16 zp (1), its add or fma (1); the fma with the
    scale into the running sum (1). Then: the product with unsc (* wmul) (2), the lane-quarter fold of the batch-1
    per-32 form (1), the sum over the nw waves (nw), the norm factor (1 + its own error, below), bias (1), residual (1),
    SiLU * mul (exp, add, divide, multiply: 4). A chained launch repeats the chain per chunk (chunk c + 1 adds chunk c's
    output as its residual).
  norm factor: the sum of squares is a sum of non-negative terms, 4 fma per float4 (4 XJ = 2 TPW per lane), a 6-level
    wave sum and nw adds; its relative error halves through the square root; then divide by K, add eps, sqrt, divide (4).
  generic kernel: a wave's interleaved tiles kt = wid, wid + 4, ...: per tile 2 halves of 16 fma + 1 fma by the scale
    (34 per tile, ceil(tiles / 4) tiles); the lane-quarter reduce (2), 4 waves (4); with a norm the staged activation is
    x * fl32(inv * g) (2) and inv comes from Kpad / 256 fma per thread, a 6-level wave sum and 4 adds; bias, residual,
    SiLU * mul as above.
The 4 is the margin the project gives its fp32 restatements (tests/xq_reference.py, tests/score_reference.py).

Tolerance of the fp8 matrix-core kernel: |inv| 1e-5 (|y| . |W_deq|) + 1e-5 + 4 B — the project's bound from
test_fp8_weight_types_decode_kernel (measured 2e-6 / 4.6e-6, profiles/r04ah_fp8_decode.txt); its accumulator is not an
fp32 adder, so no chain count applies. Its epi 1 form (kernel + silu_mul_tiles_kernel) propagates that bound through
SiLU * mul like A.

Geometry: `geometry` restates gemv_tile_k_plan / gemv_tile_geometry and launch_tile_t's balanced slices,
`fp8_geometry` restates fp8_geometry and launch_fp8_t's, `predict_form` restates the dispatch of launch_gemv_from_header /
gemv_tile_max_rows and launch_gemv_fp8_engine / gemv_fp8_mfma_supported: (kernel, chained launches, waves, tiles per
wave) with kernel 0 = generic (1, 4, 0), 1 = tile, 2 = fp8 matrix-core — what `woq_probe_gemv_f32` reports.

Inputs (`CASES`, `build`): seed 0; weights RTN-quantised by the oracle from 0.05 N(0, 1); x ~ N(0, 1) with one element
times 30; norm weights 1 + 0.1 N(0, 1). N = 32 (gate/up: inter 48), so K alone selects the form.
"""
import functools
import math

import numpy as np

from oracle import woq_oracle as orc
from tests.test_xq_reference_cpu import special_inputs
from tests.xq_reference import _silu, gemv_f64, rms_inv

F32 = np.float32
U = 2.0 ** -24
EPS = 1e-5
GENERIC = (0, 1, 4, 0)
STYPE = {"fp32": orc.F32, "fp16": orc.F16, "bf16": orc.BF16}
TABLES = {"nf4": orc.W_NF4, "fp4_e2m1": orc.W_FP4_E2M1}
FP8 = {"fp8_e4m3": orc.W_FP8_E4M3, "fp8_e5m2": orc.W_FP8_E5M2}
G128, G32A = (128, False, "fp16"), (32, True, "fp32")  # the second selects SMODE 1, ASYM and S32


# ---- geometry --------------------------------------------------------------------------------------------------------
def _slices(begin, count, nw):
    base, rem = divmod(count, nw)
    return [base + (1 if w < rem else 0) for w in range(nw)]


def _tile_one(tiles_k, cb, smode):
    """gemv_tile_geometry -> (nw, tpw, covered)"""
    tpw = 8 if (tiles_k > 16 and not (cb == 2 and smode == 1)) else 4
    nw = (tiles_k + tpw - 1) // tpw
    return nw, tpw, nw <= (8 if cb * tpw > 8 else (12 if smode == 1 else 16))


def geometry(K, epi=0, smode=0, chainable=False):
    """the tile kernel's chained launches [(first tile, tiles, waves, tiles per wave, [tiles of each wave])]; [] = not
    covered (gemv_tile_k_plan: chunks == 0)"""
    tiles_k, cb = (K + 127) // 128, 2 if epi == 1 else 1
    chunks = 1 if _tile_one(tiles_k, cb, smode)[2] else 0
    if chunks == 0 and chainable:
        chunks = next((s for s in range(2, 9) if _tile_one((tiles_k + s - 1) // s, cb, smode)[2]), 0)
    if chunks == 0:
        return []
    per, out = (tiles_k + chunks - 1) // chunks, []
    for c in range(chunks):
        begin = c * per
        count = min(per, tiles_k - begin)
        if count <= 0:
            break
        nw, tpw, ok = _tile_one(count, cb, smode)
        assert ok
        out.append((begin, count, nw, tpw, _slices(begin, count, nw)))
    return out


def fp8_geometry(K):
    """the fp8 kernel's launch [(0, tiles, waves, tiles per wave, [tiles of each wave])]; [] = not covered"""
    tiles_k = (K + 127) // 128
    tpw = 8 if tiles_k > 64 else 4
    nw = (tiles_k + tpw - 1) // tpw
    if not 1 <= nw <= (12 if tpw == 8 else 16):
        return []
    return [(0, tiles_k, nw, tpw, _slices(0, tiles_k, nw))]


def tile_lds_bytes(M, nw, tpw, cb):
    ms, nrs = min(M, 4), (M + 3) // 4
    return nw * 512 + nw * 3 * ms * (tpw * 128 + 16) + nrs * nw * cb * 64 * 4 + nrs * nw * 4 * 4


def act_order_tile_ok(K, smode):
    """gemv_tile_max_rows' rule for an act-order int4 blob at batch 1 (epi 0): K % 4 == 0, one launch (the gather form
    copies the whole vector per launch, so no chain), and the launch's LDS plus the K fp32 copy (+ 16) within 150 KiB"""
    g = geometry(K, 0, smode, False)
    return K % 4 == 0 and len(g) == 1 and tile_lds_bytes(1, g[0][2], g[0][3], 1) + K * 4 + 16 <= 150 * 1024


def predict_form(c):
    """(kernel, chained launches, waves, tiles per wave) the dispatch picks for case c"""
    K, epi, smode = c["K"], c["epi"], smode_of(c)
    aligned = not c["misalign"] and K % 4 == 0
    if c["wname"] in FP8:
        g = fp8_geometry(K)
        ok = aligned and not c["shuffle"] and (smode == 1 or c["form"][0] in (-1, 128)) and g
        ok = ok and (epi != 1 or c["gu_tmp"])
        return (2, 1, g[0][2], g[0][3]) if ok else GENERIC
    chainable = epi == 0 and not c["norm"]
    g = geometry(K, epi, smode, chainable)
    ok = aligned and g and (c["form"][0] in (-1, 32, 64, 96) or (c["form"][0] // 128) & (c["form"][0] // 128 - 1) == 0)
    if c["shuffle"]:
        ok = ok and c["wname"] == "int4_clip" and c["M"] == 1 and act_order_tile_ok(K, smode)
    return (1, len(g), g[0][2], g[0][3]) if ok else GENERIC


def smode_of(c):
    return 1 if c["form"][0] in (32, 64, 96) else 0


def slice_bounds(launches, K):
    """element ranges [k0, k1) of every wave slice of every chained launch"""
    out = []
    for begin, _, _, _, per_wave in launches:
        t0 = begin
        for cnt in per_wave:
            out.append((min(t0 * 128, K), min((t0 + cnt) * 128, K)))
            t0 += cnt
    return out


# ---- roundings behind one output -------------------------------------------------------------------------------------
def inv_ops(adds):
    return math.ceil(adds / 2) + 4


def n_ops_tile(launches, smode, asym, ndig, norm, bias, residual, epi, M=1):
    n = 0
    for _, _, nw, tpw, _ in launches:
        halves = 2 if smode == 1 else 1
        per_tile = halves * (6 * max(ndig, 1) + (7 if asym else 0) + 1)
        n += tpw * per_tile + 2 + (1 if (smode == 1 and M == 1) else 0) + nw + 1  # ... + the chained launch's add
    if norm:
        nw, tpw = launches[0][2], launches[0][3]
        n += 1 + inv_ops(2 * tpw + 6 + nw)
    return n + (1 if bias else 0) + (1 if residual else 0) + (4 if epi == 1 else 0)


def n_ops_generic(K, norm, bias, residual, epi):
    tiles, kpad = (K + 127) // 128, (K + 127) // 128 * 128
    n = (tiles + 3) // 4 * 34 + 2 + 4
    if norm:
        n += 2 + inv_ops(kpad // 256 + 6 + 4)
    return n + (1 if bias else 0) + (1 if residual else 0) + (4 if epi == 1 else 0)


# ---- the operation ---------------------------------------------------------------------------------------------------
def activation(x, g, shuffle):
    """-> (y32 fl32(x g) [M, K] at shuffle[k], y64 exact [M, K] at shuffle[k])"""
    x = np.asarray(x, F32)
    if g is None:
        y32, y64 = x, x.astype(np.float64)
    else:
        y32, y64 = (x * g).astype(F32), x.astype(np.float64) * np.asarray(g, F32).astype(np.float64)
    if shuffle is not None:
        y32, y64 = y32[:, shuffle], y64[:, shuffle]
    return y32, y64


def inv_rows(x, g, eps=EPS, K_mean=None):
    """per-row RMSNorm factor (1 without a norm); K_mean: what the sum of squares is divided by (default K)"""
    x = np.asarray(x, F32)
    if g is None:
        return np.ones(x.shape[0])
    if K_mean is None:
        return np.array([rms_inv(r, eps) for r in x])
    x64 = x.astype(np.float64)
    return 1.0 / np.sqrt((x64 * x64).sum(axis=1) / K_mean + float(eps))


def convert(y32, bounds):
    """the matrix-core kernels' fixed point, per wave slice: float64 [M, K]"""
    y = np.asarray(y32, F32).astype(np.float64)
    out = np.zeros_like(y)
    for m in range(y.shape[0]):
        for k0, k1 in bounds:
            if k1 <= k0:
                continue
            amax = np.abs(y[m, k0:k1]).max()
            e = int(np.clip(np.frexp(amax)[1], -100, 100)) if (amax > 0 and np.isfinite(amax)) else 0
            out[m, k0:k1] = np.rint(y[m, k0:k1] * 2.0 ** (21 - e)) * 2.0 ** (e - 21)
    return out


def outputs(y64, W64, inv, bias=None, residual=None, epi=0):
    """rows y64 [M, K] -> float64 [M, n_out]"""
    res = [None] * len(y64) if residual is None else residual
    return np.stack([gemv_f64(y, W64, float(i), bias, r, epi) for y, i, r in zip(y64, inv, res)])


def _silu_d(g):
    s = 1.0 / (1.0 + np.exp(-g))
    return s * (1.0 + g * (1.0 - s))


def band(rel, y64, W64, inv, bias=None, residual=None, epi=0, absolute=0.0):
    """rel * mag (+ absolute) per output, through SiLU * mul for epi 1: float64 [M, n_out]"""
    inv = np.abs(np.asarray(inv, np.float64))[:, None]
    lin = inv * (np.abs(y64) @ np.abs(W64))
    if bias is not None:
        lin = lin + np.abs(np.asarray(bias, F32).astype(np.float64))
    a = rel * lin + absolute
    if epi == 1:
        v = (y64 @ W64) * inv
        if bias is not None:
            v = v + np.asarray(bias, F32).astype(np.float64)
        v, a = v.reshape(len(y64), -1, 2, 16), a.reshape(len(y64), -1, 2, 16)
        gate, up, ag, au = v[:, :, 0], v[:, :, 1], a[:, :, 0], a[:, :, 1]
        a = ((np.abs(_silu_d(gate)) + 0.5 * ag) * ag * np.abs(up) + np.abs(_silu(gate)) * au + ag * au).reshape(len(y64), -1)
    if residual is not None:
        a = a + rel * np.abs(np.asarray(residual, F32).astype(np.float64))
    return a


def terms(c, d, x=None):
    """-> dict(r0, r1, A, B, tol [M, n_out], n_ops, form, launches). c = the case, d = build(c), x = other activation
    rows than the case's own (special inputs)"""
    K, epi = c["K"], c["epi"]
    x = d["x"] if x is None else np.asarray(x, F32)
    g, bias, res = d["g"], d["bias"], d["residual"]
    form = predict_form(c)
    y32, y64 = activation(x, g, d["shuffle"])
    inv = inv_rows(x, g)
    r0 = outputs(y64, d["W64"], inv, bias, res, epi)
    if form[0] == 0:
        launches, r1 = [], r0
        n = n_ops_generic(K, c["norm"], c["bias"], c["residual"] != "none", epi)
    else:
        launches = fp8_geometry(K) if form[0] == 2 else geometry(K, epi, smode_of(c), epi == 0 and not c["norm"])
        r1 = outputs(convert(y32, slice_bounds(launches, K)), d["W64"], inv, bias, res, epi)
        n = n_ops_tile(launches, smode_of(c), c["form"][1], d["ndig"], c["norm"], c["bias"], c["residual"] != "none", epi,
                       c["M"])
    B = float(np.abs(r1 - r0).max())
    if form[0] == 2:
        n = 0
        A = band(1e-5, y64, d["W64"], inv, None, None, epi, absolute=1e-5)
        tol = A + 4 * B
    else:
        A = band(n * U, y64, d["W64"], inv, bias, res, epi)
        tol = 4 * (A + B)
    return dict(r0=r0, r1=r1, A=A, B=B, tol=tol, n_ops=n, form=form, launches=launches, inv=inv, y64=y64, y32=y32)


# ---- the cases -------------------------------------------------------------------------------------------------------
def case(name, K, expect, form=G128, wname="int4_clip", cname="fp32", epi=0, norm=False, residual="none", bias=False,
         M=1, act="fp32", shuffle=False, misalign=False, gu_tmp=False, N=32):
    """residual: "none" | "alias" (the engine's: residual = out) | "separate"; N: output columns (epi 1: inter)"""
    return dict(name=name, K=K, expect=expect, form=form, wname=wname, cname=cname, epi=epi, norm=norm, residual=residual,
                bias=bias, M=M, act=act, shuffle=shuffle, misalign=misalign, gu_tmp=gu_tmp, N=N)


# the largest K whose act-order launch the tile kernel takes and the next K (a multiple of 4) it does not: the whole-vector
# copy (4 K + 16 bytes) fits beside the launch's own LDS at every K one launch covers, so the rule that binds is "one
# launch" — test_gemv_f32_reference_cpu.py derives both from `act_order_tile_ok`
ACT_ORDER_LAST_K, ACT_ORDER_NEXT_K = 16384, 16388
F8_128, F8_32, F8_COL = (128, False, "fp16"), (32, False, "fp32"), (-1, False, "bf16")

CASES = [
    # ---- tile kernel, int4 ----
    case("tile K2048 norm", 2048, (1, 1, 4, 4), norm=True),
    case("tile K2176 norm", 2176, (1, 1, 3, 8), norm=True),  # slices 6 / 6 / 5
    case("tile K4096 norm", 4096, (1, 1, 4, 8), norm=True),
    case("tile K4096 norm M5", 4096, (1, 1, 4, 8), norm=True, M=5),
    case("tile K11008 residual", 11008, (1, 1, 11, 8), residual="alias"),
    case("tile K16384 norm", 16384, (1, 1, 16, 8), norm=True),
    case("tile K16512 norm -> generic", 16512, GENERIC, norm=True),
    case("tile K16512 residual chained", 16512, (1, 2, 9, 8), residual="alias"),
    case("tile K4128 g32a", 4128, (1, 1, 5, 8), form=G32A),  # 33 tiles, the last holds one 32-k block
    case("tile K4128 g32a norm", 4128, (1, 1, 5, 8), form=G32A, norm=True, bias=True, residual="separate"),
    case("tile K12288 g32a norm", 12288, (1, 1, 12, 8), form=G32A, norm=True),
    case("tile K12416 g32a norm -> generic", 12416, GENERIC, form=G32A, norm=True),
    # ---- gate/up (CB = 2), with norm ----
    case("gate/up K2048", 2048, (1, 1, 4, 4), epi=1, norm=True, N=48),
    case("gate/up K4096", 4096, (1, 1, 4, 8), epi=1, norm=True, N=48),  # 512 threads
    case("gate/up K8192", 8192, (1, 1, 8, 8), epi=1, norm=True, N=48),
    case("gate/up K8320 -> generic", 8320, GENERIC, epi=1, norm=True, N=48),
    case("gate/up K6144 g32a", 6144, (1, 1, 12, 4), form=G32A, epi=1, norm=True, N=48),
    case("gate/up K6272 g32a -> generic", 6272, GENERIC, form=G32A, epi=1, norm=True, N=48),
    # ---- table types ----
    case("nf4 K4096 norm", 4096, (1, 1, 4, 8), wname="nf4", norm=True),
    case("nf4 K4096 gate/up", 4096, (1, 1, 4, 8), wname="nf4", epi=1, norm=True, N=48),
    case("fp4_e2m1 K4096 norm", 4096, (1, 1, 4, 8), wname="fp4_e2m1", norm=True),
    case("fp4_e2m1 K4096 gate/up", 4096, (1, 1, 4, 8), wname="fp4_e2m1", epi=1, norm=True, N=48),
    # ---- act-order ----
    case("act-order K4096 g128 fp32", 4096, (1, 1, 4, 8), norm=True, residual="separate", shuffle=True),
    case("act-order K4096 g128 bf16", 4096, (1, 1, 4, 8), norm=True, residual="separate", shuffle=True, act="bf16"),
    case("act-order K4096 g32a fp32", 4096, (1, 1, 4, 8), form=G32A, norm=True, residual="separate", shuffle=True),
    case("act-order K4096 g32a bf16", 4096, (1, 1, 4, 8), form=G32A, norm=True, residual="separate", shuffle=True,
         act="bf16"),
    case("act-order K16384 last", ACT_ORDER_LAST_K, (1, 1, 16, 8), norm=True, residual="separate", shuffle=True),
    case("act-order K16388 -> generic", ACT_ORDER_NEXT_K, GENERIC, norm=True, residual="separate", shuffle=True),
    # ---- the generic kernel on purpose ----
    case("generic K4098", 4098, GENERIC, form=(-1, False, "fp16"), norm=True, residual="separate"),
    case("generic misaligned rows", 4096, GENERIC, norm=True, misalign=True),
    # ---- fp8 (composite blob) ----
    case("fp8 K256 norm", 256, (2, 1, 1, 4), form=F8_128, wname="fp8_e4m3", norm=True),
    case("fp8 K4096 norm", 4096, (2, 1, 8, 4), form=F8_128, wname="fp8_e4m3", norm=True),
    case("fp8 K8192 norm", 8192, (2, 1, 16, 4), form=F8_128, wname="fp8_e4m3", norm=True),
    case("fp8 K8320 norm", 8320, (2, 1, 9, 8), form=F8_128, wname="fp8_e4m3", norm=True),  # slices 8 8 7 7 7 7 7 7 7
    case("fp8 K12288 norm", 12288, (2, 1, 12, 8), form=F8_128, wname="fp8_e4m3", norm=True),
    case("fp8 K11008 residual", 11008, (2, 1, 11, 8), form=F8_128, wname="fp8_e4m3", residual="alias"),
    case("fp8 K12416 -> generic", 12416, GENERIC, form=F8_128, wname="fp8_e4m3", norm=True, residual="separate"),
    case("fp8 K4096 g32", 4096, (2, 1, 8, 4), form=F8_32, wname="fp8_e4m3", norm=True),
    case("fp8 K11008 g32", 11008, (2, 1, 11, 8), form=F8_32, wname="fp8_e4m3", norm=True),
    case("fp8 e5m2 K4096", 4096, (2, 1, 8, 4), form=F8_COL, wname="fp8_e5m2", norm=True),
    case("fp8 gate/up K4096", 4096, (2, 1, 8, 4), form=F8_128, wname="fp8_e4m3", epi=1, norm=True, gu_tmp=True, N=48),
    case("fp8 gate/up K4096 no gu_tmp -> generic", 4096, GENERIC, form=F8_128, wname="fp8_e4m3", epi=1, norm=True, N=48),
]
# special inputs: one multi-wave K per kernel, with norm; ragged K so that the last slice is partial
SPECIAL = [
    case("special tile", 4128, (1, 1, 5, 8), form=G32A, norm=True, bias=True, residual="separate"),
    case("special generic", 4098, GENERIC, form=(-1, False, "fp16"), norm=True, bias=True, residual="separate"),
    case("special fp8", 4128, (2, 1, 9, 4), form=F8_32, wname="fp8_e4m3", norm=True, residual="separate"),
]
BY_NAME = {c["name"]: c for c in CASES + SPECIAL}
assert len(BY_NAME) == len(CASES) + len(SPECIAL)


def fuse_gate_up(gate, up):
    """[*, I] x 2 -> [*, 2 I], 16-column tiles interleaved (runtime.fuse_gate_up)"""
    lead, inter = gate.shape[:-1], gate.shape[-1]
    return np.ascontiguousarray(np.concatenate([gate.reshape(*lead, inter // 16, 1, 16),
                                                up.reshape(*lead, inter // 16, 1, 16)], axis=-2).reshape(*lead, 2 * inter))


@functools.lru_cache(maxsize=None)
def _weight(K, N, form, wname, cname, epi, shuffle):
    """-> dict(blob, W64 [K, cols], q, s, z, idx (raw g_idx), shuffle (activation index per weight row), ndig)"""
    group, asym, sname = form
    rng = np.random.default_rng(0)
    parts = []
    for _ in range(2 if epi == 1 else 1):
        w = (0.05 * rng.standard_normal((N, K))).astype(F32)
        if wname == "int4_clip":
            parts.append(orc.rtn_quantize(w, True, group, asym))
        elif wname in TABLES:
            parts.append(orc.rtn_quantize_table(w, True, group, TABLES[wname]) + (None,))
        else:
            parts.append(orc.rtn_quantize_fp8(w, True, group, FP8[wname]) + (None,))
    if epi == 1:
        q, s = fuse_gate_up(parts[0][0], parts[1][0]), fuse_gate_up(parts[0][1], parts[1][1])
        z = fuse_gate_up(parts[0][2], parts[1][2]) if asym else None
    else:
        q, s, z = parts[0]
    idx = shuf = None
    if shuffle:  # raw GPTQ g_idx in act-order positions, as test_act_order_decode_gather_vs_oracle builds it
        g = K if group == -1 else group
        idx = rng.permutation(np.arange(K, dtype=np.int32) // g).astype(np.int32)
        shuf = orc.convert_idx(idx, K, g)
    ct = {"fp32": 0, "bf16": 1}[cname]
    ndig = 0
    if wname == "int4_clip":
        blob = orc.repack(q, s, z, shuf, group, scale_type=STYPE[sname], compute_type=ct)
    elif wname in TABLES:
        blob = orc.repack_table(q, s, TABLES[wname], group, scale_type=STYPE[sname], compute_type=ct)
        ndig = 1 if wname == "fp4_e2m1" else (3 if cname == "fp32" else 2)
    else:
        blob = orc.repack_fp8(q, s, FP8[wname], None, group, scale_type=STYPE[sname], compute_type=ct)
    W = orc.dequantize_blob(blob)
    assert W.shape == (K, q.shape[1])
    return dict(blob=blob, W64=W.astype(np.float64), q=q, s=s, z=z, idx=idx, shuffle=shuf, ndig=ndig)


@functools.lru_cache(maxsize=None)
def _vectors(K, M, act):
    """x [M, K] (one element of every row times 30; rows of a batch at distinct scales), norm weight [K], bias [96],
    residual [M, 96]"""
    rng = np.random.Generator(np.random.PCG64(0).jumped())  # seed 0, a stream apart from the weights'
    x = rng.standard_normal((M, K)).astype(F32)
    for m in range(M):
        x[m, (K // 3 + 977 * m) % K] *= 30
        x[m] *= F32([1, 0.25, 3, 0.01, 7][m % 5])
    if act == "bf16":
        x = orc.bf16_round(x)
    g = (1 + 0.1 * rng.standard_normal(K)).astype(F32)
    return x, g, rng.standard_normal(96).astype(F32), rng.standard_normal((M, 96)).astype(F32)


def build(c):
    """the case's inputs: dict(x [M, K], g | None, bias | None, residual [M, n_out] | None, + _weight's entries)"""
    d = dict(_weight(c["K"], c["N"], c["form"], c["wname"], c["cname"], c["epi"], c["shuffle"]))
    x, g, b, r = _vectors(c["K"], c["M"], c["act"])
    cols = d["W64"].shape[1]
    n_out = cols // 2 if c["epi"] == 1 else cols
    d.update(x=x, g=g if c["norm"] else None, bias=b[:cols] if c["bias"] else None,
             residual=r[:, :n_out] if c["residual"] != "none" else None, n_out=n_out)
    return d


def special_rows(c):
    """name -> x [1, K]: the special activation vectors of case c (a SPECIAL case)"""
    K = c["K"]
    base = _vectors(K, 1, "fp32")[0][0].copy()
    base[K // 3] /= 30
    launches = fp8_geometry(K) if c["wname"] in FP8 else geometry(K, c["epi"], smode_of(c), False)
    out = {"all zero": np.zeros(K, F32)}
    z = base.copy()
    if c["expect"][0] != 0:
        bounds = slice_bounds(launches, K)
        z[bounds[1][0]:bounds[1][1]] = 0
        assert bounds[-1][1] == K and (K - bounds[-1][0]) % 128 != 0  # the last slice is partial
    else:  # the generic kernel has no contiguous slices: wave 1 owns the interleaved tiles kt = 1, 5, 9, ...
        for kt in range(1, (K + 127) // 128, 4):
            z[kt * 128:(kt + 1) * 128] = 0
        assert K % 128 != 0  # the last tile is partial
    out["one slice zero"] = z
    p = base.copy()
    p[K - 3] *= 30
    out["x30 in the last, partial slice"] = p
    # special_inputs without its 1e30 block (the fp32 sum of squares overflows: the norm factor has no defined value);
    # 1e-35 stays (its square underflows in fp32 and float64 alike against eps = 1e-5)
    sp = np.delete(special_inputs().reshape(-1, 16), 22, axis=0).reshape(-1)
    e = base.copy()
    e[:sp.size] = sp
    out["format extremes"] = e
    return {k: v[None, :] for k, v in out.items()}
