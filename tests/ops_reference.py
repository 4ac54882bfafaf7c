"""Float64 references, tolerance bands, fp32 restatements and the case lists of the four element ops behind the C ABI
(csrc/woq_ops.hip: rmsnorm_kernel, rope_kernel, silu_mul_kernel, gelu_kernel; qbits.rmsnorm / rope / silu_mul / gelu):
numpy only. Shared by tests/test_ops_reference_cpu.py (no GPU: what the bands accept and what they reject) and
tests/test_gpu_ops_kernel.py.

The operations (float64, on the inputs exactly as stored):
  rmsnorm   x / sqrt(mean(x^2) + eps) * w over a row of d elements, rounded ONCE to the out type. This is the project's
            definition; HF's 16-bit module rounds before the product with w (test_ops_vs_oracle_and_hf_golden keeps that
            parity). eps is the fp32 value the kernel is handed, w the fp32 weight.
  rope      rotate_half: (a, b) = (x[i], x[i + D/2]) -> (a c - b s, b c + a s), c / s the fp32 table values the kernel
            is handed at row pos[token], widened to float64 — not recomputed angles.
  silu_mul  a / (1 + e^-a) * b.
  gelu      tanh form 0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3))); erf form 0.5 v (1 + erf(v / sqrt 2)), erf =
            math.erf.

Storage. Inputs are drawn in float64 and rounded to the tensor's type first (`to_storage`); the reference works on those
stored values, so input rounding is in no band. Outputs: `attn_reference.round_to` (nearest even), except that a value
past the format's last rounding boundary goes to +-inf (`stored`): these kernels convert with a plain cast and do not
saturate, unlike the KV codecs round_to was written for (fp16: |y| >= 65520 -> inf). `half_ulp(y, fmt)` is half the
spacing of the out type at |y| (subnormal spacing below the smallest normal; fp32: 2^-150 there and nothing above it,
because the fp32 result of the last operation is stored as it is and that rounding is already counted).

Bands, u = 2^-24 (one correctly rounded fp32 operation). Every count below is read off the kernel's operation sequence;
no constant comes from a kernel's output. All conversions fp16 / bf16 -> fp32 are exact. fp32 division and sqrt are
correctly rounded (hipcc's default, no fast-math in csrc/Makefile), the library is built without fast-math, and fp32
subnormals are kept, so a result below 2^-126 carries an absolute 2^-149 (`SUB`) on top of each band.

ASSUMED, not documented: the ulp error of the device expf / tanhf / erff. No HIP math accuracy table ships with the
toolkit the library is built with, so the bands take the OpenCL full-profile limits the device math library is written
to: expf 3 ulp, tanhf 5 ulp, erff 16 ulp (`ULP_EXP`, `ULP_TANH`, `ULP_ERF`). One ulp of a result r is at most 2 u |r|.

  rmsnorm  band = K_RMS(d) u |ref| + half_ulp(out type), K_RMS(d) = m / 2 + 10, m = ceil(d / 256).
           Sum of squares: all terms >= 0, so roundings add relatively: m fma per thread, 6 shuffle adds, 3 LDS adds
           (m + 9). tot / d and + eps (2; eps >= 0, no cancellation). The square root halves the relative error carried in
           ((m + 11) / 2) and rounds once, 1 / . rounds once, v * inv and * w round once each: (m + 11) / 2 + 4 =
           m / 2 + 9.5, and 0.5 for the second-order terms. An all-zero row gives 0 * inv * w = +-0 exactly (band 0 +
           storage).
  rope     band = K_ROPE u (|a c| + |b s|) + SUB + half_ulp(storage) (second half: |b c| + |a s|), K_ROPE = 3.
           Two rounded products and a rounded sum, or one rounded product and one fma: at most 2 u (1 + u) (|a c| +
           |b s|) either way; 3 is attn_reference.rotate_error's constant. At position 0 (c = 1, s = 0) the result is
           a +- 0 = a: bit-identical for a != 0.
  silu_mul band = K_SILU u |ref| + half_ulp(storage) + SUB, K_SILU = 2 ULP_EXP + 3 = 9.
           e = expf(-a): 2 ULP_EXP u relative; 1 + e rounds once and e's error enters weighted e / (1 + e) <= 1; the
           division and the product round once each. For -a > log(FLT_MAX) = 88.7228 expf overflows, 1 + inf = inf,
           a / inf = -0 and the kernel returns -+0: there the band is |ref| itself (at most 89 |b| / FLT_MAX).
  gelu     band = K u (|v| + |ref|) + half_ulp(storage) + SUB, K_GELU_TANH = 8, K_GELU_ERF = 18.
           The |v| term is the cancellation in 1 + t for negative v: an absolute error dt in t = tanh / erf moves the
           result by |v| dt / 2 however small 1 + t is, so a purely relative band is wrong for this kernel.
           tanh form: z = c1 (v + c2 v v v): three products with fl32(c2) (4 u with the constant), the sum of two terms of
           one sign (1), the product with fl32(c1) (2): 7 u relative. |z tanh'(z)| <= 0.45, so that is 3.2 u in t; tanhf
           adds 2 ULP_TANH u |t| <= 10 u; 1 + t rounds once (<= 2 u). dr <= |v| / 2 (3.2 + 10 + 2) u + u |ref| (the last
           product) = 7.6 u |v| + u |ref| -> 8.
           erf form: x = v fl32(1 / sqrt 2) (2 u), |x erf'(x)| <= 0.49 (1 u in t), erff 2 ULP_ERF u = 32 u, 1 + t 2 u:
           |v| / 2 * 35 u + u |ref| = 17.5 u |v| + u |ref| -> 18.
           The float64 reference evaluates the same 1 + t and so carries 2^-53 |v|, 2^-29 of the band's |v| term.

`ratio(out, ref, band, fmt)` is |out - ref| / band per element; an infinite output of the reference's sign counts as
the distance from |ref| to the format's overflow boundary (0 past it), NaN must meet NaN. `inside(out, ref, b32, fmt)`
is the same band before the half ulp is added: the stored value must lie between the roundings of ref - b32 and
ref + b32, which for 16-bit storage is the rounded reference itself except next to a rounding boundary.

The fp32 restatements (`rmsnorm_f32`, `rope_f32`, `silu_mul_f32`, `gelu_f32`) replay the kernels' operation order in
numpy float32 (fma = a float64 product-and-add rounded once to fp32) and take the planted slips of the CPU test as
arguments.

Inputs: fixed seeds; `rmsnorm_inputs`, `rope_inputs`, `elementwise_inputs` are cached and their arrays read-only.
"""
import functools
import math

import numpy as np

from tests.attn_reference import FORMATS, round_to

F32 = np.float32
U = 2.0 ** -24
SUB = 2.0 ** -149
ULP_EXP, ULP_TANH, ULP_ERF = 3, 5, 16  # assumed: OpenCL full-profile limits (module docstring)
K_ROPE = 3
K_SILU = 2 * ULP_EXP + 3
K_GELU_TANH = 8
K_GELU_ERF = 18
LOG_FLT_MAX = 88.72283905206835
FLT_MAX = 3.4028234663852886e38
DTYPES = ("fp32", "fp16", "bf16")
# (mantissa bits, smallest normal exponent, first magnitude that rounds to infinity)
_FMT = {"fp32": (23, -126, FLT_MAX * (1 + 2.0 ** -25)), "fp16": (10, -14, 65520.0),
        "bf16": (7, -126, FORMATS["bf16"][2] * (1 + 2.0 ** -9))}


def k_rms(d):
    return (d + 255) // 256 / 2 + 10


# ---- storage ---------------------------------------------------------------------------------------------------------
def _bf16_bits(x32):
    """f32_to_bf16_bits of csrc/woq_device.h: nearest even, NaN kept quiet"""
    b = np.ascontiguousarray(x32, dtype=F32).view(np.uint32)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = (b + (0x7FFF + ((b >> 16) & 1))) >> 16
    return np.where(nan, (b >> 16) | 0x40, r).astype(np.uint16)


def to_bits(x, fmt):
    """x (float64 or float32 values) as the tensor's stored elements: float32 / float16 arrays, uint16 for bf16"""
    with np.errstate(over="ignore"):
        x32 = np.asarray(x, dtype=np.float64).astype(F32)
        if fmt == "fp32":
            return x32
        return x32.astype(np.float16) if fmt == "fp16" else _bf16_bits(x32)


def widen(bits, fmt):
    """stored elements -> float64, exactly"""
    if fmt == "bf16":
        return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32).astype(np.float64)
    return np.asarray(bits).astype(np.float64)


def to_storage(x, fmt):
    """the float64 values a tensor of type fmt holds after x was written to it (the device's fp32 -> fmt cast)"""
    return widen(to_bits(x, fmt), fmt)


def stored(y, fmt):
    """the float64 result y rounded once to fmt, nearest even, overflow to +-inf (these kernels do not saturate)"""
    y = np.asarray(y, dtype=np.float64)
    if fmt == "fp32":
        with np.errstate(over="ignore"):
            return y.astype(F32).astype(np.float64)
    r = round_to(y, fmt)
    r = np.where(np.abs(y) >= _FMT[fmt][2], np.copysign(np.inf, y), r)
    return np.where(np.isnan(y), np.nan, r)


def half_ulp(y, fmt):
    """half the spacing of fmt at |y|; fp32: only the subnormal half step (module docstring)"""
    m, emin, _ = _FMT[fmt]
    y = np.abs(np.asarray(y, dtype=np.float64))
    if fmt == "fp32":
        return np.full(y.shape, 2.0 ** -150)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(y))
    e = np.where(np.isfinite(e), np.maximum(e, emin), emin)
    return 0.5 * np.exp2(e - m)


def _with_storage(ref, b32, fmt):
    """the fp32 band b32 plus half an ulp of the out type at the largest magnitude the fp32 value can have"""
    mag = np.where(np.isfinite(ref), np.abs(ref) + b32, 0.0)
    return b32 + half_ulp(mag, fmt)


def ratio(out, ref, band, fmt):
    """|out - ref| / band per element (module docstring); inf where a NaN, a sign of infinity or an inf is wrong"""
    out, ref, band = (np.asarray(t, dtype=np.float64) for t in (out, ref, band))
    edge = _FMT[fmt][2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(out - ref)
        inf_out = np.isinf(out)
        same = np.sign(out) == np.sign(ref)
        err = np.where(inf_out, np.where(same, np.maximum(edge - np.abs(ref), 0.0), np.inf), err)
        r = np.where(err == 0.0, 0.0, err / band)
    nan_ref = np.isnan(ref)
    r = np.where(nan_ref, np.where(np.isnan(out), 0.0, np.inf), r)
    return np.where(~nan_ref & np.isnan(out), np.inf, r)


def inside(out, ref, b32, fmt):
    """per element: out lies in [stored(ref - b32), stored(ref + b32)]. Rounding is monotone, so an fp32 value within b32
    of ref can be stored nowhere else; away from a rounding boundary of fmt both ends are the rounded reference itself,
    which makes this the sharper statement of a 16-bit band. NaN must meet NaN."""
    out, ref, b32 = (np.asarray(t, dtype=np.float64) for t in (out, ref, b32))
    with np.errstate(invalid="ignore"):
        ok = (out >= stored(ref - b32, fmt)) & (out <= stored(ref + b32, fmt))
    return np.where(np.isnan(ref), np.isnan(out), ok)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


# ---- rmsnorm ---------------------------------------------------------------------------------------------------------
RMS_D = (1, 7, 64, 255, 256, 257, 1000, 4096, 8200)
RMS_ROWS = (1, 3, 65)
RMS_EPS = (1e-5, 1e-6)
RMS_TYPES = (("fp32", "fp32"), ("fp16", "fp16"), ("bf16", "bf16"), ("fp32", "bf16"), ("bf16", "fp32"))
RMS_FAMILIES = ("n0", "n-", "n+", "zero", "onehot", "const", "lastbig")


def rms_big_exponent(fmt):
    """the e of the N(0, 1) 2^+-e rows: 20, and 12 for fp16 storage, which holds neither 2^20 nor most of 2^-20 N(0, 1)"""
    return 12 if fmt == "fp16" else 20


@functools.lru_cache(maxsize=None)
def rmsnorm_inputs(d, in_fmt):
    """(x [65, d] as stored in in_fmt, w [d] fp32), float64 values; row r is family RMS_FAMILIES[r % 7]; a call with
    fewer rows takes the first ones. Seed: d."""
    rng = np.random.default_rng(1000 + d)
    e = rms_big_exponent(in_fmt)
    x = np.zeros((65, d))
    for r in range(65):
        fam = RMS_FAMILIES[r % 7]
        g = rng.standard_normal(d)
        if fam == "n0":
            x[r] = g
        elif fam == "n-":
            x[r] = g * 2.0 ** -e
        elif fam == "n+":
            x[r] = g * 2.0 ** e
        elif fam == "onehot":
            x[r, (37 * r) % d] = -1.5
        elif fam == "const":
            x[r] = 0.75
        elif fam == "lastbig":
            x[r] = g
            x[r, d - 1] = 1000.0
    w = (1 + 0.1 * rng.standard_normal(d)).astype(F32).astype(np.float64)
    return _frozen(to_storage(x, in_fmt), w)


def rmsnorm_ref(x, w, eps):
    """(ref, fp32 band) float64 [rows, d]; eps is rounded to fp32 as the ABI's float argument is"""
    eps = float(F32(eps))
    d = x.shape[-1]
    ref = x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + eps) * w
    return ref, k_rms(d) * U * np.abs(ref)


def rmsnorm_band(ref, b32, out_fmt):
    return _with_storage(ref, b32, out_fmt)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def rmsnorm_f32(x, w, eps, eps_scale=1.0, mean_padded=False, w_shift=0):
    """rmsnorm_kernel in numpy float32 -> the fp32 value before the store, [rows, d]. Slips: eps_scale (0 drops eps),
    mean_padded (divide by 256 ceil(d / 256)), w_shift (weight index off by that much)."""
    rows, d = x.shape
    m = (d + 255) // 256
    xp = np.zeros((rows, m * 256), dtype=F32)
    xp[:, :d] = x.astype(F32)
    xp = xp.reshape(rows, m, 256)
    ss = np.zeros((rows, 256), dtype=F32)
    for j in range(m):  # thread t: elements t, t + 256, ...
        ss = _fma(xp[:, j], xp[:, j], ss)
    ss = ss.reshape(rows, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):  # wave_sum: xor butterfly
        ss = (ss + ss[:, :, lane ^ o]).astype(F32)
    part = ss[:, :, 0]
    tot = ((part[:, 0] + part[:, 1]).astype(F32) + part[:, 2]).astype(F32) + part[:, 3]
    n = F32(m * 256 if mean_padded else d)
    wv = np.roll(w, w_shift).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):  # eps dropped: a zero row divides by zero
        inv = F32(1.0) / np.sqrt((tot.astype(F32) / n + F32(F32(eps) * F32(eps_scale))).astype(F32)).astype(F32)
        return ((x.astype(F32) * inv[:, None].astype(F32)).astype(F32) * wv[None, :]).astype(F32)


# ---- rope ------------------------------------------------------------------------------------------------------------
ROPE_SHAPES = ((1, 1, 2), (1, 1, 6), (5, 3, 128), (4, 32, 64), (7, 2, 6))
ROPE_POS = (63, 0, 17, 17, 1, 40, 2)
ROPE_MAX_POS = 64


@functools.lru_cache(maxsize=None)
def rope_tables(D):
    """cos, sin float32 [64, D / 2]: angles p * 10000^(-2 i / D) in float64, stored fp32"""
    inv = 10000.0 ** (-2.0 * np.arange(D // 2) / D)
    ang = np.arange(ROPE_MAX_POS, dtype=np.float64)[:, None] * inv[None, :]
    return _frozen(np.cos(ang).astype(F32), np.sin(ang).astype(F32))


@functools.lru_cache(maxsize=None)
def rope_inputs(shape, fmt):
    """(x [tokens, heads, D] as stored in fmt (float64 values, N(0, 1): no zeros), pos int32 [tokens])"""
    t, h, D = shape
    rng = np.random.default_rng(2000 + 131 * t + 17 * h + D)
    x = to_storage(rng.standard_normal(shape), fmt)
    assert np.all(x != 0)
    return _frozen(x, np.array(ROPE_POS[:t], dtype=np.int32))


def rope_ref(x, pos, cos, sin):
    """(ref, fp32 band) float64, x's shape"""
    h = x.shape[-1] // 2
    c, s = cos.astype(np.float64)[pos][:, None, :], sin.astype(np.float64)[pos][:, None, :]
    a, b = x[..., :h], x[..., h:]
    ref = np.concatenate([a * c - b * s, b * c + a * s], axis=-1)
    mag = np.concatenate([np.abs(a * c) + np.abs(b * s), np.abs(b * c) + np.abs(a * s)], axis=-1)
    return ref, K_ROPE * U * mag + SUB


def rope_band(ref, b32, fmt):
    return _with_storage(ref, b32, fmt)


def rope_f32(x, pos, cos, sin, fma=False, flip_sign=False, swap_halves=False, prev_pos=False):
    """rope_kernel in numpy float32 -> the fp32 values before the store. fma: the contracted form. Slips: flip_sign (of
    the sine terms), swap_halves (a and b exchanged), prev_pos (token t rotated by pos[t - 1])."""
    h = x.shape[-1] // 2
    p = np.roll(pos, 1) if prev_pos else pos
    c, s = cos[p][:, None, :].astype(F32), sin[p][:, None, :].astype(F32)
    if flip_sign:
        s = -s
    a, b = x[..., :h].astype(F32), x[..., h:].astype(F32)
    if swap_halves:
        a, b = b, a
    if fma:
        lo, hi = _fma(a, c, -(b * s)), _fma(b, c, a * s)
    else:
        lo, hi = a * c - b * s, b * c + a * s
    return np.concatenate(np.broadcast_arrays(lo, hi), axis=-1).astype(F32)


# ---- silu_mul and gelu -----------------------------------------------------------------------------------------------
ELEM_N = (1, 255, 256, 257, 524288, 524289, 1048579)
GRID_SPAN = 2048 * 256  # elements one trip of the grid-stride loop covers
_MAGS = (0.0, 1e-30, 0.5, 3.0, 5.0, 8.0, 12.0, 20.0, 87.0, 88.5, 89.0, 104.0, 1e4)
SPECIALS = tuple(s * m for m in _MAGS for s in (1.0, -1.0)) + (float("nan"),)
OVERFLOW_PAIR = (300.0, 300.0)  # silu(300) * 300 = 9e4: inf in fp16, finite in fp32 and bf16


def special_slots(n):
    """the start indices at which the specials are planted in a vector of n: the first block, the last block, and
    straddling the end of the grid-stride loop's first trip — each where it fits"""
    k = len(SPECIALS)
    starts = [0]
    if n >= 2 * k:
        starts.append(n - k)
    if n >= GRID_SPAN + 2 * k:
        starts.append(GRID_SPAN - k // 2)
    return starts


@functools.lru_cache(maxsize=8)
def elementwise_inputs(n, fmt):
    """(v, b) as stored in fmt, float64 values [n]: N(0, 1) * {0.01, 1, 8}[i % 3]; v carries the specials (gelu's x,
    silu_mul's gate), b (silu_mul's up) a NaN and the overflow pair beside them"""
    rng = np.random.default_rng(3000 + n)
    scale = np.array([0.01, 1.0, 8.0])[np.arange(n) % 3]
    v, b = rng.standard_normal(n) * scale, rng.standard_normal(n) * scale
    k = len(SPECIALS)
    for s in special_slots(n):
        m = min(k, n - s)
        v[s:s + m] = SPECIALS[:m]
    if n >= 4 * k:
        v[k], b[k] = OVERFLOW_PAIR
        b[k + 1] = np.nan
    return _frozen(to_storage(v, fmt), to_storage(b, fmt))


def silu_mul_ref(a, b):
    """(ref, fp32 band) float64"""
    with np.errstate(over="ignore", invalid="ignore"):
        ref = a / (1.0 + np.exp(-a)) * b
        band = K_SILU * U * np.abs(ref) + SUB
        band = np.where(-a > LOG_FLT_MAX, np.maximum(band, np.abs(ref) + SUB), band)
    return ref, band


def silu_mul_band(ref, b32, fmt):
    return _with_storage(ref, b32, fmt)


def silu_mul_f32(a, b, b_shift=0):
    """silu_mul_kernel in numpy float32. Slip: b_shift (the neighbouring element's b)."""
    a, b = a.astype(F32), np.roll(b, b_shift).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (a / (F32(1.0) + np.exp(-a)) * b).astype(F32)


_erf = np.frompyfunc(math.erf, 1, 1)


def erf64(x):
    """math.erf over an array (each distinct value once)"""
    x = np.asarray(x, dtype=np.float64)
    uniq, inv = np.unique(x.ravel(), return_inverse=True)
    return _erf(uniq).astype(np.float64)[inv].reshape(x.shape)


def gelu_ref(v, form):
    """(ref, fp32 band) float64; form "tanh" or "erf" """
    with np.errstate(over="ignore", invalid="ignore"):
        if form == "tanh":
            t, k = np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v * v * v)), K_GELU_TANH
        else:
            t, k = erf64(v / math.sqrt(2.0)), K_GELU_ERF
        ref = 0.5 * v * (1.0 + t)
        return ref, k * U * (np.abs(v) + np.abs(ref)) + SUB


def gelu_band(ref, b32, fmt):
    return _with_storage(ref, b32, fmt)


def gelu_f32(v, form, c2=0.044715):
    """gelu_kernel in numpy float32 (tanh / erf evaluated in float64 and rounded: a correctly rounded libm). Slip: c2."""
    v = v.astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if form == "tanh":
            z = F32(0.7978845608028654) * (v + F32(c2) * v * v * v)
            t = np.tanh(z.astype(np.float64)).astype(F32)
        else:
            t = erf64((v * F32(0.7071067811865476)).astype(F32)).astype(F32)
        return (F32(0.5) * v * (F32(1.0) + t)).astype(F32)
