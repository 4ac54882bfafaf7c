"""float64 reference of the rolling KV cache's shift (csrc/woq_kv_shift.hip), shared by the CPU and GPU tests.

The stored cache values are decoded exactly, K rows are rotated back by the float64 value of the engine's fp32 table row
`build_rope_tables(max_ctx, head_dim, theta, "cpu")[n_discard]` (deterministic, and the function the engine itself uses)
and rounded ONCE to the cache type, round-to-nearest-even: fp16 by numpy, bf16 and e4m3 on their grids in float64, the
e4m3 values then through torch's float8_e4m3fn for the bytes. Inputs are standard normal, so nothing comes near
saturation and the reference does not depend on overflow behaviour. Caches travel as their bit patterns (uint16 / uint8).
"""
import numpy as np
import torch

from intel_extension_for_transformers_amd.runtime.engine import build_rope_tables

KINDS = ("fp16", "bf16", "e4m3")
TORCH_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn}
# (significant bits with the implicit one, exponent of the smallest normal value)
_GRID = {"fp16": (11, -14), "bf16": (8, -126), "e4m3": (4, -6)}


def bits_of(t):
    """a torch tensor in a cache type -> numpy array of its bit patterns (uint16 / uint8)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint8).numpy().copy() if t.dtype == torch.float8_e4m3fn else t.view(torch.int16).numpy().view(np.uint16).copy()


def from_bits(bits, kind):
    """bit patterns -> torch tensor in the cache type"""
    if kind == "e4m3":
        return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint8)).view(torch.float8_e4m3fn)
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(TORCH_DTYPE[kind])


def decode(bits, kind):
    """bit patterns -> float64, exact"""
    if kind == "fp16":
        return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)
    if kind == "bf16":
        return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return from_bits(bits, kind).to(torch.float64).numpy()


def round_to_grid(x, kind):
    """float64 -> the nearest value of the cache type (ties to even), still float64. One rounding: x / quantum is exact
    (a power of two), np.rint rounds half to even. Values beyond the type's range are not handled (standard-normal data)."""
    sig, emin = _GRID[kind]
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)  # |x| in [2^(e-1), 2^e)
    quantum = np.ldexp(1.0, np.maximum(e - 1, emin) - (sig - 1))
    return np.rint(x / quantum) * quantum


def encode(x, kind):
    """float64 -> bit patterns of the cache type, one round-to-nearest-even"""
    r = round_to_grid(x, kind)
    if kind == "fp16":
        return r.astype(np.float16).view(np.uint16)  # exact: r is an fp16 value
    if kind == "bf16":
        return (r.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)  # exact: the low 16 bits are zero
    return bits_of(torch.from_numpy(r).to(torch.float8_e4m3fn))  # exact: r is an e4m3 value


def ulp_distance(a_bits, b_bits, kind):
    """elementwise distance in units of the cache type's last place (its values ordered on a line, -0 == +0)"""
    mag = 0x7F if kind == "e4m3" else 0x7FFF
    sign = mag + 1

    def line(b):
        b = np.asarray(b).astype(np.int64)
        return np.where(b & sign, -(b & mag), b & mag)

    return np.abs(line(a_bits) - line(b_bits))


def table_row(max_ctx, head_dim, theta, n_discard):
    """(cos, sin) of the angle of n_discard: row n_discard of the engine's fp32 tables, as float64 [head_dim / 2]"""
    cos, sin = build_rope_tables(max_ctx, head_dim, theta, "cpu")
    return cos[n_discard].numpy().astype(np.float64), sin[n_discard].numpy().astype(np.float64)


def rotate_back(a, b, c, s):
    """the kernel's rotation of one (d, d + D/2) pair: (a c + b s, b c - a s)"""
    return a * c + b * s, b * c - a * s


def shift_reference(k_bits, v_bits, kind, cos_row, sin_row, n_keep, n_discard, n_cached):
    """k_bits / v_bits: [..., positions, kv_heads, D] bit patterns of one sequence. Returns the expected bit patterns of
    rows [n_keep, n_cached - n_discard) after woq_engine_kv_shift: (K rotated back and rounded once, V copied)."""
    src = slice(n_keep + n_discard, n_cached)
    k = decode(k_bits[..., src, :, :], kind)
    half = k.shape[-1] // 2
    lo, hi = rotate_back(k[..., :half], k[..., half:], cos_row, sin_row)
    return encode(np.concatenate([lo, hi], -1), kind), np.array(v_bits[..., src, :, :], copy=True)


def emulate_kernel(k_bits, kind, cos_row32, sin_row32):
    """The kernel's own arithmetic on rows of stored values: the two products (exact in fp64: an at most 11-bit value
    times an fp32 one) and their sum in fp64, the sum rounded to fp32, that rounded to the cache type. Exact products
    make a contracted fma give the same bits, so there is one form to emulate. Returns bit patterns."""
    k = decode(k_bits, kind)
    half = k.shape[-1] // 2
    a, b = k[..., :half], k[..., half:]
    c = np.asarray(cos_row32, np.float32).astype(np.float64)
    s = np.asarray(sin_row32, np.float32).astype(np.float64)
    lo, hi = (a * c + b * s).astype(np.float32), (b * c - a * s).astype(np.float32)
    return encode(np.concatenate([lo, hi], -1).astype(np.float64), kind)


def emulate_fp32(k_bits, kind, cos_row32, sin_row32, fused):
    """The kernel's own arithmetic in fp32 on rows of stored values. fused 0: each product and sum rounded to fp32
    separately. fused 1 / 2: the contracted forms the compiler may emit — 1: fma(a, c, b * s) and fma(b, c, -(a * s)),
    2: fma(b, s, a * c) and fma(-a, s, b * c) — the inner product rounded to fp32, the outer one exact inside the fma
    (computed in float64, where a 24-bit x 24-bit product is exact and its sum with an fp32 value is exact enough to
    round once). Returns bit patterns."""
    k = decode(k_bits, kind).astype(np.float32)
    half = k.shape[-1] // 2
    a, b = k[..., :half], k[..., half:]
    c, s = np.asarray(cos_row32, np.float32), np.asarray(sin_row32, np.float32)
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)  # noqa: E731
    if not fused:
        lo, hi = (a * c) + (b * s), (b * c) - (a * s)
    elif fused == 1:
        lo = (f64(a) * f64(c) + f64(b * s)).astype(np.float32)
        hi = (f64(b) * f64(c) - f64(a * s)).astype(np.float32)
    else:
        lo = (f64(b) * f64(s) + f64(a * c)).astype(np.float32)
        hi = (f64(b * c) - f64(a) * f64(s)).astype(np.float32)
    return encode(np.concatenate([lo, hi], -1).astype(np.float64), kind)


# The GPU kernel test's cases (tests/test_gpu_kv_shift_kernel.py); tests/test_kv_shift_cpu.py runs the fp32 emulation on
# the same inputs. Caches are [max_batch][layers][max_ctx][kv_heads][head_dim]; (n_keep, n_discard, n_cached).
THETA = 10000.0
SMALL = dict(layers=2, max_batch=2, max_ctx=64)
SMALL_HEADS = {64: 2, 128: 1}  # kv heads per head_dim
SMALL_CASES = [(4, 8, 64), (0, 1, 64), (3, 7, 37), (4, 60, 64)]
LARGE = dict(layers=2, max_batch=1, max_ctx=2048, kv_heads=8, head_dim=128)
LARGE_CASES = [(4, 64, 2048), (4, 1022, 2048), (0, 1, 2048)]
K_SEED, V_SEED = 11, 12
MAX_ULP, MAX_DIFFERING = 1, 0.01  # the K rows' bound against the rounded float64 reference


def small_shape(head_dim):
    return (SMALL["max_batch"], SMALL["layers"], SMALL["max_ctx"], SMALL_HEADS[head_dim], head_dim)


def large_shape():
    return (LARGE["max_batch"], LARGE["layers"], LARGE["max_ctx"], LARGE["kv_heads"], LARGE["head_dim"])


def normal_cache(shape, kind, seed):
    """standard-normal values stored in the cache type (torch's rounding), as a torch tensor of that type"""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(shape, generator=g, dtype=torch.float32).to(TORCH_DTYPE[kind])
