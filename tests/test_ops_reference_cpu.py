"""What the bands of tests/ops_reference.py accept and what they reject, without a GPU, on every case of
tests/test_gpu_ops_kernel.py: the fp32 restatement of each kernel (numpy float32 in the kernel's operation order, stored
with the device's cast) lies inside its band; each planted slip — the kinds of mistake an edit to csrc/woq_ops.hip could
make — leaves it in at least one case; the correctly rounded reference alone uses at most half an ulp of a 16-bit band.
Also here, because they need no device: the C entry points refuse bad dtype codes, null pointers and negative sizes
before any HIP call (skipped when the library is not built)."""
import ctypes
import os

import numpy as np
import pytest

from tests import ops_reference as R


def _worst(out32, ref, band, fmt, b32=None):
    """largest err / band of an fp32 result stored in fmt; inf where, given b32, it leaves the rounded interval"""
    y = R.to_storage(out32, fmt)
    if b32 is not None and not np.all(R.inside(y, ref, b32, fmt)):
        return float("inf")
    return float(R.ratio(y, ref, band, fmt).max())


# ---- rmsnorm ---------------------------------------------------------------------------------------------------------
def _rms_cases():
    for in_fmt, out_fmt in R.RMS_TYPES:
        for d in R.RMS_D:
            x, w = R.rmsnorm_inputs(d, in_fmt)
            for rows in R.RMS_ROWS:
                for eps in R.RMS_EPS:
                    ref, b32 = R.rmsnorm_ref(x[:rows], w, eps)
                    yield (in_fmt, out_fmt, d, rows, eps), x[:rows], w, eps, ref, b32, R.rmsnorm_band(ref, b32, out_fmt), out_fmt


def test_rmsnorm_restatement_inside_band_and_slips_outside():
    slips = {"eps dropped": dict(eps_scale=0.0), "eps x 10": dict(eps_scale=10.0), "mean over padded d": dict(mean_padded=True),
             "weight index + 1": dict(w_shift=1)}
    caught = dict.fromkeys(slips, 0)
    worst = 0.0
    for case, x, w, eps, ref, b32, band, fmt in _rms_cases():
        got = _worst(R.rmsnorm_f32(x, w, eps), ref, band, fmt, b32)
        assert got <= 1.0, (case, got)
        worst = max(worst, got)
        zero = ~np.any(x != 0, axis=-1)
        assert np.all(R.rmsnorm_f32(x, w, eps)[zero] == 0) and np.all(ref[zero] == 0)
        for name, kw in slips.items():
            caught[name] += _worst(R.rmsnorm_f32(x, w, eps, **kw), ref, band, fmt) > 1.0
    print("rmsnorm restatement: worst err / band %.3f; cases rejecting each slip: %s" % (worst, caught))
    assert all(caught.values()), caught
    # the padded mean can only show where d is no multiple of 256, the shifted weight only for d > 1
    n_cases = len(R.RMS_TYPES) * len(R.RMS_ROWS) * len(R.RMS_EPS)
    assert caught["mean over padded d"] == n_cases * sum(d % 256 != 0 for d in R.RMS_D)
    assert caught["weight index + 1"] == n_cases * sum(d > 1 for d in R.RMS_D)


def test_rms_band_constant_and_families():
    assert [R.k_rms(d) for d in (1, 256, 257, 8200)] == [10.5, 10.5, 11.0, 26.5]
    x, _ = R.rmsnorm_inputs(1000, "fp32")
    assert not x[3].any() and np.count_nonzero(x[4]) == 1 and np.all(x[5] == 0.75) and x[6, -1] == 1000.0
    # mean(x^2) of the 2^-20 rows is far below eps, of the 2^20 rows far above: eps matters in one and not the other
    assert np.mean(x[1] ** 2) < 1e-3 * 1e-6 and np.mean(x[2] ** 2) > 1e9
    assert np.all(np.isfinite(R.rmsnorm_inputs(8200, "fp16")[0]))


# ---- rope ------------------------------------------------------------------------------------------------------------
def _rope_cases():
    for shape in R.ROPE_SHAPES:
        cos, sin = R.rope_tables(shape[2])
        for fmt in R.DTYPES:
            x, pos = R.rope_inputs(shape, fmt)
            ref, b32 = R.rope_ref(x, pos, cos, sin)
            yield (shape, fmt), x, pos, cos, sin, ref, b32, R.rope_band(ref, b32, fmt), fmt


def test_rope_restatement_inside_band_and_slips_outside():
    slips = {"sine sign": dict(flip_sign=True), "halves swapped": dict(swap_halves=True), "position of t - 1": dict(prev_pos=True)}
    caught = dict.fromkeys(slips, 0)
    worst = 0.0
    for case, x, pos, cos, sin, ref, b32, band, fmt in _rope_cases():
        for fma in (False, True):  # the compiler may contract either product into the sum
            got = _worst(R.rope_f32(x, pos, cos, sin, fma=fma), ref, band, fmt, b32)
            assert got <= 1.0, (case, fma, got)
            worst = max(worst, got)
        at0 = pos == 0
        assert np.array_equal(R.rope_f32(x, pos, cos, sin)[at0], x[at0].astype(np.float32))
        for name, kw in slips.items():
            caught[name] += _worst(R.rope_f32(x, pos, cos, sin, **kw), ref, band, fmt) > 1.0
    print("rope restatement: worst err / band %.3f; cases rejecting each slip: %s" % (worst, caught))
    n = len(R.ROPE_SHAPES) * len(R.DTYPES)
    assert caught["sine sign"] == n and caught["halves swapped"] == n
    assert caught["position of t - 1"] == len(R.DTYPES) * sum(s[0] > 1 for s in R.ROPE_SHAPES)  # one token: no t - 1


def test_rope_cases_cover_what_they_claim():
    assert sorted({s[2] // 2 for s in R.ROPE_SHAPES}) == [1, 3, 32, 64]
    blocks = [s[0] * s[1] * (s[2] // 2) / 256 for s in R.ROPE_SHAPES]
    assert blocks[2] == 3.75 and blocks[3] == 16.0 and max(blocks[0], blocks[1], blocks[4]) < 1
    pos = np.array(R.ROPE_POS)
    assert pos.max() == R.ROPE_MAX_POS - 1 and pos.min() == 0 and np.any(np.diff(pos) == 0) and np.any(np.diff(pos) < 0)
    cos, sin = R.rope_tables(6)
    assert cos.dtype == np.float32 and cos.shape == (64, 3) and np.all(cos[0] == 1) and np.all(sin[0] == 0)


# ---- silu_mul and gelu -----------------------------------------------------------------------------------------------
def test_silu_mul_restatement_inside_band_and_slip_outside():
    caught, worst = 0, 0.0
    for fmt in R.DTYPES:
        for n in R.ELEM_N:
            a, b = R.elementwise_inputs(n, fmt)
            ref, b32 = R.silu_mul_ref(a, b)
            band = R.silu_mul_band(ref, b32, fmt)
            got = _worst(R.silu_mul_f32(a, b), ref, band, fmt, b32)
            assert got <= 1.0, (fmt, n, got)
            worst = max(worst, got)
            caught += _worst(R.silu_mul_f32(a, b, b_shift=1), ref, band, fmt) > 1.0
    print("silu_mul restatement: worst err / band %.3f; cases rejecting the neighbour's b: %d" % (worst, caught))
    assert caught == len(R.DTYPES) * (len(R.ELEM_N) - 1)  # n = 1 has no neighbour


def test_silu_mul_specials():
    a, b = R.elementwise_inputs(1048579, "fp32")
    ref, b32 = R.silu_mul_ref(a, b)
    out = R.silu_mul_f32(a, b).astype(np.float64)
    flushed = -a > R.LOG_FLT_MAX
    assert flushed.sum() == 3 * 3  # -89, -104, -1e4 at each of the three slots
    assert np.all(out[flushed] == 0) and np.all(np.abs(ref[flushed]) <= 89 * np.abs(b[flushed]) / R.FLT_MAX)
    assert np.all(b32[flushed] >= np.abs(ref[flushed]))
    assert np.isnan(ref).sum() == 3 + 1 and np.array_equal(np.isnan(out), np.isnan(ref))  # NaN gates, one NaN up
    k = len(R.SPECIALS)
    assert R.special_slots(1048579) == [0, 1048579 - k, R.GRID_SPAN - k // 2]
    assert R.special_slots(524288) == [0, 524288 - k] and R.special_slots(1) == [0]
    # the overflow pair: finite in fp32 and bf16, infinite in fp16, in the reference as in the restatement
    for fmt, inf in (("fp32", False), ("bf16", False), ("fp16", True)):
        a, b = R.elementwise_inputs(257, fmt)
        y = R.stored(R.silu_mul_ref(a, b)[0], fmt)
        assert (a[k], b[k]) == R.OVERFLOW_PAIR and np.isinf(y[k]) == inf
        assert np.isinf(R.to_storage(R.silu_mul_f32(a, b), fmt)[k]) == inf


def test_gelu_restatement_inside_band_and_slips_outside():
    caught = {"0.044 for 0.044715": 0, "erf where tanh was asked": 0, "tanh where erf was asked": 0}
    by_specials = dict.fromkeys(caught, 0)
    worst = {"tanh": 0.0, "erf": 0.0}
    for fmt in R.DTYPES:
        for n in R.ELEM_N:
            v, _ = R.elementwise_inputs(n, fmt)
            out = {f: R.gelu_f32(v, f) for f in ("tanh", "erf")}
            for form, other in (("tanh", "erf"), ("erf", "tanh")):
                ref, b32 = R.gelu_ref(v, form)
                band = R.gelu_band(ref, b32, fmt)
                got = _worst(out[form], ref, band, fmt, b32)
                assert got <= 1.0, (fmt, n, form, got)
                worst[form] = max(worst[form], got)
                key = "%s where %s was asked" % (other, form)
                caught[key] += _worst(out[other], ref, band, fmt) > 1.0
                k = len(R.SPECIALS)
                if n >= k:  # the specials alone separate the two forms
                    by_specials[key] += _worst(out[other][:k], ref[:k], band[:k], fmt) > 1.0
                if form == "tanh":
                    caught["0.044 for 0.044715"] += _worst(R.gelu_f32(v, "tanh", c2=0.044), ref, band, fmt) > 1.0
    print("gelu restatement: worst err / band %s; cases rejecting each slip: %s" % (worst, caught))
    big = len(R.DTYPES) * sum(n >= len(R.SPECIALS) for n in R.ELEM_N)
    assert all(c >= big for c in caught.values()), caught
    assert by_specials["erf where tanh was asked"] == big and by_specials["tanh where erf was asked"] == big


def test_gelu_band_needs_the_absolute_term():
    """at v = -5 the fp32 result keeps about three digits: a relative band rejects the correct kernel there, and the
    golden test's 1e-5 absolute cannot see a wrong cubic constant there; the band sees it at v = -3"""
    v = np.array([-5.0, -3.0])
    ref, b32 = R.gelu_ref(v, "tanh")
    good, bad = R.gelu_f32(v, "tanh").astype(np.float64), R.gelu_f32(v, "tanh", c2=0.044).astype(np.float64)
    assert abs(good - ref)[0] > 100 * R.U * abs(ref[0]) and np.all(abs(good - ref) <= b32)
    assert abs(bad - ref)[0] < 1e-5 and abs(bad - ref)[1] > 10 * b32[1]


# ---- 16-bit outputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_rounded_reference_uses_at_most_half_an_ulp(fmt):
    a, b = R.elementwise_inputs(524289, fmt)
    refs = [R.silu_mul_ref(a, b), R.gelu_ref(a, "tanh"), R.gelu_ref(a, "erf")]
    x, w = R.rmsnorm_inputs(1000, fmt)
    refs.append(R.rmsnorm_ref(x, w, 1e-5))
    xr, pos = R.rope_inputs((5, 3, 128), fmt)
    refs.append(R.rope_ref(xr, pos, *R.rope_tables(128)))
    for ref, b32 in refs:
        y = R.stored(ref, fmt)
        fin = np.isfinite(y) & np.isfinite(ref)
        err = np.abs(y - ref)[fin]
        assert np.all(err <= R.half_ulp(ref, fmt)[fin])
        assert np.all(err <= (R._with_storage(ref, b32, fmt) - b32)[fin])
        assert np.all(R.ratio(y, ref, R._with_storage(ref, b32, fmt), fmt) <= 1.0)
    # storage: nearest even, no saturation
    assert R.stored(65519.9, "fp16") == 65504 and np.isposinf(R.stored(65520.0, "fp16")) and np.isneginf(R.stored(-7e4, "fp16"))
    assert R.stored(1 + 2.0 ** -11, "fp16") == 1 and R.stored(1 + 3 * 2.0 ** -11, "fp16") == 1 + 2.0 ** -9
    probe = np.array([1.0039062, -3.3e38, 1e-40, 65519.0, 0.1])
    assert np.array_equal(R.to_storage(probe, fmt)[np.isfinite(R.stored(probe, fmt))],
                          R.stored(probe.astype(np.float32), fmt)[np.isfinite(R.stored(probe, fmt))])


# ---- the C entry points refuse before any HIP call -------------------------------------------------------------------
def _abi():
    from intel_extension_for_transformers_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libwoq_hip.so is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    vp, ci, cf, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    lib.woq_rmsnorm.argtypes = [vp, ci, vp, cf, ci, ci, vp, ci, vp]
    lib.woq_rope.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, vp]
    lib.woq_silu_mul.argtypes = [vp, vp, ci, cs, vp, vp]
    lib.woq_gelu.argtypes = [vp, ci, cs, ci, vp, vp]
    lib.woq_last_error.restype = ctypes.c_char_p
    return lib, _lib


def test_abi_refuses_bad_arguments_before_any_launch():
    """Every call here is refused by a check in front of the launch (read in csrc/woq_ops.hip: shape, dtype codes, the
    zero-size return, null pointers, then the launch). The non-null pointers are host buffers no kernel ever sees."""
    lib, L = _abi()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    F32, BF16, F16, FP8 = L.F32, L.BF16, L.F16, 3

    def refused(rc):
        assert rc != 0 and lib.woq_last_error().decode().startswith("QBits:"), rc

    for bad in (FP8, 4, -1, 77):
        refused(lib.woq_rmsnorm(p, bad, p, 1e-5, 1, 8, p, F32, None))
        refused(lib.woq_rmsnorm(p, F32, p, 1e-5, 1, 8, p, bad, None))
        refused(lib.woq_rope(p, bad, p, p, p, 1, 1, 8, None))
        refused(lib.woq_silu_mul(p, p, bad, 8, p, None))
        refused(lib.woq_gelu(p, bad, 8, 1, p, None))
        refused(lib.woq_rmsnorm(p, bad, p, 1e-5, 0, 8, p, F32, None))  # also with nothing to do
    for dt in (F32, BF16, F16):
        refused(lib.woq_rmsnorm(None, dt, p, 1e-5, 1, 8, p, dt, None))
        refused(lib.woq_rmsnorm(p, dt, None, 1e-5, 1, 8, p, dt, None))
        refused(lib.woq_rmsnorm(p, dt, p, 1e-5, 1, 8, None, dt, None))
        refused(lib.woq_rope(None, dt, p, p, p, 1, 1, 8, None))
        refused(lib.woq_rope(p, dt, None, p, p, 1, 1, 8, None))
        refused(lib.woq_rope(p, dt, p, None, p, 1, 1, 8, None))
        refused(lib.woq_rope(p, dt, p, p, None, 1, 1, 8, None))
        refused(lib.woq_silu_mul(None, p, dt, 8, p, None))
        refused(lib.woq_silu_mul(p, None, dt, 8, p, None))
        refused(lib.woq_silu_mul(p, p, dt, 8, None, None))
        refused(lib.woq_gelu(None, dt, 8, 1, p, None))
        refused(lib.woq_gelu(p, dt, 8, 0, None, None))
    for d in (0, -1, -256):
        refused(lib.woq_rmsnorm(p, F32, p, 1e-5, 1, d, p, F32, None))
    refused(lib.woq_rmsnorm(p, F32, p, 1e-5, -1, 8, p, F32, None))
    refused(lib.woq_rope(p, F32, p, p, p, -1, 1, 8, None))
    refused(lib.woq_rope(p, F32, p, p, p, 1, -1, 8, None))
    refused(lib.woq_rope(p, F32, p, p, p, -1, -1, 8, None))  # the product of the two would be positive
    refused(lib.woq_rope(p, F32, p, p, p, 1, 1, -8, None))
    refused(lib.woq_rope(p, F32, p, p, p, 1, 1, 7, None))
    # nothing to do is still no error, null pointers included
    assert lib.woq_rmsnorm(None, F32, None, 1e-5, 0, 8, None, F32, None) == 0
    assert lib.woq_rope(None, F16, None, None, None, 0, 4, 8, None) == 0
    assert lib.woq_silu_mul(None, None, BF16, 0, None, None) == 0
    assert lib.woq_gelu(None, F32, 0, 1, None, None) == 0


def test_header_states_the_accepted_types():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "woq_hip.h")).read()
    for name in ("woq_rmsnorm", "woq_rope", "woq_silu_mul", "woq_gelu"):
        decl = header[:header.index("WOQ_API int %s(" % name)].rsplit("/*", 1)[1]
        assert "WOQ_F32, WOQ_F16 or WOQ_BF16" in decl, name
