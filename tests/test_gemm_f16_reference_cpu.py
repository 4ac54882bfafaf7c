"""No-GPU checks of tests/gemm_f16_reference.py, the reference of tests/test_gpu_prefill_gemm_epilogues.py.

(a) Forms: `woq_probe_gemm_plan` (the plan launch_gemm_f16 itself follows) gives every GPU case the form bits, K slices,
half-tile layout and pack-pass rows the case claims, and the restated device-side choice of the pack pass (`pack_mode`)
gives the MODE and cached-chunk count it claims: a plan threshold that moves fails here, not silently on the device.

(b) Corruptions: the float64 computation, made wrong the way a subtly wrong kernel would be, leaves the band of the
right one (`terms(...)["tol"]`, never changed here) in at least one element — on the GPU cases' own inputs, for every
case that claims to cover the corruption:
  mean over Kpad instead of K               the K = 480 cases (Kpad 512)
  eps dropped                               every norm case with the 1e-4 row (row 1)
  norm weight not gathered under act-order  the act-order cases
  up tile from the wrong neighbour          every epi 1 case: n_in + 8 instead of n_in + 16, and gate / up swapped
  bias added to gate only                   every epi 1 case with a bias
  residual added before SiLU                the epi 1 cases with a residual
  ldo used as the residual's row stride     the cases whose residual has a stride of its own
  no fp16 clamp                             the saturation cases
  one K slice of the split dropped          every split-K case (each slice in turn)

Also: the band admits the correctly rounded reference of every case (the inputs put no fp16 result where the format
cannot follow a relative bound).

(c) Refusal: the reference refuses what the launcher refuses — epi 1 with N % 32 != 0 or an odd tile count.
"""
import os

import numpy as np
import pytest

from intel_extension_for_transformers_amd import _lib as L
from tests import gemm_f16_reference as R

needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libwoq_hip.so not built (python __graft_entry__.py)")

DT = {"fp32": L.F32, "bf16": L.BF16, "fp16": L.F16}
SMALL = R.CASES + R.SCALAR_BASES + R.ALIAS_CASES + R.SATURATION + R.WORKSPACE  # everything but the 256-row cases


def _ids(cases):
    return [c["name"] for c in cases]


def _variants(c):
    return [c] + (R.scalar_variants(c) if c in R.SCALAR_BASES else [])


# ---- (a) forms -------------------------------------------------------------------------------------------------------
@needs_lib
@pytest.mark.parametrize("c", R.ALL, ids=_ids(R.ALL))
def test_case_names_its_form(c):
    for v in _variants(c):
        group, asym, st = v["quant"]
        fp8 = v["wname"] in R.G.FP8
        lda = v["K"] + v["lda_pad"]
        p = L.probe_gemm_plan(v["K"], v["N"], group, L.WEIGHT_TYPES[v["wname"]], DT[st],
                              L.C_FP32 if v["fp32_class"] else L.C_BF16, asym, v["shuffle"], v["M"], DT[v["act"]], lda,
                              aligned=True, has_norm=v["norm"], fp8=fp8)
        assert (p["form"], p["nz"], p["half_tiles"], p["row_blocks"]) == v["expect"], v["name"]
        assert R.pack_mode(v["K"], v["act"], lda, v["shuffle"], raw=bool(p["form"] & L.GEMM_FORM_RAW)) == v["pack"], v["name"]
        if p["form"] & L.GEMM_FORM_SPLITK:  # the restated slice length gives the plan's slice count
            per = R.kper(v["M"], v["N"], v["K"])
            assert per > 0 and -(-((v["K"] + 127) // 128) // per) == p["nz"], v["name"]
        else:
            assert p["nz"] == 1 and (fp8 or v["wname"] in R.G.TABLES or R.kper(v["M"], v["N"], v["K"]) == 0), v["name"]


def test_form_bits_mirror_the_binding():
    assert (R.FRAG, R.SPLITK, R.FP32C, R.HS, R.RING, R.TALL, R.RAW) == (
        L.GEMM_FORM_FRAG, L.GEMM_FORM_SPLITK, L.GEMM_FORM_FP32, L.GEMM_FORM_HANDSCHED, L.GEMM_FORM_RING, L.GEMM_FORM_TALL,
        L.GEMM_FORM_RAW)


def test_the_list_holds_what_it_is_for():
    """the pack pass's four chunk forms for both row types, MODE 2 both ways, M = 1 / 40 / 130, every kernel form with
    norm + epi 0, norm + epi 1 and the in-place residual, N = 32 / 288 / 40 / 17"""
    packs = {(c["pack"], c["epi"]) for c in R.CASES if c["norm"]}
    assert {((m, n), e) for m in (0, 1) for n in (2, 4, 8, 0) for e in (0, 1)} <= packs and ((2, 0), 0) in packs
    assert {c["M"] for c in R.CASES if c["norm"]} == {1, 40, 130}
    assert any(c["shuffle"] and c["norm"] and c["epi"] == e for c in R.CASES for e in (0, 1))
    assert any(c["lda_pad"] and c["norm"] and not c["shuffle"] for c in R.CASES)
    for form in (R.HS | R.RING, 0, R.HS, R.SPLITK, R.FRAG):
        got = {(c["norm"], c["epi"], c["residual"]) for c in R.CASES if c["expect"][0] == form}
        assert {(True, 0, "none"), (True, 1, "none"), (False, 0, "alias")} <= got, form
    assert any(c["expect"][0] & R.RAW and c["residual"] == "alias" for c in R.CASES)
    assert {c["wname"] for c in R.CASES if c["expect"][0] & R.FRAG} == {"nf4", "fp4_e2m1", "fp8_e4m3"}
    assert {c["N"] for c in R.CASES if c["epi"] == 1} >= {32, 96, 288} and {c["N"] for c in R.CASES if c["epi"] == 0} >= {40, 17}
    assert any(c["fp32_class"] and c["norm"] for c in R.CASES)
    assert [(c["M"], c["N"], c["K"]) for c in R.TALL_CASES] == [(2049, 22016, 256), (2177, 22016, 256)]


def test_special_rows_are_what_they_say():
    c = R.BY_NAME["norm fp32 K512 epi0"]
    d = R.build(c)
    x = d["x"]
    assert not x[0].any() and 0 < np.abs(x[1]).max() <= 4e-4 and np.abs(x[2]).argmax() == c["K"] // 3
    assert (x[1].astype(np.float64) ** 2).mean() < 0.1 * R.EPS  # eps dominates
    t = R.terms(c, d)
    assert np.array_equal(t["exp"][0], d["bias"].astype(np.float64)) and (t["tol"][0] <= 1.1e-5 + 2.0 ** -10 * 5).all()
    assert np.abs(x[3]).max() > 2.0 ** 12 and abs(t["inv"][3] * 2.0 ** 12 - 1) < 0.2


@pytest.mark.parametrize("c", SMALL, ids=_ids(SMALL))
def test_band_admits_the_correctly_rounded_reference(c):
    """no input of the list puts a result where the output type cannot follow the band (fp16 below its normal range
    with a bound under the subnormal step)"""
    t = R.terms(c, R.build(c))
    assert np.isfinite(t["exp"]).all() and (t["tol"] > 0).all()
    assert (np.abs(R.round_out(t["exp"], c["out"]) - t["exp"]) <= t["tol"]).all()


# ---- (b) corruptions -------------------------------------------------------------------------------------------------
def _ctx(c):
    d = R.build(c)
    return d, R.terms(c, d)


def _leaves_band(c, t, wrong):
    bad = np.abs(wrong - t["exp"]) > t["tol"]
    assert bad.any(), c["name"]
    return bad


KPAD = [c for c in SMALL if c["norm"] and c["K"] % 128 != 0]
EPS_ROW = [c for c in SMALL if c["norm"] and c["M"] >= 4]
ACT_ORDER = [c for c in SMALL if c["shuffle"] and c["norm"]]
EPI1 = [c for c in SMALL if c["epi"] == 1]
EPI1_BIAS = [c for c in EPI1 if c["bias"]]
EPI1_RES = [c for c in EPI1 if c["residual"] != "none"]
OWN_STRIDE = [c for c in SMALL if c["residual"] == "separate" and c["ld_res_pad"] != c["ldo_pad"]]
SPLIT = [c for c in SMALL if c["expect"][0] & R.SPLITK]


def test_every_corruption_has_cases():
    assert len(KPAD) >= 2 and len(EPS_ROW) >= 20 and len(ACT_ORDER) >= 3 and len(EPI1) >= 20 and len(EPI1_BIAS) >= 4
    assert len(EPI1_RES) >= 2 and len(OWN_STRIDE) >= 4 and len(R.SATURATION) >= 2 and len(SPLIT) >= 12
    assert {bool(c["expect"][0] & R.SPLITK) for c in EPI1_RES} == {False, True}
    assert {bool(c["expect"][0] & R.SPLITK) for c in R.SATURATION} == {False, True}


@pytest.mark.parametrize("c", KPAD, ids=_ids(KPAD))
def test_mean_over_kpad(c):
    d, t = _ctx(c)
    _leaves_band(c, t, R.terms(c, d, K_mean=(c["K"] + 127) // 128 * 128)["exp"])


@pytest.mark.parametrize("c", EPS_ROW, ids=_ids(EPS_ROW))
def test_eps_dropped(c):
    d, t = _ctx(c)
    with np.errstate(all="ignore"):  # the all-zero row has no factor without eps
        bad = _leaves_band(c, t, R.terms(c, d, eps=0.0)["exp"])
    assert bad[1].any()  # the row where eps dominates


@pytest.mark.parametrize("c", ACT_ORDER, ids=_ids(ACT_ORDER))
def test_norm_weight_in_weight_row_order(c):
    d, t = _ctx(c)
    y = d["x"].astype(np.float64)[:, d["shuffle"]] * d["g"].astype(np.float64)[None, :]  # g[k], not g[shuffle[k]]
    _leaves_band(c, t, R.terms(c, d, y=y)["exp"])


def _pairs(c, d, t):
    """gate, up [M, tile pairs, 16] of the right computation, bias in"""
    lin = t["pre"] if d["bias"] is None else t["pre"] + d["bias"].astype(np.float64)
    v = lin.reshape(len(lin), -1, 2, 16)
    return lin, v[:, :, 0], v[:, :, 1]


def _finish(c, d, val):
    """what follows SiLU * mul: + residual, clamp"""
    if d["residual"] is not None:
        val = val + d["residual"].astype(np.float64)
    return np.clip(val, -R.F16_MAX, R.F16_MAX) if c["out"] == "fp16" else val


@pytest.mark.parametrize("c", EPI1, ids=_ids(EPI1))
def test_up_tile_from_the_wrong_neighbour(c):
    d, t = _ctx(c)
    lin, gate, up = _pairs(c, d, t)
    M = len(lin)
    n_in = (np.arange(d["n_out"]) // 16) * 32 + np.arange(d["n_out"]) % 16
    near = R._silu(lin[:, n_in]) * lin[:, n_in + 8]  # n_in + 8: half a tile short of the up tile
    _leaves_band(c, t, _finish(c, d, near))
    swapped = (R._silu(up) * gate).reshape(M, -1)
    _leaves_band(c, t, _finish(c, d, swapped))


@pytest.mark.parametrize("c", EPI1_BIAS, ids=_ids(EPI1_BIAS))
def test_bias_added_to_gate_only(c):
    d, t = _ctx(c)
    b = d["bias"].copy().reshape(-1, 2, 16)
    b[:, 1] = 0
    _leaves_band(c, t, R.terms(c, d, bias=b.reshape(-1))["exp"])


@pytest.mark.parametrize("c", EPI1_RES, ids=_ids(EPI1_RES))
def test_residual_added_before_silu(c):
    d, t = _ctx(c)
    _, gate, up = _pairs(c, d, t)
    res = d["residual"].astype(np.float64).reshape(gate.shape)
    _leaves_band(c, t, (R._silu(gate + res) * up).reshape(len(gate), -1))


@pytest.mark.parametrize("c", OWN_STRIDE, ids=_ids(OWN_STRIDE))
def test_ldo_used_as_the_residual_stride(c):
    d, t = _ctx(c)
    M, n_out = c["M"], d["n_out"]
    ld_res, ldo = n_out + c["ld_res_pad"], n_out + c["ldo_pad"]
    flat = np.zeros(M * max(ld_res, ldo) + n_out)  # the residual buffer as the device holds it, zeros between the rows
    for m in range(M):
        flat[m * ld_res:m * ld_res + n_out] = d["residual"][m]
    wrong_res = np.stack([flat[m * ldo:m * ldo + n_out] for m in range(M)])
    wrong = t["unclamped"] - d["residual"].astype(np.float64) + wrong_res
    bad = _leaves_band(c, t, wrong)
    assert not bad[0].any()  # row 0 starts at offset 0 either way


@pytest.mark.parametrize("c", R.SATURATION, ids=_ids(R.SATURATION))
def test_no_fp16_clamp(c):
    d, t = _ctx(c)
    sure = R.saturated(t)
    frac = sure.mean()
    assert 0.01 <= frac <= 0.5 and (t["unclamped"][sure] > 0).any() and (t["unclamped"][sure] < 0).any(), frac
    bad = _leaves_band(c, t, R.terms(c, d, clamp=False)["exp"])
    assert bad.sum() >= 0.5 * sure.sum()
    for out in ("bf16", "fp32"):  # the same inputs, no clamp: the band follows the value
        u = R.terms(c, d, out=out)
        assert np.array_equal(u["exp"], t["unclamped"]) and np.abs(u["exp"]).max() > 2 * R.F16_MAX


@pytest.mark.parametrize("c", SPLIT, ids=_ids(SPLIT))
def test_one_k_slice_dropped(c):
    d, t = _ctx(c)
    per = R.kper(c["M"], c["N"], c["K"]) * 128
    assert per > 0
    base = R.activation(d["x"], d["g"], d["shuffle"])
    for k0 in range(0, c["K"], per):
        y = base.copy()
        y[:, k0:k0 + per] = 0
        _leaves_band(c, t, R.terms(c, d, y=y)["exp"])


# ---- (c) refusal -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [48, 16, 40, 17, 80])
def test_reference_refuses_what_the_launcher_refuses(N):
    x, W = np.ones((2, 128), np.float32), np.ones((128, N))
    with pytest.raises(RuntimeError, match="QBits: the SiLU\\*mul epilogue needs whole gate / up column-tile pairs"):
        R.reference(x, W, epi=1)
    with pytest.raises(RuntimeError, match="QBits: the SiLU\\*mul epilogue"):
        R.epilogue(np.ones((2, N)), 1e-5, epi=1)
    assert R.reference(x, W, epi=0)["exp"].shape == (2, N) and R.reference(x, np.ones((128, 64)), epi=1)["exp"].shape == (2, 32)
    assert R.REFUSED["N"] == 48 and R.REFUSED["epi"] == 1
