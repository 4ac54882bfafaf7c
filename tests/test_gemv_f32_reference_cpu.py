"""No-GPU checks of tests/gemv_f32_reference.py, the reference of tests/test_gpu_f32_gemv_kernel.py.

(a) Geometry: the restated dispatch and launch geometry name the form every GPU case claims (the GPU test asserts the
same tuple against what `woq_probe_gemv_f32` reports), so a case list that drifts from its form fails here.

(b) Sensitivity: the float64 computation, corrupted the way a subtly wrong kernel would be, leaves the tolerance band of
the uncorrupted one for at least one output — on the GPU cases' own inputs — so the GPU test would fail on such a kernel.
The band is `terms(...)["tol"]`, never changed here. Inputs chosen per corruption (all of them GPU cases):
  one wave's sum of squares left out      "tile K16384 norm" (16 waves: the smallest share a wave can have), the wave
                                          WITHOUT the x 30 element; also the fp8 kernel's "fp8 K8192 norm"
  mean over Kpad instead of K             "tile K4128 g32a norm" (Kpad 4224), "generic K4098"
  g[k] instead of g[shuffle[k]]           the four "act-order K4096" cases and the K = 16384 one
  the last, partial tile dropped          "tile K4128 g32a" (the tile holds one 32-k block), "generic K4098" (2 values)
  the residual added twice                "tile K16512 residual chained" (chunk 1 taking the caller's residual as well)
  gate and up of one tile pair swapped    every gate/up case
  the wrong row's norm factor             "tile K4096 norm M5" (rows at distinct scales)
"""
import numpy as np
import pytest

from tests import gemv_f32_reference as R


@pytest.mark.parametrize("c", R.CASES + R.SPECIAL, ids=lambda c: c["name"])
def test_case_names_its_form(c):
    assert R.predict_form(c) == c["expect"]


def test_geometry_restates_the_launch_rules():
    g, f = R.geometry, R.fp8_geometry
    assert g(2048)[0][2:] == (4, 4, [4] * 4) and g(2176)[0][2:] == (3, 8, [6, 6, 5]) and g(4096)[0][2:] == (4, 8, [8] * 4)
    assert g(11008)[0][2:] == (11, 8, [8] * 9 + [7] * 2) and g(16384)[0][2:4] == (16, 8)
    assert g(16512) == [] and g(16512, chainable=True) == [(0, 65, 9, 8, [8] * 2 + [7] * 7), (65, 64, 8, 8, [8] * 8)]
    assert g(4128, smode=1)[0][1:] == (33, 5, 8, [7, 7, 7, 6, 6])
    assert g(12288, smode=1)[0][2:4] == (12, 8) and g(12416, smode=1) == [] and g(12416, smode=0)[0][2] == 13
    assert g(2048, epi=1)[0][2:4] == (4, 4) and g(4096, epi=1)[0][2:4] == (4, 8) and g(8192, epi=1)[0][2:4] == (8, 8)
    assert g(8320, epi=1) == []  # (a gate/up launch is never chainable: predict_form)
    assert g(6144, epi=1, smode=1)[0][2:4] == (12, 4) and g(6272, epi=1, smode=1) == []
    assert f(256)[0][2:] == (1, 4, [2]) and f(4096)[0][2:4] == (8, 4) and f(8192)[0][2:4] == (16, 4)
    assert f(8320)[0][2:] == (9, 8, [8, 8, 7, 7, 7, 7, 7, 7, 7]) and f(11008)[0][2:4] == (11, 8)
    assert f(12288)[0][2:4] == (12, 8) and f(12416) == []


def test_act_order_limits_come_from_the_rule():
    """the largest K (a multiple of 4) whose act-order launch the tile kernel takes, and the next one, for both forms; the
    whole-vector copy itself fits at every K one launch covers, so the one-launch rule is what binds"""
    for smode, last in ((0, 16384), (1, 12288)):
        ks = [K for K in range(4, 20000, 4) if R.act_order_tile_ok(K, smode)]
        assert ks[-1] == last and not R.act_order_tile_ok(last + 4, smode)
        assert all(R.tile_lds_bytes(1, R.geometry(K, 0, smode)[0][2], R.geometry(K, 0, smode)[0][3], 1) + 4 * K + 16
                   <= 150 * 1024 for K in range(128, last + 1, 128))
    assert (R.ACT_ORDER_LAST_K, R.ACT_ORDER_NEXT_K) == (16384, 16388)


def test_slices_cover_k_once():
    for c in R.CASES:
        form = R.predict_form(c)
        if form[0] == 0:
            continue
        launches = R.fp8_geometry(c["K"]) if form[0] == 2 else R.geometry(c["K"], c["epi"], R.smode_of(c),
                                                                           c["epi"] == 0 and not c["norm"])
        b = R.slice_bounds(launches, c["K"])
        assert b[0][0] == 0 and b[-1][1] == c["K"] and all(p[1] == n[0] for p, n in zip(b, b[1:]))


def test_conversion_is_within_half_a_unit():
    c = R.BY_NAME["tile K4128 g32a norm"]
    d = R.build(c)
    t = R.terms(c, d)
    for k0, k1 in R.slice_bounds(t["launches"], c["K"]):
        seg = t["y32"][0, k0:k1].astype(np.float64)
        err = np.abs(R.convert(t["y32"], [(k0, k1)])[0, k0:k1] - seg).max()
        assert err <= np.abs(seg).max() * 2.0 ** -21  # half a unit 2^(e - 22), the maximum in [2^(e - 1), 2^e)
    assert 0 < t["B"] < 1e-4 and (t["tol"] > 0).all() and t["tol"].max() < 2e-2 * np.abs(t["r0"]).max()


# ---- sensitivity -----------------------------------------------------------------------------------------------------
def _leaves_band(c, t, wrong):
    bad = np.abs(wrong - t["r0"]) > t["tol"]
    assert bad.any(), c["name"]
    return int(bad.sum())


def _ctx(name):
    c = R.BY_NAME[name]
    d = R.build(c)
    return c, d, R.terms(c, d)


@pytest.mark.parametrize("name", ["tile K16384 norm", "fp8 K8192 norm"])
def test_a_waves_sum_of_squares_left_out(name):
    c, d, t = _ctx(name)
    x64 = d["x"].astype(np.float64)
    hot = int(np.abs(d["x"][0]).argmax())
    for k0, k1 in R.slice_bounds(t["launches"], c["K"]):
        if k0 <= hot < k1:
            continue  # the wave holding the x 30 element would be the easy one
        ss = (x64 * x64).sum() - (x64[0, k0:k1] ** 2).sum()
        inv = np.array([1.0 / np.sqrt(ss / c["K"] + R.EPS)])
        _leaves_band(c, t, R.outputs(t["y64"], d["W64"], inv, d["bias"], d["residual"], c["epi"]))


@pytest.mark.parametrize("name", ["tile K4128 g32a norm", "generic K4098"])
def test_mean_over_kpad(name):
    c, d, t = _ctx(name)
    inv = R.inv_rows(d["x"], d["g"], K_mean=(c["K"] + 127) // 128 * 128)
    _leaves_band(c, t, R.outputs(t["y64"], d["W64"], inv, d["bias"], d["residual"], c["epi"]))


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["shuffle"] and c["expect"][0] == 1])
def test_norm_weight_in_weight_row_order(name):
    c, d, t = _ctx(name)
    y = d["x"].astype(np.float64)[:, d["shuffle"]] * d["g"].astype(np.float64)[None, :]  # g[k], not g[shuffle[k]]
    _leaves_band(c, t, R.outputs(y, d["W64"], t["inv"], d["bias"], d["residual"], c["epi"]))


@pytest.mark.parametrize("name", ["tile K4128 g32a", "tile K4128 g32a norm", "generic K4098"])
def test_last_partial_tile_dropped(name):
    c, d, t = _ctx(name)
    y = t["y64"].copy()
    y[:, c["K"] // 128 * 128:] = 0
    _leaves_band(c, t, R.outputs(y, d["W64"], t["inv"], d["bias"], d["residual"], c["epi"]))


def test_residual_added_twice_across_the_chain():
    c, d, t = _ctx("tile K16512 residual chained")
    assert t["form"][1] == 2
    _leaves_band(c, t, t["r0"] + d["residual"].astype(np.float64))


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["epi"] == 1])
def test_gate_and_up_of_one_pair_swapped(name):
    c, d, t = _ctx(name)
    W = d["W64"].copy()
    W[:, 32:48], W[:, 48:64] = d["W64"][:, 48:64], d["W64"][:, 32:48]  # the second pair
    wrong = R.outputs(t["y64"], W, t["inv"], d["bias"], d["residual"], 1)
    assert _leaves_band(c, t, wrong) >= 8 and (np.abs(wrong - t["r0"])[:, :16] <= t["tol"][:, :16]).all()


def test_wrong_rows_norm_factor():
    c, d, t = _ctx("tile K4096 norm M5")
    assert len(set(np.round(t["inv"], 3))) == 5  # distinct row scales
    wrong = R.outputs(t["y64"], d["W64"], np.roll(t["inv"], 1), d["bias"], d["residual"], c["epi"])
    bad = (np.abs(wrong - t["r0"]) > t["tol"]).any(axis=1)
    assert bad.all()


def test_special_rows_are_what_they_say():
    for c in R.SPECIAL:
        rows = R.special_rows(c)
        assert not rows["all zero"].any() and set(rows) == {"all zero", "one slice zero",
                                                            "x30 in the last, partial slice", "format extremes"}
        assert np.abs(rows["x30 in the last, partial slice"][0]).argmax() == c["K"] - 3
        assert np.isfinite(rows["format extremes"]).all() and np.abs(rows["format extremes"]).max() == 1e3
