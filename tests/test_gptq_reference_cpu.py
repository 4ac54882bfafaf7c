"""tests/gptq_reference.py held to what it claims, without a GPU: with U = I it is the RTN rule; the lattice family
is exact in fp32 (so the device must reproduce it bit for bit); on correlated inputs it beats RTN by a margin (so the
GPU tests' "below the RTN loss" says something)."""
import numpy as np
import pytest

from tests import gptq_reference as G
from tests import quant_reference as Q


@pytest.mark.parametrize("bits,asym", [(4, False), (4, True), (8, False), (3, True), (2, False)])
@pytest.mark.parametrize("K,N,group", [(128, 24, 32), (160, 24, 64), (96, 17, 128)])
def test_identity_factor_is_rtn(K, N, group, bits, asym):
    """U = I: no error reaches another row, so codes, scales and zero points are quant_reference.quantize's."""
    w, _, _ = Q.families(K, N, group, G.WNAME[bits], asym)
    ref = Q.quantize(w, group, G.WNAME[bits], asym)
    scale = zp = None
    q = np.zeros((K, N), np.int64)
    cur = w.astype(np.float64)
    for c0 in range(0, K, 128):
        B = min(128, K - c0)
        r = G.sweep_block(cur, np.eye(K), c0, B, group, bits, asym, scale, zp)
        cur, scale, zp = r["w"], r["scale"], r["zp"]
        q[c0:c0 + B] = r["q"][c0:c0 + B]
    assert np.array_equal(q, ref["code"])
    assert np.array_equal(scale, ref["s"])
    if asym:
        assert np.array_equal(zp, ref["z"])
    assert np.array_equal(cur, ref["deq"])


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("K,N,group", [(128, 64, 32), (160, 96, 64), (256, 200, 128), (256, 64, -1)])
def test_lattice_is_exact_in_fp32(K, N, group, bits):
    """Every operation on the lattice family is exact in fp32: a float32 run equals the float64 one bit for bit, every
    scale is 1, nothing but the planted rows reaches the range's end, and exact ties occur."""
    w, u = G.lattice(K, N, group, bits)
    g, _ = Q.group_of(K, group)
    outs = []
    for dtype in (np.float64, np.float32):
        cur, scale = w.astype(dtype), None
        q, errs = np.zeros((K, N), np.int64), []
        for c0 in range(0, K, 128):
            B = min(128, K - c0)
            r = G.sweep_block(cur, u, c0, B, group, bits, False, scale, None, dtype=dtype)
            cur, scale = r["w"], r["scale"]
            q[c0:c0 + B] = r["q"][c0:c0 + B]
            errs.append(r["err"])
            cur[c0 + B:] -= (u[c0:c0 + B, c0 + B:].T.astype(dtype) @ r["err"]).astype(dtype)
        outs.append((q, scale, np.concatenate(errs), cur))
    (q64, s64, e64, w64), (q32, s32, e32, w32) = outs
    assert e32.dtype == np.float32 and w32.dtype == np.float32
    assert np.array_equal(q64, q32) and np.array_equal(s64, s32)
    assert np.array_equal(e64, e32.astype(np.float64)) and np.array_equal(w64, w32.astype(np.float64))
    assert (s64 == 1.0).all()
    qmax = 2 ** (bits - 1) - 1
    inner = np.ones(K, bool)
    inner[::g] = False
    assert np.abs(q64[inner]).max() < qmax and np.abs(e64).max() == 0.5
    assert (np.abs(e64) == 0.5).sum() > N  # exact ties, resolved half to even in both runs


@pytest.mark.parametrize("desc_act,static_groups", [(False, False), (True, False), (True, True)])
def test_reference_beats_rtn_on_correlated_inputs(desc_act, static_groups):
    K, N, group = 256, 96, 64
    w, H = G.correlated(K, N, seed=0)
    r = G.quantize_weight(w, H, 4, group, True, damp_percent=0.01, desc_act=desc_act, static_groups=static_groups)
    rtn = Q.quantize(w, group, "int4_clip")
    deq = G.dequantize(r["q"], r["scale"], r["zp"], group, r["g_idx"])
    assert np.allclose(deq, r["deq"], rtol=0, atol=1e-12)
    loss, loss_rtn = G.hessian_loss(w, deq, r["Hd"]), G.hessian_loss(w, rtn["deq"], r["Hd"])
    print("gptq %.4f rtn %.4f ratio %.3f (sum err^2 %.4f)" % (loss, loss_rtn, loss / loss_rtn, 2 * r["loss"]))
    assert loss < 0.75 * loss_rtn
    if not static_groups:  # no clipping to speak of: the sweep's own account of the loss is the Hessian's
        assert abs(2 * r["loss"] - loss) <= 0.02 * loss
    if r["g_idx"] is not None:
        assert sorted(np.bincount(r["g_idx"]).tolist()) == [group] * (K // group)


def test_replay_check_accepts_the_reference_and_rejects_a_wrong_factor():
    """replay_check on a float32 run of the reference itself passes; with one element of U changed it fails."""
    K, N, group = 128, 24, 32
    w, H = G.correlated(K, N, seed=1)
    _, Hd, _, _, _ = G.prepare(w, H, group, 4, False, 0.01, False, False)
    u = G.upper_factor(Hd).astype(np.float32)
    r = G.sweep_block(w, u, 0, K, group, 4, False, dtype=np.float32)
    rep = G.replay_check(w, u, 0, K, group, 4, False, r["q"], r["scale"], None, r["err"], r["w"])
    assert rep["err"] <= 1 and rep["code"] <= 1
    bad = u.copy()
    bad[3, 40] *= 1.5
    with pytest.raises(AssertionError):
        G.replay_check(w, bad, 0, K, group, 4, False, r["q"], r["scale"], None, r["err"], r["w"])
