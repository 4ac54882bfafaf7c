"""The GPTQ sweep kernel alone (`qbits.gptq_sweep`, csrc/woq_gptq.hip) against tests/gptq_reference.py:
  identity  U = I: codes, scales and zero points are the RTN quantiser's, exactly
  lattice   every operation exact in fp32: codes, scales and errors equal the float64 reference bit for bit, ties too
  replay    realistic values: each step held to the definition with the device's own earlier errors as the givens
Blocks of a weight with more than 128 rows are swept one launch each, the rows after a block updated by one fp32 GEMM
in between, as the driver does."""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import qbits
from tests import gptq_reference as G
from tests import quant_reference as Q

pytestmark = pytest.mark.gpu

SHAPES = [(128, 64, 32), (160, 96, 64), (256, 200, 128), (256, 96, -1), (256, 64, 256), (160, 200, 128)]
TYPES = [(4, False), (4, True), (8, False), (8, True), (3, False), (3, True), (2, False), (2, True)]


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


def _sweep_all(w, u, group, bits, asym, scale=None, zp=None, params_given=False, col_group=None, each=None):
    """sweep every block of w (numpy fp32 [K, N]) on the device -> numpy (q int64 in the rule's domain, scale float64,
    zp int64 in the rule's domain or None, err fp32 [K, N], w fp32 after). `each(c0, B, w_entry, out)` sees every block:
    the weight at its entry and the device's results after it."""
    K, N = w.shape
    g, n_groups = Q.group_of(K, group)
    off = 2 ** (bits - 1)
    wd, ud = _dev(w, torch.float32), _dev(u, torch.float32)
    qd = torch.zeros(K, N, dtype=torch.int8, device="cuda")
    sd = _dev(scale, torch.float32) if scale is not None else torch.zeros(n_groups, N, device="cuda")
    zd = None
    if asym:
        zd = _dev(np.asarray(zp) - off, torch.int8) if zp is not None else torch.zeros(n_groups, N, dtype=torch.int8,
                                                                                       device="cuda")
    cg = _dev(col_group, torch.int32) if col_group is not None else None
    errs = torch.zeros(K, N, device="cuda")

    def host():
        q = qd.cpu().numpy().astype(np.int64)
        return dict(q=q + off if asym else q, scale=sd.cpu().numpy().astype(np.float64),
                    zp=zd.cpu().numpy().astype(np.int64) + off if asym else None, err=errs.cpu().numpy(),
                    w=wd.cpu().numpy())

    for c0 in range(0, K, 128):
        B = min(128, K - c0)
        entry = wd.cpu().numpy() if each else None
        err = torch.zeros(B, N, device="cuda")
        qbits.gptq_sweep(wd, ud, c0, B, group, bits, asym, qd, sd, zd, err, params_given, cg)
        errs[c0:c0 + B] = err
        if each:
            each(c0, B, entry, host())
        if c0 + B < K:
            wd[c0 + B:].addmm_(ud[c0:c0 + B, c0 + B:].t(), err, alpha=-1.0)
    torch.cuda.synchronize()
    return host()


@pytest.mark.parametrize("bits,asym", TYPES)
@pytest.mark.parametrize("K,N,group", SHAPES)
def test_identity_factor_is_the_rtn_quantiser(K, N, group, bits, asym):
    wname = G.WNAME[bits]
    w, fam, _ = Q.families(K, N, group, wname, asym)
    out = _sweep_all(w, np.eye(K, dtype=np.float32), group, bits, asym)
    Q.check(w, group, wname, "fp32", asym, out["scale"], out["zp"], out["w"], fam)
    # the package's own RTN quantiser on the same weight: the same scales, zero points and codes, exactly
    blob = qbits.quantize_to_packed_weight(_dev(w, torch.float32), False, group, "fp32", wname, "fp32", asym)
    s = qbits.acquire_packed_weight_info(blob, 9).cpu().numpy().astype(np.float64)
    assert np.array_equal(out["scale"], s)
    off = 2 ** (bits - 1)
    z = None
    if asym:
        z = qbits.acquire_packed_weight_info(blob, 10).cpu().numpy().astype(np.int64) + off
        assert np.array_equal(out["zp"], z)
    deq = torch.empty(K, N, dtype=torch.float32, device="cuda")
    qbits.dequantize_packed_weight(blob, deq, False, "fp32", wname, "fp32")
    g, _ = Q.group_of(K, group)
    rows = np.arange(K) // g
    codes = np.rint(deq.cpu().numpy().astype(np.float64) / s[rows]).astype(np.int64) + (z[rows] if asym else 0)
    assert np.array_equal(out["q"], codes)
    assert np.array_equal(out["err"], np.asarray(w - out["w"], np.float32))  # u_jj = 1: the error is w - d, one rounding


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("K,N,group", SHAPES[:5])
def test_lattice_bit_exact(K, N, group, bits):
    w, u = G.lattice(K, N, group, bits)
    cur, scale = w.astype(np.float64), None
    q, errs = np.zeros((K, N), np.int64), []
    for c0 in range(0, K, 128):
        B = min(128, K - c0)
        r = G.sweep_block(cur, u, c0, B, group, bits, False, scale)
        cur, scale = r["w"], r["scale"]
        q[c0:c0 + B] = r["q"][c0:c0 + B]
        errs.append(r["err"])
        cur[c0 + B:] -= u[c0:c0 + B, c0 + B:].T.astype(np.float64) @ r["err"]
    err = np.concatenate(errs)
    assert (np.abs(err) == 0.5).sum() > N  # exact ties are there to be resolved
    out = _sweep_all(w, u, group, bits, False)
    assert np.array_equal(out["scale"], scale) and (scale == 1.0).all()
    assert np.array_equal(out["q"], q), np.argwhere(out["q"] != q)[:4]
    assert np.array_equal(out["err"].astype(np.float64), err)
    assert np.array_equal(out["w"].astype(np.float64), cur)


def _factor(H, damp=0.01):
    Hd = np.array(H, np.float64)
    Hd[np.diag_indices_from(Hd)] += damp * np.mean(np.diag(Hd))
    return G.upper_factor(Hd).astype(np.float32)


@pytest.mark.parametrize("bits,asym", [(4, False), (4, True), (8, True), (3, False), (2, True)])
@pytest.mark.parametrize("K,N,group", SHAPES)
def test_replay(K, N, group, bits, asym):
    w, H = G.correlated(K, N, seed=K + N)
    u = _factor(H)
    worst = dict(code=0.0, err=0.0, scale=0.0, zp=0.0)

    def each(c0, B, entry, out):
        rep = G.replay_check(entry, u, c0, B, group, bits, asym, out["q"], out["scale"], out["zp"],
                             out["err"][c0:c0 + B], out["w"])
        for key, v in rep.items():
            worst[key] = max(worst[key], v)

    out = _sweep_all(w, u, group, bits, asym, each=each)
    print("replay K=%d N=%d group=%d bits=%d asym=%d: largest err / bound %s" % (K, N, group, bits, asym, worst))
    # the sweep did something: later rows moved, and not by rounding noise
    rtn = Q.quantize(w, group, G.WNAME[bits], asym)
    assert (out["q"] != rtn["code"]).mean() > 0.01


@pytest.mark.parametrize("bits,asym", [(4, False), (4, True), (8, False)])
@pytest.mark.parametrize("K,N,group", [(160, 96, 32), (256, 200, 64)])
def test_replay_given_parameters_and_row_groups(K, N, group, bits, asym):
    """static groups under an act-order permutation: parameters are read, each working row's group comes from
    col_group"""
    w, H = G.correlated(K, N, seed=7)
    W, Hd, perm, scale0, zp0 = G.prepare(w, H, group, bits, asym, 0.01, True, True)
    u = G.upper_factor(Hd).astype(np.float32)
    col_group = perm // group
    wp = W.astype(np.float32)

    def each(c0, B, entry, out):
        G.replay_check(entry, u, c0, B, group, bits, asym, out["q"], out["scale"], out["zp"], out["err"][c0:c0 + B],
                       out["w"], params_given=True, col_group=col_group)

    out = _sweep_all(wp, u, group, bits, asym, scale=scale0, zp=zp0, params_given=True, col_group=col_group, each=each)
    assert np.array_equal(out["scale"], scale0.astype(np.float32).astype(np.float64))  # read, not written
    if asym:
        assert np.array_equal(out["zp"], zp0)


def test_launcher_refuses_what_it_cannot_sweep():
    w = torch.zeros(160, 64, device="cuda")
    u = torch.eye(160, device="cuda")
    q = torch.zeros(160, 64, dtype=torch.int8, device="cuda")
    s = torch.zeros(5, 64, device="cuda")
    err = torch.zeros(128, 64, device="cuda")
    with pytest.raises(RuntimeError, match="QBits"):
        qbits.gptq_sweep(w, u, 128, 64, 32, 4, False, q, s, None, err)  # the block runs past the weight
    with pytest.raises(RuntimeError, match="QBits"):
        qbits.gptq_sweep(w, u, 0, 128, 32, 5, False, q, s, None, err)  # bits
    with pytest.raises(RuntimeError, match="QBits"):
        qbits.gptq_sweep(w, u, 0, 128, 32, 4, True, q, s, None, err)  # asym without zero points
    with pytest.raises(RuntimeError, match="QBits"):
        qbits.gptq_sweep(w, u, 16, 128, 32, 4, False, q, s, None, err)  # a group start off the 32-row grid
