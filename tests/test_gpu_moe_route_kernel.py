"""`qbits.moe_route` (csrc/woq_moe_route.hip) alone against the float64 statement and the derived tolerances of
tests/moe_route_reference.py: T = 1 is the decode form (several workgroups and a ticket from E = 8 on), T = 7 / 17 / 130 the
MFMA form with a ragged last tile and several tiles; (132, 60, 4) has H no multiple of 16 or 128 and E no multiple of 16.
"""
import numpy as np
import pytest
import torch

from tests import moe_route_reference as RR

pytestmark = pytest.mark.gpu

SHAPES = [(128, 4, 2), (128, 8, 3), (256, 128, 8), (132, 60, 4), (128, 4, 1), (128, 4, 4)]
EPS = 1e-6


def _inputs(H, E, T, wdtype, norm):
    rng = np.random.default_rng(1000 * H + 10 * E + T + 14)  # + 14: every row's margin clears twice its logit band
    x = rng.standard_normal((T, H)).astype(np.float32)
    W = torch.from_numpy((0.1 * rng.standard_normal((E, H))).astype(np.float32)).to(wdtype)
    g = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32) if norm else None
    return x, W, g


def _route(x, W, k, renorm, g, **kw):
    from intel_extension_for_transformers_amd import qbits

    return qbits.moe_route(torch.from_numpy(x).cuda(), W.cuda(), k, renorm,
                           None if g is None else torch.from_numpy(g).cuda(), EPS, **kw)


def _worst(got, ref, tol):
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    assert (err[tol == 0] == 0).all()
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "plain"])
@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("renorm", [True, False], ids=["renorm", "raw"])
@pytest.mark.parametrize("T", [1, 7, 17, 130])
@pytest.mark.parametrize("H,E,k", SHAPES)
def test_router_against_float64(H, E, k, T, renorm, wdtype, norm):
    x, W, g = _inputs(H, E, T, wdtype, norm)
    ref = RR.reference(x, W.float().numpy(), k, renorm, g, EPS)
    assert (ref["margin"] > 2 * ref["band"]).all(), "inputs: a routing margin inside the logit band"
    xn, idx, w = _route(x, W, k, renorm, g)
    again = _route(x, W, k, renorm, g)
    assert np.array_equal(idx.cpu().numpy(), ref["idx"])
    r_xn, r_w = _worst(xn, ref["xn"], ref["tol_xn"]), _worst(w, ref["w"], ref["tol_w"])
    print("\nroute H=%d E=%d k=%d T=%d: worst err / tol xn %.3f w %.3f" % (H, E, k, T, r_xn, r_w))
    assert r_xn <= 1.0 and r_w <= 1.0
    for a, b in zip((xn, idx, w), again):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    if T == 1:  # the plan tables are the routing sorted by expert; asking for them changes no other byte
        *one, (srt, pos_of, blocks, nblocks) = _route(x, W, k, renorm, g, plan=True)
        for a, b in zip((xn, idx, w), one):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        order = np.argsort(ref["idx"][0], kind="stable")
        assert np.array_equal(srt.cpu().numpy(), order) and np.array_equal(pos_of.cpu().numpy(), np.argsort(order))
        want = [[int(ref["idx"][0][s]), p, 1, 0] for p, s in enumerate(order)]
        assert blocks.cpu().numpy().tolist() == want and int(nblocks) == k


@pytest.mark.parametrize("T", [1, 17])
def test_equal_rows_lower_id_first(T):
    """exactly representable values; router rows 1 and 2 are identical and lead: slots (1, 2) with equal weights"""
    x = np.tile((np.arange(128) % 5 - 2).astype(np.float32), (T, 1))
    W = np.zeros((4, 128), np.float32)
    W[1] = W[2] = x[0] / 64
    W[3] = -x[0] / 64
    _, idx, w = _route(x, torch.from_numpy(W), 2, True, None)
    assert np.array_equal(idx.cpu().numpy(), np.tile([1, 2], (T, 1)))
    assert torch.equal(w.cpu(), torch.full((T, 2), 0.5))
    x[0, 3] = np.nan  # a NaN row: ties all round, the lowest ids, NaN weights
    _, idx, w = _route(x, torch.from_numpy(W), 2, True, None)
    assert idx[0].tolist() == [0, 1] and bool(torch.isnan(w[0]).all())
