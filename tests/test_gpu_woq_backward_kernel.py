"""`qbits.woq_linear_backward` (csrc/woq_linear_bwd.hip) alone against the float64 statement of
tests/woq_backward_reference.py. Every call writes into a NaN-filled output whose rows are longer than K, from a
gradient buffer whose rows are longer than N with NaN in the gaps and in rows beyond M."""
import functools

import numpy as np
import pytest
import torch

from tests import woq_backward_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(256, 96, 32), (384, 200, 128), (200, 70, 64), (512, 20, -1)]  # ragged K, N off 16 and off the n step of 64,
# a short last group, both scale modes
ROWS = [1, 17, 130, 300]  # under one fragment, a ragged fragment, two workgroups, a ragged third
WTYPES = [("int4_clip", False), ("int4_clip", True), ("int8", True)]
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the reference's arrays are read-only


def _pack(d, wname, group):
    from intel_extension_for_transformers_amd import qbits

    e8, e32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)
    return qbits.repack_quantized_weight(_dev(d["q"]), _dev(d["s"]), e8 if d["z"] is None else _dev(d["z"]),
                                         e32 if d["g_idx"] is None else _dev(d["g_idx"]), wname, "fp32", "bf16",
                                         d["z"] is not None, group)


@functools.lru_cache(maxsize=None)
def _blob(K, N, group, wname, asym, act_order=False):
    d = R.weight(K, N, group, wname, asym, act_order)
    return d, _pack(d, wname, group)


@functools.lru_cache(maxsize=None)
def _grad(M, N):
    dY = R.gradient(M, N, seed=M + N)
    dY.setflags(write=False)
    return dY


def _run(blob, dY, K, gdtype=torch.float32, odtype=torch.float32, pad=(5, 3)):
    """dY: torch tensor [M, N] (host or device) -> the [M, K] result as a host tensor of odtype; checks the gaps"""
    from intel_extension_for_transformers_amd import qbits

    M, N = dY.shape
    gbuf = torch.full((M + 2, N + pad[0]), float("nan"), dtype=gdtype, device="cuda")
    gbuf[:M, :N] = dY.to("cuda", gdtype)
    obuf = torch.full((M + 1, K + pad[1]), float("nan"), dtype=odtype, device="cuda")
    got = qbits.woq_linear_backward(gbuf[:M, :N], blob, grad_input=obuf[:M, :K])
    assert got.data_ptr() == obuf.data_ptr()
    torch.cuda.synchronize()
    host = obuf.cpu()
    assert torch.isnan(host[:M, K:]).all() and torch.isnan(host[M:]).all(), "the call wrote outside [M, K]"
    assert not torch.isnan(host[:M, :K]).any(), "NaN reached the output (or an element was not written)"
    return host[:M, :K].clone()


def _check(got, dY, d):
    ref, S = R.backward(dY, d["W"], d["shuffle"])
    tol = R.bound(dY, d["W"], S)
    err = np.abs(got.double().numpy() - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print("worst error / bound = %.3f" % worst)
    assert (err <= tol).all(), "worst error / bound = %.3f at %s" % (worst, np.unravel_index((err / np.maximum(
        tol, 1e-300)).argmax(), err.shape))


@pytest.mark.parametrize("wname,asym", WTYPES)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N,group", SHAPES)
def test_backward_vs_float64(K, N, group, M, wname, asym):
    d, blob = _blob(K, N, group, wname, asym)
    dY = _grad(M, N)
    _check(_run(blob, torch.from_numpy(dY.copy()), K), dY, d)


@pytest.mark.parametrize("wname,K,N,group", [("nf4", 256, 96, 32), ("fp4_e2m1", 384, 200, 128),
                                             ("fp4_e2m1_bnb", 200, 70, 64), ("int3_clip", 200, 70, 64),
                                             ("int2_clip", 512, 20, -1)])
def test_backward_other_weight_types(wname, K, N, group):
    d, blob = _blob(K, N, group, wname, False)
    dY = _grad(130, N)
    _check(_run(blob, torch.from_numpy(dY.copy()), K), dY, d)


@pytest.mark.parametrize("M", [17, 300])
def test_backward_act_order(M):
    """the result lands in column shuffle[j]: the transpose of the forward's gather"""
    K, N, group = 384, 200, 128
    d, blob = _blob(K, N, group, "int4_clip", False, True)
    dY = _grad(M, N)
    _check(_run(blob, torch.from_numpy(dY.copy()), K), dY, d)


@pytest.mark.parametrize("gname", ["bf16", "fp16"])
def test_16bit_gradients_and_outputs(gname):
    """a 16-bit gradient is taken as the values it holds; a 16-bit output is the fp32 output rounded once"""
    K, N, group = 384, 200, 128
    d, blob = _blob(K, N, group, "int4_clip", True)
    g16 = torch.from_numpy(R.gradient(130, N, seed=5, span=6 if gname == "fp16" else 30)).to(TORCH[gname])
    dY = g16.double().numpy()
    out32 = _run(blob, g16, K, gdtype=TORCH[gname])
    _check(out32, dY, d)
    for oname in ("bf16", "fp16"):
        out16 = _run(blob, g16, K, gdtype=TORCH[gname], odtype=TORCH[oname])
        assert torch.equal(out16, out32.to(TORCH[oname])), oname


@pytest.mark.parametrize("K,N,group,asym", [(256, 96, 32, True), (384, 200, 128, False), (200, 70, 64, True),
                                            (512, 20, -1, False)])
def test_one_hot_rows_return_the_weight(K, N, group, asym):
    """dY = I_N returns the dequantised weight to two 11-bit roundings: every nibble, scale and zero point of the
    tile walk is pinned"""
    d = R.uniform_weight(K, N, group, asym, seed=K)
    blob = _pack(d, "int4_clip", group)
    got = _run(blob, torch.eye(N), K).double().numpy()
    W = d["W"]
    err = np.abs(got - W.T)
    assert (err <= 2.0 ** -10 * np.abs(W.T)).all(), float((err / np.maximum(np.abs(W.T), 1e-300)).max())


def test_same_bytes_twice_scaling_and_zero():
    K, N, group = 384, 200, 128
    d, blob = _blob(K, N, group, "int4_clip", True)
    dY = torch.from_numpy(R.gradient(130, N, seed=9, span=0))
    a, b = _run(blob, dY, K), _run(blob, dY, K)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a second call gave other bytes"
    # rows scaled by powers of two: the results scale exactly
    e = torch.where(torch.arange(130) % 2 == 0, 40, -40).double()
    scaled = _run(blob, (dY.double() * torch.exp2(e)[:, None]).float(), K)
    assert torch.equal(scaled.double(), a.double() * torch.exp2(e)[:, None])
    z = _run(blob, torch.zeros(17, N), K)
    assert torch.equal(z.view(torch.int32), torch.zeros(17, K, dtype=torch.int32)), "dY = 0 must give +0 everywhere"


def test_refusals_launch_nothing():
    from intel_extension_for_transformers_amd import qbits

    K, N, group = 256, 96, 32
    _, blob = _blob(K, N, group, "int4_clip", False)
    g = torch.ones(4, N, device="cuda")
    out = torch.full((4, K), float("nan"), device="cuda")

    def refused(*a, **kw):
        with pytest.raises(RuntimeError, match="QBits:"):
            qbits.woq_linear_backward(*a, **kw)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), "a refused call wrote to the output"

    refused(g.to(torch.float64), blob, grad_input=out)                      # dtype
    refused(g, blob, grad_input=out.to(torch.float64))
    refused(g.cpu(), blob, grad_input=out)                                  # device
    refused(g, blob, grad_input=torch.empty(4, K))
    refused(g[:, : N - 1], blob, grad_input=out)                            # shape
    refused(g, blob, grad_input=out[:3])
    refused(torch.ones(N, 4, device="cuda").t(), blob, grad_input=out)      # rows without unit stride
    refused(g, blob, grad_input=out, dtype=torch.float16)
    need = qbits.woq_linear_backward_workspace(4, blob)
    assert need == 2 * 128 * 128 + 512 + 256  # the header's formula: Mpad 128, N 96 -> 128
    small = torch.empty(need - 256, dtype=torch.uint8, device="cuda")
    qbits.set_woq_workspace(small)
    try:
        with pytest.raises(RuntimeError, match="QBits:.*%d" % need):
            qbits.woq_linear_backward(g, blob, grad_input=out)
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    finally:
        qbits.set_woq_workspace(None)
    # the sizing function does not grow with K
    _, wide = _blob(512, 20, -1, "int4_clip", False)
    assert qbits.woq_linear_backward_workspace(4, wide) == 2 * 128 * 64 + 512 + 256
    # and a caller's workspace of exactly that size is enough
    qbits.set_woq_workspace(torch.empty(need, dtype=torch.uint8, device="cuda"))
    try:
        qbits.woq_linear_backward(g, blob, grad_input=out)
        torch.cuda.synchronize()
        assert not torch.isnan(out).any()
    finally:
        qbits.set_woq_workspace(None)
