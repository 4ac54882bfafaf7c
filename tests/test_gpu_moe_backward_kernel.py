"""`qbits.moe_backward` (csrc/woq_moe_bwd.hip) against the float64 autograd statement and the derived tolerance of
tests/moe_backward_reference.py.

Shapes (H, I, E, k) and routing are tests/test_gpu_moe_prompt_kernel.py's: (256, 160, 4, 2), (128, 96, 8, 3) and
(272, 160, 4, 2) — a ragged K tile on both products, 2 I and H off the step of 64, a last workgroup with dead columns — at
T = 1, 37 and 300 (expert 0: 130 rows = two blocks, the second of two rows; expert 1: exactly 128; expert 2: one; one
expert none where E = 8; one slot with the id E). Every call writes into NaN-filled rows longer than H.
"""
import numpy as np
import pytest
import torch

from tests import moe_backward_reference as BR
from tests import test_gpu_moe_kernel as K
from tests import test_gpu_moe_prompt_kernel as P

pytestmark = pytest.mark.gpu

CASES = [(s, q, t, "int4_clip", "fp32", "int64") for s in ("h256", "h128", "h272") for q in K.QUANTS for t in (1, 37, 300)] + [
    ("h128", "g32a", 37, "int8", "fp32", "int64"), ("h256", "g128s", 37, "nf4", "fp32", "int64"),
    ("h256", "g32a", 37, "int4_clip", "bf16", "int64"), ("h128", "g32a", 300, "int4_clip", "fp32", "int32")]
_OTHER = {}
# Beside the elementwise bound, which charges every rounding its worst case with one sign and so would pass a systematic
# error of a per cent: the error's norm over the reference's. Each of the three fp16 products behind dX (the recompute of
# g and u, dOut Wd^T, [dg | du] Wgu^T) rounds its two operands, 2^-11 for the row image and 2^-10 for the weight's two
# roundings: at most 3 * 2^-11 per term, 3 * 2^-11 / sqrt(3) in root mean square for roundings spread evenly, and the three
# products independent: sqrt(3) * 3 / sqrt(3) = 3 units of 2^-11, taken as 4. A 16-bit input or output adds its own
# half unit (2^-bits). dw has two of the three products behind it and the same limit.
RMS_LIMIT = 4 * 2.0 ** -11


def _experts(shape, quant, wtype):
    """K._experts for int4; the same fp weights quantised as `wtype` otherwise"""
    from intel_extension_for_transformers_amd import qbits

    if wtype == "int4_clip":
        return K._experts(shape, quant)
    if (shape, quant, wtype) not in _OTHER:
        H, I, E, _ = K.SHAPES[shape]
        group, asym, stype = K.QUANTS[quant]
        g = torch.Generator().manual_seed(3)
        blobs, deq = [], []
        for n, k in ((2 * I, H), (H, I)):
            w = 0.05 * torch.randn(E, n, k, generator=g)
            packed = [qbits.quantize_to_packed_weight(w[e].cuda(), True, group, "fp32", wtype, stype, asym) for e in range(E)]
            full = []
            for p in packed:
                out = torch.empty(k, n, dtype=torch.float32, device="cuda")
                qbits.dequantize_packed_weight(p, out, False, "fp32", wtype, stype)
                full.append(out.cpu().numpy().astype(np.float64))
            blobs.append(torch.stack(packed).view(torch.uint8))
            deq.append(full)
        _OTHER[(shape, quant, wtype)] = (blobs[0], blobs[1], deq[0], deq[1])
    return _OTHER[(shape, quant, wtype)]


def _inputs(shape, T, act):
    """P._inputs plus dOut: N(0, 1) rows times 2^e, e spread over [-8, 8]"""
    x, idx, w = P._inputs(shape, T, act, "")
    rng = np.random.default_rng(101 + T)
    dout = rng.standard_normal(tuple(x.shape)) * 2.0 ** rng.integers(-8, 9, (T, 1))
    return x, idx, w, torch.from_numpy(dout.astype(np.float32)).to(K.DTYPES[act][0])


def _run(shape, quant, T, wtype, act, itype, out_dtype=None, dout=None):
    """-> (grad_hidden, grad_weights); grad_hidden is a view into NaN-filled rows of H + 8, checked here"""
    from intel_extension_for_transformers_amd import qbits

    H = K.SHAPES[shape][0]
    gu, dn, _, _ = _experts(shape, quant, wtype)
    x, idx, w, g = _inputs(shape, T, act)
    g = g if dout is None else dout
    idx = torch.from_numpy(idx).to(torch.int64 if itype == "int64" else torch.int32)
    wide = torch.full((T, H + 8), float("nan"), dtype=out_dtype or x.dtype, device="cuda")
    gx, gw = qbits.moe_backward(g.cuda(), x.cuda(), idx.cuda(), torch.from_numpy(w).cuda(), gu, dn, grad_hidden=wide[:, :H])
    assert gx.data_ptr() == wide.data_ptr() and torch.isnan(wide[:, H:]).all() and not torch.isnan(wide[:, :H]).any()
    assert gw.dtype == torch.float32 and not torch.isnan(gw).any()
    return gx, gw


@pytest.mark.parametrize("shape,quant,T,wtype,act,itype", CASES)
def test_backward_against_float64_autograd(shape, quant, T, wtype, act, itype):
    gx, gw = _run(shape, quant, T, wtype, act, itype)
    _, _, Wgu, Wdn = _experts(shape, quant, wtype)
    x, idx, w, g = _inputs(shape, T, act)
    x64, g64 = x.float().numpy(), g.float().numpy()
    rx, rw = BR.reference(x64, idx, w, g64, Wgu, Wdn)
    bx, bw = BR.bound(x64, idx, w, g64, Wgu, Wdn, rx, 2 if wtype == "int8" else 1, K.DTYPES[act][1])
    worst, rms = [], []
    for got, ref, tol in ((gx, rx, bx), (gw, rw, bw)):
        err = np.abs(got.float().cpu().numpy().astype(np.float64) - ref)
        worst.append(float(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf)).max()))
        rms.append(float(np.linalg.norm(err) / np.linalg.norm(ref)))
    print("\nmoe backward %s %s T=%d %s %s: worst |got - ref| / bound dX %.3f dw %.3f; relative rms error dX %.2e dw %.2e (limit %.2e)"
          % (shape, quant, T, wtype, act, *worst, *rms, RMS_LIMIT + 2.0 ** -K.DTYPES[act][1]))
    assert max(worst) <= 1.0, (shape, quant, T, wtype, act, worst)
    assert max(rms) <= RMS_LIMIT + 2.0 ** -K.DTYPES[act][1], (shape, quant, T, wtype, act, rms)
    dropped = torch.from_numpy((idx < 0) | (idx >= K.SHAPES[shape][2]))
    assert (gw.cpu()[dropped].view(torch.int32) == 0).all()  # +0 exactly
    if act == "bf16":  # a bf16 grad_hidden is the fp32 one rounded once
        g32, _ = _run(shape, quant, T, wtype, act, itype, out_dtype=torch.float32)
        assert torch.equal(gx.view(torch.int16), g32.to(torch.bfloat16).view(torch.int16))


def test_two_calls_give_the_same_bytes_and_zero_gives_plus_zero():
    case = ("h128", "g32a", 300, "int4_clip", "fp32", "int64")
    (ax, aw), (bx, bw) = _run(*case), _run(*case)
    assert ax.data_ptr() != bx.data_ptr()
    assert torch.equal(ax.view(torch.int32), bx.view(torch.int32)) and torch.equal(aw.view(torch.int32), bw.view(torch.int32))
    zx, zw = _run(*case, dout=torch.zeros(300, 128))
    assert (zx.view(torch.int32) == 0).all() and (zw.view(torch.int32) == 0).all()


@pytest.mark.parametrize("what", ["dtype", "weights_dtype", "device", "shape", "stride", "workspace", "act_order"])
def test_refusals_raise_and_leave_the_output_untouched(what):
    from intel_extension_for_transformers_amd import qbits
    from tests.test_gpu_woq_backward_kernel import _blob

    H, I, E, k = K.SHAPES["h128"]
    gu, dn, _, _ = K._experts("h128", "g32a")
    x, idx, w, g = (t.cuda() if torch.is_tensor(t) else torch.from_numpy(t).cuda() for t in _inputs("h128", 5, "fp32"))
    kw = {}
    if what == "dtype":
        g = g.double()
    elif what == "weights_dtype":
        w = w.double()
    elif what == "device":
        g = g.cpu()
    elif what == "shape":
        g = g[:, :H - 4]
    elif what == "stride":
        g = torch.randn(5, 2 * H, device="cuda")[:, ::2]
    elif what == "workspace":
        kw["workspace"] = torch.empty(4096, dtype=torch.uint8, device="cuda")
    else:  # E copies of one act-order blob of the gate/up geometry
        blob = _blob(H, 2 * I, 32, "int4_clip", True, act_order=True)[1]
        gu = torch.stack([blob] * E).view(torch.uint8)
    out = torch.full((5, H), float("nan"), device="cuda")
    match = "QBits:.*%d" % qbits.moe_backward_workspace(5, k, E, H, I) if what == "workspace" else "QBits:"
    with pytest.raises(RuntimeError, match=match):
        qbits.moe_backward(g, x, idx, w, gu, dn, grad_hidden=out, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
