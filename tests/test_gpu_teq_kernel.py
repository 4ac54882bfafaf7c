"""The TEQ kernels alone (`qbits.teq_forward / teq_grad`, csrc/woq_teq.hip) against the float64 reference
tests/teq_reference.py, on inputs that reference has made unambiguous between fp32 and float64 arithmetic (no t and no
zero point near a half-integer, no second row near a group's max / min / max-magnitude)."""
import functools

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import qbits
from tests import quant_reference as Q
from tests import teq_reference as R

pytestmark = pytest.mark.gpu

# the kernel's three forms: (256, 96, 32) one thread per column and group (groups under 64 rows), 96 columns = one full
# and one half column block; (384, 200, 128) and (200, 70, 64) a group split over 4 threads, 64 columns a workgroup, so
# 200 and 70 columns are several workgroups with a ragged last one, and (200, 70, 64) has a short last group (8 rows:
# two rows a slice); (512, 20, -1) one group of 512 rows split over 16 threads (groups longer than 256 rows)
SHAPES = [(256, 96, 32), (384, 200, 128), (200, 70, 64), (512, 20, -1)]
CASES = [(K, N, g, bits, asym) for (K, N, g) in SHAPES for bits, asym in ((4, False), (4, True), (8, True))]
WNAME = {4: "int4_clip", 8: "int8"}
EPS = 2.0 ** -24
GRAD_SLOP = 2.0 ** -20  # times the sum of the |terms| of the row (the issue's bound)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


def _grad(w, a, g, group, bits, asym):
    out = torch.full((w.shape[0],), float("nan"), dtype=torch.float32, device="cuda")
    assert qbits.teq_grad(w, a, g, group, bits, asym, out=out) is out
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(K, N, group, bits, asym):
    """the inputs, the reference and everything the device computes for one case, once"""
    w, a, g = R.inputs(K, N, group, bits, asym, seed=K + bits)
    f = R.forward(w, a, group, bits, asym)
    da, mag = R.gradients(w, a, g, group, bits, asym, f)
    bare, _ = R.gradients(w, a, g, group, bits, asym, f, scatter=False)
    wd, ad, gd = (_dev(x) for x in (w, a, g))
    out = {dt: torch.full((K, N), float("nan"), dtype=dt, device="cuda")
           for dt in (torch.float32, torch.float16, torch.bfloat16)}
    for dt, o in out.items():
        assert qbits.teq_forward(wd, ad, group, bits, asym, out=o) is o
    grad = _grad(wd, ad, gd, group, bits, asym)
    again = _grad(wd, ad, gd, group, bits, asym)
    g16 = gd.to(torch.bfloat16)
    grad16 = _grad(wd, ad, g16, group, bits, asym)
    grad16w = _grad(wd, ad, g16.float(), group, bits, asym)
    torch.cuda.synchronize()
    return dict(w=w, a=a, g=g, f=f, da=da, mag=mag, bare=bare, wd=wd, out={dt: o.cpu() for dt, o in out.items()},
                grad=grad, again=again, grad16=grad16, grad16w=grad16w)


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_forward(K, N, group, bits, asym):
    """the codes W~ a / s imply equal the reference's at every element; |W~ - ref| <= 8 * 2^-24 |ref| (the product u,
    the range's subtraction and division inside s, the product c s and the division by a: five roundings, with room);
    the 16-bit outputs are that fp32 value rounded once; the all-zero cell gives 0"""
    c = _case(K, N, group, bits, asym)
    f = c["f"]
    g = R.group_of(K, group)[0]
    got = c["out"][torch.float32].numpy()
    sk = np.repeat(f["s"], g, axis=0)[:K]
    implied = got.astype(np.float64) * c["a"].astype(np.float64)[:, None] / sk
    codes = np.rint(implied).astype(np.int64)
    err = np.abs(got.astype(np.float64) - f["W"])
    print("forward K=%d N=%d group=%d bits=%d asym=%d: codes differing %d of %d, implied codes off an integer by %.3g, "
          "max err / |ref| %.3g eps" % (K, N, group, bits, asym, int((codes != f["q"]).sum()), K * N,
                                        np.abs(implied - codes).max(),
                                        (err / np.where(f["W"] == 0, 1.0, np.abs(f["W"]))).max() / EPS))
    assert np.isfinite(got).all()
    assert np.abs(implied - codes).max() < 0.01  # an integer, unmistakably
    assert np.array_equal(codes, f["q"]), np.argwhere(codes != f["q"])[:4]
    assert (err <= 8 * EPS * np.abs(f["W"])).all(), np.argwhere(err > 8 * EPS * np.abs(f["W"]))[:4]
    assert not got[:g, 0].any()  # the all-zero cell
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(c["out"][dt], c["out"][torch.float32].to(dt)), dt  # that value rounded once


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_unit_scale_is_the_rtn_blob(K, N, group, bits, asym):
    """a = 1: W~ is bit-equal to the package's RTN, quantised and dequantised, at 4 bits. At 8 bits that cannot hold
    together with W~ being the rule's one product (c - z) s: the package stores int8 as two int4 planes and dequantises
    it as two products and a sum (tests/test_gpu_autoround_kernel.py and tests/test_gpu_awq_kernel.py make the same
    exception); there W~ is within levels * FP32_SLOP steps of the blob's value (the two extra roundings,
    quant_reference.bounds' form) and its implied codes and the blob's scales are the rule's."""
    c = _case(K, N, group, bits, asym)
    wd = c["wd"]
    got = qbits.teq_forward(wd, torch.ones(K, device="cuda"), group, bits, asym)
    blob = qbits.quantize_to_packed_weight(wd, False, group, "fp32", WNAME[bits], "fp32", asym)
    deq = torch.empty(K, N, dtype=torch.float32, device="cuda")
    qbits.dequantize_packed_weight(blob, deq, False, "fp32", WNAME[bits], "fp32")
    print("rtn K=%d N=%d group=%d bits=%d asym=%d: elements differing %d" % (K, N, group, bits, asym,
                                                                             int((got != deq).sum())))
    if bits == 4:
        assert torch.equal(got, deq)
    else:
        g = R.group_of(K, group)[0]
        scale = qbits.acquire_packed_weight_info(blob, 9)
        step = scale.repeat_interleave(g, 0)[:K].double()
        assert ((got.double() - deq.double()).abs() <= R.consts(bits)[0] * Q.FP32_SLOP * step).all()
        f = R.forward(c["w"], np.ones(K), group, bits, asym)
        assert np.array_equal(np.rint(got.double().cpu().numpy() / step.cpu().numpy()).astype(np.int64), f["q"])


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_gradient(K, N, group, bits, asym):
    """|da_dev - da_ref| <= B[k] = 2^-20 * the sum of the |terms| of row k (summed in the reference), da finite
    everywhere, and the scatter terms E really there: the reference without them is further than B from the reference
    on most of the rows an E term lands on, and the device is within B of the full one on every row.
    The worst err / B per case is printed. Measured on the MI355X over the twelve cases (profiles/r18_teq.txt): the
    largest is 0.065 (512 x 20, one group of 512 rows, 4 bits sym), 0.014 - 0.026 for the grouped shapes; a
    sequentially summed fp32 restatement of the closed form on the CPU reaches 0.056. The constant is left at the
    issue's 2^-20."""
    c = _case(K, N, group, bits, asym)
    B = GRAD_SLOP * c["mag"]
    err = np.abs(c["grad"].astype(np.float64) - c["da"])
    ratio = (err / np.where(B == 0, 1.0, B)).max()
    landed = np.abs(c["da"] - c["bare"]) > 0
    moved = np.abs(c["da"] - c["bare"]) > B
    print("grad K=%d N=%d group=%d bits=%d asym=%d: max err %.3g, worst err / B %.4f, rows with B = 0: %d, rows an E "
          "lands on %d, of them moved by more than B %d"
          % (K, N, group, bits, asym, err.max(), ratio, int((B == 0).sum()), int(landed.sum()),
             int((moved & landed).sum())))
    assert np.isfinite(c["grad"]).all()
    assert (err <= B).all(), np.argwhere(err > B)[:4]
    assert landed.sum() >= min(N, R.group_of(K, group)[0]) // 4 and (moved & landed).sum() > 0.5 * landed.sum()
    # so a device result without E could not pass: it would sit at `bare`, further than B from the reference there
    assert (np.abs(c["grad"].astype(np.float64) - c["bare"]) > B)[moved].all()


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_zero_cell_gives_nothing_through_s(K, N, group, bits, asym):
    """the all-zero first group of column 0 has s replaced by 1: no E term from it. With g zero outside that cell's
    column the gradient of the group's rows is exactly that column's direct terms, all 0 (w = 0 there)."""
    c = _case(K, N, group, bits, asym)
    g0 = R.group_of(K, group)[0]
    g = np.zeros_like(c["g"])
    g[:, 0] = c["g"][:, 0]
    got = _grad(c["wd"], _dev(c["a"]), _dev(g), group, bits, asym)
    want, mag = R.gradients(c["w"], c["a"], g, group, bits, asym, c["f"])
    assert not want[:g0].any() and not got[:g0].any()
    assert (np.abs(got.astype(np.float64) - want) <= GRAD_SLOP * mag).all()
    if K > g0:
        assert got[g0:].any()


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_same_bytes_twice_and_bf16_gradient(K, N, group, bits, asym):
    c = _case(K, N, group, bits, asym)
    assert np.array_equal(c["grad"], c["again"])
    assert np.array_equal(c["grad16"], c["grad16w"])  # g as bf16 = that bf16 value widened to fp32
    assert not np.array_equal(c["grad16"], c["grad"])  # and it is the bf16 value that was read


def test_gradient_with_a_workspace_set():
    """the launcher's scratch from `set_woq_workspace`: the same bytes as from its own allocation"""
    K, N, group, bits, asym = 384, 200, 128, 4, True
    c = _case(K, N, group, bits, asym)
    ws = torch.empty(1 << 20, dtype=torch.int8, device="cuda")
    qbits.set_woq_workspace(ws)
    try:
        got = _grad(c["wd"], _dev(c["a"]), _dev(c["g"]), group, bits, asym)
    finally:
        qbits.set_woq_workspace(torch.empty(0, dtype=torch.int8, device="cuda"))
    assert np.array_equal(got, c["grad"])


def test_launchers_refuse_what_they_cannot_run():
    K, N, group = 64, 32, 32
    w = torch.zeros(K, N, device="cuda")
    a = torch.ones(K, device="cuda")
    g = torch.zeros(K, N, device="cuda")
    out = torch.full((K, N), 7.0, device="cuda")
    da = torch.full((K,), 7.0, device="cuda")
    bad = [
        (w.half(), a),                                    # wrong dtype
        (w, a.double()),
        (torch.zeros(N, K, device="cuda").t(), a),        # not contiguous
        (w, torch.ones(2 * K, device="cuda")[::2]),
        (w, torch.ones(K + 1, device="cuda")),            # a of the wrong length
        (w, torch.ones(K, 1, device="cuda")),
        (w.cpu(), a),                                     # not on the device
        (w, a.cpu()),
    ]
    for args in bad:
        with pytest.raises(RuntimeError, match="QBits: teq_forward"):
            qbits.teq_forward(*args, group, 4, True, out=out)
        with pytest.raises(RuntimeError, match="QBits: teq_grad"):
            qbits.teq_grad(*args, g, group, 4, True, out=da)
    for bad_g in (g.double(), torch.zeros(N, K, device="cuda").t(), torch.zeros(K, N + 1, device="cuda"), g.cpu()):
        with pytest.raises(RuntimeError, match="QBits: teq_grad"):
            qbits.teq_grad(w, a, bad_g, group, 4, True, out=da)
    with pytest.raises(RuntimeError, match="QBits: teq_grad"):
        qbits.teq_grad(w, a, g, group, 4, True, out=torch.zeros(K + 1, device="cuda"))
    with pytest.raises(RuntimeError, match="QBits: teq_forward"):
        qbits.teq_forward(w, a, group, 4, True, out=torch.zeros(K, N, dtype=torch.float64, device="cuda"))
    for bits in (1, 5, 16):  # the launchers' own refusal
        with pytest.raises(RuntimeError, match="QBits: teq_forward: bits must be 2, 3, 4 or 8"):
            qbits.teq_forward(w, a, group, bits, True, out=out)
        with pytest.raises(RuntimeError, match="QBits: teq_grad: bits must be 2, 3, 4 or 8"):
            qbits.teq_grad(w, a, g, group, bits, True, out=da)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0)) and torch.equal(da, torch.full_like(da, 7.0))  # nothing ran
