"""The AutoRound kernels alone (`qbits.autoround_forward / autoround_step / autoround_codes`, csrc/woq_autoround.hip)
against the float64 reference tests/autoround_reference.py, on inputs that reference has made unambiguous between fp32
and float64 arithmetic (no t and no zero point near a half-integer, no sym side near a tie)."""
import functools

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import qbits
from tests import autoround_reference as R
from tests import quant_reference as Q

pytestmark = pytest.mark.gpu

# the kernel's three paths: (256, 96, 32) one thread per column and group (groups under 64 rows); (384, 200, 128) and
# (200, 70, 64) a group split over 4 threads, 64 columns a workgroup, so 200 and 70 columns are several workgroups with
# a ragged last one, and (200, 70, 64) has a short last group (8 rows: two rows a slice); (512, 20, -1) one group of
# 512 rows, split over 16 threads (groups longer than 256 rows)
SHAPES = [(256, 96, 32), (384, 200, 128), (200, 70, 64), (512, 20, -1)]
CASES = [(K, N, g, 4, asym) for (K, N, g) in SHAPES for asym in (True, False)] + [(256, 96, 32, 8, True)]
WNAME = {4: "int4_clip", 8: "int8"}
LR_V, LR_MM = 2.0 ** -7, 2.0 ** -6
EPS = 2.0 ** -24
GRAD_SLOP = 2.0 ** -20  # times the rows of the group times the sum of the |terms| (the issue's bound)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _step(w, V, alpha, beta, g, group, bits, asym):
    """one step on copies -> (V', alpha', beta', dalpha, dbeta) as numpy"""
    v, a, b = _dev(V), _dev(alpha), _dev(beta)
    da, db = _nan(*alpha.shape), _nan(*alpha.shape)
    qbits.autoround_step(w, v, a, b, g, group, bits, asym, LR_V, LR_MM, da, db)
    return tuple(t.cpu().numpy() for t in (v, a, b, da, db))


@functools.lru_cache(maxsize=None)
def _case(K, N, group, bits, asym):
    """the inputs, the reference and everything the device computes for one case, once"""
    w, V, alpha, beta, g = R.inputs(K, N, group, bits, asym, seed=K + bits)
    f = R.forward(w, V, alpha, beta, group, bits, asym)
    gr = R.gradients(w, V, alpha, beta, g, group, bits, asym, f)
    wd, vd, ad, bd, gd = (_dev(x) for x in (w, V, alpha, beta, g))
    q, scale, zp = qbits.autoround_codes(wd, vd, ad, bd, group, bits, asym)
    out = {dt: torch.full((K, N), float("nan"), dtype=dt, device="cuda")
           for dt in (torch.float32, torch.float16, torch.bfloat16)}
    for dt, o in out.items():
        assert qbits.autoround_forward(wd, vd, ad, bd, group, bits, asym, out=o) is o
    step = _step(wd, V, alpha, beta, gd, group, bits, asym)
    again = _step(wd, V, alpha, beta, gd, group, bits, asym)
    g16 = gd.to(torch.bfloat16)
    step16 = _step(wd, V, alpha, beta, g16, group, bits, asym)
    step16w = _step(wd, V, alpha, beta, g16.float(), group, bits, asym)
    torch.cuda.synchronize()
    return dict(w=w, V=V, alpha=alpha, beta=beta, g=g, f=f, gr=gr, wd=wd, q=q.cpu().numpy(), scale=scale.cpu().numpy(),
                zp=None if zp is None else zp.cpu().numpy(), out={dt: o.cpu() for dt, o in out.items()}, step=step,
                again=again, step16=step16, step16w=step16w)


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_forward_and_codes(K, N, group, bits, asym):
    c = _case(K, N, group, bits, asym)
    f = c["f"]
    g, G = R.group_of(K, group)
    L, qmax, off = R.consts(bits)
    assert c["q"].dtype == np.int8 and c["scale"].shape == (G, N)
    codes = c["q"].astype(np.int64) + (off if asym else 0)
    print("forward K=%d N=%d group=%d bits=%d asym=%d: codes differing %d of %d, clipped %.1f%%, max scale err %.3g"
          % (K, N, group, bits, asym, int((codes != f["c"]).sum()), K * N, 100 * f["clipped"].mean(),
             (np.abs(c["scale"] - f["s"]) / f["s"]).max()))
    assert np.array_equal(codes, f["c"]), np.argwhere(codes != f["c"])[:4]
    assert (np.abs(c["scale"].astype(np.float64) - f["s"]) <= Q.FP32_SLOP * f["s"]).all()
    assert c["scale"][0, 0] == 1.0  # the all-zero cell
    if asym:
        assert np.array_equal(c["zp"].astype(np.int64) + off, f["z"])
    else:
        assert c["zp"] is None
    # W~ = (c - z) s: one fp32 product with the device's own scale
    sk = np.repeat(c["scale"], g, axis=0)[:K]
    want = f["q"].astype(np.float32) * sk
    got = c["out"][torch.float32]
    assert np.array_equal(got.numpy(), want)
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(c["out"][dt], got.to(dt)), dt  # that value rounded once


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_neutral_parameters_are_the_rtn_blob(K, N, group, bits, asym):
    """V = 0, alpha = beta = 1: bit-equal to the package's RTN, quantised and dequantised.

    At 4 bits W~ itself is bit-equal to the dequantised RTN blob. At 8 bits that cannot hold together with W~ being the
    rule's one product (c - z) s (test_forward_and_codes): the package stores int8 as two int4 planes and dequantises it
    as two products and a sum (tests/test_gpu_awq_kernel.py makes the same exception), 3292 of 24576 elements differ in
    the last bit on the MI355X. There the statement is made on what the blob holds: the blob repacked from
    autoround_codes at the neutral parameters dequantises bit-equal to the RTN blob, its scales and zero points are
    the RTN blob's, and W~ is within levels * FP32_SLOP steps (the two extra roundings, quant_reference.bounds' form)."""
    c = _case(K, N, group, bits, asym)
    G = R.group_of(K, group)[1]
    wd = c["wd"]
    ones = torch.ones(G, N, device="cuda")

    def deq_of(blob):
        out = torch.empty(K, N, dtype=torch.float32, device="cuda")
        qbits.dequantize_packed_weight(blob, out, False, "fp32", WNAME[bits], "fp32")
        return out

    got = qbits.autoround_forward(wd, torch.zeros_like(wd), ones, ones.clone(), group, bits, asym)
    blob = qbits.quantize_to_packed_weight(wd, False, group, "fp32", WNAME[bits], "fp32", asym)
    deq = deq_of(blob)
    print("rtn K=%d N=%d group=%d bits=%d asym=%d: elements differing %d" % (K, N, group, bits, asym,
                                                                             int((got != deq).sum())))
    q, scale, zp = qbits.autoround_codes(wd, torch.zeros_like(wd), ones, ones.clone(), group, bits, asym)
    assert torch.equal(scale, qbits.acquire_packed_weight_info(blob, 9))
    if asym:
        assert torch.equal(zp, qbits.acquire_packed_weight_info(blob, 10))
    if bits == 4:
        assert torch.equal(got, deq)
    else:
        empty8, empty32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)
        mine = qbits.repack_quantized_weight(q, scale, zp if asym else empty8, empty32, WNAME[bits], "fp32", "fp32",
                                             asym, group)
        assert torch.equal(deq_of(mine), deq)
        g = R.group_of(K, group)[0]
        step = scale.repeat_interleave(g, 0)[:K].double()
        assert ((got.double() - deq.double()).abs() <= R.consts(bits)[0] * Q.FP32_SLOP * step).all()


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_step_moves_every_v(K, N, group, bits, asym):
    """V' = clamp(V - lr sign(g) [code not clipped]) at every element, to one fp32 rounding of the subtraction"""
    c = _case(K, N, group, bits, asym)
    want = R.sign_step(c["V"], np.where(c["gr"]["step_mask"], c["g"], 0.0), LR_V, -0.5, 0.5)
    got = c["step"][0].astype(np.float64)
    err = np.abs(got - want)
    print("step V K=%d N=%d group=%d bits=%d asym=%d: moved %d, held by the clip %d, max err %.3g"
          % (K, N, group, bits, asym, int((got != c["V"]).sum()), int(c["f"]["clipped"].sum()), err.max()))
    assert np.isfinite(got).all() and (err <= EPS * np.abs(want)).all(), np.argwhere(err > EPS * np.abs(want))[:4]
    assert np.array_equal(got[c["f"]["clipped"]], c["V"][c["f"]["clipped"]].astype(np.float64))
    assert np.abs(got).max() <= 0.5 and (got != c["V"]).sum() > 0.5 * K * N


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_step_range_factor_gradients(K, N, group, bits, asym):
    """raw dalpha / dbeta: |dev - ref| <= B = 2^-20 * rows of the group * sum |terms| (summed in the reference).
    Measured on the MI355X over the nine cases (profiles/r17_autoround.txt): the worst err / B is 0.368 (dbeta,
    256 x 96, group 32, 8 bits asym), 0.196 at 4 bits (200 x 70, group 64, its 8-row last group), 0.0001 for the group
    of 512 rows; the constant is left at the issue's 2^-20."""
    c = _case(K, N, group, bits, asym)
    gr = c["gr"]
    _, _, _, da, db = c["step"]
    worst = 0.0
    for name, dev, ref, sums in (("dalpha", da, gr["dalpha"], gr["sum_a"]), ("dbeta", db, gr["dbeta"], gr["sum_b"])):
        B = GRAD_SLOP * gr["rows"][:, None] * sums
        err = np.abs(dev.astype(np.float64) - ref)
        ratio = (err / np.where(B == 0, 1.0, B)).max()
        worst = max(worst, ratio)
        print("step %s K=%d N=%d group=%d bits=%d asym=%d: max err %.3g, worst err / B %.4f, cells with B = 0: %d"
              % (name, K, N, group, bits, asym, err.max(), ratio, int((B == 0).sum())))
        assert np.isfinite(dev).all() and (err <= B).all(), np.argwhere(err > B)[:4]
    assert (da[0, 0], db[0, 0]) == (0.0, 0.0)


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_step_moves_alpha_and_beta(K, N, group, bits, asym):
    """the stepped alpha / beta equal the reference's wherever |ref grad| > B; at most 1 % of the cells fall under that
    rule; the all-zero cell is left as it was. A cell whose reference gradient is exactly 0 (B is 0 there too: the sym
    side the maximum does not take, a one-sided group's other factor, the all-zero cell) is not counted under the rule
    but held to the stronger statement that it does not move."""
    c = _case(K, N, group, bits, asym)
    gr = c["gr"]
    _, a1, b1, _, _ = c["step"]
    left_out = total = 0
    for name, dev, p, ref, sums in (("alpha", a1, c["alpha"], gr["dalpha"], gr["sum_a"]),
                                    ("beta", b1, c["beta"], gr["dbeta"], gr["sum_b"])):
        B = GRAD_SLOP * gr["rows"][:, None] * sums
        sure = np.abs(ref) > B
        want = R.sign_step(p, ref, LR_MM, 0.0, 1.0)
        err = np.abs(dev.astype(np.float64) - want)
        assert (err <= EPS)[sure].all(), (name, np.argwhere(sure & (err > EPS))[:4])
        assert (dev >= 0).all() and (dev <= 1).all()
        # a cell the rule leaves out and whose reference gradient is exactly 0 (sym: the side not taken; the all-zero
        # cell) must not move at all
        still = ref == 0
        assert np.array_equal(dev[still], p[still]), name
        left_out += int((~sure & ~still).sum())
        total += sure.size
    print("step alpha / beta K=%d N=%d group=%d bits=%d asym=%d: %d of %d cells under the bound" % (
        K, N, group, bits, asym, left_out, total))
    assert left_out <= 0.01 * total
    assert (a1[0, 0], b1[0, 0]) == (c["alpha"][0, 0], c["beta"][0, 0])
    assert (a1 != c["alpha"]).any() and (b1 != c["beta"]).any()


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_same_bits_twice_and_bf16_gradient(K, N, group, bits, asym):
    c = _case(K, N, group, bits, asym)
    for x, y in zip(c["step"], c["again"]):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(c["step16"], c["step16w"]):  # g as bf16 = that bf16 value widened to fp32
        assert np.array_equal(x, y, equal_nan=True)
    assert not np.array_equal(c["step16"][3], c["step"][3])  # and it is the bf16 value that was read


def test_launchers_refuse_what_they_cannot_run():
    K, N, group = 64, 32, 32
    w = torch.zeros(K, N, device="cuda")
    v = torch.zeros(K, N, device="cuda")
    a = torch.ones(2, N, device="cuda")
    b = torch.ones(2, N, device="cuda")
    g = torch.zeros(K, N, device="cuda")
    bad = [
        (w.half(), v, a, b),                                  # wrong dtype
        (w, v.double(), a, b),
        (torch.zeros(N, K, device="cuda").t(), v, a, b),      # not contiguous
        (w, v, torch.ones(3, N, device="cuda"), b),           # alpha of the wrong shape
        (w, v, a, torch.ones(2, N + 1, device="cuda")),
        (w.cpu(), v, a, b),                                   # not on the device
    ]
    for args in bad:
        with pytest.raises(RuntimeError, match="QBits: autoround_forward"):
            qbits.autoround_forward(*args, group, 4, True)
        with pytest.raises(RuntimeError, match="QBits: autoround_step"):
            qbits.autoround_step(*args, g, group, 4, True, 0.01, 0.01)
        with pytest.raises(RuntimeError, match="QBits: autoround_codes"):
            qbits.autoround_codes(*args, group, 4, True)
    with pytest.raises(RuntimeError, match="QBits: autoround_step"):
        qbits.autoround_step(w, v, a, b, g.double(), group, 4, True, 0.01, 0.01)
    with pytest.raises(RuntimeError, match="QBits: autoround_step"):
        qbits.autoround_step(w, v, a, b, torch.zeros(N, K, device="cuda").t(), group, 4, True, 0.01, 0.01)
    with pytest.raises(RuntimeError, match="QBits: autoround_step"):
        qbits.autoround_step(w, v, a, b, g, group, 4, True, 0.01, 0.01, dalpha=torch.zeros(3, N, device="cuda"))
    with pytest.raises(RuntimeError, match="QBits: autoround_forward"):
        qbits.autoround_forward(w, v, a, b, group, 4, True, out=torch.zeros(K, N, dtype=torch.float64, device="cuda"))
    for bits in (1, 5, 16):  # the launcher's own refusal
        with pytest.raises(RuntimeError, match="bits must be 2, 3, 4 or 8"):
            qbits.autoround_forward(w, v, a, b, group, bits, True)
    with pytest.raises(RuntimeError, match="learning rate"):
        qbits.autoround_step(w, v, a, b, g, group, 4, True, -0.01, 0.01)
    assert torch.equal(v, torch.zeros_like(v)) and torch.equal(a, torch.ones_like(a))  # nothing ran
