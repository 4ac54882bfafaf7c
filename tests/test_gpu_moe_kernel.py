"""`qbits.moe_forward` (csrc/woq_moe.hip: plan, gate/up, down, combine) alone against the float64 statement and the derived
tolerance of tests/moe_reference.py, and the per-expert loop form on the same inputs under the same tolerance.

Shapes (H, I, E, k): (256, 160, 4, 2) and (128, 96, 8, 3) — I = 160 and I = 96 leave the down product a padded last K tile,
k = 3 is no power of two. Quantisation: g128 symmetric with fp16 scales (scale_mode 0; the down blobs hold one short group)
and g32 asymmetric with fp32 scales (scale_mode 1, zero points). T in {1, 5, 37}; at T = 37 the routing is set by hand:
expert 0 receives 20 rows (two blocks), expert 1 none, and one slot carries the id E, which is dropped.
"""
import numpy as np
import pytest
import torch

from tests import moe_reference as MR

pytestmark = pytest.mark.gpu

SHAPES = {"h256": (256, 160, 4, 2), "h128": (128, 96, 8, 3)}
QUANTS = {"g128s": (128, False, "fp16"), "g32a": (32, True, "fp32")}
CASES = [(s, q, t, "fp32", "int64") for s in SHAPES for q in QUANTS for t in (1, 5, 37)] + [
    ("h256", "g32a", 5, "bf16", "int64"), ("h128", "g128s", 37, "fp16", "int64"), ("h128", "g32a", 37, "fp32", "int32")]
DTYPES = {"fp32": (torch.float32, 24), "bf16": (torch.bfloat16, 8), "fp16": (torch.float16, 11)}
_EXPERTS = {}


def _experts(shape, quant):
    """-> (gate_up blobs, down blobs uint8 [E, stride], Wgu E x [H, 2I], Wdn E x [I, H] float64), built once"""
    from intel_extension_for_transformers_amd import qbits

    if (shape, quant) not in _EXPERTS:
        H, I, E, _ = SHAPES[shape]
        group, asym, stype = QUANTS[quant]
        g = torch.Generator().manual_seed(3)
        blobs, deq = [], []
        for n, k in ((2 * I, H), (H, I)):
            w = 0.05 * torch.randn(E, n, k, generator=g)
            packed = [qbits.quantize_to_packed_weight(w[e].cuda(), True, group, "fp32", "int4_clip", stype, asym)
                      for e in range(E)]
            full = []
            for p in packed:
                out = torch.empty(k, n, dtype=torch.float32, device="cuda")
                qbits.dequantize_packed_weight(p, out, False, "fp32", "int4_clip", stype)
                full.append(out.cpu().numpy().astype(np.float64))
            blobs.append(torch.stack(packed).view(torch.uint8))
            deq.append(full)
        _EXPERTS[(shape, quant)] = (blobs[0], blobs[1], deq[0], deq[1])
    return _EXPERTS[(shape, quant)]


def _inputs(shape, T, act):
    H, _, E, k = SHAPES[shape]
    rng = np.random.default_rng(11 + T)
    x = torch.from_numpy(rng.standard_normal((T, H)).astype(np.float32)).to(DTYPES[act][0])
    x[0, H // 3] *= 30
    w = rng.random((T, k)).astype(np.float32)
    if T == 37:
        idx = rng.integers(2, E, (T, k))
        idx[:20, 0] = 0
        idx[30, k - 1] = E
    else:
        idx = np.argsort(rng.random((T, E)), axis=1)[:, :k]
    return x, idx.astype(np.int64), w


def _check(got, shape, quant, T, act, what):
    _, _, Wgu, Wdn = _experts(shape, quant)
    x, idx, w = _inputs(shape, T, act)
    smode_asym = (1 if QUANTS[quant][0] == 32 else 0, QUANTS[quant][1])
    ref, tol, B = MR.reference(x.float().numpy(), idx, w, Wgu, Wdn, smode_asym, DTYPES[act][1])
    ratio = np.abs(got.float().cpu().numpy().astype(np.float64) - ref) / tol
    print("\n%s %s %s T=%d %s: worst |out - ref| / tol %.3f (B %.3g)" % (what, shape, quant, T, act, ratio.max(), B))
    assert np.isfinite(ratio).all() and ratio.max() <= 1.0, (what, shape, quant, T, act, float(ratio.max()))


def _run(shape, quant, T, act, itype):
    from intel_extension_for_transformers_amd import qbits

    gu, dn, _, _ = _experts(shape, quant)
    x, idx, w = _inputs(shape, T, act)
    idx = torch.from_numpy(idx).to(torch.int64 if itype == "int64" else torch.int32)
    return qbits.moe_forward(x.cuda(), idx.cuda(), torch.from_numpy(w).cuda(), gu, dn)


@pytest.mark.parametrize("shape,quant,T,act,itype", CASES)
def test_grouped_form_against_float64(shape, quant, T, act, itype):
    got = _run(shape, quant, T, act, itype)
    assert got.dtype == DTYPES[act][0]
    _check(got, shape, quant, T, act, "grouped")


def test_two_calls_give_the_same_bytes():
    a, b = _run("h128", "g32a", 37, "fp32", "int64"), _run("h128", "g32a", 37, "fp32", "int64")
    assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("shape,quant", [("h256", "g128s"), ("h128", "g32a")])
def test_loop_form_meets_the_same_tolerance(shape, quant):
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.moe import QuantizedMoEExpertsQBits

    H, I, E, _ = SHAPES[shape]
    group, asym, stype = QUANTS[quant]
    mod = QuantizedMoEExpertsQBits(E, H, I, weight_dtype="int4_clip", scale_dtype=stype, blocksize=group,
                                   scheme="asym" if asym else "sym", device="cuda")
    mod.gate_up_blobs, mod.down_blobs = _experts(shape, quant)[:2]
    x, idx, w = _inputs(shape, 37, "fp32")
    got = mod.loop_forward(x.cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda())
    _check(got, shape, quant, 37, "fp32", "loop")
