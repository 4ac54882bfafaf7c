"""`qbits.moe_forward(form="prompt")` (csrc/woq_moe_prompt.hip: a three-launch plan, gate/up and down on the fp16 MFMA,
combine) against the float64 statement and the derived tolerance of tests/moe_prompt_reference.py.

Shapes (H, I, E, k): tests/test_gpu_moe_kernel.py's (256, 160, 4, 2) and (128, 96, 8, 3) plus (272, 160, 4, 2): a padded
last K tile in the down product, gate/up pairs that do not fill a workgroup's four waves, and a down launch whose last
workgroup has one live column tile. Quantisation: g128 sym / fp16 scales and g32 asym / fp32 scales. T = 1 and 37 with
that file's routing; at T = 300 the routing is set by hand, R = 128 the row tile: expert 0 receives R + 2 rows (two
blocks, the second with two rows), expert 1 exactly R, expert 2 a single row, expert 3 none where E = 8 (with E = 4 it
takes the rest: 2 T slots do not fit otherwise), and one slot carries the id E.
"""
import numpy as np
import pytest
import torch

from tests import moe_prompt_reference as PR
from tests import test_gpu_moe_kernel as K

pytestmark = pytest.mark.gpu

K.SHAPES.setdefault("h272", (272, 160, 4, 2))
R = 128
BASE = [(s, q, t, "fp32", "int64", "") for s in ("h256", "h128", "h272") for q in K.QUANTS for t in (1, 37, 300)]
CASES = BASE + [
    ("h256", "g32a", 37, "bf16", "int64", ""), ("h128", "g128s", 300, "fp16", "int64", ""),
    ("h128", "g32a", 300, "fp32", "int32", ""),
    ("h128", "g32a", 37, "fp32", "int64", "tiny"),     # fp weights times 2^-12: scales under fp16's normal range
    ("h256", "g32a", 37, "fp32", "int64", "outlier"),  # one element times 30 (K._inputs) and one row times 2^12
    ("h128", "g32a", 2731, "fp32", "int64", ""),       # T k = 8193: more than eight plan segments
]
_TINY = {}


def _experts(shape, quant, variant):
    """K._experts, or for "tiny" the same fp weights times 2^-12 quantised the same way"""
    from intel_extension_for_transformers_amd import qbits

    if variant != "tiny":
        return K._experts(shape, quant)
    if (shape, quant) not in _TINY:
        H, I, E, _ = K.SHAPES[shape]
        group, asym, stype = K.QUANTS[quant]
        g = torch.Generator().manual_seed(3)
        blobs, deq = [], []
        for n, k in ((2 * I, H), (H, I)):
            w = 0.05 * 2.0 ** -12 * torch.randn(E, n, k, generator=g)
            packed = [qbits.quantize_to_packed_weight(w[e].cuda(), True, group, "fp32", "int4_clip", stype, asym)
                      for e in range(E)]
            full = []
            for p in packed:
                out = torch.empty(k, n, dtype=torch.float32, device="cuda")
                qbits.dequantize_packed_weight(p, out, False, "fp32", "int4_clip", stype)
                full.append(out.cpu().numpy().astype(np.float64))
            blobs.append(torch.stack(packed).view(torch.uint8))
            deq.append(full)
        _TINY[(shape, quant)] = (blobs[0], blobs[1], deq[0], deq[1])
    return _TINY[(shape, quant)]


def _inputs(shape, T, act, variant):
    _, _, E, k = K.SHAPES[shape]
    if T <= 37:
        x, idx, w = K._inputs(shape, T, act)
    else:
        rng = np.random.default_rng(11 + T)
        x = torch.from_numpy(rng.standard_normal((T, K.SHAPES[shape][0])).astype(np.float32)).to(K.DTYPES[act][0])
        w = rng.random((T, k)).astype(np.float32)
        idx = rng.integers(0, E, (T, k))
        if T == 300:
            fixed = [0] * (R + 2) + [1] * R + [2, E]
            rest = rng.integers(4 if E > 4 else 3, E, T * k - len(fixed))
            idx = rng.permutation(np.concatenate([fixed, rest])).reshape(T, k)
        idx = idx.astype(np.int64)
    if variant == "outlier":
        x[T // 2] *= 4096.0
    return x, idx, w


def _run(shape, quant, T, act, itype, variant):
    from intel_extension_for_transformers_amd import qbits

    gu, dn, _, _ = _experts(shape, quant, variant)
    x, idx, w = _inputs(shape, T, act, variant)
    idx = torch.from_numpy(idx).to(torch.int64 if itype == "int64" else torch.int32)
    return qbits.moe_forward(x.cuda(), idx.cuda(), torch.from_numpy(w).cuda(), gu, dn, form="prompt")


@pytest.mark.parametrize("shape,quant,T,act,itype,variant", CASES)
def test_prompt_form_against_float64(shape, quant, T, act, itype, variant):
    got = _run(shape, quant, T, act, itype, variant)
    assert got.dtype == K.DTYPES[act][0]
    _, _, Wgu, Wdn = _experts(shape, quant, variant)
    x, idx, w = _inputs(shape, T, act, variant)
    ref, tol = PR.reference(x.float().numpy(), idx, w, Wgu, Wdn, K.DTYPES[act][1])
    err = np.abs(got.float().cpu().numpy().astype(np.float64) - ref)
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    print("\nprompt %s %s T=%d %s %s: worst |out - ref| / tol %.3f" % (shape, quant, T, act, variant, ratio.max()))
    assert np.isfinite(ratio).all() and ratio.max() <= 1.0, (shape, quant, T, act, variant, float(ratio.max()))


def test_two_calls_give_the_same_bytes():
    a, b = (_run("h128", "g32a", 300, "fp32", "int64", "") for _ in range(2))
    assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a_call_above_the_slot_limit_is_refused_and_the_module_chunks_it():
    from intel_extension_for_transformers_amd import qbits
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.moe import QuantizedMoEExpertsQBits

    H, I, E, k = K.SHAPES["h128"]
    group, asym, stype = K.QUANTS["g32a"]
    gu, dn, _, _ = K._experts("h128", "g32a")
    T = qbits.MOE_PROMPT_MAX_SLOTS // k + 1  # T k = 65538
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, H, generator=g).cuda()
    idx = torch.randint(0, E, (T, k), generator=g).cuda()
    w = torch.rand(T, k, generator=g).cuda()
    with pytest.raises(RuntimeError, match=str(qbits.MOE_PROMPT_MAX_SLOTS)):
        qbits.moe_forward(x, idx, w, gu, dn, form="prompt")
    mod = QuantizedMoEExpertsQBits(E, H, I, weight_dtype="int4_clip", scale_dtype=stype, blocksize=group,
                                   scheme="asym" if asym else "sym", device="cuda")
    mod.gate_up_blobs, mod.down_blobs = gu, dn
    got = mod(x, idx, w)
    parts = [qbits.moe_forward(x[s], idx[s], w[s], gu, dn, form="prompt") for s in (slice(0, T - 1), slice(T - 1, T))]
    assert torch.equal(got.view(torch.int32), torch.cat(parts).view(torch.int32))
