"""nf4 / fp4_e2m1 / fp4_e2m1_bnb / int8 expert blobs through `qbits.moe_forward` in both forms (csrc/woq_moe.hip's digit-plane
and two-plane B operands, csrc/woq_moe_prompt.hip's fp16 table and 16 hi + lo fragments) against the float64 statement of
tests/moe_reference.py, with that file's derived tolerance (grouped) and tests/moe_prompt_reference.py's (prompt); shapes,
inputs and hand-set routings are tests/test_gpu_moe_kernel.py's and tests/test_gpu_moe_prompt_kernel.py's.

The reference weights are `qbits.dequantize_packed_weight` of each blob. The grouped form does not multiply by exactly
those for nf4: its digit planes hold round(table S) / S, S = 2^22 at compute fp32 (three planes) and 127 * 256 otherwise
(two), so every weight is off by at most |s| / (2 S) (csrc/woq_gemv_common.h; both fp4 tables are exact). `_plane_term`
carries that through the block as moe_reference carries its A and the sum is added to the tolerance. The int8 form adds
the planes' int32 fragments before the one conversion to fp32, so it rounds where an asymmetric int4 tile rounds: its
tolerance is MR.reference's with asym set. The prompt form's fp16(table value) is one rounding of the weight operand,
2^-11, inside the 2^-10 that moe_prompt_reference's 2^-9 grants the weight (scale_mode 1: two more, 2^-9 in all).
"""
import numpy as np
import pytest
import torch

from tests import moe_prompt_reference as PR
from tests import moe_reference as MR
from tests import test_gpu_moe_kernel as K
from tests import test_gpu_moe_prompt_kernel as P
from tests.gemv_f32_reference import _silu_d
from tests.xq_reference import _silu

pytestmark = pytest.mark.gpu

# name: (weight_dtype, group, asym, scale_dtype, compute_dtype)
KINDS = {
    "nf4_g128": ("nf4", 128, False, "fp16", "fp32"), "nf4_g32": ("nf4", 32, False, "fp32", "fp32"),
    "nf4_g128_c16": ("nf4", 128, False, "fp16", "bf16"),  # the two-plane table
    "fp4_g128": ("fp4_e2m1", 128, False, "fp16", "fp32"), "fp4_g32": ("fp4_e2m1", 32, False, "fp32", "fp32"),
    "bnb_g128": ("fp4_e2m1_bnb", 128, False, "fp16", "fp32"),
    "int8_g128s": ("int8", 128, False, "fp16", "fp32"), "int8_g32a": ("int8", 32, True, "fp32", "fp32"),
}
_BUILT = {}


def _experts(shape, kind):
    """-> (module, Wgu E x [H, 2I], Wdn E x [I, H] float64): RTN through `set_fp_weights`, built once"""
    from intel_extension_for_transformers_amd import qbits
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.moe import QuantizedMoEExpertsQBits

    if (shape, kind) not in _BUILT:
        H, I, E, _ = K.SHAPES[shape]
        wdt, group, asym, stype, cdt = KINDS[kind]
        g = torch.Generator().manual_seed(3)
        mod = QuantizedMoEExpertsQBits(E, H, I, compute_dtype=cdt, weight_dtype=wdt, bits=8 if wdt == "int8" else 4,
                                       scale_dtype=stype, blocksize=group, scheme="asym" if asym else "sym", device="cuda")
        mod.set_fp_weights(0.05 * torch.randn(E, 2 * I, H, generator=g), 0.05 * torch.randn(E, H, I, generator=g))
        deq = []
        for name, (k, n) in (("gate_up_proj", (H, 2 * I)), ("down_proj", (I, H))):
            full = []
            for blob in mod._expert_views(name):
                out = torch.empty(k, n, dtype=torch.float32, device="cuda")
                qbits.dequantize_packed_weight(blob, out, False, cdt, wdt, stype)
                full.append(out.cpu().numpy().astype(np.float64))
            deq.append(full)
        _BUILT[(shape, kind)] = (mod, deq[0], deq[1])
    return _BUILT[(shape, kind)]


def _plane_term(x, idx, w, Wgu, Wdn, kind):
    """[T, H]: what weights off by at most eps |s| can move the block's output; zero unless the planes are inexact"""
    wdt, group, _, _, cdt = KINDS[kind]
    if wdt != "nf4":
        return 0.0
    eps = 0.5 / (2.0 ** 22 if cdt == "fp32" else 127.0 * 256.0)

    def scales(W):  # nf4's largest table entry is 1, at both ends: |s| = the largest |weight| of the group
        kk = W.shape[0]
        return np.concatenate([np.repeat(np.abs(W[k0:k0 + group]).max(0, keepdims=True), min(group, kk - k0), 0)
                               for k0 in range(0, kk, group)])

    inter, x64, D = Wdn[0].shape[0], np.abs(x.astype(np.float64)), np.zeros(x.shape)
    for t in range(x.shape[0]):
        for j in range(idx.shape[1]):
            e = int(idx[t, j])
            if not 0 <= e < len(Wgu):
                continue
            gu, d_gu = x[t].astype(np.float64) @ Wgu[e], eps * (x64[t] @ scales(Wgu[e]))
            g, u, d_g, d_u = gu[:inter], gu[inter:], d_gu[:inter], d_gu[inter:]
            d_h = (np.abs(_silu_d(g)) + 0.5 * d_g) * d_g * np.abs(u) + np.abs(_silu(g)) * d_u + d_g * d_u
            D[t] += abs(float(w[t, j])) * (d_h @ np.abs(Wdn[e]) + eps * ((np.abs(_silu(g) * u) + d_h) @ scales(Wdn[e])))
    return D


def _check(got, shape, kind, T, form, what):
    _, Wgu, Wdn = _experts(shape, kind)
    x, idx, w = P._inputs(shape, T, "fp32", "")
    xf = x.float().numpy()
    if form == "prompt":
        ref, tol = PR.reference(xf, idx, w, Wgu, Wdn)
    else:
        wdt, group = KINDS[kind][:2]
        ref, tol, _ = MR.reference(xf, idx, w, Wgu, Wdn, (1 if group == 32 else 0, KINDS[kind][2] or wdt == "int8"))
        tol = tol + _plane_term(xf, idx, w, Wgu, Wdn, kind)
    ratio = np.abs(got.float().cpu().numpy().astype(np.float64) - ref) / tol
    print("\n%s %s %s T=%d: worst |out - ref| / tol %.3f" % (what, shape, kind, T, ratio.max()))
    assert np.isfinite(ratio).all() and ratio.max() <= 1.0, (what, shape, kind, T, float(ratio.max()))


def _run(shape, kind, T, form):
    from intel_extension_for_transformers_amd import qbits

    mod = _experts(shape, kind)[0]
    x, idx, w = P._inputs(shape, T, "fp32", "")
    return qbits.moe_forward(x.cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda(), mod.gate_up_blobs,
                             mod.down_blobs, form=form)


@pytest.mark.parametrize("T", [1, 5, 37])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", ["h256", "h128"])
def test_grouped_form_against_float64(shape, kind, T):
    _check(_run(shape, kind, T, "grouped"), shape, kind, T, "grouped", "grouped")


@pytest.mark.parametrize("T", [37, 300])
@pytest.mark.parametrize("kind", [k for k in KINDS if k != "nf4_g128_c16"])  # this form does not read the compute type
@pytest.mark.parametrize("shape", ["h128", "h272"])
def test_prompt_form_against_float64(shape, kind, T):
    _check(_run(shape, kind, T, "prompt"), shape, kind, T, "prompt", "prompt")


@pytest.mark.parametrize("form,T", [("grouped", 37), ("prompt", 300)])
def test_two_calls_give_the_same_bytes(form, T):
    a, b = (_run("h128", "int8_g32a", T, form) for _ in range(2))
    assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("T,form", [(5, "grouped"), (64, "prompt")])
@pytest.mark.parametrize("kind", ["nf4_g128", "int8_g128s"])
def test_module_routes_to_the_form_and_the_loop_meets_the_same_tolerance(kind, T, form):
    mod = _experts("h128", kind)[0]
    assert mod.grouped_supported() and (T >= mod.prompt_min_tokens) == (form == "prompt")
    x, idx, w = P._inputs("h128", T, "fp32", "")
    args = (x.cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda())
    got = mod(*args)
    assert torch.equal(got.view(torch.int32), _run("h128", kind, T, form).view(torch.int32))
    _check(got, "h128", kind, T, form, "module")
    _check(mod.loop_forward(*args), "h128", kind, T, form, "loop")
