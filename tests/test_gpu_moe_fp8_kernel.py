"""fp8_e4m3 / fp8_e5m2 expert blobs through `qbits.moe_forward` in both forms (csrc/woq_moe.hip moe_fp8_gemm_kernel: the
code bytes as the B operand of the fp8 MFMA, the activation as six base-16 digits; csrc/woq_moe_prompt.hip's exact fp16
value of the code byte) against the float64 statement of tests/moe_reference.py. Shapes, inputs and hand-set routings are
tests/test_gpu_moe_kernel.py's and tests/test_gpu_moe_prompt_kernel.py's, plus (H, I, E, k) = (1152, 32, 3, 2): nine
k-tiles, so a second 1024-k chunk of one tile — a per-chunk exponent and the chunk-boundary tile (E = 3, not 2: K._inputs'
routing at T = 37 draws ids from [2, E)).

The reference weights are `qbits.dequantize_packed_weight` of each blob; both forms multiply by exactly those.
Grouped tolerance A8 + 4 B: B = MR.reference's fixed-point term (same format, same 1024-k chunks); A8 = MR.block's band
with the per-product coefficient n(K) 2^-24 replaced by 1e-5, the project's bound for this MFMA's accumulation, which
is no fp32 adder (tests/test_gpu_wtypes_decode.py; measured 2e-6 / 4.6e-6, profiles/r04ah_fp8_decode.txt) and carries its
own margin. Prompt tolerance: PR.reference's, unchanged — the weight operand is exact.
"""
import numpy as np
import pytest
import torch

from oracle import woq_oracle as orc
from tests import moe_prompt_reference as PR
from tests import moe_reference as MR
from tests import test_gpu_moe_kernel as K
from tests import test_gpu_moe_prompt_kernel as P
from tests.gemv_f32_reference import _silu_d
from tests.xq_reference import _silu

pytestmark = pytest.mark.gpu

K.SHAPES.setdefault("h1152", (1152, 32, 3, 2))
# name: (weight_dtype, group, scale_dtype); "all_*": every finite code, uniformly, at 2^-10 of an RTN-sized scale
KINDS = {"e4m3_g128": ("fp8_e4m3", 128, "fp16"), "e4m3_g32": ("fp8_e4m3", 32, "fp32"),
         "e5m2_g128": ("fp8_e5m2", 128, "fp16"), "e5m2_g32_e8m0": ("fp8_e5m2", 32, "fp8_e8m0"),
         "all_e4m3": ("fp8_e4m3", 128, "fp32"), "all_e5m2": ("fp8_e5m2", 128, "fp32")}
_BUILT = {}


def _experts(shape, kind):
    """-> (module, Wgu E x [H, 2I], Wdn E x [I, H] float64), built once"""
    from intel_extension_for_transformers_amd import qbits
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.moe import QuantizedMoEExpertsQBits

    if (shape, kind) not in _BUILT:
        H, I, E, _ = K.SHAPES[shape]
        wdt, group, stype = KINDS[kind]
        mod = QuantizedMoEExpertsQBits(E, H, I, weight_dtype=wdt, bits=8, scale_dtype=stype, blocksize=group, device="cuda")
        if kind.startswith("all_"):
            rng = np.random.default_rng(63)
            wt = orc.W_FP8_E4M3 if wdt == "fp8_e4m3" else orc.W_FP8_E5M2
            finite = np.flatnonzero(np.isfinite(orc.FP8_TABLES[wt])).astype(np.uint8)
            none8, none32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)

            def blob(k, n):
                codes = finite[rng.integers(0, finite.size, size=(k, n))]
                s = ((0.1 + 0.1 * rng.random(((k + group - 1) // group, n))) / orc.FP8_MAX[wt] * 2.0 ** -10).astype(np.float32)
                return qbits.repack_quantized_weight(torch.from_numpy(codes.view(np.int8)).cuda(), torch.from_numpy(s).cuda(),
                                                     none8, none32, wdt, stype, "fp32", False, group)

            mod._adopt([blob(H, 2 * I) for _ in range(E)], [blob(I, H) for _ in range(E)])
        else:
            g = torch.Generator().manual_seed(3)
            mod.set_fp_weights(0.05 * torch.randn(E, 2 * I, H, generator=g), 0.05 * torch.randn(E, H, I, generator=g))
        deq = []
        for name, (k, n) in (("gate_up_proj", (H, 2 * I)), ("down_proj", (I, H))):
            full = []
            for b in mod._expert_views(name):
                out = torch.empty(k, n, dtype=torch.float32, device="cuda")
                qbits.dequantize_packed_weight(b, out, False, "fp32", wdt, stype)
                full.append(out.cpu().numpy().astype(np.float64))
            deq.append(full)
        _BUILT[(shape, kind)] = (mod, deq[0], deq[1])
    return _BUILT[(shape, kind)]


def _check(got, shape, kind, T, form, what, act="fp32"):
    _, Wgu, Wdn = _experts(shape, kind)
    x, idx, w = P._inputs(shape, T, act, "")
    xf = x.float().numpy()
    if form == "prompt":
        ref, tol = PR.reference(xf, idx, w, Wgu, Wdn)
    else:
        bits = K.DTYPES[act][1]  # (inert in the call below, whose own tolerance is dropped; charged by hand further down)
        ref, _, B = MR.reference(xf, idx, w, Wgu, Wdn, (1 if KINDS[kind][1] == 32 else 0, False), bits)
        inter, x64, c, tol = Wdn[0].shape[0], xf.astype(np.float64), 1e-5, np.zeros(ref.shape)  # A8: MR.block's A, n U -> c
        for t in range(T):
            mag = np.zeros(ref.shape[1])
            for j in range(idx.shape[1]):
                e = int(idx[t, j])
                if not 0 <= e < len(Wgu):
                    continue
                gu, a_gu = x64[t] @ Wgu[e], c * (np.abs(x64[t]) @ np.abs(Wgu[e]))
                g, u, a_g, a_u = gu[:inter], gu[inter:], a_gu[:inter], a_gu[inter:]
                h = _silu(g) * u
                a_h = (np.abs(_silu_d(g)) + 0.5 * a_g) * a_g * np.abs(u) + np.abs(_silu(g)) * a_u + a_g * a_u + 4 * MR.U * np.abs(h)
                tol[t] += abs(float(w[t, j])) * (a_h @ np.abs(Wdn[e]) + c * (np.abs(h) @ np.abs(Wdn[e])))
                mag += abs(float(w[t, j])) * np.abs(h @ Wdn[e])
            tol[t] += (idx.shape[1] + 1) * MR.U * mag
        tol = tol + 4 * B
        if bits != 24:  # the one rounding of the output to its type, as MR.reference charges it
            tol = tol + 2.0 ** -bits * np.abs(ref)
    if kind.startswith("all_"):
        tol = tol + 1e-5
    ratio = np.abs(got.float().cpu().numpy().astype(np.float64) - ref) / tol
    print("\n%s %s %s T=%d: worst |out - ref| / tol %.3f" % (what, shape, kind, T, ratio.max()))
    assert np.isfinite(ratio).all() and ratio.max() <= 1.0, (what, shape, kind, T, float(ratio.max()))


def _run(shape, kind, T, form, act="fp32"):
    from intel_extension_for_transformers_amd import qbits

    mod = _experts(shape, kind)[0]
    x, idx, w = P._inputs(shape, T, act, "")
    return qbits.moe_forward(x.cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda(), mod.gate_up_blobs,
                             mod.down_blobs, form=form)


RTN = [k for k in KINDS if not k.startswith("all_")]


@pytest.mark.parametrize("T", [1, 2, 5, 37])
@pytest.mark.parametrize("kind", RTN)
@pytest.mark.parametrize("shape", ["h256", "h128", "h1152"])
def test_grouped_form_against_float64(shape, kind, T):
    _check(_run(shape, kind, T, "grouped"), shape, kind, T, "grouped", "grouped")


@pytest.mark.parametrize("T", [1, 5])  # the pair packing | the row-set packing
@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_grouped_form_half_precision_rows_against_float64(act, T):
    """the kernel's bf16 / fp16 row load; the output is of the activations' type, whose rounding joins the tolerance"""
    got = _run("h128", "e4m3_g32", T, "grouped", act)
    assert got.dtype == K.DTYPES[act][0]
    _check(got, "h128", "e4m3_g32", T, "grouped", "grouped " + act, act)


@pytest.mark.parametrize("T", [37, 300])
@pytest.mark.parametrize("kind", RTN)
@pytest.mark.parametrize("shape", ["h128", "h272"])
def test_prompt_form_against_float64(shape, kind, T):
    _check(_run(shape, kind, T, "prompt"), shape, kind, T, "prompt", "prompt")


@pytest.mark.parametrize("T,form", [(5, "grouped"), (64, "prompt")])
@pytest.mark.parametrize("kind", ["all_e4m3", "all_e5m2"])
def test_every_finite_code(kind, T, form):
    _check(_run("h128", kind, T, form), "h128", kind, T, form, "codes")


@pytest.mark.parametrize("form,T", [("grouped", 37), ("prompt", 300)])
def test_two_calls_give_the_same_bytes(form, T):
    a, b = (_run("h128", "e4m3_g32", T, form) for _ in range(2))
    assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("T,form", [(5, "grouped"), (64, "prompt")])
@pytest.mark.parametrize("kind", ["e4m3_g128", "e5m2_g32_e8m0"])
def test_module_routes_to_the_form_and_the_loop_meets_the_same_tolerance(kind, T, form):
    mod = _experts("h128", kind)[0]
    assert mod.grouped_supported() and (T >= mod.prompt_min_tokens) == (form == "prompt")
    x, idx, w = P._inputs("h128", T, "fp32", "")
    args = (x.cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda())
    got = mod(*args)
    assert torch.equal(got.view(torch.int32), _run("h128", kind, T, form).view(torch.int32))
    _check(got, "h128", kind, T, form, "module")
    _check(mod.loop_forward(*args), "h128", kind, T, form, "loop")
