"""The prompt pass's MFMA GEMM with what only the engine asks of it — RMSNorm fused into the pack pass, the SiLU * mul
epilogue over interleaved gate / up tiles, the residual added in place, fp16 saturation — through `woq_probe_gemm_f16`
(launch_gemm_f16 unchanged), against tests/gemm_f16_reference.py (float64).

The cases, their inputs and the band are the reference module's (`CASES` ..., `build`, `terms`); nothing here is decided
from a kernel's output, and tests/test_gemm_f16_reference_cpu.py shows without a GPU what the band rejects. Per case: the
form `woq_gemm_form_log` reports equals the form the case names; the output is a window of a NaN-filled (M + 3) x ldo
buffer (holding the residual where the residual aliases it), so unwritten elements and stores past M / n_out are seen;
every element is within the band of the reference; a second call into a fresh buffer is bit-identical; an all-zero row
gives the bias (+ residual) exactly when no SiLU * mul follows. Every case prints its form and the largest
|out - ref| / band.

Largest |out - ref| / band per kind of case, MI355X, beside what the correctly rounded reference alone reaches in the
same case (the band's output-type term: 2^-10 |ref| is twice fp16's half step, 2^-8 |ref| is bf16's largest half step;
rows whose bound A is small — the all-zero row, where the result is the bias — are decided by that term alone). In every
case above 0.5 the two numbers are equal: the worst element is the rounding of the reference, not the kernel.
  pack pass norm branch (MODE 0 / 1 / 2, 2 / 4 / 8 chunks, two sweeps)  0.460  (0.460)
  ring                                                                  0.427  (0.427)
  compiler-scheduled (K = 384)                                          0.460  (0.460)
  hand-scheduled without ring (group 32, asymmetric, fp32 scales)       0.427  (0.427)
  raw-A                                                                 0.545  (0.545)  epi 1 -> fp16
  split-K (2 .. 15 slices)                                              0.470  (0.470)
  fragment image (nf4, fp4_e2m1, fp8_e4m3)                              0.413  (0.413)
  fp32-class (band 1e-4 of the row maximum, fp32 out)                   0.291  (0.000)
  256-row tiles                                                         0.224  (0.150)
  in-place residual, fp32 out                                           0.162  (0.000)
  edges (N = 32 / 288 / 40 / 17), direct and split-K                    0.578  (0.578)  bf16 rows -> bf16 out
  scalar stores                                                         0.924  (0.924)  bf16 out, the all-zero row
  saturation, the bf16 / fp32 twins                                     0.632  (0.632)  bf16 out
  caller workspace                                                      0.452  (0.452)
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from oracle import woq_oracle as orc
from tests import gemm_f16_reference as R

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NAN = float("nan")
_BLOBS = {}


def _ids(cases):
    return [c["name"] for c in cases]


def _dev(a, dt=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dt is None else t.to(dt)


def _dev_blob(c, d):
    """the oracle's blob, byte for byte (the device repack equals it: tests/test_gpu_f32_gemv_kernel.py)"""
    key = (c["K"], c["N"], c["quant"], c["wname"], c["epi"], c["shuffle"])
    if key not in _BLOBS:
        _BLOBS[key] = _dev(d["blob"])
    return _BLOBS[key]


def _launch(c, d, blob, ws=None, ws_bytes=0):
    """one probe call on fresh buffers -> out [M, n_out] (cpu tensor of the output type); asserts the guards"""
    M, K, n_out = c["M"], c["K"], d["n_out"]
    lda, ldo, off = K + c["lda_pad"], n_out + c["ldo_pad"], c["out_off"]
    xbuf = torch.zeros(M * lda + 8, dtype=DT[c["act"]], device="cuda")
    xbuf[:M * lda].view(M, lda)[:, :K].copy_(_dev(d["x"]))
    flat = torch.full((off + (M + 3) * ldo,), NAN, dtype=DT[c["out"]], device="cuda")
    win = flat[off:].view(M + 3, ldo)
    res, ld_res = None, 0
    if c["residual"] == "alias":
        win[:M, :n_out].copy_(_dev(d["residual"]))
        res, ld_res = win, ldo
    elif c["residual"] == "separate":
        ld_res = n_out + c["ld_res_pad"]
        res = torch.zeros(M * ld_res + 8, device="cuda")
        res[:M * ld_res].view(M, ld_res)[:, :n_out].copy_(_dev(d["residual"]))
    L.probe_gemm_f16(xbuf, blob, win, M, lda=lda, ldo=ldo, norm_w=_dev(d["g"]), eps=R.EPS, epi=c["epi"], bias=_dev(d["bias"]),
                     residual=res, ld_res=ld_res, fp32_class=c["fp32_class"], ws=ws, ws_bytes=ws_bytes)
    torch.cuda.synchronize()
    flat = flat.cpu()
    win = flat[off:].view(M + 3, ldo)
    assert bool(torch.isnan(flat[:off]).all()) and bool(torch.isnan(win[M:]).all()) and bool(
        torch.isnan(win[:, n_out:]).all()), c["name"] + ": written outside the M x n_out window"
    return win[:M, :n_out].contiguous()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check(c, d, got, rows=None):
    """every element against the band -> (worst |out - ref| / band, terms, what rounding the reference alone reaches)"""
    t = R.terms(c, d, rows)
    g = got.to(torch.float64).numpy()
    assert not np.isnan(g).any(), "%s: %d output elements never stored, first at %s" % (
        c["name"], int(np.isnan(g).sum()), tuple(np.argwhere(np.isnan(g))[0]))
    err = np.abs(g - t["exp"])
    ratio = err / t["tol"]
    bad = err > t["tol"]
    assert not bad.any(), "%s: %d elements outside the band, first at %s, worst ratio %.3f" % (
        c["name"], int(bad.sum()), tuple(np.argwhere(bad)[0]), float(ratio.max()))
    rounding = float((np.abs(R.round_out(t["exp"], c["out"]) - t["exp"]) / t["tol"]).max())
    return float(ratio.max()), t, rounding


def _run(c, **kw):
    """-> (out, reference terms, inputs)"""
    d = R.build(c)
    blob = _dev_blob(c, d)
    L.gemm_form_log()
    got = _launch(c, d, blob, **kw)
    again = _launch(c, d, blob, **kw)
    forms = L.gemm_form_log()
    assert forms == [c["expect"][0]] * 2, (c["name"], forms)  # the form first, then the numbers
    worst, t, rounding = _check(c, d, got)
    print("%s [%s]: form %d, %d K slices, worst |out - ref| / band %.3f (the rounded reference: %.3f)" % (
        c["name"], c["kind"], forms[0], c["expect"][1], worst, rounding))
    assert torch.equal(_bits(got), _bits(again)), c["name"] + ": a repeated call differs"
    if c["M"] >= 4 and c["rows"] == "mixed" and c["epi"] == 0:  # the all-zero row: the product is exactly 0
        want = np.zeros(d["n_out"], np.float32) if d["bias"] is None else d["bias"]
        if d["residual"] is not None:
            want = (want + d["residual"][0]).astype(np.float32)
        assert torch.equal(got[0], torch.from_numpy(want).to(DT[c["out"]])), c["name"] + ": the all-zero row"
    return got, t, d


@pytest.mark.parametrize("c", R.CASES, ids=_ids(R.CASES))
def test_case(c):
    _run(c)


@pytest.mark.parametrize("c", R.SCALAR_BASES, ids=_ids(R.SCALAR_BASES))
def test_scalar_stores_agree_with_paired_stores(c):
    """odd ldo, odd ld_res, an output pointer off the pair alignment: gemm_epilogue's scalar path, bit for bit what the
    paired path stores for the same inputs"""
    got, _, d = _run(c)
    for v in R.scalar_variants(c):
        other, _, _ = _run(v)
        assert torch.equal(_bits(got), _bits(other)), v["name"]


@pytest.mark.parametrize("c", R.ALIAS_CASES, ids=_ids(R.ALIAS_CASES))
def test_residual_in_place_equals_a_separate_copy(c):
    got, _, _ = _run(c)
    other, _, _ = _run(dict(c, name=c["name"] + " / separate copy", residual="separate"))
    assert torch.equal(_bits(got), _bits(other)), c["name"]


@pytest.mark.parametrize("c", R.SATURATION, ids=_ids(R.SATURATION))
def test_fp16_stores_saturate(c):
    got, t, d = _run(c)
    sure = R.saturated(t)
    assert 0.01 <= sure.mean() <= 0.5  # (tests/test_gemm_f16_reference_cpu.py: both signs among them)
    g = got.to(torch.float64).numpy()
    assert np.array_equal(g[sure], np.sign(t["unclamped"][sure]) * R.F16_MAX), c["name"]
    assert np.isfinite(g).all() and np.abs(g).max() == R.F16_MAX
    for out in ("bf16", "fp32"):  # not clamped
        wide, tw, _ = _run(dict(c, name="%s / %s out" % (c["name"], out), out=out))
        assert float(wide.to(torch.float64).abs().max()) > 2 * R.F16_MAX and np.array_equal(tw["exp"], t["unclamped"])


def test_silu_mul_refuses_half_a_tile_pair():
    """epi 1 with N = 48: the launcher's message, nothing written, no launch logged"""
    c = R.REFUSED
    M, n_out = c["M"], c["N"] // 2
    d = R.build(dict(c, epi=0))  # a plain blob of 48 columns
    win = torch.full((M + 3, n_out + 2), NAN, dtype=torch.float16, device="cuda")
    L.gemm_form_log()
    with pytest.raises(RuntimeError, match="QBits: the SiLU\\*mul epilogue needs whole gate / up column-tile pairs"):
        L.probe_gemm_f16(_dev(d["x"]), _dev(d["blob"]), win, M, lda=c["K"], ldo=n_out + 2, norm_w=_dev(d["g"]), eps=R.EPS,
                         epi=1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(win).all()) and L.gemm_form_log() == []


def test_probe_refuses_an_int8_composite():
    rng = np.random.default_rng(0)
    q8, s, _ = orc.rtn_quantize_int8((0.05 * rng.standard_normal((32, 256))).astype(np.float32), True, 128, False)
    blob = _dev(orc.repack_int8(q8, s, None, None, 128))
    out = torch.full((40, 32), NAN, device="cuda")
    with pytest.raises(RuntimeError, match="QBits: the prefill GEMM probe takes no int8 composite"):
        L.probe_gemm_f16(torch.zeros(40, 256, device="cuda"), blob, out, 40)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("c", R.WORKSPACE, ids=_ids(R.WORKSPACE))
def test_fragment_image_in_a_caller_workspace(c):
    """a workspace of exactly the plan's bytes holds the call; one byte less and the launcher takes per-call scratch
    (ws_bytes < plan.ws.total) and leaves the caller's workspace alone. Same bits both ways, and as without one."""
    group, asym, st = c["quant"]
    plan = L.probe_gemm_plan(c["K"], c["N"], group, L.WEIGHT_TYPES[c["wname"]], L.torch_dtype_code(DT[st]), L.C_BF16, asym,
                             False, c["M"], L.torch_dtype_code(DT[c["act"]]), c["K"], has_norm=True,
                             fp8=c["wname"] in R.G.FP8)
    total, guard = plan["ws_total"], 4096
    assert plan["form"] == R.FRAG and total > 0
    ws = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    base, _, _ = _run(c)
    got, _, _ = _run(dict(c, name=c["name"] + " / exact workspace"), ws=ws, ws_bytes=total)
    assert bool((ws[total:] == 0xA5).all()), "written behind the workspace"
    assert not bool((ws[:total] == 0xA5).all())
    ws.fill_(0xA5)
    short, _, _ = _run(dict(c, name=c["name"] + " / one byte short"), ws=ws, ws_bytes=total - 1)
    assert bool((ws == 0xA5).all()), "a workspace that is too small was used"
    assert torch.equal(_bits(base), _bits(got)) and torch.equal(_bits(base), _bits(short))


@pytest.mark.parametrize("c", R.TALL_CASES, ids=_ids(R.TALL_CASES))
def test_tall_tiles_behind_the_norm_and_silu_mul(c):
    """256-row tiles: the qkv form (norm, fp16 out), and gate/up at nb_m128 = 18, where the second epilogue call of the
    last workgroup (row0 + 128 < M) runs with one live row. The reference goes over the rows in blocks of 256."""
    d = R.build(c)
    blob = _dev_blob(c, d)
    L.gemm_form_log()
    got = _launch(c, d, blob)
    again = _launch(c, d, blob)
    forms = L.gemm_form_log()
    assert forms == [c["expect"][0]] * 2, (c["name"], forms)
    worst = rounding = 0.0
    for r0 in range(0, c["M"], 256):
        rows = slice(r0, min(r0 + 256, c["M"]))
        w, _, r = _check(c, d, got[rows], rows)
        worst, rounding = max(worst, w), max(rounding, r)
    print("%s [%s]: form %d, 1 K slices, worst |out - ref| / band %.3f (the rounded reference: %.3f)" % (
        c["name"], c["kind"], forms[0], worst, rounding))
    assert torch.equal(_bits(got), _bits(again)), c["name"] + ": a repeated call differs"
