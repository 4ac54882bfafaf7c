"""The fp32-activation decode GEMVs alone, with their fused epilogues, through `woq_probe_gemv_f32` — the tile kernel
(csrc/woq_gemv_i8.hip), the generic kernel (csrc/woq_gemv.hip) and the fp8 matrix-core kernel with its SiLU * mul pairing
launch (csrc/woq_gemv_fp8.hip), as `engine_linear_f32` runs them — against tests/gemv_f32_reference.py (float64).

The cases, their inputs and the tolerance are the reference module's (`CASES`, `SPECIAL`, `build`, `terms`): the tile and
generic kernels within 4 (A + B) of R0, the fp8 kernel within the project's 1e-5 sum|x g||w| |inv| + 1e-5 + 4 B; nothing
here is decided from a kernel's output. Per case: the device repack equals the oracle's blob byte for byte; the probe's
`form_out` equals the form the case names (asserted before any number); `out` is NaN inside its window (the residual where
the residual aliases it) and a sentinel behind it, the padding columns of a row stride and the sentinel survive; two runs
into fresh buffers are bit-equal. Every case prints max A, B and the largest |out - R0| / tolerance.

Largest observed |out - R0| / tolerance per kernel form, MI355X (observed |out - R0| sits at B, the activation's fixed
point, or below it for every matrix-core form: the counted fp32 chain A is a worst-case sum and leaves two to three
orders of magnitude unused, the fp8 bound one to two):
  tile, per-128 / per-column scales   0.015  (K 2048, 4 x 4; 0.001 at K 16384)
  tile, per-32 scales + zero points   0.028  (special inputs, format extremes; 0.001 on the N(0, 1) cases)
  CB = 2 gate/up                      0.010  (K 2048; 0.002 at K 8192, 0.001 per-32 at K 6144)
  table types (nf4, fp4_e2m1)         0.005  (fp4_e2m1 gate/up)
  act-order gather                    0.003  (K 4096 per-128, fp32 and bf16 rows; 0.001 at K 16384)
  chained (2 launches, K 16512)       0.001
  generic kernel                      0.001  (format extremes; 2e-5 .. 2e-4 on the N(0, 1) cases, B = 0)
  fp8 matrix-core                     0.089  (special inputs, format extremes; <= 0.017 on the N(0, 1) cases)
  fp8 + silu_mul_tiles                0.014
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import gemv_f32_reference as R

pytestmark = pytest.mark.gpu

SENT = 777.0
_BLOBS = {}


def _dev(a, dt=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dt is None else t.to(dt)


def _dev_blob(c, d):
    """the device repack of the same (q, scale, zp, g_idx): equal to the oracle's blob byte for byte"""
    from intel_extension_for_transformers_amd import qbits

    key = (c["K"], c["N"], c["form"], c["wname"], c["cname"], c["epi"], c["shuffle"])
    if key not in _BLOBS:
        group, asym, sname = c["form"]
        e8, e32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)
        blob = qbits.repack_quantized_weight(_dev(d["q"].view(np.int8)), _dev(d["s"]), e8 if d["z"] is None else _dev(d["z"]),
                                             e32 if d["idx"] is None else _dev(d["idx"]), c["wname"], sname, c["cname"],
                                             asym, group)
        assert np.array_equal(blob.cpu().numpy().view(np.uint8), d["blob"]), "device repack != oracle repack"
        _BLOBS[key] = blob
    return _BLOBS[key]


def _launch(c, d, x, blob):
    """one probe call on fresh buffers -> (form, out [M, n_out] fp32 numpy)"""
    M, K, n_out = x.shape[0], c["K"], d["n_out"]
    lda = K + 8 if (c["misalign"] or M > 1) else K
    xbuf = torch.zeros(M * lda + 8, dtype=torch.bfloat16 if c["act"] == "bf16" else torch.float32, device="cuda")
    xt = xbuf[1:] if c["misalign"] else xbuf  # rows one element off 16-byte alignment
    xt[:M * lda].view(M, lda)[:, :K].copy_(_dev(x))
    ldo = n_out + 8 if M > 1 else n_out
    obuf = torch.full((M * ldo + 64,), SENT, device="cuda")
    win = obuf[:M * ldo].view(M, ldo)
    win.fill_(float("nan"))
    res, ld_res = None, None
    if c["residual"] == "alias":
        win[:, :n_out].copy_(_dev(d["residual"]))
        res, ld_res = obuf, ldo
    elif c["residual"] == "separate":
        res, ld_res = _dev(d["residual"]), n_out
    gu = torch.full((2 * n_out,), float("nan"), device="cuda") if c["gu_tmp"] else None
    form = L.probe_gemv_f32(xt, blob, obuf, M=M, lda=lda, ldo=ldo, norm_w=_dev(d["g"]), eps=R.EPS, epi=c["epi"],
                            bias=_dev(d["bias"]), residual=res, ld_res=ld_res, gu_tmp=gu)
    torch.cuda.synchronize()
    o = obuf.cpu().numpy()
    assert (o[M * ldo:] == SENT).all(), c["name"] + ": written behind the window"
    o = o[:M * ldo].reshape(M, ldo)
    assert np.isnan(o[:, n_out:]).all(), c["name"] + ": written between the rows"
    return form, o[:, :n_out].copy()


def _run(c, x=None, what=None):
    what = what or c["name"]
    d = R.build(c)
    t = R.terms(c, d, x)
    assert t["form"] == c["expect"], what
    x = d["x"] if x is None else x
    blob = _dev_blob(c, d)
    form, out = _launch(c, d, x, blob)
    assert form == c["expect"], (what, form)  # the form first, then the numbers
    err = np.abs(out.astype(np.float64) - t["r0"])
    ratio = float((err / t["tol"]).max())
    print("%s: form %s, n_ops %d, max A = %.3e, B = %.3e, max tolerance = %.3e, max |out - R0| = %.3e, worst ratio %.2e"
          % (what, form, t["n_ops"], float(t["A"].max()), t["B"], float(t["tol"].max()), float(err.max()), ratio))
    assert np.isfinite(out).all() and (err <= t["tol"]).all(), what
    form2, out2 = _launch(c, d, x, blob)
    assert form2 == form and np.array_equal(out.view(np.int32), out2.view(np.int32)), what + ": two runs differ"
    return out, t, d


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c["name"])
def test_case(c):
    _run(c)


def test_one_tile_past_the_longest_k_chains_two_tile_launches():
    """what test_gpu_parity.py::test_decode_gemv_longest_k reaches through woq_linear at K = 16512 (no norm, no residual,
    fp32 out): two chained tile launches, not the generic kernel"""
    c = R.case("tile K16512 plain chained", 16512, (1, 2, 9, 8))
    _run(c)


@pytest.mark.parametrize("row", ["all zero", "one slice zero", "x30 in the last, partial slice", "format extremes"])
@pytest.mark.parametrize("c", R.SPECIAL, ids=lambda c: c["name"])
def test_special_inputs(c, row):
    x = R.special_rows(c)[row]
    out, t, d = _run(c, x, "%s, %s" % (c["name"], row))
    if row == "all zero":  # the factor is 1 / sqrt(eps), the product exactly 0: bias + residual in fp32, exactly
        want = np.zeros_like(out) if d["bias"] is None else np.broadcast_to(d["bias"], out.shape)
        want = (want + d["residual"]).astype(np.float32)
        assert np.array_equal(out, want), c["name"]


def test_the_fp8_engine_form_refuses_what_it_does_not_take():
    """M > 1, 16-bit rows or a bias with an fp8 composite blob: the engine's fp8 launcher has none of them"""
    c = R.BY_NAME["fp8 K256 norm"]
    d = R.build(c)
    blob = _dev_blob(c, d)
    out = torch.full((2 * 32 + 16,), SENT, device="cuda")
    x = torch.zeros(2 * 256, device="cuda")
    for kw in (dict(M=2), dict(bias=torch.zeros(32, device="cuda")), dict(x16=True)):
        xin = x.to(torch.bfloat16) if kw.pop("x16", False) else x
        with pytest.raises(RuntimeError, match="QBits: the engine's fp8 GEMV takes one fp32 row and no bias"):
            L.probe_gemv_f32(xin, blob, out, lda=256, ldo=32, **kw)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()
