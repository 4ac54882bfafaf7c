"""The prompt pass's MFMA GEMM in the form the plan picks for each shape (csrc/woq_gemm_f16.hip plan_gemm_f16, carried
out by launch_gemm_f16), every form asserted through `woq_gemm_form_log` so that a threshold change cannot quietly move a case
off the kernel it covers. Centre: the 256-row workgroup tiles of csrc/woq_gemm_f16t.h (`gemm_f16t_kernel`, chosen from
2048 rows when ceil(row blocks / 2) x column blocks >= 1024) at row counts that end anywhere in the last workgroup —
no second 128-row image (odd row-block count), a partial one, one row in it — with a partly live last column tile,
K padding, the shortest K loops, every scale type / mode, bias, 16-bit and strided outputs, the int8 residual
epilogue, the raw-A form (WOQ_GEMM_TALL_RAW=1, a fresh process) and the engine's own prompt pass.

Reference: oracle.linear_rows (dequantise -> matmul in fp64) on the same blob, applied to the activations exactly as
the kernel received them. Activation rows and scale rows carry exp(normal(0, 2)) factors (exponent clipped at +-4), so
per-row scaling matters. Bound (test_gpu_parity.py test_woq_linear_prefill_f16_operand_variants): 2e-3 *
rowmax|ref - bias| plus the output type's own rounding (bf16 2^-8, fp16 2^-10 of |ref|). Every row is checked; the
output is a NaN-filled (M + 3) x ldo buffer, so unwritten elements and stores past M / N are seen, and a second call
into a re-poisoned buffer must be bit-identical.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from oracle import woq_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
OUT_EPS = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -10}

HS, RING, TALL, RAW = L.GEMM_FORM_HANDSCHED, L.GEMM_FORM_RING, L.GEMM_FORM_TALL, L.GEMM_FORM_RAW
F_RING = HS | RING
F_TALL = HS | RING | TALL
F_RING_RAW = HS | RING | RAW
F_TALL_RAW = HS | RING | TALL | RAW

# (group, asym, scale type)
Q = [(128, False, "fp16"), (32, True, "fp16"), (128, True, "bf16"), (32, False, "fp32"), (-1, False, "fp32")]


def _inputs(M, N, K, group, asym, scale_type, act, wbits=4, seed=0, bias=False):
    """Host (q, scale, zp), activations in `act` dtype and an optional fp32 bias. The activations carry one power-of-two
    factor that puts the largest |output| near 1024, so fp16 outputs stay finite whatever the row / scale factors."""
    rng = np.random.default_rng(seed)
    g = K if group == -1 else group
    G = -(-K // g)
    lo, hi = (-8, 8) if wbits == 4 else (-128, 128)
    q = rng.integers(lo, hi, (K, N), dtype=np.int8)
    s = ((rng.random((G, N)) + 0.5) * 0.01 * np.exp(np.clip(rng.normal(0, 2, (G, 1)), -4, 4))).astype(np.float32)
    z = rng.integers(lo, hi, (G, N), dtype=np.int8) if asym else None
    r = np.exp(np.clip(rng.normal(0, 2, (M, 1)), -4, 4))
    x = rng.standard_normal((M, K)) * r
    s_used = torch.from_numpy(s).to(DT[scale_type]).float().numpy()
    w = q[:, :256].astype(np.float64) - (0 if z is None else np.repeat(z[:, :256], g, 0)[:K])
    w *= np.repeat(s_used[:, :256], g, 0)[:K]
    est = float(np.abs(x[np.argsort(r[:, 0])[-4:]] @ w).max())
    x *= 2.0 ** np.floor(np.log2(1024.0 / est))
    xt = torch.from_numpy(x.astype(np.float32)).to(DT[act])
    b = rng.random(N, dtype=np.float32) if bias else None
    return q, s, z, xt, b


def _blob(q, s, z, group, scale_type, compute="bf16", wtype="int4_clip"):
    from intel_extension_for_transformers_amd import qbits

    e8, e32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)
    return qbits.repack_quantized_weight(torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda(),
                                         e8 if z is None else torch.from_numpy(z).cuda(), e32, wtype, scale_type,
                                         compute, z is not None, group)


def _linear(x, blob, bias, out):
    """the C entry point with the output's own row stride as ldo (test_gpu_parity.py strided-rows idiom)"""
    from intel_extension_for_transformers_amd import qbits

    hdr = qbits.header_of(blob)
    L.check(L.lib().woq_linear(ctypes.c_void_p(x.data_ptr()), L.torch_dtype_code(x.dtype), x.stride(0),
                               ctypes.c_void_p(blob.data_ptr()), ctypes.byref(hdr),
                               None if bias is None else ctypes.c_void_p(bias.data_ptr()),
                               ctypes.c_void_p(out.data_ptr()), L.torch_dtype_code(out.dtype), out.stride(0),
                               x.shape[0], L.stream_ptr()))


def _poisoned_calls(x, blob, bias, N, out_dtype, ldo):
    """two calls, each into a fresh NaN-filled (M + 3) x ldo buffer; returns (first buffer, second == first, guards
    still NaN after both)"""
    M = x.shape[0]
    xd = x.cuda()
    bd = None if bias is None else torch.from_numpy(bias).cuda()
    bufs = []
    for _ in range(2):
        buf = torch.full((M + 3, ldo), float("nan"), dtype=DT[out_dtype], device="cuda")
        _linear(xd, blob, bd, buf[:M, :N])
        torch.cuda.synchronize()
        bufs.append(buf)
    same = bool(torch.equal(bufs[0][:M, :N], bufs[1][:M, :N]))
    guards = all(bool(torch.isnan(b[M:]).all()) and bool(torch.isnan(b[:, N:]).all()) for b in bufs)
    return bufs[0][:M, :N].cpu(), same, guards


def _stored(got, what):
    g = got.float().numpy()
    assert not np.isnan(g).any(), "%s: %d output elements never stored, first at %s" % (
        what, int(np.isnan(g).sum()), tuple(np.argwhere(np.isnan(g))[0]))
    return g


def _check(got, x, blob_host, bias, out_dtype, what):
    """every row vs oracle.linear_rows; returns the worst row error over its row maximum"""
    g = _stored(got, what)
    ref = orc.linear_rows(x.float().numpy(), blob_host)
    if bias is not None:
        ref = ref + bias
    scale = np.abs(ref - (0 if bias is None else bias)).max(axis=1, keepdims=True)
    err = np.abs(g - ref)
    bad = err > 2e-3 * scale + OUT_EPS[out_dtype] * np.abs(ref) + 1e-5
    assert not bad.any(), "%s: %d elements off, first at %s, worst %.3e of rowmax" % (
        what, int(bad.sum()), tuple(np.argwhere(bad)[0]), float((err / scale).max()))
    return float((err / scale).max())


def _run_case(M, N, K, quant, act, out_dtype, form, ldo=None, compute="bf16", seed=0, wbits=4):
    group, asym, st = quant
    q, s, z, x, bias = _inputs(M, N, K, group, asym, st, act, wbits=wbits, seed=seed, bias=out_dtype == "fp32")
    blob = _blob(q, s, z, group, st, compute, "int4_clip" if wbits == 4 else "int8")
    L.gemm_form_log()
    got, same, guards = _poisoned_calls(x, blob, bias, N, out_dtype, ldo or N + 2)
    launches = 1 if wbits == 4 else 2  # int8: two int4 GEMMs, the second adding the first through `residual`
    what = "M=%d N=%d K=%d %s act=%s out=%s" % (M, N, K, quant, act, out_dtype)
    assert L.gemm_form_log() == [form] * (2 * launches), what
    assert guards, "%s: rows past M or columns past N were written" % what
    _stored(got, what)
    assert same, "%s: a repeated call differs" % what
    worst = _check(got, x, blob.cpu().numpy().view(np.uint8), bias, out_dtype, what)
    print("%s: form %d, worst row error / rowmax %.3e" % (what, form, worst))


# (M, N, K, quantisation, activations, output) — nb_m = ceil(M / 128); tall from ceil(nb_m / 2) * nb_n >= 1024
TALL_CASES = [
    (2048, 22016, 512, Q[0], "fp32", "fp32"),  # whole 256-row tiles
    (2049, 22016, 256, Q[1], "bf16", "bf16"),  # nb_m 17: one live row, the second image does not exist
    (2049, 22016, 768, Q[2], "fp32", "fp16"),
    (2049, 22016, 480, Q[3], "fp16", "fp32"),  # K padding (Kpad 512); fp16 rows with K % 128 != 0: packed
    (2148, 22016, 512, Q[3], "bf16", "fp16"),  # nb_m 17: 100 rows
    (2148, 22016, 256, Q[4], "fp32", "bf16"),
    (2148, 22016, 480, Q[1], "fp16", "bf16"),
    (2213, 22016, 768, Q[0], "bf16", "fp32"),  # nb_m 18: the second image holds 37 rows
    (2213, 22016, 512, Q[2], "bf16", "bf16"),
    (2213, 22016, 256, Q[4], "fp32", "fp16"),
    (2560, 12288, 512, Q[0], "fp32", "fp32"),  # the seam: 10 x 96 workgroups, 128-row ring
    (2560, 12288, 256, Q[2], "bf16", "bf16"),
    (2561, 12288, 512, Q[0], "fp32", "fp32"),  # 11 x 96: tall
    (2561, 12288, 768, Q[1], "bf16", "fp16"),
    (2561, 12288, 480, Q[3], "fp16", "bf16"),
    (2829, 12288, 256, Q[2], "fp32", "fp32"),  # nb_m 23, odd
    (2829, 12288, 768, Q[3], "bf16", "bf16"),
    (2829, 12288, 512, Q[4], "bf16", "fp16"),
    (2829, 12288, 480, Q[1], "fp16", "fp16"),
    (4225, 12288, 512, Q[1], "fp32", "bf16"),  # nb_m 34: one row in the second image
    (4225, 12288, 256, Q[3], "bf16", "fp32"),
    (4225, 12288, 768, Q[4], "fp32", "fp32"),
    (4225, 12288, 480, Q[3], "fp16", "fp16"),
    (2829, 12296, 512, Q[0], "bf16", "fp32"),  # last column workgroup: one 16-column tile, 8 columns live
    (2829, 12296, 768, Q[2], "fp32", "bf16"),
    (2829, 12296, 256, Q[1], "fp32", "fp16"),
    (2829, 12296, 480, Q[3], "fp16", "fp32"),
    (2829, 12296, 512, Q[4], "bf16", "bf16"),
    (2829, 12288, 4096, Q[1], "bf16", "fp16"),  # the Llama-2-7B qkv shape
]


@pytest.mark.parametrize("M,N,K,quant,act,out_dtype", TALL_CASES,
                         ids=["M%d-N%d-K%d-g%d%s-%s-%s-%s" % (M, N, K, qq[0], "a" if qq[1] else "s", qq[2], a, o)
                              for M, N, K, qq, a, o in TALL_CASES])
def test_tall_gemm_ragged_rows_vs_oracle(M, N, K, quant, act, out_dtype):
    """(a) default selection at 2048+ rows: 256-row tiles everywhere but the 2560-row seam case at N = 12288"""
    _run_case(M, N, K, quant, act, out_dtype, F_RING if (M, N) == (2560, 12288) else F_TALL, seed=M + N + K)


def test_tall_gemm_odd_ldo_vs_oracle():
    """(a) ldo = N + 1: the scalar-store epilogue of the 256-row kernel"""
    _run_case(2213, 22016, 512, Q[0], "bf16", "fp32", F_TALL, ldo=22017, seed=5)


@pytest.mark.parametrize("M,N,quant", [(2049, 22016, (128, False, "fp16")), (2829, 12288, (32, True, "bf16"))])
def test_tall_gemm_int8_residual_vs_oracle(M, N, quant):
    """(b) int8 weights: two int4 GEMMs on the same rows, the second adding the first (fp32, through `residual`) —
    both on the 256-row kernel"""
    _run_case(M, N, 512, quant, "bf16", "fp32", F_TALL, wbits=8, seed=M)


def _nf4_blob(N, K, compute, seed):
    from intel_extension_for_transformers_amd import qbits

    w = (np.random.default_rng(seed).standard_normal((N, K)) * 0.05).astype(np.float32)
    return qbits.quantize_to_packed_weight(torch.from_numpy(w).cuda(), True, 128, compute, "nf4", "fp32", False)


# (what, M, N, K, quantisation or "nf4", activations, compute, expected form)
DISPATCH = [
    ("split-K", 17, 4096, 4096, Q[0], "fp32", "bf16", L.GEMM_FORM_SPLITK),
    ("odd K-tile count: hipcc's schedule", 200, 1024, 640, Q[0], "fp32", "bf16", 0),
    ("ring, packed A", 200, 1024, 512, Q[0], "fp32", "bf16", F_RING),
    ("ring, raw A", 200, 1024, 512, Q[0], "fp16", "bf16", F_RING_RAW),
    ("fp32-class", 200, 1024, 512, Q[0], "fp32", "fp32", L.GEMM_FORM_FP32),
    ("group 32 asym fp32 scales: two-tile form", 200, 1024, 512, (32, True, "fp32"), "fp32", "bf16", HS),
    ("group 32 asym fp32 scales at a tall size: not ring", 2829, 12288, 512, (32, True, "fp32"), "bf16", "bf16", HS),
    ("nf4: fragment image", 200, 1024, 512, "nf4", "fp32", "bf16", L.GEMM_FORM_FRAG),
    ("nf4 fp32-class", 200, 1024, 512, "nf4", "fp32", "fp32", L.GEMM_FORM_FRAG | L.GEMM_FORM_FP32),
    ("seam 2560: ring", 2560, 12288, 256, Q[0], "bf16", "bf16", F_RING),
    ("seam 2561: tall", 2561, 12288, 256, Q[0], "bf16", "bf16", F_TALL),
    ("fp16 rows at a tall size: ring raw A", 2829, 12288, 512, Q[0], "fp16", "bf16", F_RING_RAW),
]


@pytest.mark.parametrize("what,M,N,K,quant,act,compute,form", DISPATCH, ids=[d[0] for d in DISPATCH])
def test_gemm_dispatch_map(what, M, N, K, quant, act, compute, form):
    """(c) the selector's choice for a few shapes, each also against the oracle (a threshold change shows up here)"""
    if quant == "nf4":
        blob = _nf4_blob(N, K, compute, M + K)
        _, _, _, x, _ = _inputs(M, 256, K, 128, False, "fp32", act, seed=M + K)
        L.gemm_form_log()
        got, same, guards = _poisoned_calls(x, blob, None, N, "fp32", N + 2)
        assert L.gemm_form_log() == [form] * 2, what
        _stored(got, what)
        assert guards and same, what
        _check(got, x, blob.cpu().numpy().view(np.uint8), None, "fp32", what)
    else:
        _run_case(M, N, K, quant, act, "fp32", form, compute=compute, seed=M + K)


# ---- (d) raw-A 256-row tiles (WOQ_GEMM_TALL_RAW=1, read once per process) from a cold start, in a child process -----
CHILD_CASES = [  # (M, N, quantisation, activations, weight bits, expected form); K = 512; the first one is the
    (2829, 12288, Q[0], "fp32", 4, F_TALL),  # child's first GEMM launch
    (2049, 22016, Q[0], "fp16", 4, F_TALL_RAW),
    (2213, 22016, Q[1], "fp16", 4, F_TALL_RAW),
    (2829, 22016, Q[2], "fp16", 4, F_TALL_RAW),
    (2829, 12288, Q[0], "fp16", 8, F_TALL_RAW),  # raw A + residual
]


def _child_main(out_dir):
    """run in a fresh process by test_tall_gemm_raw_a_cold_start: the CHILD_CASES calls, results saved for the parent"""
    torch.cuda.set_device(0)
    for i, (M, N, quant, act, wbits, _) in enumerate(CHILD_CASES):
        group, asym, st = quant
        q, s, z, x, bias = _inputs(M, N, 512, group, asym, st, act, wbits=wbits, seed=100 + i, bias=True)
        blob = _blob(q, s, z, group, st, "bf16", "int4_clip" if wbits == 4 else "int8")
        got, same, guards = _poisoned_calls(x, blob, bias, N, "fp32", N + 2)
        torch.save(dict(got=got, same=same, guards=guards, forms=L.gemm_form_log(), blob=blob.cpu()),
                   os.path.join(out_dir, "case%d.pt" % i))


def test_tall_gemm_raw_a_cold_start(tmp_path):
    """(d) WOQ_GEMM_TALL_RAW=1 in a fresh process whose first GEMM launches are 256-row calls into NaN-poisoned
    outputs: packed A, raw fp16 A at ragged rows, int8 raw A with the residual add"""
    env = dict(os.environ, WOQ_GEMM_TALL_RAW="1")
    code = "import sys; from tests.test_gpu_prefill_gemm_forms import _child_main; _child_main(sys.argv[1])"
    p = subprocess.run([sys.executable, "-c", code, str(tmp_path)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    for i, (M, N, quant, act, wbits, form) in enumerate(CHILD_CASES):
        r = torch.load(str(tmp_path / ("case%d.pt" % i)))
        what = "child case %d: M=%d N=%d %s act=%s int%d" % (i, M, N, quant, act, wbits)
        assert r["forms"] == [form] * (2 if wbits == 4 else 4), (what, r["forms"])
        assert r["guards"], "%s: rows past M or columns past N were written" % what
        _stored(r["got"], what)
        assert r["same"], "%s: a repeated call differs" % what
        group, asym, st = quant
        _, _, _, x, bias = _inputs(M, N, 512, group, asym, st, act, wbits=wbits, seed=100 + i, bias=True)
        worst = _check(r["got"], x, r["blob"].numpy().view(np.uint8), bias, "fp32", what)
        print("%s: worst row error / rowmax %.3e" % (what, worst))


# ---- 3. the engine's prompt pass at a size where qkv and gate/up take the 256-row kernel ---------------------------
@pytest.mark.parametrize("group,asym", [(128, False), (32, True)])
def test_engine_prompt_pass_on_tall_gemm_vs_oracle(group, asym):
    """Llama-2-7B hidden / heads / MLP geometry (inter 11008), two layers, one prompt of 2829 tokens (nb_m 23, odd):
    qkv (RMSNorm pack pass) and gate/up (SiLU * mul epilogue, fp16 out) on 256-row tiles, o / down on the raw-A ring.
    Layer 0's cache covers every row of the qkv GEMM; layer 1's cache at each position depends on layer 0's o, gate/up
    and down rows at that position, so every row of the gate/up epilogue is covered; the logits cover the last row.
    Layer 1 bound 1.5e-2 of max instead of KV_TOL: after the 11008-wide MLP the fp16-operand rounding tail is longer
    (measured worst 1.02e-2 of max at group 128 sym, one position; 3.2e-3 at group 32 asym). The 128-row ring kernel
    (WOQ_GEMM_TALL=0) gives the same cache bit for bit, so the tail does not come from the 256-row tiles."""
    from tests.test_gpu_attention_fullgeom import KV_TOL, PF_TOL, build_attention_geometry, check_cache_rows

    T = 2829
    eng, oracle, cfg = build_attention_geometry(inter=11008, vocab=512, max_ctx=2880, layers=2, group=group, asym=asym)
    prompt = np.random.default_rng(T + group).integers(0, cfg["vocab"], T).tolist()
    L.gemm_form_log()
    got = eng.prefill(prompt, greedy=True)[0].cpu().numpy().copy()
    assert L.gemm_form_log() == [F_TALL, F_RING_RAW, F_TALL, F_RING_RAW] * 2
    ref = oracle.forward_prompt(prompt)
    w0 = check_cache_rows(eng, oracle, 0, T, layer=0)
    w1 = check_cache_rows(eng, oracle, 0, T, layer=1, tol=1.5e-2)
    err = float(np.abs(got - ref).max())
    print("group %d asym %s: cache rows worst %.2e (layer 0), %.2e (layer 1) of max, logits %.2e of max" % (
        group, asym, w0, w1, err / np.abs(ref).max()))
    assert w0 <= KV_TOL
    assert err <= PF_TOL * np.abs(ref).max() + 1e-3
    assert int(got.argmax()) == int(ref.argmax())
    assert eng.status() == 0
