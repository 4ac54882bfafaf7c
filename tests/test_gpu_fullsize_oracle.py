"""Full-size parity against the CPU ORACLE (not against the HIP library's own dequantise): every linear shape of
the BASELINE.json configurations at batch 1, and a Llama-2-7B-shaped decoder of 8 layers whose logits are compared
with `LlamaOracle` on the same (q, scale, zp).

north_star: "Outputs match the reference's own CPU int4 path on the same inputs within a stated fp tolerance (logits
max-abs)". The oracle is the reference's definition of that path (autograd/functions.py:41-63: dequantise -> matmul
-> + bias) evaluated with double accumulation. Stated tolerances:
  per linear : max|y_gpu - y_oracle| <= 1e-4 * max|y_oracle| + 1e-6      (reference's own: allclose(rtol=0.03))
  decoder    : max|logit_gpu - logit_oracle| <= 2e-3 * max|logit_oracle| + 1e-4, identical greedy token
               (fp16 KV cache / embedding / lm_head storage on the GPU side, fp32 in the oracle)
(q, scale, zp) are generated on the HOST and packed twice — by the oracle's repack and by the device repack — and the
two blobs must agree byte for byte before anything is multiplied.
"""
import numpy as np
import pytest
import torch

from oracle import woq_oracle as orc

pytestmark = pytest.mark.gpu

# (K, N) of the fused projections: qkv, o, gate/up, down
LLAMA2_7B = {"qkv": (4096, 12288), "o": (4096, 4096), "gate_up": (4096, 22016), "down": (11008, 4096)}
LLAMA2_70B_TP8 = {"qkv": (8192, 1280), "o": (1024, 8192), "gate_up": (8192, 7168), "down": (3584, 8192)}
LLAMA2_70B_TP2 = {"qkv": (8192, 5120), "o": (4096, 8192), "gate_up": (8192, 28672), "down": (14336, 8192)}
LLAMA2_70B = {"qkv": (8192, 10240), "o": (8192, 8192), "down": (28672, 8192)}  # gate/up 8192 x 57344: see TP2 (same K)
MISTRAL_7B = {"qkv": (4096, 6144), "gate_up": (4096, 28672), "down": (14336, 4096)}

CASES = []
for model, shapes, quant in (("llama2-7b", LLAMA2_7B, [(128, False), (32, True)]),
                             ("llama2-70b-tp8", LLAMA2_70B_TP8, [(128, False)]),
                             ("llama2-70b-tp2", LLAMA2_70B_TP2, [(128, False)]),
                             ("llama2-70b", LLAMA2_70B, [(128, False)]),
                             ("mistral-7b", MISTRAL_7B, [(128, False)])):
    for name, (K, N) in shapes.items():
        for group, asym in quant:
            CASES.append(pytest.param(K, N, group, asym, id="%s-%s-g%d-%s" % (model, name, group,
                                                                             "asym" if asym else "sym")))


def _host_qsz(rng, K, N, group, asym):
    G = K // group
    q = rng.integers(-8, 8, (K, N), dtype=np.int8)
    s = ((rng.random((G, N), dtype=np.float32) + 0.5) * 0.005).astype(np.float32)
    z = rng.integers(-8, 8, (G, N), dtype=np.int8) if asym else None
    return q, s, z


def _gpu_pack(qbits, q, s, z, group, scale_dtype="fp16"):
    e8, e32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)
    return qbits.repack_quantized_weight(torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda(),
                                         e8 if z is None else torch.from_numpy(z).cuda(), e32, "int4_clip",
                                         scale_dtype, "fp32", z is not None, group)


@pytest.mark.parametrize("K,N,group,asym", CASES)
def test_fullsize_woq_linear_vs_oracle(K, N, group, asym):
    from intel_extension_for_transformers_amd import qbits

    rng = np.random.default_rng(K * 7 + N + group)
    q, s, z = _host_qsz(rng, K, N, group, asym)
    ref_blob = orc.repack(q, s, z, None, group, scale_type=orc.F16)
    blob = _gpu_pack(qbits, q, s, z, group)
    assert np.array_equal(blob.cpu().numpy().view(np.uint8), ref_blob), "device repack != oracle repack"
    worst = 0.0
    for M in (1, 3):  # the decode kernel's one-row and multi-row forms
        x = rng.standard_normal((M, K)).astype(np.float32)
        bias = rng.standard_normal(N).astype(np.float32) if M == 3 else None
        out = torch.empty(M, N, device="cuda")
        qbits.woq_linear(torch.from_numpy(x).cuda(), blob, torch.empty(0) if bias is None else torch.from_numpy(bias).cuda(),
                         out, "fp32", "int4_clip", "fp16", asym)
        ref = orc.woq_linear(x, ref_blob, bias)
        err = np.abs(out.cpu().numpy() - ref).max()
        worst = max(worst, err / np.abs(ref).max())
        assert err <= 1e-4 * np.abs(ref).max() + 1e-6, (M, err, np.abs(ref).max())
    print("K=%d N=%d g%d %s: worst max-abs error / max|ref| = %.2e" % (K, N, group, "asym" if asym else "sym", worst))


def build_7b_shape(n_layers, group, asym, seed=11, max_ctx=64, kv_dtype=torch.float16):
    """Llama-2-7B-shaped decoder with `n_layers` layers, (q, scale, zp) generated on the host; returns the engine and
    the oracle decoder over the same tensors (separate q / k / v / gate / up blobs on the oracle side, fused ones on
    the engine side — the two packings are independent code)."""
    from intel_extension_for_transformers_amd import qbits
    from intel_extension_for_transformers_amd.runtime import WoqDecoderEngine, fuse_gate_up

    cfg = dict(hidden=4096, inter=11008, heads=32, kv_heads=32, head_dim=128, layers=n_layers, vocab=32000, eps=1e-5,
               theta=10000.0)
    rng = np.random.default_rng(seed)
    H, I, NH, KV, D = cfg["hidden"], cfg["inter"], cfg["heads"], cfg["kv_heads"], cfg["head_dim"]
    eng = WoqDecoderEngine(H, I, NH, KV, D, n_layers, cfg["vocab"], max_ctx=max_ctx, rms_eps=cfg["eps"],
                           rope_theta=cfg["theta"], kv_dtype=kv_dtype)
    tt = torch.from_numpy
    layers = []
    for l in range(n_layers):
        parts = {n: _host_qsz(rng, k, nn, group, asym)
                 for n, (k, nn) in dict(q=(H, NH * D), k=(H, KV * D), v=(H, KV * D), o=(NH * D, H), gate=(H, I),
                                        up=(H, I), down=(I, H)).items()}
        ly = {n: orc.repack(q, s, z, None, group, scale_type=orc.F16) for n, (q, s, z) in parts.items()}
        cat = lambda i: np.concatenate([parts["q"][i], parts["k"][i], parts["v"][i]], 1)  # noqa: E731
        qkv = _gpu_pack(qbits, cat(0), cat(1), cat(2) if asym else None, group)
        o = _gpu_pack(qbits, *parts["o"], group)
        fz = fuse_gate_up(tt(parts["gate"][2]), tt(parts["up"][2])).numpy() if asym else None
        gu = _gpu_pack(qbits, fuse_gate_up(tt(parts["gate"][0]), tt(parts["up"][0])).numpy(),
                       fuse_gate_up(tt(parts["gate"][1]), tt(parts["up"][1])).numpy(), fz, group)
        down = _gpu_pack(qbits, *parts["down"], group)
        ly["ln1"] = (1 + 0.05 * rng.standard_normal(H)).astype(np.float32)
        ly["ln2"] = (1 + 0.05 * rng.standard_normal(H)).astype(np.float32)
        eng.set_layer(l, qkv, o, gu, down, tt(ly["ln1"]), tt(ly["ln2"]))
        layers.append(ly)
        del parts
    embed = tt((rng.standard_normal((cfg["vocab"], H)) * 0.5).astype(np.float32)).half()
    lm = tt((rng.standard_normal((cfg["vocab"], H)) * 0.02).astype(np.float32)).half()
    norm = (1 + 0.05 * rng.standard_normal(H)).astype(np.float32)
    eng.set_head(embed, tt(norm), lm)
    return eng, orc.LlamaOracle(cfg, embed.float().numpy(), layers, norm, lm.float().numpy()), cfg


@pytest.mark.parametrize("group,asym", [(128, False), (32, True)])
def test_llama2_7b_shape_decoder_logits_vs_oracle(group, asym):
    """8 layers of the real Llama-2-7B geometry (hidden 4096, inter 11008, 32 heads, vocab 32000): three decode steps
    (so the last one attends over a cache), then the same three tokens as one prompt pass."""
    eng, oracle, cfg = build_7b_shape(8, group, asym)
    toks = [11, 20000, 317]
    worst = 0.0
    for i, t in enumerate(toks):
        eng.token.fill_(t)
        eng.pos.fill_(i)
        eng.step(greedy=False)
        got = eng.logits.cpu().numpy()
        ref = oracle.forward_token(t, i)
        err = float(np.abs(got - ref).max())
        worst = max(worst, err / float(np.abs(ref).max()))
        assert err <= 2e-3 * np.abs(ref).max() + 1e-4, (i, err, np.abs(ref).max())
        assert int(got.argmax()) == int(ref.argmax())
    print("7B shape, 8 layers, g%d %s: worst logits max-abs / max|logit| = %.2e (decode)" % (
        group, "asym" if asym else "sym", worst))
    got = eng.prefill(toks, greedy=False)[0].cpu().numpy()
    perr = float(np.abs(got - ref).max())
    assert perr <= 1e-2 * np.abs(ref).max() + 1e-3, perr  # prompt pass: fp16-operand GEMMs (tests/test_gpu_engine.py)
    assert int(got.argmax()) == int(ref.argmax())


def test_qbits_debug_switch_full_size(monkeypatch):
    """QBITS_DEBUG (reference autograd/functions.py:108,203) flips QuantizedLinearQBits.forward between the fused
    kernel and qbits_woq_linear_ref_impl (dequantise -> matmul); both arms agree at a full-size shape, and the
    reference arm agrees with the oracle."""
    from intel_extension_for_transformers_amd.transformers.llm.quantization.autograd import (
        matmul_kbit, qbits_woq_linear_ref_impl)
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    K, N, group = 11008, 4096, 128
    rng = np.random.default_rng(5)
    q, s, z = _host_qsz(rng, K, N, group, True)
    m = QuantizedLinearQBits(K, N, bias=True, compute_dtype="fp32", weight_dtype="int4_clip", scale_dtype="fp16",
                             blocksize=group, scheme="asym", device="cuda")
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32))

    class _Q:
        quant_method, sym = "rtn", False

    m.set_weights_bias(torch.from_numpy(q + 8), torch.from_numpy(s), torch.from_numpy(z + 8), None, _Q(), bias)
    x = torch.from_numpy(rng.standard_normal((2, K)).astype(np.float32)).cuda()
    monkeypatch.delenv("QBITS_DEBUG", raising=False)
    fused = m(x)
    monkeypatch.setenv("QBITS_DEBUG", "1")
    ref_arm = m(x)
    monkeypatch.delenv("QBITS_DEBUG")
    ref = orc.woq_linear(x.cpu().numpy(), orc.repack(q, s, z, None, group, scale_type=orc.F16), bias.numpy())
    scale = np.abs(ref).max()
    assert np.abs(fused.cpu().numpy() - ref).max() <= 1e-4 * scale
    assert np.abs(ref_arm.cpu().numpy() - ref).max() <= 1e-4 * scale  # torch fp32 matmul order
    direct = qbits_woq_linear_ref_impl(x, m.weight.data, bias.cuda(), "fp32", "int4_clip", "fp16")
    assert torch.equal(direct, ref_arm.float())
    out = torch.empty(2, N, device="cuda")
    assert matmul_kbit(x, m.weight, bias.cuda(), out, "fp32", "int4_clip", "fp16", "asym") is out
    assert torch.equal(out, fused)
    with pytest.raises(NotImplementedError):
        matmul_kbit(x, m.weight, None, out, "fp32", "int4_clip", "fp16", "asym", do_dequant=True)


@pytest.mark.parametrize("kv_dtype,group,asym", [(torch.float16, 128, False), (torch.float8_e4m3fn, 128, False),
                                                  (torch.float16, 32, True)])
def test_in_launch_handoffs_equal_separate_launches(kv_dtype, group, asym):
    """csrc/woq_gemv_attn.hip: the decode layer's qkv GEMV + attention as ONE launch (resident attention workgroups
    pick a head's q / k / v up as tagged granules while the strips are still finishing) against separate launches,
    same engine, same cache contents. The same instruction stream on the same values: logits and greedy tokens
    bit-identical. After a 200-token prompt pass (several passes of cached positions per wave — round 4 prefetches the
    V rows of the second 16-position run as well), over eager steps and graph replays; the sticky status stays clear.
    (Round 3's second in-launch form, the layer as two chained launches, was a measured negative and left the library in
    round 4: tools/rejected/woq_gemv_chain.hip.)"""
    eng, _, cfg = build_7b_shape(4, group, asym, kv_dtype=kv_dtype, max_ctx=512)
    rng = np.random.default_rng(11)
    prompt = rng.integers(0, cfg["vocab"], 200).tolist()
    out = {}
    for mode in ("separate", "fused"):
        eng.set_fuse_attn(mode != "separate")
        assert eng.uses_fused_attn() == (mode != "separate")
        eng.prefill(prompt, greedy=True)
        logs = []
        for _ in range(6):
            eng.step(greedy=True)
            logs.append(eng.logits.clone())
        eng.capture(greedy=True)
        eng.replay(20)
        torch.cuda.synchronize()
        logs.append(eng.logits.clone())
        out[mode] = (torch.stack(logs), eng.token_log()[200:227].clone())
    assert eng.status() == 0
    assert torch.equal(out["fused"][0], out["separate"][0]) and torch.equal(out["fused"][1], out["separate"][1])


PREFILL_SHAPES = [("qkv", 4096, 12288), ("o", 4096, 4096), ("gate_up", 4096, 22016), ("down", 11008, 4096)]


def _sampled_rows(M, n, rng):
    """first / last row of the first, a middle and the last 128-row tile (the XCD-aware super-tile mapping and the
    raw-A row clamp live at those edges), the rest random"""
    mid = (M // 2) & ~127
    fixed = {0, 127, mid, mid + 127, M - 128, M - 1}
    return sorted(fixed | set(int(r) for r in rng.integers(0, M, n - len(fixed))))


@pytest.mark.parametrize("name,K,N", PREFILL_SHAPES)
@pytest.mark.parametrize("group,asym", [(128, False), (32, True)])
@pytest.mark.parametrize("act_dtype", [torch.float32, torch.float16])
def test_prefill_gemm_at_measured_size_vs_oracle(name, K, N, group, asym, act_dtype, M=8192):
    """The prompt pass's one-product MFMA GEMM (compute "bf16") at the M the bench line measures, every Llama-2-7B
    projection, both BASELINE quantisation variants: fp32 rows run the 256-row tiles (csrc/woq_gemm_f16t.h, packed A),
    fp16 rows the 128-row ring kernel fetching them raw (raw-A 256-row tiles are off by default); 8 x 8 super-tile
    mapping. 64 sampled rows against oracle.woq_linear on the same blob. The reference's own test compares at m = 256
    (qbits_ut/test_weightonly.py:51-88); bound 2e-3 * rowmax (fp16-operand products)."""
    from intel_extension_for_transformers_amd import _lib as L
    from intel_extension_for_transformers_amd import qbits

    rng = np.random.default_rng(K + N + group + M)
    q, s, z = _host_qsz(rng, K, N, group, asym)
    e8, e32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)
    blob = qbits.repack_quantized_weight(torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda(),
                                         e8 if z is None else torch.from_numpy(z).cuda(), e32, "int4_clip", "fp16",
                                         "bf16", asym, group)
    g = torch.Generator(device="cuda").manual_seed(K + M)
    x = torch.randn(M, K, generator=g, device="cuda", dtype=torch.float32).to(act_dtype)
    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32)
    L.gemm_form_log()
    qbits.woq_linear(x, blob, torch.empty(0), out, "bf16", "int4_clip", "fp16", asym)
    torch.cuda.synchronize()
    ring = L.GEMM_FORM_HANDSCHED | L.GEMM_FORM_RING
    assert L.gemm_form_log() == [ring | (L.GEMM_FORM_RAW if act_dtype == torch.float16 else L.GEMM_FORM_TALL)]
    assert not torch.isnan(out).any(), "output elements left unwritten"
    rows = _sampled_rows(M, 64, rng)
    got = out[rows].cpu().numpy()
    ref = orc.woq_linear(x[rows].float().cpu().numpy(), blob.cpu().numpy().view(np.uint8))
    rel = (np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max()
    assert rel <= 2e-3, (name, group, asym, str(act_dtype), float(rel))


@pytest.mark.parametrize("M", [2048, 2148, 2213, 4096 + 129])
@pytest.mark.parametrize("group,asym", [(128, False), (32, True)])
@pytest.mark.parametrize("act_dtype", [torch.float32, torch.float16])
def test_prefill_gemm_256_row_tiles_ragged_rows_vs_oracle(M, group, asym, act_dtype, N=384):
    """Round 6: from 2048 rows the one-product GEMM runs 256-row workgroup tiles (csrc/woq_gemm_f16t.h: two 128-row
    half-tile images per LDS slot) once ceil(row blocks / 2) x column blocks >= 1024. At N = 384 (3 column blocks)
    these row counts stay on the 128-row ring kernel; the N = 22016 twin below (172 column blocks) runs the 256-row
    tiles with fp32 rows. fp16 rows take the ring kernel raw at both widths (raw-A 256-row tiles are off by default).
    Row counts that end inside the first image of the last
    workgroup (2148: its second image does not exist and is clamped), inside its second image (2213), on a tile edge
    (2048) and one past a 128-row edge (4225); EVERY row against oracle.linear_rows, NaN-poisoned output first, the
    kernel form asserted."""
    from intel_extension_for_transformers_amd import _lib as L
    from intel_extension_for_transformers_amd import qbits

    K = 512
    rng = np.random.default_rng(M + group)
    q, s, z = _host_qsz(rng, K, N, group, asym)
    e8, e32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)
    blob = qbits.repack_quantized_weight(torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda(),
                                         e8 if z is None else torch.from_numpy(z).cuda(), e32, "int4_clip", "fp16",
                                         "bf16", asym, group)
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn(M, K, generator=g, device="cuda", dtype=torch.float32).to(act_dtype)
    out = torch.full((M + 3, N), float("nan"), device="cuda", dtype=torch.float32)  # three guard rows behind the result
    L.gemm_form_log()
    qbits.woq_linear(x, blob, torch.empty(0), out[:M], "bf16", "int4_clip", "fp16", asym)
    torch.cuda.synchronize()
    ring = L.GEMM_FORM_HANDSCHED | L.GEMM_FORM_RING
    raw = act_dtype == torch.float16
    assert L.gemm_form_log() == [ring | (L.GEMM_FORM_RAW if raw else L.GEMM_FORM_TALL if N == 22016 else 0)]
    assert not torch.isnan(out[:M]).any(), "output elements left unwritten"
    assert torch.isnan(out[M:]).all(), "rows past M were written"
    ref = orc.linear_rows(x.float().cpu().numpy(), blob.cpu().numpy().view(np.uint8))
    rel = (np.abs(out[:M].cpu().numpy() - ref).max(axis=1) / np.abs(ref).max(axis=1)).max()
    assert rel <= 2e-3, (M, group, asym, str(act_dtype), float(rel))


@pytest.mark.parametrize("M", [2048, 2148, 2213, 4096 + 129])
@pytest.mark.parametrize("group,asym", [(128, False), (32, True)])
@pytest.mark.parametrize("act_dtype", [torch.float32, torch.float16])
def test_prefill_gemm_256_row_tiles_ragged_rows_n22016_vs_oracle(M, group, asym, act_dtype):
    """The test above at the gate/up width N = 22016, where fp32 rows select the 256-row kernel at these row counts."""
    test_prefill_gemm_256_row_tiles_ragged_rows_vs_oracle(M, group, asym, act_dtype, N=22016)


@pytest.mark.parametrize("group,asym", [(128, False), (32, True)])
def test_prefill_gemm_qkv_at_32x2048_rows_vs_oracle(group, asym):
    """BASELINE configs[2]'s prompt pass feeds its GEMMs M = 32 x 2048 = 65 536 rows: the qkv projection at that M."""
    test_prefill_gemm_at_measured_size_vs_oracle("qkv", 4096, 12288, group, asym, torch.float32, M=65536)
