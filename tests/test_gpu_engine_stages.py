"""The engine's decode step and prompt pass, stage by stage (csrc/woq_engine.hip engine_step_impl / engine_prefill_impl).

Every kernel on the hot path has its own float64 test through a probe entry point, held to bounds around 1e-6 relative;
the engine that strings them together was held only to the whole-model oracle at 2e-3 (decode) and 1e-2 (prompt pass) of
max|logit|. A wiring slip of relative size 1e-4 — the wrong norm weight in an epilogue, sums of squares of the wrong
vector, another eps, a dropped bias, a wrong `seq_stride` or `start` — passes both. Here:

A. decode: one greedy step driven through `eng.phase` (residual stream and the step's K / V rows read after every phase,
   the same step through `eng.step()` from the same restored state must leave the same bytes) against the same step
   re-assembled from the probes on caller-owned buffers and a copy of the cache (tests/engine_stage_shadow.py): hidden and
   the appended K / V row after every phase, logits, token, position and log entry byte for byte; no other cache row
   changed on either side; `eng.status()` 0. Every case first asserts, through `eng.attn_plan()`, the attention form and
   slice merge it was written for.
B. prompt pass: `eng.prefill` against probe_gemm_f16 / probe_rope_append / probe_attn_prefill / probe_lm_head /
   probe_greedy_tail strung together: the final residual rows, every layer's cache over all positions and sequences
   (layer l's rows are functions of every layer below it), the last-position logits of every sequence, token and position
   byte for byte; only the rows [start, start + T) of the sequences in the call changed; the GEMM forms
   (`L.gemm_form_log()`) of the two passes equal. The prefill GEMM's plan reads only the shape, the row count, the
   activation type, its leading dimension and pointer alignment (plan_gemm_f16), not the workspace, so the probe chooses
   the engine's form at every shape here.
C. every probe output of the shadow chains against the float64 value of its own actual input, with the member kernel's
   existing reference module and tolerance terms (xq_reference.tolerance_terms / lm_head_tolerance_terms,
   gemv_f32_reference.terms, gemm_f16_reference.reference, attn_reference / qknorm_reference with the bounds at the top of
   test_gpu_attention_kernels.py / test_gpu_qknorm_kernels.py): the kernel tests feed N(0, 1) and special inputs, this
   holds the same bounds on attention outputs into o_proj, SiLU products into down_proj and post-residual hiddens.
D. the comparison can fail: the shadow perturbed in one wiring decision at a time differs from the healthy engine at the
   first stage the perturbation reaches and at no earlier one.

No stage needed a bound in place of bit equality: every decode and prompt-pass stage of every case below is byte-equal.

Section D, the norm weight after the last layer. The last layer's down_proj emits no XQ vector (engine_mlp_block_xq
passes none), and the next step's embedding kernel multiplies layer 0's ln1 in itself (engine_embed): a norm weight handed
to the last down_proj reaches no stage of this step or the next. The shadow models that (its riding norm weight starts
from the embedding's at every step), so that perturbation is run over two steps only to show that it stays invisible; the
reachable form of the same slip — layer 0's down_proj handed layer 0's own ln1 instead of layer 1's — must be caught at
layer 1's attention stage.

Worst err / bound per stage on an MI355X (printed by every test under -s; the bounds are not tightened to these):
  decode GEMVs, XQ step, hidden 256    qkv 0.288, o 0.250, gate_up 0.537, down 0.250  (0.250 = the kernel equals the
                                       reference's fp32 restatement bit for bit: |out - R1| = A of the allowed 4 A)
  decode GEMVs, XQ step, hidden 4096   qkv 0.250, o 0.250, gate_up 0.409, down 0.250  (all five wide cases)
  decode GEMVs, fp32-activation step   qkv 0.236, o 0.127, gate_up 0.158, down 0.079  (worst: fp8 weights; int4 / nf4 /
                                       act-order <= 0.046)
  decode attention                     per head, slices, fused launch 0.003; grouped matrix-core form (fp8 cache) 0.033
  lm_head                              0.250 (of 4 A, as above)
  prompt-pass GEMMs, hidden 256        qkv 0.251, o 0.228, gate_up 0.203, down 0.242
  prompt-pass GEMMs, hidden 4096       qkv 0.198, o 0.124, gate_up 0.154, down 0.134  (T 150)
  attn_prefill                         tiny 0.259, wide (T 150, 32 / 8 heads) 0.322
  RoPE / append, decode's K / V rows   every stored value within its kernel test's bound of the float64 row (asserted:
                                       the rounded rotation, one unit of storage only at a tie; with a q / k norm one
                                       unit of the rounded row, q within one fp16 ulp of the row's largest magnitude)
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import engine_stage_shadow as S
from tests.test_gpu_engine import _tiny

pytestmark = pytest.mark.gpu

G32A, G128, COL = (32, True, "fp32"), (128, False, "fp16"), (-1, False, "bf16")
PROMPT = [3, 17, 200, 5, 99, 42]
WORST = {}


def _note(case, ratios):
    for k, v in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("\n%s worst err/bound: %s" % (case, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (case, bad)


def _model(*quant, **kw):
    """-> (engine, the (q, scale, zp) the builder packed its blobs from, per layer)"""
    parts = []
    return _tiny(*quant, parts_out=parts, **kw)[0], parts


def _views(eng, parts):
    """per layer and projection: the float64 matrix and the restatement's view of the blob the engine was handed (parts:
    what the builder recorded, or views built from it earlier); the device blob must be the oracle's repack byte for byte"""
    out = []
    for l, info in enumerate(parts):
        vs = {}
        for proj in ("qkv", "o", "gate_up", "down"):
            vs[proj] = info[proj] if "raw" not in info else S.weight_view(info["raw"][proj], info)
            dev = eng.layer_tensors[l][proj].cpu().numpy().view(np.uint8)
            assert np.array_equal(dev, vs[proj]["blob"]), "layer %d %s: device repack != oracle repack" % (l, proj)
        out.append(vs)
    return out


def _assert_plan(eng, form, merge):
    p = eng.attn_plan()
    assert p["form"] == form and p["merge"] == merge and not p["refused"], p
    # the probe plans for itself from the same options: it must cut the context into the engine's slices
    c, o = eng.cfg, S.attn_options(eng)
    mine = L.probe_attn_decode_plan(c.heads, c.kv_heads, c.head_dim, c.kv_dtype, c.max_ctx, window=int(c.reserved[2]),
                                    splits=o["splits"], grouped=bool(o["grouped"]), chunk_fixed=o["chunk"], xq=False,
                                    granules=False)
    assert mine["slices"] == p["slices"] and mine["chunk_fixed"] == p["chunk_fixed"], (mine, p)
    if form != L.ATTN_GROUPED:
        assert mine["span"] == p["span"] and mine["spw"] == p["spw"], (mine, p)
    else:
        assert mine["form"] == L.ATTN_GROUPED, mine


def _start(eng, pos):
    """a cache with `pos` positions of content (one prompt pass), the next token and the position in place"""
    if pos == 0:
        eng.token.fill_(PROMPT[0])
        eng.pos.fill_(0)
    else:
        prompt = (PROMPT * (pos // len(PROMPT) + 1))[:pos] if pos > len(PROMPT) else PROMPT[:pos]
        eng.prefill(prompt, greedy=True)
        assert int(eng.pos.item()) == pos
    torch.cuda.synchronize()


def _poison_cache(eng, first):
    """rows `first` .. of every layer and sequence, K and V: finite garbage (bytes 0x3C: 1.06 in fp16, 0.0115 in bf16,
    1.5 in e4m3). A pass must not read them, and a row it appends then always changes — an engine shared between cases
    would otherwise find its own earlier bytes there"""
    for which in ("k", "v"):
        eng.kv_cache(which).view(torch.uint8)[:, :, first:] = 0x3C
    torch.cuda.synchronize()


def _decode_stage_ratios(w, views, record, fmt, grouped):
    cos, sin = w.cos.double().cpu().numpy(), w.sin.double().cpu().numpy()
    ratios = {}
    for r in record:
        if r["kind"] == "gemv":
            wv = views[r["layer"]][r["proj"]]
            if r["xq"]:
                v = S.xq_gemv_ratio(wv, r["x"], r["out"], r["g"], w.eps, r["bias"], r["residual"], r["epi"])
            else:
                v = S.f32_gemv_ratio(wv, r["x"], r["out"], r["form"], r["g"], w.eps, r["bias"], r["residual"], r["epi"],
                                     gu_tmp=True)
            key = r["proj"]
        elif r["kind"] == "attn":
            v, rows = S.decode_attention_ratio(r["qkv"], r["k"], r["v"], r["out"], r["pos"], w.NH, w.KV, w.D, cos, sin, fmt,
                                               w.window, r["q_w"], r["k_w"], w.qk_eps, grouped)
            assert rows, "layer %d: the appended K / V row is not the float64 row rounded to the cache type" % r["layer"]
            key = "attention"
        else:
            v = S.lm_head_ratio(r["hidden"], w.norm.cpu().numpy(), w.eps, w.lm, r["logits"])
            key = "lm_head"
        ratios[key] = max(ratios.get(key, 0.0), v)
    return ratios


def _check_decode(eng, parts, case, xq=True):
    """sections A and C for one assembled engine in its current state"""
    assert eng.uses_xq() == xq
    w = S.Wiring(eng)
    _poison_cache(eng, int(eng.pos.item()))  # the step's own row and every row it must not see
    snap = S.snapshot(eng)
    before = dict(k=S._raw(snap["k"]), v=S._raw(snap["v"]))
    pos0 = int(snap["pos"].item())
    own = [(0, l, pos0) for l in range(w.layers)]
    # engine: by phase, then the real step from the same state
    phases, after = S.engine_decode_trace(eng, by_phase=True)
    assert eng.status() == 0
    for which in ("k", "v"):
        assert S.changed_rows(before[which], after[which]) == own, (case, which, "engine rows changed")
    S.restore(eng, snap)
    whole, after2 = S.engine_decode_trace(eng, by_phase=False)
    assert eng.status() == 0
    assert S.first_difference(S.whole_step_view(phases), whole) is None, (case, "phases != step()")
    assert all(np.array_equal(after[x], after2[x]) for x in ("k", "v")), (case, "phases != step(): cache")
    S.restore(eng, snap)
    # shadow
    st = S.ShadowState(snap, eng.device)
    record = []
    shadow = S.shadow_decode_step(w, st, xq, S.attn_options(eng), handoff=xq, record=record)
    assert int(st.status.item()) == 0
    diff = S.first_difference(phases, shadow)
    assert diff is None, (case, "engine != shadow, first at", diff)
    for which, t in (("k", st.k), ("v", st.v)):
        assert S.changed_rows(before[which], S._raw(t)) == own, (case, which, "shadow rows changed")
        assert np.array_equal(S._raw(t), after[which]), (case, which, "caches differ")
    grouped = eng.attn_plan()["form"] == L.ATTN_GROUPED
    _note(case, _decode_stage_ratios(w, _views(eng, parts), record, S.KV_FMT[w.kv_code], grouped))


# ---- A + C: tiny geometry, XQ step -----------------------------------------------------------------------------------
# quantisation variants x positions, the attention variants spread over them: per head, three context slices + the
# combine launch, a sliding window shorter than the context
TINY_CASES = [
    ("g32a-fp32 pos 0 per head", G32A, 0, {}, L.ATTN_MERGE_NONE),
    ("g32a-fp32 pos 6 per head", G32A, 6, {}, L.ATTN_MERGE_NONE),
    ("g32a-fp32 pos 6 three slices", G32A, 6, dict(attn_splits=3), L.ATTN_MERGE_COMBINE),
    ("g128-fp16 pos 0 three slices", G128, 0, dict(attn_splits=3), L.ATTN_MERGE_COMBINE),
    ("g128-fp16 pos 6 per head", G128, 6, {}, L.ATTN_MERGE_NONE),
    ("g128-fp16 pos 6 window 4", G128, 6, dict(window=4), L.ATTN_MERGE_NONE),
    ("col-bf16 pos 0 per head", COL, 0, {}, L.ATTN_MERGE_NONE),
    ("col-bf16 pos 6 three slices", COL, 6, dict(attn_splits=3), L.ATTN_MERGE_COMBINE),
    ("col-bf16 pos 6 window 4 three slices", COL, 6, dict(window=4, attn_splits=3), L.ATTN_MERGE_COMBINE),
]


@pytest.mark.parametrize("case,quant,pos,kw,merge", TINY_CASES, ids=[c[0].replace(" ", "-") for c in TINY_CASES])
def test_decode_step_equals_probe_chain_tiny(case, quant, pos, kw, merge):
    eng, parts = _model(*quant, seed=11, **kw)
    _assert_plan(eng, L.ATTN_PER_HEAD, merge)  # hidden 256: two K tiles, below what the fused launch covers
    _start(eng, pos)
    _check_decode(eng, parts, "decode tiny " + case)


# ---- A + C: layer extras on the separate launches --------------------------------------------------------------------
def _with_extras(eng, kind, seed=5):
    g = torch.Generator().manual_seed(seed)
    c = eng.cfg
    for l in range(c.layers):
        if kind == "bias":
            eng.set_layer_extras(l, qkv_bias=0.5 * torch.randn((c.heads + 2 * c.kv_heads) * c.head_dim, generator=g))
        else:
            eng.set_layer_extras(l, q_norm=0.5 + torch.rand(c.head_dim, generator=g), k_norm=0.5 + torch.rand(c.head_dim, generator=g))


@pytest.mark.parametrize("kind", ["bias", "qknorm"])
@pytest.mark.parametrize("pos", [0, 6])
def test_decode_step_with_layer_extras_tiny(kind, pos):
    eng, parts = _model(*G128, seed=12)
    _with_extras(eng, kind)
    _assert_plan(eng, L.ATTN_PER_HEAD, L.ATTN_MERGE_NONE)
    _start(eng, pos)
    _check_decode(eng, parts, "decode tiny %s pos %d" % (kind, pos))


# ---- A + C: the fp32-activation step ---------------------------------------------------------------------------------
F32_CASES = {
    "int4 WOQ_ENGINE_XQ=0": dict(quant=G32A, env=True),
    "nf4": dict(quant=G128, weight_dtype="nf4", env=True),
    "fp8_e4m3 weights": dict(quant=G128, weight_dtype="fp8_e4m3"),
    "act-order": dict(quant=G128, act_order=True),
}


@pytest.mark.parametrize("name", list(F32_CASES))
def test_decode_step_equals_probe_chain_fp32_activations(name, monkeypatch):
    """the engines that hand fp32 between their kernels: the switch, a table type under the switch (nf4 blobs qualify
    for the XQ step), fp8-weight layers with their gate/up scratch, act-order blobs (which the XQ GEMV refuses)"""
    c = F32_CASES[name]
    if c.get("env"):
        monkeypatch.setenv("WOQ_ENGINE_XQ", "0")
    kw = {k: v for k, v in c.items() if k not in ("quant", "env")}
    eng, parts = _model(*c["quant"], seed=13, **kw)
    _assert_plan(eng, L.ATTN_PER_HEAD, L.ATTN_MERGE_NONE)
    _start(eng, 6)
    _check_decode(eng, parts, "decode fp32 step " + name, xq=False)


# ---- A + C: wide geometry ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    """hidden 4096 = 32 x 128 heads, 8 kv heads: one engine per cache type, built on first use and shared by the cases that
    only flip options (`get` puts every option a case could have left behind back first), freed with the module. The
    builder's seed fixes the weights, so the engines share one set of float64 views."""
    from tests.test_gpu_attention_fullgeom import build_attention_geometry

    engines, views = {}, []

    def get(kv_dtype, splits=1, grouped=False, extras=None):
        if kv_dtype not in engines:
            parts = []
            engines[kv_dtype] = build_attention_geometry(kv_heads=8, kv_dtype=kv_dtype, max_ctx=256, max_batch=1,
                                                         parts_out=parts)[0]
            if not views:
                views.extend(_views(engines[kv_dtype], parts))
        eng = engines[kv_dtype]
        eng.set_attn_splits(splits)
        eng.set_attn_grouped(grouped)
        eng.set_attn_chunk(0)
        eng.set_fuse_attn(True)
        for l in range(eng.cfg.layers):
            eng.set_layer_extras(l)
        if extras:
            _with_extras(eng, extras)
        return eng, views

    yield get
    engines.clear()
    views.clear()


WIDE_PROMPT = np.random.default_rng(41).integers(0, 512, 150)
WIDE_CASES = [
    ("fused fp16", torch.float16, dict(splits=1, grouped=False), L.ATTN_FUSED, L.ATTN_MERGE_NONE, None),
    ("fused four slices bf16", torch.bfloat16, dict(splits=4, grouped=False), L.ATTN_FUSED, L.ATTN_MERGE_A2A, None),
    ("grouped four slices fp8", torch.float8_e4m3fn, dict(splits=4, grouped=True), L.ATTN_GROUPED, L.ATTN_MERGE_A2A, None),
    ("fused fp16 qkv bias", torch.float16, dict(splits=1, grouped=False), L.ATTN_FUSED, L.ATTN_MERGE_NONE, "bias"),
    ("fused fp16 q/k norm", torch.float16, dict(splits=1, grouped=False), L.ATTN_FUSED, L.ATTN_MERGE_NONE, "qknorm"),
]


@pytest.mark.parametrize("case,kv_dtype,opt,form,merge,extras", WIDE_CASES, ids=[c[0].replace(" ", "-") for c in WIDE_CASES])
def test_decode_step_equals_probe_chain_wide(wide, case, kv_dtype, opt, form, merge, extras):
    """position 150 after one prompt pass; K = 4096 GEMVs, where the accumulation is 16 times as deep as at hidden 256"""
    eng, views = wide(kv_dtype, extras=extras, **opt)
    _assert_plan(eng, form, merge)
    eng.prefill(WIDE_PROMPT.tolist(), greedy=True)
    assert int(eng.pos.item()) == 150
    _check_decode(eng, views, "decode wide " + case)


# ---- B + C: the prompt pass ------------------------------------------------------------------------------------------
def _prefill_stage_ratios(w, views, record):
    like = dict(NH=w.NH, KV=w.KV, D=w.D, fmt=S.KV_FMT[w.kv_code], window=w.window, qk_eps=w.qk_eps,
                cos=w.cos.double().cpu().numpy(), sin=w.sin.double().cpu().numpy())
    ratios = {}
    for r in record:
        if r["kind"] == "gemm":
            v = S.gemm_ratio(views[r["layer"]][r["proj"]], r["x"], r["out"], r["g"], w.eps, r["bias"], r["residual"], r["epi"],
                             r["out_kind"])
            key = "gemm " + r["proj"]
        elif r["kind"] == "rope_attn":
            rows, v = S.rope_attn_ratio(r, like)
            assert rows, "layer %d: rotated q / appended K / V rows are not the float64 rows rounded to storage" % r["layer"]
            key = "attn_prefill"
        else:
            v = S.lm_head_ratio(r["hidden"], w.norm.cpu().numpy(), w.eps, w.lm, r["logits"])
            key = "lm_head"
        ratios[key] = max(ratios.get(key, 0.0), v)
    return ratios


def _check_prefill(eng, parts, case, tokens, start=0):
    w = S.Wiring(eng)
    tokens = np.asarray(tokens)
    tokens = tokens[None] if tokens.ndim == 1 else tokens
    n_seq, T = tokens.shape
    _poison_cache(eng, start)
    snap = S.snapshot(eng)
    before = dict(k=S._raw(snap["k"]), v=S._raw(snap["v"]))
    got, forms = S.engine_prefill_trace(eng, tokens, start)
    assert eng.status() == 0
    st = S.ShadowState(snap, eng.device)
    record = []
    want, forms2 = S.shadow_prefill(w, st, tokens, start, record=record)
    assert len(forms) == 4 * w.layers and forms == forms2, (case, "GEMM forms", forms, forms2)
    diff = S.first_difference(got, want)
    assert diff is None, (case, "engine != shadow, first at", diff)
    own = sorted((s, l, p) for s in range(n_seq) for l in range(w.layers) for p in range(start, start + T))
    for which in ("k", "v"):
        assert S.changed_rows(before[which], dict(got)["prefill"][which]) == own, (case, which, "rows changed")
    _note(case, _prefill_stage_ratios(w, _views(eng, parts), record))


PREFILL_TOKENS = np.random.default_rng(43).integers(0, 384, (2, 130))


@pytest.mark.parametrize("T", [1, 7, 40, 130])
def test_prompt_pass_equals_probe_chain_tiny(T):
    eng, parts = _model(*G128, seed=14, max_ctx=256)
    _check_prefill(eng, parts, "prompt pass tiny T %d" % T, PREFILL_TOKENS[0, :T])


def test_prompt_pass_second_chunk():
    """start_pos > 0 on top of a first chunk: `start` in rope_append, attn_prefill and the position the tail leaves"""
    eng, parts = _model(*G32A, seed=14, max_ctx=256)
    _check_prefill(eng, parts, "prompt pass chunk 0", PREFILL_TOKENS[0, :40])
    _check_prefill(eng, parts, "prompt pass chunk 1 (start 40)", PREFILL_TOKENS[0, 40:47], start=40)


def test_prompt_pass_two_sequences():
    """n_seq = 2 with max_batch = 2: `seq_stride`, and sequence 0 alone feeding the decode step's buffers"""
    eng, parts = _model(*G128, seed=14, max_ctx=64, max_batch=2)
    _check_prefill(eng, parts, "prompt pass 2 x 40", PREFILL_TOKENS[:, :40])
    # a one-sequence call leaves sequence 1's rows alone (asserted through `own` inside)
    _check_prefill(eng, parts, "prompt pass 1 x 7 beside a second sequence", PREFILL_TOKENS[1, :7], start=40)


@pytest.mark.parametrize("name,kw,extras", [("window 16", dict(window=16), None), ("fp8 cache", dict(kv_dtype=torch.float8_e4m3fn), None),
                                            ("bf16 cache col scales", dict(kv_dtype=torch.bfloat16), None),
                                            ("qkv bias", {}, "bias"), ("q/k norm", {}, "qknorm")])
def test_prompt_pass_variants(name, kw, extras):
    quant = COL if "col" in name else G128
    eng, parts = _model(*quant, seed=15, max_ctx=64, **kw)
    if extras:
        _with_extras(eng, extras)
    _check_prefill(eng, parts, "prompt pass " + name, PREFILL_TOKENS[0, :40])


def test_prompt_pass_equals_probe_chain_wide(wide):
    """T = 150 at 32 / 8 heads x 128: every GEMM at K = 4096 against float64 too"""
    eng, views = wide(torch.float16)
    _check_prefill(eng, views, "prompt pass wide T 150", WIDE_PROMPT)


# ---- D: the comparison can fail --------------------------------------------------------------------------------------
def test_perturbed_shadow_is_caught_at_its_first_stage():
    """Probes and a healthy engine only. The embedding table is scaled by 2^-9 so that eps (1e-5) is of the size of the
    first norm's mean square (4e-6): at mean squares near 1 an eps off by 2^-10 relative moves the sum by a sixth of an
    fp32 unit in the last place and is rounded away, which no comparison could see."""
    eng, _, _ = _tiny(*G128, seed=16)
    _with_extras(eng, "bias")
    ht = eng.head_tensors
    eng.set_head(ht["embed"] * 2.0 ** -9, ht["norm"], ht["lm_head"])
    _start(eng, 6)
    w = S.Wiring(eng)
    snap = S.snapshot(eng)
    phases, _ = S.engine_decode_trace(eng, by_phase=True)
    snap2 = S.snapshot(eng)
    phases2, _ = S.engine_decode_trace(eng, by_phase=True)  # the next step, for the perturbation that needs two
    assert eng.status() == 0
    attn = S.attn_options(eng)

    def run(wp, steps=1, touch=None):
        st = S.ShadowState(snap, eng.device)
        if touch:
            touch(st)
        out = [S.first_difference(phases, S.shadow_decode_step(wp, st, True, attn))]
        if steps == 2:
            assert S.first_difference([("state", dict(token=S._raw(snap2["token"]), pos=S._raw(snap2["pos"])))],
                                      [("state", dict(token=S._raw(st.token), pos=S._raw(st.pos)))]) is None
            out.append(S.first_difference(phases2, S.shadow_decode_step(wp, st, True, attn)))
        return out

    assert run(w, 2) == [None, None]  # the healthy shadow, both steps
    p = w.copy()
    p.after_mlp[0] = w.lt[1]["ln2"]  # ln2 in place of ln1 on layer 1's qkv GEMV
    assert run(p)[0][0] == "L1.attn"
    p = w.copy()
    p.eps = w.eps * (1 + 2.0 ** -10)
    assert float(np.float32(p.eps)) != float(np.float32(w.eps)) and run(p)[0][0] == "L0.attn"
    p = w.copy()
    p.after_mlp[1] = w.lt[0]["ln1"]  # a hand-off after the last layer: dead (module docstring)
    assert run(p, 2) == [None, None]
    p = w.copy()
    p.after_mlp[0] = w.lt[0]["ln1"]  # the reachable form: layer 0's down_proj carries layer 0's ln1
    assert run(p)[0][0] == "L1.attn"
    p = w.copy()
    p.lt[1]["qkv_bias"] = None  # layer 1's qkv bias dropped
    assert run(p)[0][0] == "L1.attn"

    def one_ulp(st):  # layer 0's K row pos - 1, first element, one unit in the last place
        row = st.k[0, 0, 5].view(torch.int16)
        row[0, 0] += 1

    d = run(w, touch=one_ulp)[0]
    assert d == ("L0.attn", "hidden"), d  # the appended rows are still equal: only what attended over the row moved


# ---- E: a mis-assembled engine is an error, not a launch -------------------------------------------------------------
def _bare(like, layers_from=(), extras_from=None):
    """an engine of `like`'s shape with its head set and the listed (layer index, source engine) layers"""
    from intel_extension_for_transformers_amd.runtime import WoqDecoderEngine

    c = like.cfg
    eng = WoqDecoderEngine(c.hidden, c.inter, c.heads, c.kv_heads, c.head_dim, c.layers, c.vocab, max_ctx=c.max_ctx,
                           rms_eps=c.rms_eps, rope_theta=c.rope_theta)
    ht = like.head_tensors
    eng.set_head(ht["embed"], ht["norm"], ht["lm_head"])
    for l, src in layers_from:
        t = src.layer_tensors[l]
        eng.set_layer(l, t["qkv"], t["o"], t["gate_up"], t["down"], t["ln1"], t["ln2"])
    return eng


def _layer_args(src, l):
    t = src.layer_tensors[l]
    return (t["qkv"], t["o"], t["gate_up"], t["down"], t["ln1"], t["ln2"])


def test_set_layer_refuses_mixed_kinds_in_either_order():
    """set-up calls only: nothing is launched on these engines"""
    ints, _, _ = _tiny(*G128, seed=17)
    fp8s, _, _ = _tiny(*G128, seed=17, weight_dtype="fp8_e4m3")
    eng = _bare(ints, [(0, ints)])
    with pytest.raises(RuntimeError, match="^QBits: fp8 and integer layers cannot be mixed"):
        eng.set_layer(1, *_layer_args(fp8s, 1))  # integer, then fp8: was accepted
    eng = _bare(ints, [(0, fp8s)])
    with pytest.raises(RuntimeError, match="^QBits: fp8 and integer layers cannot be mixed"):
        eng.set_layer(1, *_layer_args(ints, 1))
    # the refused engine takes the layer of its own kind afterwards, and a layer may be set again
    eng.set_layer(1, *_layer_args(fp8s, 1))
    eng.set_layer(0, *_layer_args(fp8s, 0))


def test_refused_set_layer_leaves_the_engine_as_it_was():
    """a call refused for the kind of its blobs and one refused for a shape, on a complete engine: it then steps bit for
    bit like an engine that never saw them (the layer used to be overwritten before the checks)"""
    a, _, _ = _tiny(*G128, seed=18)
    b, _, _ = _tiny(*G128, seed=18)
    fp8s, _, _ = _tiny(*G128, seed=18, weight_dtype="fp8_e4m3")
    with pytest.raises(RuntimeError, match="^QBits: fp8 and integer layers cannot be mixed"):
        a.set_layer(1, *_layer_args(fp8s, 1))
    t = a.layer_tensors[0]
    with pytest.raises(RuntimeError, match="^QBits: o_proj blob shape mismatch"):
        a.set_layer(0, t["qkv"], t["gate_up"], t["gate_up"], t["down"], t["ln2"], t["ln1"])
    assert a.uses_xq() and b.uses_xq()
    for eng in (a, b):
        eng.prefill(PROMPT, greedy=True)
        for _ in range(3):
            eng.step(greedy=True)
    torch.cuda.synchronize()
    assert a.status() == 0 and b.status() == 0
    assert S.first_difference([("end", dict(logits=S._raw(a.logits), token=S._raw(a.token), hidden=S._raw(a.hidden),
                                            k=S._raw(a.kv_cache("k")), v=S._raw(a.kv_cache("v"))))],
                              [("end", dict(logits=S._raw(b.logits), token=S._raw(b.token), hidden=S._raw(b.hidden),
                                            k=S._raw(b.kv_cache("k")), v=S._raw(b.kv_cache("v"))))]) is None


def test_engine_with_an_unset_layer_refuses_every_launching_call():
    """engine_layers_problem is asked in woq_engine_step / _steps / _phase / _capture / _prefill / _prefill_scored before
    the first launch of each (and in the timing hooks): an unset layer holds null blobs"""
    full, _, _ = _tiny(*G128, seed=19)
    eng = _bare(full, [(0, full)])  # layer 1 never set
    eng.set_logprobs(True)  # (allocates the logs: prefill_scored asks for them before it asks for the layers)
    eng.set_logprobs(False)
    unset = "^QBits: engine layer not set"
    for call in (lambda: eng.step(greedy=True), lambda: eng.run(2, greedy=True), lambda: eng.phase(0, 0),
                 lambda: eng.phase(0, 2), lambda: eng.capture(greedy=True), lambda: eng.prefill(PROMPT),
                 lambda: eng.prefill_scored(PROMPT, PROMPT), lambda: eng.time_gemv(reps=1)):
        with pytest.raises(RuntimeError, match=unset):
            call()
    torch.cuda.synchronize()
    assert eng.status() == 0
    # once the layer is there the same engine steps like the complete one
    eng.set_layer(1, *_layer_args(full, 1))
    for e in (eng, full):
        e.prefill(PROMPT, greedy=True)
        e.step(greedy=True)
    assert np.array_equal(S._raw(eng.logits), S._raw(full.logits)) and int(eng.token.item()) == int(full.token.item())


def test_report_worst_ratios():
    """under -s: the table of the module docstring"""
    print("\nworst err/bound per stage over this run: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
