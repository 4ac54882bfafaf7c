"""The engine's decode step and prompt pass re-assembled from the single-kernel probes of include/woq_hip_experimental.h
(the "shadow"), for tests/test_gpu_engine_stages.py, and the float64 value of every shadow stage on the data the model
really produces there.

What the shadow is: the same launches the engine issues (csrc/woq_engine.hip engine_step_impl / engine_prefill_impl), each
through its probe on caller-owned buffers and a copy of the KV cache, strung together here in Python. Which norm weight
multiplies which activation, which eps, which bias, which cache row, `seq_stride` and `start` are decided in this file,
independently of woq_engine.hip; the kernels are the library's own. The engine's pass and the shadow's are compared byte
for byte, stage by stage (`first_difference`).

The XQ hand-off. In the engine's XQ step the producer of an activation multiplies the NEXT consumer's norm weight in and
emits the product as an XQ vector with the sums of squares of the un-multiplied value: the embedding carries layer 0's
ln1, o_proj carries ln2, down_proj carries the next layer's ln1 and nothing after the last layer. `woq_probe_gemv_xq` takes
fp32 and converts it itself (times `in_norm_w`), through the same device function as the producers' epilogues. The shadow
therefore keeps "the norm weight that rides with the residual stream" as state (`Wiring.after_embed / after_attn /
after_mlp`), set where the engine's producer sets it and read where the engine's consumer reads it; with `handoff=True` it
also lets the producing probe emit its XQ vector and requires it to equal `woq_probe_xq_from_f32` of the same fp32 values,
byte for byte, sums of squares included.

Plain arithmetic of this file's own (`decode_attention_f64`, `changed_rows`, `first_difference`, `weight_view`,
`stored_ok`) has tests/test_engine_stage_shadow_cpu.py; everything else calls the existing reference modules.
"""
import numpy as np

from oracle import woq_oracle as orc
from tests import attn_reference as R
from tests import gemm_f16_reference as GM
from tests import gemv_f32_reference as G
from tests import qknorm_reference as QN
from tests import xq_reference as X

F32 = np.float32
STYPE = {"fp32": orc.F32, "fp16": orc.F16, "bf16": orc.BF16}
TABLES = {"nf4": orc.W_NF4, "fp4_e2m1": orc.W_FP4_E2M1, "fp4_e2m1_bnb": orc.W_FP4_E2M1_BNB}
KV_FMT = {2: "fp16", 1: "bf16", 3: "fp8"}  # _lib.F16 / BF16 / FP8_E4M3 -> attn_reference.FORMATS


# ---- plain helpers (numpy only) --------------------------------------------------------------------------------------
def first_difference(a, b):
    """a, b: traces = lists of (stage name, {field: numpy array}) -> (stage, field) of the first field whose BYTES differ,
    ("<shape>", ...) if the traces do not line up, None when they are equal"""
    if [n for n, _ in a] != [n for n, _ in b]:
        return ("<shape>", "stages %s vs %s" % ([n for n, _ in a], [n for n, _ in b]))
    for (name, fa), (_, fb) in zip(a, b):
        if sorted(fa) != sorted(fb):
            return ("<shape>", "%s: fields %s vs %s" % (name, sorted(fa), sorted(fb)))
        for key in fa:
            x, y = np.ascontiguousarray(fa[key]), np.ascontiguousarray(fb[key])
            if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
                return (name, key)
    return None


def changed_rows(before, after):
    """caches [..., max_ctx, kv_heads, head_dim] as raw integer arrays -> sorted list of the index tuples (all axes but
    the last two) of the rows whose bytes differ"""
    b, a = np.asarray(before), np.asarray(after)
    assert b.shape == a.shape and b.dtype == a.dtype
    diff = (b != a).reshape(b.shape[:-2] + (-1,)).any(axis=-1)
    return sorted(tuple(int(i) for i in idx) for idx in np.argwhere(diff))


def stored_ok(got, lo, hi):
    """every stored value lies between the two roundings `attn_reference.stored_bounds` allows"""
    return bool(((got >= lo) & (got <= hi)).all())


def decode_attention_f64(qkv, K, V, pos, heads, kv_heads, HD, cos, sin, window=0, q_w=None, k_w=None, eps=0.0):
    """One decode step's attention in float64. qkv fp32 [(heads + 2 kv) * HD] un-rotated; K, V [pos + 1, kv, HD] = the
    cache AS STORED after the step (row pos = the appended one); cos / sin [positions, HD / 2]; q_w / k_w: the per-head
    RMSNorm weights in front of the rotation (Qwen3) or None. -> (out [heads, HD], the new k normalised and rotated but
    unrounded [kv, HD], the bound of the fp32 rotation's error on it, the new v unrounded [kv, HD])"""
    rep = heads // kv_heads
    x = np.asarray(qkv, F32).astype(np.float64)
    q = x[:heads * HD].reshape(heads, HD)
    k = x[heads * HD:(heads + kv_heads) * HD].reshape(kv_heads, HD)
    v = x[(heads + kv_heads) * HD:].reshape(kv_heads, HD)
    if q_w is not None:
        q, k = QN.qk_norm(q, q_w, eps), QN.qk_norm(k, k_w, eps)
    c, s = cos[pos], sin[pos]
    qr, kr = R.rotate(q, c, s), R.rotate(k, c, s)
    out = np.concatenate([R.attend(qr[h][None], K[:, h // rep], V[:, h // rep], [pos], window)[0] for h in range(heads)])
    return out, kr, R.rotate_error(k, c, s), v


def weight_view(raw, info):
    """raw = (q [K, N], scales, zp | None, g_idx | None) and info = dict(cpu_pack, group, asym, scale_dtype, weight_dtype,
    compute_dtype) as tests/test_gpu_engine.py `_tiny` records them -> dict(blob (the oracle's repack), W64 (its
    dequantisation, [K, N] float64), codes, scales_kn, zp_kn (the XQ restatement's view, checked to dequantise to W64),
    smode, ndig, table, shuffle (activation index per weight row | None), K, N, form, wname, cname)"""
    q, s, z, gi = raw
    group, sname, wname, cname = info["group"], info["scale_dtype"], info["weight_dtype"], info["compute_dtype"]
    blob = info["cpu_pack"](q, s, z, gi)
    h = orc.header(blob)
    K, N = q.shape
    g = K if group in (-1, 0) or group > K else group
    W = orc.dequantize_blob(blob)
    out = dict(blob=blob, W64=W.astype(np.float64), K=K, N=N, smode=h["scale_mode"], form=(group, bool(info["asym"]), sname),
               wname=wname, cname=cname, ndig=0, table=None, codes=None, scales_kn=None, zp_kn=None,
               shuffle=None if gi is None else orc.convert_idx(gi, K, g))
    if wname in TABLES:
        out["ndig"] = 1 if wname == "fp4_e2m1" else (3 if (wname == "nf4" and cname == "fp32") else 2)
        out["table"] = X.table_planes(TABLES[wname], out["ndig"])
    if wname in TABLES or wname == "int4_clip":
        if sname == "fp16":
            st = s.astype(np.float16).astype(F32)
        else:
            st = orc.bf16_round(s) if sname == "bf16" else s
        rep = lambda a: np.repeat(a, g, axis=0)[:K]  # noqa: E731
        out["codes"], out["scales_kn"] = q.astype(np.int64), rep(st)
        out["zp_kn"] = rep(z).astype(np.int64) if z is not None else None
        if gi is None:  # (an act-order blob stores its rows permuted: only the fp32-activation step takes it)
            if wname == "int4_clip":
                mine = ((out["codes"] - (0 if z is None else out["zp_kn"])) * out["scales_kn"].astype(np.float64)).astype(F32)
            else:
                mine = (orc.LUTS[TABLES[wname]][q] * out["scales_kn"]).astype(F32)
            assert np.array_equal(mine, W), "the restatement's view of the blob does not dequantise to the oracle's matrix"
    return out


# ---- float64 of one shadow stage, with the member kernel's own bound ------------------------------------------------
def xq_gemv_ratio(wv, x, out, g=None, eps=0.0, bias=None, residual=None, epi=0):
    """the XQ GEMV's output against tests/xq_reference.py: -> worst |out - R0| / (4 (A + B)) (and asserts nothing)"""
    launches = X.geometry(wv["K"], epi, wv["smode"], wv["ndig"])
    assert launches, "K not covered by the XQ GEMV"
    restate = lambda y32, inv32: X.gemv_f32(y32, wv["codes"], wv["scales_kn"], wv["zp_kn"], launches, wv["smode"],  # noqa: E731
                                            inv32, bias, residual, epi, wv["table"])
    r0, r1, a, b = X.tolerance_terms(x, g, eps, wv["W64"], restate, bias, residual, epi)
    o = np.asarray(out, F32).astype(np.float64)
    return max(float(np.abs(o - r0).max()) / (4 * (a + b)), float(np.abs(o - r1).max()) / (4 * a))


def f32_gemv_ratio(wv, x, out, form_got, g=None, eps=0.0, bias=None, residual=None, epi=0, gu_tmp=False):
    """the fp32-activation GEMV's output against tests/gemv_f32_reference.py `terms`; also requires the kernel the probe
    reports to be the one the reference's dispatch restatement predicts (its bound is per kernel)"""
    assert float(eps) == float(F32(G.EPS)) or g is None, "gemv_f32_reference.terms is written for eps = 1e-5"
    c = G.case("stage", wv["K"], None, form=wv["form"], wname=wv["wname"], cname=wv["cname"], epi=epi, norm=g is not None,
               residual="separate" if residual is not None else "none", bias=bias is not None, shuffle=wv["shuffle"] is not None,
               gu_tmp=gu_tmp, N=wv["N"] // 2 if epi == 1 else wv["N"])
    d = dict(x=np.asarray(x, F32)[None], g=g, bias=bias, residual=None if residual is None else np.asarray(residual, F32)[None],
             W64=wv["W64"], shuffle=wv["shuffle"], ndig=wv["ndig"])
    t = G.terms(c, d)
    assert tuple(form_got) == tuple(t["form"]), ("kernel form", tuple(form_got), tuple(t["form"]))
    err = np.abs(np.asarray(out, F32).astype(np.float64)[None] - t["r0"])
    return float((err / t["tol"]).max())


def gemm_ratio(wv, x, out, g=None, eps=0.0, bias=None, residual=None, epi=0, out_kind="fp16"):
    """one prompt-pass GEMM against tests/gemm_f16_reference.py `reference` and its band; x [M, K] as the kernel receives it"""
    t = GM.reference(np.asarray(x, F32), wv["W64"], wv["shuffle"], g, eps, bias, residual, epi, out_kind)
    err = np.abs(np.asarray(out).astype(np.float64) - t["exp"])
    return float((err / t["tol"]).max())


def lm_head_ratio(hidden, norm_w, eps, W, logits):
    a = X.lm_head_tolerance_terms(hidden, norm_w, eps, W)
    ref = X.lm_head_f64(hidden, norm_w, eps, W)
    return float(np.abs(np.asarray(logits, F32).astype(np.float64) - ref).max()) / (4 * a)


def decode_attention_ratio(qkv, k_rows, v_rows, out, pos, heads, kv_heads, HD, cos, sin, fmt, window=0, q_w=None, k_w=None,
                           eps=0.0, grouped=False):
    """k_rows / v_rows [pos + 1, kv, HD] float64 = the cache as stored after the step. -> (worst err / bound of the output,
    True when the appended k / v rows are the float64 values rounded to `fmt`). Bounds: tests/test_gpu_attention_kernels.py
    (fp32 kernel 1e-4 max|ref| + 1e-6; grouped matrix-core form 2^-10 max visible |v| + 2^-11 |ref| + 1e-6) and, with a
    q / k norm, tests/test_gpu_qknorm_kernels.py's stored-row bound: the float64 normalised, rotated k rounded to the cache
    type, within one unit of the cache type's last place"""
    ref, kr, kerr, v = decode_attention_f64(qkv, k_rows, v_rows, pos, heads, kv_heads, HD, cos, sin, window, q_w, k_w, eps)
    got = np.asarray(out, F32).astype(np.float64).reshape(heads, HD)
    ref = ref.reshape(heads, HD)
    if grouped:
        rep = heads // kv_heads
        lo = max(0, pos + 1 - window) if window > 0 else 0
        vmax = np.array([np.abs(v_rows[lo:pos + 1, h // rep]).max() for h in range(heads)])
        bound = 2.0 ** -10 * vmax[:, None] + 2.0 ** -11 * np.abs(ref) + 1e-6
    else:
        bound = 1e-4 * np.abs(ref).max() + 1e-6
    ratio = float((np.abs(got - ref) / bound).max())
    if q_w is None:
        rows = stored_ok(k_rows[pos], *R.stored_bounds(kr, kerr, fmt)) and np.array_equal(v_rows[pos], R.round_to(v, fmt))
    else:
        want_k = R.round_to(kr, fmt)
        rows = bool((np.abs(k_rows[pos] - want_k) <= QN.ulp(want_k, fmt)).all()) and \
            np.array_equal(v_rows[pos], R.round_to(v, fmt))
    return ratio, rows


# ---- the model as the shadow sees it ---------------------------------------------------------------------------------
class Wiring:
    """Everything the shadow strings the probes together with, read off an assembled engine once: shapes, the device
    blobs and norm weights the engine was handed (`eng.layer_tensors` / `eng.head_tensors`), RoPE tables built by the
    same function, and which norm weight rides into which producer's epilogue. A perturbed shadow (section D of the test
    file) is a `copy()` with one entry changed."""

    def __init__(self, eng):
        from intel_extension_for_transformers_amd.runtime.engine import build_rope_tables

        c = eng.cfg
        self.H, self.I, self.NH, self.KV, self.D = c.hidden, c.inter, c.heads, c.kv_heads, c.head_dim
        self.layers, self.vocab, self.max_ctx, self.eps = c.layers, c.vocab, c.max_ctx, float(c.rms_eps)
        self.qk_eps = self.eps
        self.window, self.kv_code, self.max_batch = int(c.reserved[2]), int(c.kv_dtype), eng.max_batch
        self.lt = [dict(eng.layer_tensors[l]) for l in range(self.layers)]
        self.embed, self.norm, self.lm = (eng.head_tensors[k] for k in ("embed", "norm", "lm_head"))
        self.cos, self.sin = build_rope_tables(c.max_ctx, c.head_dim, c.rope_theta, eng.device)
        # the norm weight multiplied into the residual stream by its producer, for the next consumer
        self.after_embed = self.lt[0]["ln1"]
        self.after_attn = [t["ln2"] for t in self.lt]
        self.after_mlp = [self.lt[l + 1]["ln1"] if l + 1 < self.layers else None for l in range(self.layers)]
        self.seq_stride = self.layers * self.max_ctx * self.KV * self.D  # cache elements between sequences

    def copy(self):
        import copy

        w = copy.copy(self)
        w.lt = [dict(t) for t in self.lt]
        w.after_attn, w.after_mlp = list(self.after_attn), list(self.after_mlp)
        return w

    def extra(self, l, name):
        return self.lt[l].get(name)


def attn_options(eng):
    """the decode attention options the engine was left with (what its own plan starts from)"""
    from intel_extension_for_transformers_amd import _lib as L

    lib = L.lib()
    return dict(splits=int(lib.woq_engine_attn_splits(eng._h)), grouped=int(lib.woq_engine_attn_grouped(eng._h)),
                chunk=int(lib.woq_engine_attn_chunk(eng._h)))


def _raw(t):
    """a device tensor's bytes as a numpy integer array of its element size"""
    import torch

    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).cpu().numpy()


def snapshot(eng):
    return dict(k=eng.kv_cache("k").clone(), v=eng.kv_cache("v").clone(), token=eng.token.clone(), pos=eng.pos.clone(),
                log=eng.token_log().clone())


def restore(eng, s):
    import torch

    for which in ("k", "v"):
        eng.kv_cache(which).view(torch.uint8).copy_(s[which].view(torch.uint8))
    eng.token.copy_(s["token"])
    eng.pos.copy_(s["pos"])
    eng.token_log().copy_(s["log"])
    torch.cuda.synchronize()


def _stage_names(layers):
    return [n for l in range(layers) for n in ("L%d.attn" % l, "L%d.mlp" % l)] + ["head"]


def engine_decode_trace(eng, by_phase=True):
    """One greedy decode step of the engine from its current state. by_phase: through woq_engine_phase, reading the
    residual stream and the step's K / V rows after every phase; otherwise `step()`, whose trace holds only what a whole
    step leaves (the last residual stream, every layer's K / V row at the step's position, logits, token, position, log
    entry). -> (trace, caches after the step as raw arrays)"""
    import torch

    c = eng.cfg
    pos0 = int(eng.pos.item())
    row = lambda which, l: _raw(eng.kv_cache(which)[0, l, pos0])  # noqa: E731
    tr = []
    if by_phase:
        for l in range(c.layers):
            eng.phase(l, 0, greedy=True)
            tr.append(("L%d.attn" % l, dict(hidden=_raw(eng.hidden), k=row("k", l), v=row("v", l))))
            eng.phase(l, 1, greedy=True)
            tr.append(("L%d.mlp" % l, dict(hidden=_raw(eng.hidden))))
        eng.phase(0, 2, greedy=True)
    else:
        eng.step(greedy=True)
    torch.cuda.synchronize()
    head = dict(logits=_raw(eng.logits), token=_raw(eng.token), pos=_raw(eng.pos), log=_raw(eng.token_log()[pos0:pos0 + 1]))
    if not by_phase:
        head.update(hidden=_raw(eng.hidden), k=np.stack([row("k", l) for l in range(c.layers)]),
                    v=np.stack([row("v", l) for l in range(c.layers)]))
    tr.append(("head", head))
    return tr, dict(k=_raw(eng.kv_cache("k")), v=_raw(eng.kv_cache("v")))


def whole_step_view(trace):
    """what `engine_decode_trace(by_phase=False)` holds, taken from a by-phase trace"""
    d = dict(trace)
    layers = (len(trace) - 1) // 2
    head = dict(d["head"])
    head.update(hidden=d["L%d.mlp" % (layers - 1)]["hidden"], k=np.stack([d["L%d.attn" % l]["k"] for l in range(layers)]),
                v=np.stack([d["L%d.attn" % l]["v"] for l in range(layers)]))
    return [("head", head)]


class ShadowState:
    """the shadow's own token, position, token log, status word and KV cache copy (sequence-major like the engine's)"""

    def __init__(self, snap, dev):
        import torch

        self.k, self.v = snap["k"].clone(), snap["v"].clone()
        self.token, self.pos, self.log = snap["token"].clone(), snap["pos"].clone(), snap["log"].clone()
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)


def shadow_decode_step(w, st, xq, attn, handoff=False, record=None):
    """One greedy decode step re-assembled from the probes over `st` (a ShadowState). xq: the XQ step's GEMVs
    (woq_probe_gemv_xq) or the fp32-activation step's (woq_probe_gemv_f32); attn: `attn_options` of the engine.
    record: a list that receives one dict per probe call (kind, layer, numpy inputs and outputs) for the float64 checks.
    -> trace"""
    import torch

    from intel_extension_for_transformers_amd import _lib as L

    dev = st.token.device
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)  # noqa: E731
    pos0 = int(st.pos.item())
    NQ = (w.NH + 2 * w.KV) * w.D
    np_ = lambda t: None if t is None else t.detach().float().cpu().numpy()  # noqa: E731
    gu_tmp = f32(2 * w.I)

    def xo_buffers(n):
        return (torch.zeros(L.xq_limb_bytes(n), dtype=torch.uint8, device=dev), f32(n // 16), f32(n // 16))

    def gemv(kind, l, x, blob, n_out, norm_w=None, bias=None, residual=None, epi=0, next_norm=None, emit=False):
        out = f32(n_out)
        form = None
        if xq:
            xo = ssq = None
            if emit:
                xo, ssq = xo_buffers(n_out), f32(n_out // 16)
            L.probe_gemv_xq(x, blob, epi, norm_w, w.eps if norm_w is not None else 0.0, bias, residual,
                            next_norm if emit else None, out, xo, ssq)
            if emit:  # the producer's XQ vector is the conversion of the very fp32 values it stored
                xo2, ssq2 = xo_buffers(n_out), f32(n_out // 16)
                L.probe_xq_from_f32(out, next_norm, *xo2, ssq2)
                nb = n_out // 16
                same = (torch.equal(xo[0][:nb * 48], xo2[0][:nb * 48]) and torch.equal(xo[1].view(torch.int32), xo2[1].view(torch.int32))
                        and torch.equal(xo[2].view(torch.int32), xo2[2].view(torch.int32))
                        and torch.equal(ssq.view(torch.int32), ssq2.view(torch.int32)))
                assert same, "layer %d %s: the epilogue's XQ vector differs from xq_from_f32 of its own fp32 output" % (l, kind)
        else:
            form = L.probe_gemv_f32(x, blob, out, norm_w=norm_w, eps=w.eps if norm_w is not None else 0.0, epi=epi, bias=bias,
                                    residual=residual, gu_tmp=gu_tmp)
        if record is not None:
            record.append(dict(kind="gemv", proj=kind, layer=l, x=np_(x), g=np_(norm_w), bias=np_(bias), residual=np_(residual),
                               epi=epi, out=np_(out), form=form, xq=xq))
        return out

    h = f32(w.H)
    L.probe_embed(w.embed, st.token, h, pos=st.pos, max_ctx=w.max_ctx, status=st.status)
    if handoff and xq:  # the embedding's own XQ vector against the conversion of the row it stored
        xo, ssq, h2 = xo_buffers(w.H), f32(w.H // 16), f32(w.H)
        L.probe_embed(w.embed, st.token, h2, norm_w=w.after_embed, xo=xo, ssq_out=ssq, pos=st.pos, max_ctx=w.max_ctx, status=st.status)
        xo2, ssq2 = xo_buffers(w.H), f32(w.H // 16)
        L.probe_xq_from_f32(h, w.after_embed, *xo2, ssq2)
        nb = w.H // 16
        assert torch.equal(h.view(torch.int32), h2.view(torch.int32)) and torch.equal(xo[0][:nb * 48], xo2[0][:nb * 48]) and \
            torch.equal(xo[1].view(torch.int32), xo2[1].view(torch.int32)) and torch.equal(ssq.view(torch.int32), ssq2.view(torch.int32)), \
            "the embedding's XQ vector differs from xq_from_f32 of its own row"
    riding = w.after_embed  # the norm weight the producer multiplied in for the next consumer
    tr = []
    for l in range(w.layers):
        t = w.lt[l]
        kc, vc = st.k[0, l], st.v[0, l]
        qkv = gemv("qkv", l, h, t["qkv"], NQ, norm_w=riding, bias=w.extra(l, "qkv_bias"))
        a = f32(w.NH * w.D)
        q_n, k_n = w.extra(l, "q_norm"), w.extra(l, "k_norm")
        if q_n is not None:
            L.probe_attn_decode_qknorm(qkv, kc, vc, w.kv_code, st.pos, w.cos, w.sin, w.NH, w.KV, w.D, w.max_ctx, w.window,
                                       attn["splits"], 0, q_n, k_n, w.qk_eps, a)
        else:
            L.probe_attn_decode(qkv, kc, vc, w.kv_code, st.pos, w.cos, w.sin, w.NH, w.KV, w.D, w.max_ctx, w.window,
                                attn["splits"], attn["grouped"], 0, attn["chunk"], a)
        if record is not None:
            record.append(dict(kind="attn", layer=l, qkv=np_(qkv), k=np_(kc[:pos0 + 1]).astype(np.float64),
                               v=np_(vc[:pos0 + 1]).astype(np.float64), out=np_(a), pos=pos0, q_w=np_(q_n), k_w=np_(k_n)))
        riding = w.after_attn[l]
        h = gemv("o", l, a, t["o"], w.H, residual=h, next_norm=riding, emit=handoff)
        tr.append(("L%d.attn" % l, dict(hidden=_raw(h), k=_raw(kc[pos0]), v=_raw(vc[pos0]))))
        act = gemv("gate_up", l, h, t["gate_up"], w.I, norm_w=riding, epi=1, emit=handoff)
        riding = w.after_mlp[l]
        h = gemv("down", l, act, t["down"], w.H, residual=h, next_norm=riding, emit=handoff and riding is not None)
        tr.append(("L%d.mlp" % l, dict(hidden=_raw(h))))
    logits = f32(w.vocab)
    npairs = (w.vocab + 15) // 16
    pmax, pidx = f32(npairs), torch.empty(npairs, dtype=torch.int32, device=dev)
    L.probe_lm_head(h, w.norm, w.eps, w.lm, logits, pmax, pidx)
    if record is not None:
        record.append(dict(kind="lm_head", hidden=np_(h), logits=np_(logits)))
    L.probe_greedy_tail(1, w.vocab, st.token, st.pos, pmax=pmax, pidx=pidx, log=st.log, status=st.status)
    torch.cuda.synchronize()
    tr.append(("head", dict(logits=_raw(logits), token=_raw(st.token), pos=_raw(st.pos), log=_raw(st.log[pos0:pos0 + 1]))))
    return tr


# ---- prompt pass -----------------------------------------------------------------------------------------------------
def engine_prefill_trace(eng, tokens, start):
    """`eng.prefill(tokens, start_pos=start, greedy=True)` -> (trace with one stage, GEMM forms the pass logged)"""
    import torch

    from intel_extension_for_transformers_amd import _lib as L

    t = torch.as_tensor(np.asarray(tokens), dtype=torch.int32)
    t = t[None] if t.dim() == 1 else t
    n_seq, T = t.shape
    L.gemm_form_log()
    lg = eng.prefill(t, start_pos=start, greedy=True)
    torch.cuda.synchronize()
    forms = L.gemm_form_log()
    tr = [("prefill", dict(rows=_raw(eng.prefill_rows(n_seq * T)), logits=_raw(lg), token=_raw(eng.token), pos=_raw(eng.pos),
                           k=_raw(eng.kv_cache("k")), v=_raw(eng.kv_cache("v"))))]
    return tr, forms


def shadow_prefill(w, st, tokens, start, record=None):
    """The prompt pass re-assembled from the probes over `st`'s cache copy. -> (trace, GEMM forms logged)"""
    import torch

    from intel_extension_for_transformers_amd import _lib as L

    dev = st.token.device
    t = torch.as_tensor(np.asarray(tokens), dtype=torch.int64, device=dev)
    t = t[None] if t.dim() == 1 else t
    n_seq, T = t.shape
    M, NQ = n_seq * T, (w.NH + 2 * w.KV) * w.D
    np_ = lambda x: None if x is None else x.detach().float().cpu().numpy()  # noqa: E731
    h = w.embed[t.reshape(-1)].float().contiguous()  # the gather is exact
    qkv = torch.empty(M, NQ, dtype=torch.float16, device=dev)
    a = torch.empty(M, w.NH * w.D, dtype=torch.float16, device=dev)
    act = torch.empty(M, w.I, dtype=torch.float16, device=dev)
    L.gemm_form_log()

    def gemm(kind, l, x, blob, out, norm_w=None, bias=None, residual=None, epi=0):
        x0 = np_(x) if record is not None else None
        r0 = np_(residual) if record is not None else None
        L.probe_gemm_f16(x, blob, out, M, norm_w=norm_w, eps=w.eps if norm_w is not None else 0.0, epi=epi, bias=bias,
                         residual=residual, ld_res=w.H if residual is not None else None)
        if record is not None:
            record.append(dict(kind="gemm", proj=kind, layer=l, x=x0, g=np_(norm_w), bias=np_(bias), residual=r0, epi=epi,
                               out=np_(out), out_kind="fp32" if out.dtype == torch.float32 else "fp16"))

    for l in range(w.layers):
        tl = w.lt[l]
        kc, vc = st.k[0, l], st.v[0, l]
        gemm("qkv", l, h, tl["qkv"], qkv, norm_w=tl["ln1"], bias=w.extra(l, "qkv_bias"))
        q_n, k_n = w.extra(l, "q_norm"), w.extra(l, "k_norm")
        qkv0 = np_(qkv) if record is not None else None
        if q_n is not None:
            L.probe_rope_append_qknorm(qkv, n_seq, T, start, w.NH, w.KV, w.D, w.cos, w.sin, kc, vc, w.kv_code, w.seq_stride,
                                       q_n, k_n, w.qk_eps)
        else:
            L.probe_rope_append(qkv, n_seq, T, start, w.NH, w.KV, w.D, w.cos, w.sin, kc, vc, w.kv_code, w.seq_stride)
        L.probe_attn_prefill(qkv, n_seq, T, start, w.NH, w.KV, w.D, kc, vc, w.kv_code, w.seq_stride, a, w.window)
        if record is not None:
            record.append(dict(kind="rope_attn", layer=l, qkv_in=qkv0, qkv=np_(qkv), out=np_(a), n_seq=n_seq, T=T, start=start,
                               k=np_(st.k[:n_seq, l, :start + T]).astype(np.float64),
                               v=np_(st.v[:n_seq, l, :start + T]).astype(np.float64), q_w=np_(q_n), k_w=np_(k_n)))
        gemm("o", l, a, tl["o"], h, residual=h)
        gemm("gate_up", l, h, tl["gate_up"], act, norm_w=tl["ln2"], epi=1)
        gemm("down", l, act, tl["down"], h, residual=h)
    last = h.view(n_seq, T, w.H)[:, -1].contiguous()
    logits = torch.empty(n_seq, w.vocab, dtype=torch.float32, device=dev)
    for s in range(n_seq):
        L.probe_lm_head(last[s], w.norm, w.eps, w.lm, logits[s])
        if record is not None:
            record.append(dict(kind="lm_head", hidden=np_(last[s]), logits=np_(logits[s])))
    st.pos.fill_(start + T - 1)
    L.probe_greedy_tail(0, w.vocab, st.token, st.pos, logits=logits[0])
    torch.cuda.synchronize()
    forms = L.gemm_form_log()
    tr = [("prefill", dict(rows=_raw(h), logits=_raw(logits), token=_raw(st.token), pos=_raw(st.pos), k=_raw(st.k), v=_raw(st.v)))]
    return tr, forms


def rope_attn_ratio(rec, w_like):
    """a prompt pass's rope_append + attn_prefill stage (a `record` entry of shadow_prefill) against float64. -> (True when
    the rotated q rows and the appended K / V rows are the float64 rotation rounded to storage, worst err / bound of the
    attention output). Bounds: tests/test_gpu_attention_kernels.py — rotation rounded to the storage type, one unit of
    storage only at a rounding tie; fp16-operand attention 2^-10 max visible |v| + 2^-11 |ref| — and with a q / k norm
    tests/test_gpu_qknorm_kernels.py's bounds: q rows within one fp16 ulp of the row's largest reference magnitude, K rows
    within one unit of the cache type's last place of the rounded reference"""
    NH, KV, D, fmt, window, eps = (w_like[k] for k in ("NH", "KV", "D", "fmt", "window", "qk_eps"))
    cos, sin = w_like["cos"], w_like["sin"]
    n_seq, T, start = rec["n_seq"], rec["T"], rec["start"]
    pos = start + np.arange(T)
    x = rec["qkv_in"].astype(np.float64).reshape(n_seq, T, NH + 2 * KV, D)
    got = rec["qkv"].astype(np.float64).reshape(n_seq, T, NH + 2 * KV, D)
    c, s = cos[pos][None, :, None, :], sin[pos][None, :, None, :]
    xq, xk, xv = x[:, :, :NH], x[:, :, NH:NH + KV], x[:, :, NH + KV:]
    rows_ok = np.array_equal(got[:, :, NH:], x[:, :, NH:])  # the k / v slots of qkv stay as they were
    K, V = rec["k"], rec["v"]  # [n_seq, start + T, KV, D] as stored
    if rec["q_w"] is None:
        rows_ok = rows_ok and stored_ok(got[:, :, :NH], *R.stored_bounds(R.rotate(xq, c, s), R.rotate_error(xq, c, s), "fp16"))
        rows_ok = rows_ok and stored_ok(K[:, start:], *R.stored_bounds(R.rotate(xk, c, s), R.rotate_error(xk, c, s), fmt))
    else:
        qr, kr = QN.normed_rotated(xq, rec["q_w"], eps, c, s), QN.normed_rotated(xk, rec["k_w"], eps, c, s)
        q_bound = QN.ulp(np.abs(qr).max(axis=-1, keepdims=True), "fp16")
        rows_ok = rows_ok and bool((np.abs(got[:, :, :NH] - qr) <= q_bound).all())
        want_k = R.round_to(kr, fmt)
        rows_ok = rows_ok and bool((np.abs(K[:, start:] - want_k) <= QN.ulp(want_k, fmt)).all())
    rows_ok = rows_ok and np.array_equal(V[:, start:], R.round_to(xv, fmt))
    out = rec["out"].astype(np.float64).reshape(n_seq, T, NH, D)
    rep, worst = NH // KV, 0.0
    for sq in range(n_seq):
        for hd in range(NH):
            ref, vmax, _ = R.attend(got[sq, :, hd], K[sq, :, hd // rep], V[sq, :, hd // rep], pos, window)
            bound = 2.0 ** -10 * vmax[:, None] + 2.0 ** -11 * np.abs(ref)
            worst = max(worst, float((np.abs(out[sq, :, hd] - ref) / np.maximum(bound, 1e-300)).max()))
    return bool(rows_ok), worst
