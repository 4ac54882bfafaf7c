"""The engine's decode step and prompt pass WITH unmerged LoRA adapters, re-assembled from the single-kernel probes: the
chain of tests/engine_stage_shadow.py (imported, not edited) with the adapter launches placed where csrc/woq_engine.hip
places them, decided in this file independently of it.

Decode step. In front of every fused projection that has an installed part, `woq_probe_lora_delta` runs over the
projection's own input and its output is fed as `bias` into the existing GEMV probe:
  XQ step            the input is the XQ vector the producer emitted, i.e. `woq_probe_xq_from_f32` of the fp32 values times
                     the norm weight that rides with them (the existing stage tests hold the producers' vectors to exactly
                     that), with its sums of squares where the consumer normalises (qkv, gate/up) and none for o / down;
  fp32 step          the fp32 vector and the consumer's norm weight (or none).
A projection without an installed part gets its static bias (or none) and no launch.

Prompt pass. qkv: base GEMM, then shrink over the fp32 rows (ln1) and the expand onto the fp16 q | k | v rows, before RoPE;
o_proj / down_proj: shrink over the fp16 input rows and the expand onto the fp32 residual rows, then the base GEMM with its
residual slot; gate/up: base GEMM with a plain epilogue into fp16 [rows][2 inter], shrink over the fp32 rows (ln2), the
expand's SiLU * mul store into the activation rows.
"""
import numpy as np

from tests import engine_stage_shadow as S

TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
KIND_PARTS = {"qkv": ("q_proj", "k_proj", "v_proj"), "o": ("o_proj",), "gate_up": ("gate_proj", "up_proj"), "down": ("down_proj",)}


class LoraWiring:
    """{(layer, target): (A, B, scaling)} as device fp32 tensors, and the part lists the probes take"""

    def __init__(self, eng, entries):
        import torch

        self.dev = eng.device
        self.entries = {k: (a.detach().to(eng.device, torch.float32).contiguous(),
                            b.detach().to(eng.device, torch.float32).contiguous(), float(s))
                        for k, (a, b, s) in entries.items()}
        c = eng.cfg
        attn, kv = c.heads * c.head_dim, c.kv_heads * c.head_dim
        self.cols = dict(q_proj=attn, k_proj=kv, v_proj=kv, o_proj=c.hidden, gate_proj=c.inter, up_proj=c.inter,
                         down_proj=c.hidden)

    def parts(self, l, kind):
        """-> ([(A, B, s) | (None, n_cols, 0.0)], True when at least one part is installed)"""
        out = [self.entries.get((l, t), (None, self.cols[t], 0.0)) for t in KIND_PARTS[kind]]
        return out, any(p[0] is not None for p in out)


def _delta_bias(w, lw, l, kind, x, norm_w, static_bias, xq, n_cols):
    """the `bias` the projection's GEMV probe gets"""
    import torch

    from intel_extension_for_transformers_amd import _lib as L

    parts, on = lw.parts(l, kind)
    if not on:
        return static_bias
    out = torch.full((n_cols,), float("nan"), dtype=torch.float32, device=lw.dev)
    if xq:
        K = x.numel()
        limbs = torch.zeros(L.xq_limb_bytes(K), dtype=torch.uint8, device=lw.dev)
        u, sx, ssq = (torch.empty(K // 16, dtype=torch.float32, device=lw.dev) for _ in range(3))
        L.probe_xq_from_f32(x, norm_w, limbs, u, sx, ssq)
        L.probe_lora_delta(parts, out, xq=(limbs, u, sx), ssq=ssq if norm_w is not None else None, eps=w.eps,
                           base_bias=static_bias, interleave=kind == "gate_up")
    else:
        L.probe_lora_delta(parts, out, x=x, norm_w=norm_w, eps=w.eps, base_bias=static_bias, interleave=kind == "gate_up")
    return out


def shadow_decode_step(w, lw, st, xq, attn):
    """One greedy decode step from the probes over `st` (engine_stage_shadow.ShadowState), adapters included. -> trace"""
    import torch

    from intel_extension_for_transformers_amd import _lib as L

    dev = st.token.device
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)  # noqa: E731
    pos0 = int(st.pos.item())
    NQ = (w.NH + 2 * w.KV) * w.D
    gu_tmp = f32(2 * w.I)

    def gemv(kind, l, x, blob, n_out, n_cols, norm_w=None, static_bias=None, residual=None, epi=0):
        bias = _delta_bias(w, lw, l, kind, x, norm_w, static_bias, xq, n_cols)
        out = f32(n_out)
        eps = w.eps if norm_w is not None else 0.0
        if xq:
            L.probe_gemv_xq(x, blob, epi, norm_w, eps, bias, residual, None, out, None, None)
        else:
            L.probe_gemv_f32(x, blob, out, norm_w=norm_w, eps=eps, epi=epi, bias=bias, residual=residual, gu_tmp=gu_tmp)
        return out

    h = f32(w.H)
    L.probe_embed(w.embed, st.token, h, pos=st.pos, max_ctx=w.max_ctx, status=st.status)
    riding = w.after_embed
    tr = []
    for l in range(w.layers):
        t = w.lt[l]
        kc, vc = st.k[0, l], st.v[0, l]
        qkv = gemv("qkv", l, h, t["qkv"], NQ, NQ, norm_w=riding, static_bias=w.extra(l, "qkv_bias"))
        a = f32(w.NH * w.D)
        L.probe_attn_decode(qkv, kc, vc, w.kv_code, st.pos, w.cos, w.sin, w.NH, w.KV, w.D, w.max_ctx, w.window,
                            attn["splits"], attn["grouped"], 0, attn["chunk"], a)
        riding = w.after_attn[l]
        h = gemv("o", l, a, t["o"], w.H, w.H, residual=h)
        tr.append(("L%d.attn" % l, dict(hidden=S._raw(h), k=S._raw(kc[pos0]), v=S._raw(vc[pos0]))))
        act = gemv("gate_up", l, h, t["gate_up"], w.I, 2 * w.I, norm_w=riding, epi=1)
        riding = w.after_mlp[l]
        h = gemv("down", l, act, t["down"], w.H, w.H, residual=h)
        tr.append(("L%d.mlp" % l, dict(hidden=S._raw(h))))
    logits = f32(w.vocab)
    npairs = (w.vocab + 15) // 16
    pmax, pidx = f32(npairs), torch.empty(npairs, dtype=torch.int32, device=dev)
    L.probe_lm_head(h, w.norm, w.eps, w.lm, logits, pmax, pidx)
    L.probe_greedy_tail(1, w.vocab, st.token, st.pos, pmax=pmax, pidx=pidx, log=st.log, status=st.status)
    torch.cuda.synchronize()
    tr.append(("head", dict(logits=S._raw(logits), token=S._raw(st.token), pos=S._raw(st.pos), log=S._raw(st.log[pos0:pos0 + 1]))))
    return tr


def shadow_prefill(w, lw, st, tokens, start):
    """The prompt pass from the probes over `st`'s cache copy, adapters included. -> trace"""
    import torch

    from intel_extension_for_transformers_amd import _lib as L

    dev = st.token.device
    t = torch.as_tensor(np.asarray(tokens), dtype=torch.int64, device=dev)
    t = t[None] if t.dim() == 1 else t
    n_seq, T = t.shape
    M, NQ = n_seq * T, (w.NH + 2 * w.KV) * w.D
    h = w.embed[t.reshape(-1)].float().contiguous()
    qkv = torch.empty(M, NQ, dtype=torch.float16, device=dev)
    a = torch.empty(M, w.NH * w.D, dtype=torch.float16, device=dev)
    act = torch.empty(M, w.I, dtype=torch.float16, device=dev)
    gu = torch.empty(M, 2 * w.I, dtype=torch.float16, device=dev)

    def gemm(x, blob, out, norm_w=None, bias=None, residual=None, epi=0):
        L.probe_gemm_f16(x, blob, out, M, norm_w=norm_w, eps=w.eps if norm_w is not None else 0.0, epi=epi, bias=bias,
                         residual=residual, ld_res=w.H if residual is not None else None)

    def rows(l, kind, x, K, norm_w, mode, out, n_cols, ldo, gu_rows=None):
        parts, on = lw.parts(l, kind)
        if not on:
            return False
        live = [p[0] for p in parts if p[0] is not None]
        r_tot = sum(int(a_.shape[0]) for a_ in live)
        T_ = torch.full((M, r_tot + 3), float("nan"), dtype=torch.float32, device=dev)
        L.probe_lora_shrink(x, M, K, live, T_, norm_w=norm_w, eps=w.eps)
        b_parts = [(None, p[1], p[2]) if p[0] is not None else p for p in parts]
        L.probe_lora_expand(mode, T_, M, n_cols, b_parts, out, ldo, gu=gu_rows, ld_gu=2 * w.I if gu_rows is not None else 0)
        return True

    for l in range(w.layers):
        tl = w.lt[l]
        kc, vc = st.k[0, l], st.v[0, l]
        gemm(h, tl["qkv"], qkv, norm_w=tl["ln1"], bias=w.extra(l, "qkv_bias"))
        rows(l, "qkv", h, w.H, tl["ln1"], L.LORA_EXPAND_ADD_F16, qkv, NQ, NQ)
        L.probe_rope_append(qkv, n_seq, T, start, w.NH, w.KV, w.D, w.cos, w.sin, kc, vc, w.kv_code, w.seq_stride)
        L.probe_attn_prefill(qkv, n_seq, T, start, w.NH, w.KV, w.D, kc, vc, w.kv_code, w.seq_stride, a, w.window)
        rows(l, "o", a, w.NH * w.D, None, L.LORA_EXPAND_ADD_F32, h, w.H, w.H)
        gemm(a, tl["o"], h, residual=h)
        if lw.parts(l, "gate_up")[1]:
            gemm(h, tl["gate_up"], gu, norm_w=tl["ln2"], epi=0)
            rows(l, "gate_up", h, w.H, tl["ln2"], L.LORA_EXPAND_SILU, act, 2 * w.I, w.I, gu_rows=gu)
        else:
            gemm(h, tl["gate_up"], act, norm_w=tl["ln2"], epi=1)
        rows(l, "down", act, w.I, None, L.LORA_EXPAND_ADD_F32, h, w.H, w.H)
        gemm(act, tl["down"], h, residual=h)
    last = h.view(n_seq, T, w.H)[:, -1].contiguous()
    logits = torch.empty(n_seq, w.vocab, dtype=torch.float32, device=dev)
    for s in range(n_seq):
        L.probe_lm_head(last[s], w.norm, w.eps, w.lm, logits[s])
    st.pos.fill_(start + T - 1)
    L.probe_greedy_tail(0, w.vocab, st.token, st.pos, logits=logits[0])
    torch.cuda.synchronize()
    return [("prefill", dict(rows=S._raw(h), logits=S._raw(logits), token=S._raw(st.token), pos=S._raw(st.pos),
                             k=S._raw(st.k), v=S._raw(st.v)))]
