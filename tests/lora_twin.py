"""A float64 twin of a Llama-class decoder whose projections are dense dequantised matrices plus unmerged LoRA adapters:
y = x W_deq + s (x A^T) B^T. numpy only; the tests build it from the same quantised model the engine is built over
(tests/test_gpu_lora_engine.py, tests/test_gpu_lora_serving.py) or, without a GPU, from the oracle's RTN of the same
random-init weights.

The head is the engine's: embedding and lm_head rounded to fp16 as `optimize_transformers` hands them over, RoPE tables
from `runtime.engine.build_rope_tables` (fp32 angles). Every adapter application also returns the derived tolerance of
tests/lora_reference.py; `forward` keeps the largest per projection and returns their sum over all adapter applications
as `lora_tol`: what the adapter arithmetic may add to a logit if every such perturbation reached it with gain 1 (the
norms and the softmax keep gains near or below 1 on these models). On the tiny model it comes to about 6e-4, the same
order as the engine's own measure there (2e-3 max|logit| + 1e-4 with max|logit| near 0.5).
"""
import numpy as np

from tests import lora_reference as R

PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _rms(x, w, eps):
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * w


def _rot(x, cos, sin):
    """HF rotate_half form: x [T, heads, D], cos / sin [T, D / 2]"""
    d = x.shape[-1] // 2
    c, s = np.concatenate([cos, cos], -1)[:, None, :], np.concatenate([sin, sin], -1)[:, None, :]
    return x * c + np.concatenate([-x[..., d:], x[..., :d]], -1) * s


class Twin:
    def __init__(self, heads, kv_heads, head_dim, eps, theta, layers, embed, norm, lm_head, adapters=None, max_pos=256):
        """layers: per layer a dict of the seven W_deq [K, N] float64 and ln1 / ln2; embed / lm_head [vocab, hidden]
        (rounded to fp16 here); adapters: {(layer, target): (A, B, scaling)} numpy or None"""
        import torch

        from intel_extension_for_transformers_amd.runtime.engine import build_rope_tables

        self.NH, self.KV, self.D, self.eps = heads, kv_heads, head_dim, float(eps)
        self.layers = layers
        f16 = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float64)  # noqa: E731
        self.embed, self.lm, self.norm = f16(embed), f16(lm_head), np.asarray(norm, np.float64)
        cos, sin = build_rope_tables(max_pos, head_dim, float(theta), torch.device("cpu"))
        self.cos, self.sin = cos.double().numpy(), sin.double().numpy()
        self.adapters = adapters or {}

    def _lin(self, l, name, x, tol):
        y = x @ self.layers[l][name]
        ad = self.adapters.get((l, name))
        if ad is not None:
            d, t = R._two_stage(x, np.ones(x.shape[0]), ad, x.shape[-1])
            y = y + d
            tol.append(float(t.max()))
        return y

    def forward(self, tokens):
        """tokens [T] -> (logits float64 [T, vocab], lora_tol)"""
        tok = np.asarray(tokens, np.int64)
        T = len(tok)
        h = self.embed[tok]
        tol = []
        rep = self.NH // self.KV
        causal = np.tril(np.ones((T, T), bool))
        for l, W in enumerate(self.layers):
            x = _rms(h, W["ln1"], self.eps)
            q = self._lin(l, "q_proj", x, tol).reshape(T, self.NH, self.D)
            k = self._lin(l, "k_proj", x, tol).reshape(T, self.KV, self.D)
            v = self._lin(l, "v_proj", x, tol).reshape(T, self.KV, self.D)
            q, k = _rot(q, self.cos[:T], self.sin[:T]), _rot(k, self.cos[:T], self.sin[:T])
            out = np.empty((T, self.NH, self.D))
            for hd in range(self.NH):
                s = (q[:, hd] @ k[:, hd // rep].T) / np.sqrt(self.D)
                s = np.where(causal, s, -np.inf)
                p = np.exp(s - s.max(axis=-1, keepdims=True))
                out[:, hd] = (p / p.sum(axis=-1, keepdims=True)) @ v[:, hd // rep]
            h = h + self._lin(l, "o_proj", out.reshape(T, -1), tol)
            x = _rms(h, W["ln2"], self.eps)
            g, u = self._lin(l, "gate_proj", x, tol), self._lin(l, "up_proj", x, tol)
            h = h + self._lin(l, "down_proj", g / (1.0 + np.exp(-g)) * u, tol)
        return _rms(h, self.norm, self.eps) @ self.lm.T, float(sum(tol))

    def greedy(self, prompt, n_new):
        """-> (tokens generated, per step: (top-1 / top-2 logit margin, largest |logit|, lora_tol)); step 0 is the prompt
        pass's pick"""
        seq, steps = list(prompt), []
        for _ in range(n_new):
            logits, lt = self.forward(seq)
            last = np.sort(logits[-1])
            steps.append((float(last[-1] - last[-2]), float(np.abs(last).max()), lt))
            seq.append(int(np.argmax(logits[-1])))
        return seq[len(prompt):], steps


def _theta(c):
    theta = getattr(c, "rope_theta", None)
    return float(theta if theta is not None else (getattr(c, "rope_parameters", None) or {}).get("rope_theta", 10000.0))


def twin_from_fp(fp, adapters=None, group=32):
    """the twin of a random-init HF Llama quantised by the oracle's RTN (sym int4, groups of `group`): what the GPU-less
    seed search uses; the GPU tests take the device's dequantised weights instead (`twin_from_quantised`)"""
    from oracle import woq_oracle as orc

    c = fp.config
    layers = []
    for layer in fp.model.layers:
        W = {}
        for name in PROJ:
            m = getattr(layer.self_attn if name[0] in "qkvo" else layer.mlp, name)
            q, s, _ = orc.rtn_quantize(m.weight.detach().float().numpy(), True, group, False)
            W[name] = orc.dequant_raw(q, s, None, group).astype(np.float64)
        W["ln1"] = layer.input_layernorm.weight.detach().double().numpy()
        W["ln2"] = layer.post_attention_layernorm.weight.detach().double().numpy()
        layers.append(W)
    return Twin(c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.rms_norm_eps, _theta(c), layers,
                fp.model.embed_tokens.weight.detach().float().numpy(), fp.model.norm.weight.detach().double().numpy(),
                fp.lm_head.weight.detach().float().numpy(), adapters)


def twin_from_quantised(q, deq, adapters=None):
    """the twin of a quantised (and possibly wrapped) model: `deq(module)` -> its dequantised weight [K, N] (device fp32)"""
    c = q.config
    layers = []
    for layer in q.model.layers:
        W = {}
        for name in PROJ:
            m = getattr(layer.self_attn if name[0] in "qkvo" else layer.mlp, name)
            W[name] = deq(m).double().cpu().numpy()
        W["ln1"] = layer.input_layernorm.weight.detach().double().cpu().numpy()
        W["ln2"] = layer.post_attention_layernorm.weight.detach().double().cpu().numpy()
        layers.append(W)
    return Twin(c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.rms_norm_eps, _theta(c), layers,
                q.model.embed_tokens.weight.detach().float().cpu().numpy(), q.model.norm.weight.detach().double().cpu().numpy(),
                q.lm_head.weight.detach().float().cpu().numpy(), adapters)


def adapters_of(model):
    """{(layer, target): (A, B, scaling)} numpy fp32 of a wrapped model's QuantizedLoraLinearQBits modules"""
    out = {}
    for name, m in model.named_modules():
        if hasattr(m, "lora_A") and hasattr(m, "scaling"):
            parts = name.split(".")
            out[(int(parts[parts.index("layers") + 1]), parts[-1])] = (
                m.lora_A["default"].weight.detach().float().cpu().numpy(),
                m.lora_B["default"].weight.detach().float().cpu().numpy(), float(m.scaling))
    return out


def random_adapters(cfg_shapes, layers, targets, r, alpha, seed, b_scale=0.1):
    """random adapters as `get_peft_model` + a drawn lora_B would leave them: A uniform in +-1 / sqrt(K) (Kaiming, a =
    sqrt 5), B ~ b_scale N(0, 1). cfg_shapes: {target: (K, N)}"""
    rng = np.random.default_rng(seed)
    out = {}
    for l in range(layers):
        for t in targets:
            K, N = cfg_shapes[t]
            out[(l, t)] = (rng.uniform(-1, 1, (r, K)).astype(np.float32) / np.float32(np.sqrt(K)),
                           (b_scale * rng.standard_normal((N, r))).astype(np.float32), float(alpha) / r)
    return out
