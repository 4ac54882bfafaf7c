"""Python handle of the native batch-1 decode engine (csrc/woq_engine.hip).

The engine is the MI355X counterpart of `ipex.optimize_transformers(qmodel, ...)`, the reference's own
precedent for swapping HF's RMSNorm / RoPE / MLP glue for fused device kernels after `from_pretrained`
(docs/weightonlyquant.md:199-202, README.md:290): quantised-linear replacement happens at load, the fused
decode path is an optional post-pass over the same WQH1 blobs. torch is plumbing here (device memory,
streams); every kernel is in libwoq_hip.so.
"""
import ctypes
import math
import os

import numpy as np
import torch

from .. import _lib as L
from .. import qbits
from . import request
# the request loops live in runtime/request.py; their public names stay part of this module's API, like StreamingConfig
from .request import DeviceSampler, _controls, generate_sampled, iter_sampled, iter_sampled_auto, request_seed  # noqa: F401
from .streaming import StreamingConfig, plan_steps, plan_stream  # noqa: F401


ENGINE_MODEL_TYPES = ("llama", "mistral", "qwen2", "qwen3")  # the one list: engine_supports reads it, nothing else does
ROPE_TYPES = ("default", "linear", "llama3", "yarn")  # build_rope_tables' parameterisations


def rope_scaling_of(config):
    """(rope type, parameter dict) of an HF config: `rope_scaling` or `rope_parameters`, whichever it has."""
    rs = getattr(config, "rope_scaling", None) or getattr(config, "rope_parameters", None) or {}
    if not isinstance(rs, dict):
        return "default", {}
    return (rs.get("rope_type") or rs.get("type") or "default"), rs


def rope_inv_freq(head_dim, theta=10000.0, rope_scaling=None, max_position_embeddings=None):
    """(inv_freq fp32 [head_dim / 2], attention factor): HF's `default`, `linear`, `llama3` and `yarn` RoPE
    parameterisations restated in HF's operation order (transformers/modeling_rope_utils.py: the fp32 tensor ops, the
    Python-float scalars). Anything else raises."""
    rtype, rs = ("default", {}) if not rope_scaling else \
        ((rope_scaling.get("rope_type") or rope_scaling.get("type") or "default"), rope_scaling)
    if rtype not in ROPE_TYPES:
        raise RuntimeError("QBits: the fused decode engine implements plain RoPE only (rope scaling %r)" % rtype)
    dim = head_dim
    inv_freq = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.int64).float() / dim))
    if rtype == "default":
        return inv_freq, 1.0
    factor = rs.get("factor")
    if rtype == "linear":
        return inv_freq / factor, 1.0
    orig = rs.get("original_max_position_embeddings") or max_position_embeddings
    if orig is None:
        raise RuntimeError("QBits: rope scaling %r needs original_max_position_embeddings" % rtype)
    if rtype == "llama3":
        low_f, high_f = rs["low_freq_factor"], rs["high_freq_factor"]
        low_wavelen, high_wavelen = orig / low_f, orig / high_f
        wavelen = 2 * math.pi / inv_freq
        scaled = torch.where(wavelen > low_wavelen, inv_freq / factor, inv_freq)
        smooth = (orig / wavelen - low_f) / (high_f - low_f)
        smoothed = (1 - smooth) * scaled / factor + smooth * scaled
        medium = ~(wavelen < high_wavelen) * ~(wavelen > low_wavelen)
        return torch.where(medium, smoothed, scaled), 1.0
    # yarn
    if factor is None:
        factor = max_position_embeddings / orig

    def mscale_of(scale, mscale=1):
        return 1.0 if scale <= 1 else 0.1 * mscale * math.log(scale) + 1.0

    att = rs.get("attention_factor")
    if att is None:
        ms, ms_all = rs.get("mscale"), rs.get("mscale_all_dim")
        att = float(mscale_of(factor, ms) / mscale_of(factor, ms_all)) if ms and ms_all else mscale_of(factor)
    beta_fast, beta_slow = rs.get("beta_fast") or 32, rs.get("beta_slow") or 1

    def correction_dim(rot):
        return (dim * math.log(orig / (rot * 2 * math.pi))) / (2 * math.log(theta))

    low, high = correction_dim(beta_fast), correction_dim(beta_slow)
    if rs.get("truncate", True):
        low, high = math.floor(low), math.ceil(high)
    low, high = max(low, 0), min(high, dim - 1)
    if low == high:
        high += 0.001
    pos_freqs = theta ** (torch.arange(0, dim, 2).float() / dim)
    extrapolation, interpolation = 1.0 / pos_freqs, 1.0 / (factor * pos_freqs)
    ramp = torch.clamp((torch.arange(dim // 2, dtype=torch.float32) - low) / (high - low), 0, 1)
    ext = 1 - ramp
    return interpolation * (1 - ext) + extrapolation * ext, float(att)


def build_rope_tables(max_pos, head_dim, theta=10000.0, device="cuda", rope_scaling=None,
                      max_position_embeddings=None):
    """cos/sin [max_pos, head_dim/2] fp32: HF's rotary module for the `default` parameterisation and, with
    `rope_scaling` (an HF rope_scaling / rope_parameters dict), for `linear`, `llama3` and `yarn`: the angles are
    position * inv_freq in fp32, and cos / sin are multiplied by HF's attention factor (yarn; 1 elsewhere —
    rope_inv_freq returns it, and a rolling KV cache refuses tables where it is not 1). `dynamic`, `longrope` and
    anything unknown raise."""
    inv_freq, att = rope_inv_freq(head_dim, theta, rope_scaling, max_position_embeddings)
    ang = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv_freq[None, :]
    cos, sin = ang.cos(), ang.sin()
    if att != 1.0:
        cos, sin = cos * att, sin * att
    return cos.contiguous().to(device), sin.contiguous().to(device)


def engine_window(config):
    """The sliding window (0 = full causal attention) the engine runs an HF config with. llama / mistral:
    `sliding_window` as it stands. qwen2 / qwen3: from `layer_types` when present (all full: 0, all sliding:
    `sliding_window`, mixed: refused), else `sliding_window` only under `use_sliding_window`."""
    window = int(getattr(config, "sliding_window", None) or 0)
    if getattr(config, "model_type", "") not in ("qwen2", "qwen3"):
        return window  # Mistral v0.1: 4096; null / absent = full causal attention
    kinds = set(getattr(config, "layer_types", None) or ())
    if kinds:
        if kinds == {"full_attention"}:
            return 0
        if kinds == {"sliding_attention"}:
            return window
        raise RuntimeError("QBits: the fused decode engine runs one attention form in every layer (layer_types mixes %s)"
                           % " and ".join(sorted(kinds)))
    return window if getattr(config, "use_sliding_window", False) else 0


def engine_supports(config):
    """(ok, reason): does the fused decode engine take a model of this HF config? The one acceptance rule —
    optimize_transformers, the engine-backed `generate`, NeuralChat's engine gate and the tensor-parallel host all ask
    here. A refusal's reason names the config field that caused it. (What only the modules can tell — the weight types,
    a bias that the config does not announce — optimize_transformers checks on the model itself.)"""
    mt = getattr(config, "model_type", "")
    if mt not in ENGINE_MODEL_TYPES:
        return False, "QBits: the fused decode engine covers Llama-class decoders (model_type %s), got %r" % (
            " / ".join(ENGINE_MODEL_TYPES), mt)
    rtype, rs = rope_scaling_of(config)
    if rtype not in ROPE_TYPES:
        return False, "QBits: the fused decode engine implements plain RoPE only (rope scaling %r)" % rtype
    if (rs.get("partial_rotary_factor") or getattr(config, "partial_rotary_factor", None) or 1.0) != 1.0:
        return False, "QBits: the fused decode engine rotates whole heads only (partial_rotary_factor)"
    if getattr(config, "hidden_act", "silu") not in ("silu", "swish"):
        return False, "QBits: the fused decode engine implements the SiLU-gated MLP only (hidden_act %r)" % config.hidden_act
    # llama / mistral / qwen3: attention_bias puts a bias on o_proj as well; qwen2's q / k / v biases are not a config field
    if mt != "qwen2" and getattr(config, "attention_bias", False):
        return False, "QBits: the fused decode engine does not take biased projections (attention_bias: o_proj)"
    if getattr(config, "mlp_bias", False):
        return False, "QBits: the fused decode engine does not take biased projections (mlp_bias)"
    try:
        engine_window(config)
    except RuntimeError as e:
        return False, str(e)
    return True, ""


def fuse_gate_up(gate, up):
    """[*, I] x 2 -> [*, 2I] with 16-column tiles interleaved (gate tile t, up tile t, gate tile t+1, ...), the
    column order the fused SiLU*mul GEMV epilogue expects."""
    lead = gate.shape[:-1]
    inter = gate.shape[-1]
    assert inter % 16 == 0, "intermediate size must be a multiple of 16"
    g = gate.reshape(*lead, inter // 16, 1, 16)
    u = up.reshape(*lead, inter // 16, 1, 16)
    return torch.cat([g, u], dim=-2).reshape(*lead, 2 * inter).contiguous()


def _kv_code(dt):
    """KV-cache storage dtype -> ABI code: fp16 / bf16, or fp8 (torch.float8_e4m3fn or the string "fp8_e4m3")."""
    if dt in ("fp8", "fp8_e4m3") or dt == getattr(torch, "float8_e4m3fn", None):
        return L.FP8_E4M3
    return L.torch_dtype_code(dt)


class WoqDecoderEngine:
    """Owns the native engine plus the torch tensors whose device memory it points at."""

    def __init__(self, hidden, inter, heads, kv_heads, head_dim, layers, vocab, max_ctx=2048, rms_eps=1e-5,
                 rope_theta=10000.0, kv_dtype=torch.float16, tp_rank=0, tp_size=1, device=None, max_batch=1,
                 attn_splits=0, sliding_window=0, attn_grouped=False):
        L.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.cfg = L.EngineConfig(hidden=hidden, inter=inter, heads=heads, kv_heads=kv_heads, head_dim=head_dim,
                                  layers=layers, vocab=vocab, max_ctx=max_ctx, rms_eps=rms_eps, rope_theta=rope_theta,
                                  tp_rank=tp_rank, tp_size=tp_size, kv_dtype=_kv_code(kv_dtype))
        self.kv_dtype = kv_dtype
        self.cfg.reserved[0] = int(max_batch)
        self.cfg.reserved[1] = int(attn_splits)
        self.cfg.reserved[2] = int(sliding_window or 0)
        self.max_batch = int(max_batch)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            L.check(L.lib().woq_engine_create(ctypes.byref(self.cfg), ctypes.byref(self._h)))
        if attn_grouped:
            self.set_attn_grouped(True)
        self.token = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.pos = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.logits = torch.zeros(vocab, dtype=torch.float32, device=self.device)
        self.hidden = torch.zeros(hidden, dtype=torch.float32, device=self.device)
        L.check(L.lib().woq_engine_bind_io(self._h, self.token.data_ptr(), self.pos.data_ptr(),
                                           self.logits.data_ptr(), self.hidden.data_ptr()))
        self._keep = []  # tensors the engine holds raw pointers to
        self.layer_tensors, self.head_tensors = {}, {}  # the same, by name (inspection / parity checks)
        self._allreduce_cb = None
        self._comm = None
        self.captured = False
        self.sampler_installed = False     # native sampler in the chaining tail (set_sampler / clear_sampler)
        self.controls_installed = False    # ... with logit bias / presence / frequency penalty / min_p beside it
        self.native_sampled_requests = 0   # requests that ran with it (iter_generate)
        self.logprobs_on = False           # log-probability record after every chaining pick (set_logprobs)
        self.guide_installed = False       # token guide in the chaining tail (set_guide / clear_guide)
        self._guide = None                 # ... the TokenGuide, its prefix and whether set_guide installed the sampler
        self._guide_prefix = ()
        self._guide_owns_sampler = False
        # hipGraph capture is not allowed on the legacy null stream torch uses by default
        self._stream = torch.cuda.Stream(device=self.device)

    def __del__(self):
        try:
            if self._h:
                L.lib().woq_engine_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_layer(self, idx, qkv_blob, o_blob, gate_up_blob, down_blob, ln1, ln2):
        ln1 = ln1.to(self.device, torch.float32).contiguous()
        ln2 = ln2.to(self.device, torch.float32).contiguous()
        w = L.LayerWeights(qkv_blob=qkv_blob.data_ptr(), o_blob=o_blob.data_ptr(),
                           gate_up_blob=gate_up_blob.data_ptr(), down_blob=down_blob.data_ptr(),
                           ln1=ln1.data_ptr(), ln2=ln2.data_ptr(), qkv_hdr=qbits.header_of(qkv_blob),
                           o_hdr=qbits.header_of(o_blob), gate_up_hdr=qbits.header_of(gate_up_blob),
                           down_hdr=qbits.header_of(down_blob))
        L.check(L.lib().woq_engine_set_layer(self._h, idx, ctypes.byref(w)))
        self._keep += [qkv_blob, o_blob, gate_up_blob, down_blob, ln1, ln2]
        self.layer_tensors[idx] = dict(qkv=qkv_blob, o=o_blob, gate_up=gate_up_blob, down=down_blob, ln1=ln1, ln2=ln2)

    def set_layer_extras(self, idx, qkv_bias=None, q_norm=None, k_norm=None):
        """Optional extras of layer `idx` (woq_engine_set_layer_extras; after set_layer): `qkv_bias`
        [(heads + 2 kv_heads) * head_dim] added to the fused q|k|v projection (Qwen2), `q_norm` / `k_norm` [head_dim]
        = the weights of the per-head RMSNorm on q and k in front of RoPE (Qwen3; both or neither). One GPU only."""
        def dev(t):
            return None if t is None else t.detach().to(self.device, torch.float32).contiguous()

        qkv_bias, q_norm, k_norm = dev(qkv_bias), dev(q_norm), dev(k_norm)
        n_qkv = (self.cfg.heads + 2 * self.cfg.kv_heads) * self.cfg.head_dim
        for t, n, what in ((qkv_bias, n_qkv, "qkv_bias"), (q_norm, self.cfg.head_dim, "q_norm"),
                           (k_norm, self.cfg.head_dim, "k_norm")):
            if t is not None and t.numel() != n:
                raise RuntimeError("QBits: %s has %d elements, the engine's shape needs %d" % (what, t.numel(), n))
        L.check(L.lib().woq_engine_set_layer_extras(self._h, int(idx), *(None if t is None else t.data_ptr()
                                                                         for t in (qkv_bias, q_norm, k_norm))))
        self.captured = False  # (the native side dropped its graphs if the extras changed)
        self._keep += [t for t in (qkv_bias, q_norm, k_norm) if t is not None]
        self.layer_tensors.setdefault(idx, {}).update(qkv_bias=qkv_bias, q_norm=q_norm, k_norm=k_norm)

    # ---- unmerged LoRA adapters (include/woq_hip.h woq_engine_set_lora; csrc/woq_lora.hip) ----------------------------
    def _lora_shape(self, target):
        """(K, N) of a target's projection: A is [r, K], B is [N, r]"""
        c = self.cfg
        attn, kv = c.heads * c.head_dim, c.kv_heads * c.head_dim
        return {"q_proj": (c.hidden, attn), "k_proj": (c.hidden, kv), "v_proj": (c.hidden, kv), "o_proj": (attn, c.hidden),
                "gate_proj": (c.hidden, c.inter), "up_proj": (c.hidden, c.inter), "down_proj": (c.inter, c.hidden)}[target]

    @staticmethod
    def _lora_entries(source):
        """{(layer, target name): (A, B, scaling)} of a model wrapped by `get_peft_model` / `load_peft_adapter`, of a
        PEFT adapter directory (adapter_config.json + adapter_model.safetensors), or of such a dict itself."""
        from ..transformers.llm.quantization import lora

        def place(path):
            parts = path.split(".")
            if "layers" not in parts or parts[-1] not in L.LORA_TARGETS:
                raise RuntimeError("QBits: the engine carries adapters on %s of the decoder layers; %r is not one"
                                   % (" / ".join(L.LORA_TARGETS), path))
            return int(parts[parts.index("layers") + 1]), parts[-1]

        out = {}
        if isinstance(source, dict):  # {(layer, target name): (A [r, K], B [N, r], scaling)} as it stands
            for layer, target in source:
                place("layers.%d.%s" % (int(layer), target))
            return {(int(l), t): v for (l, t), v in source.items()}
        if isinstance(source, (str, os.PathLike)):
            from safetensors.torch import load_file

            cfg = lora.LoraConfig.from_pretrained(source)
            tensors = load_file(os.path.join(source, lora.WEIGHTS_NAME))
            halves = {}
            for key, t in tensors.items():
                prefix, _, rest = key.partition("base_model.model.")
                path, _, which = rest.rpartition(".lora_")
                if prefix or which.split(".")[0] not in ("A", "B"):
                    raise RuntimeError("QBits: adapter key %r is no LoRA weight" % key)
                halves.setdefault(place(path), {})[which.split(".")[0]] = t
            for where, ab in halves.items():
                if set(ab) != {"A", "B"}:
                    raise RuntimeError("QBits: the adapter holds only lora_%s for layer %d %s" % (next(iter(ab)), *where))
                out[where] = (ab["A"], ab["B"], float(cfg.lora_alpha) / int(ab["A"].shape[0]))
            return out
        for name, m in lora._lora_modules(source):
            if m.merged:
                raise RuntimeError("QBits: %s is merged into its blob; unmerge() it or serve the merged model" % name)
            out[place(name)] = (m.lora_A[m.active_adapter].weight, m.lora_B[m.active_adapter].weight, float(m.scaling))
        return out

    def _lora_kinds(self, placed):
        kind = {"q_proj": 0, "k_proj": 0, "v_proj": 0, "o_proj": 1, "gate_proj": 2, "up_proj": 2, "down_proj": 3}
        return {(l, kind[t]) for l, t in placed}

    def set_lora(self, source, r_max=None):
        """Installs the adapter of `source` (a model wrapped by `get_peft_model` / `load_peft_adapter`, a PEFT adapter
        directory, or a dict {(layer, "q_proj" | ... | "down_proj"): (A [r, K], B [N, r], scaling)}) on the engine, unmerged: every targeted projection computes x W + scaling * (x A^T) B^T in
        the decode step and the prompt pass. The values are COPIED (fp32): the engine sees those of the last `set_lora`,
        whatever happens to the modules afterwards. Targets the previous adapter had and this one has not are removed.
        `r_max` (default: this adapter's largest rank) sizes the engine's tables on the first call; a later adapter of
        the same targets and ranks up to it keeps a captured graph."""
        entries = self._lora_entries(source)
        if not entries:
            raise RuntimeError("QBits: no LoRA adapter found to install")
        staged = {}
        for (layer, target), (a, b, s) in entries.items():
            K, N = self._lora_shape(target)
            r = int(a.shape[0])
            if not 0 <= layer < self.cfg.layers:
                raise RuntimeError("QBits: the adapter names layer %d; the engine has %d" % (layer, self.cfg.layers))
            if tuple(a.shape) != (r, K) or tuple(b.shape) != (N, r):
                raise RuntimeError("QBits: layer %d %s: lora_A is %s and lora_B is %s; the engine's projection needs "
                                   "[r, %d] and [%d, r]" % (layer, target, tuple(a.shape), tuple(b.shape), K, N))
            if not 1 <= r <= L.LORA_MAX_RANK:
                raise RuntimeError("QBits: LoRA ranks run from 1 to %d (layer %d %s has %d)" % (L.LORA_MAX_RANK, layer, target, r))
            staged[(layer, target)] = (a.detach().to(self.device, torch.float32).contiguous(),
                                       b.detach().to(self.device, torch.float32).contiguous(), r, float(s))
        lib = L.lib()
        biggest = max(v[2] for v in staged.values())
        have = getattr(self, "lora_r_max", 0)
        want = have or (int(r_max) if r_max is not None else biggest)
        if biggest > want:  # (before anything changes)
            raise RuntimeError("QBits: the adapter's rank (%d) exceeds the r_max of woq_engine_lora_reserve (%d)" % (biggest, want))
        if have == 0:
            L.check(lib.woq_engine_lora_reserve(self._h, want))
            self.lora_r_max, self._lora_placed = want, set()
        before = self._lora_kinds(self._lora_placed)
        try:
            for (layer, target), (a, b, r, s) in staged.items():
                L.check(lib.woq_engine_set_lora(self._h, layer, L.LORA_TARGETS.index(target), a.data_ptr(), b.data_ptr(), r, s))
                self._lora_placed.add((layer, target))
            for layer, target in sorted(self._lora_placed - set(staged)):
                L.check(lib.woq_engine_set_lora(self._h, layer, L.LORA_TARGETS.index(target), None, None, 0, 0.0))
                self._lora_placed.discard((layer, target))
        finally:
            if self._lora_kinds(self._lora_placed) != before:
                self.captured = False  # (the native side dropped its graphs: other launches in the step)

    def clear_lora(self):
        """Removes every installed adapter target: the step and the prompt pass are the adapter-less ones again."""
        if getattr(self, "lora_r_max", 0) == 0:
            return
        L.check(L.lib().woq_engine_clear_lora(self._h))
        if self._lora_placed:
            self.captured = False
        self._lora_placed = set()

    @property
    def lora_on(self):
        """True while at least one projection of the engine carries an adapter."""
        return L.lib().woq_engine_lora_on(self._h) > 0

    def set_head(self, embed, final_norm, lm_head, cos=None, sin=None, attention_factor=1.0):
        """`cos` / `sin`: caller-built tables (build_rope_tables) and the attention factor they were multiplied by."""
        self.rope_attention_factor = float(attention_factor)
        embed = embed.to(self.device).contiguous()
        lm_head = lm_head.to(self.device).contiguous()
        final_norm = final_norm.to(self.device, torch.float32).contiguous()
        if cos is None:
            cos, sin = build_rope_tables(self.cfg.max_ctx, self.cfg.head_dim, self.cfg.rope_theta, self.device)
        L.check(L.lib().woq_engine_set_head(self._h, embed.data_ptr(), L.torch_dtype_code(embed.dtype),
                                            final_norm.data_ptr(), lm_head.data_ptr(),
                                            L.torch_dtype_code(lm_head.dtype), cos.data_ptr(), sin.data_ptr()))
        self._keep += [embed, lm_head, final_norm, cos, sin]
        self.head_tensors = dict(embed=embed, norm=final_norm, lm_head=lm_head)

    def reset(self, token=0, pos=0):
        self.token.fill_(int(token))
        self.pos.fill_(int(pos))

    def step(self, greedy=True):
        L.check(L.lib().woq_engine_step(self._h, int(greedy), L.stream_ptr()))

    # How a burst of decode steps is issued: "graph" = hipGraphLaunch of the captured step on the CALLER'S stream (no
    # host work per token: immune to host jitter), "eager" = `n` steps issued back to back by one native call
    # (`woq_engine_steps`; ~0.34 ms of launch calls per 7B token, ahead of the device). Same kernels, same device time:
    # 1.04 ms per Llama-2-7B token either way (profiles/r04ab_stream_mode_probe.txt). What made the replayed graph 12 %
    # slower through round 3 (1.17 ms) was not the graph but the way it was launched: on the engine's capture stream,
    # bracketed by `wait_stream` in both directions — after a cross-stream event wait every kernel boundary of the
    # following launches on that stream costs ~1 us more. Round 4 first switched to eager bursts (profiles/r04g_*), then
    # found the cause; the graph is launched on the current stream now. WOQ_ENGINE_LAUNCH=graph|eager picks the default.
    LAUNCH = os.environ.get("WOQ_ENGINE_LAUNCH", "graph")

    @property
    def launch(self):
        return getattr(self, "_launch", None) or type(self).LAUNCH

    @launch.setter
    def launch(self, mode):
        if mode not in ("eager", "graph"):
            raise ValueError("launch mode is 'eager' or 'graph'")
        self._launch = mode

    def capture(self, greedy=True):
        """Capture one token step into a hipGraph (on the engine's own stream)."""
        cur = torch.cuda.current_stream(self.device)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            L.check(L.lib().woq_engine_capture(self._h, int(greedy), L.stream_ptr()))
        cur.wait_stream(self._stream)
        self.captured = True
        self._captured_greedy = bool(greedy)

    def prepare_decode(self, greedy=True):
        """Whatever `replay` needs before a burst: a captured graph in "graph" mode, nothing in "eager" mode."""
        if self.launch == "graph" and not self.captured:
            self.capture(greedy=greedy)
        self._burst_greedy = bool(greedy)

    def run(self, n=1, greedy=True):
        """`n` decode steps issued eagerly by one native call (greedy: token / position chain on the device)."""
        L.check(L.lib().woq_engine_steps(self._h, int(n), int(greedy), L.stream_ptr()))

    def replay_graph(self, n=1):
        """Replay the captured hipGraph n times on the CURRENT stream (greedy chaining stays on the device). Only the
        capture needs a stream of its own; replaying on that stream behind `wait_stream` calls was what made graph
        replays ~1 us per kernel boundary slower than eager launches (profiles/r04ab_stream_mode_probe.txt)."""
        L.check(L.lib().woq_engine_replay(self._h, int(n), L.stream_ptr()))

    def replay_graph_round3(self, n=1):
        """MEASUREMENT ONLY: the graph replayed the way rounds 1-3 did it — on the engine's capture stream, bracketed by
        `wait_stream` in both directions. bench.py times it next to the other two so that the cause of round 3's 12 %
        stays on record in every line."""
        self._on_own_stream(lambda: L.check(L.lib().woq_engine_replay(self._h, int(n), L.stream_ptr())))

    def replay(self, n=1):
        """A burst of `n` decode steps of the kind last captured / prepared (greedy chaining stays on the device): the
        captured graph in "graph" mode, `run` in "eager" mode (same kernels, same results — the tests hold graph replays
        and eager steps to bit-identical tokens)."""
        if self.launch == "graph":
            return self.replay_graph(n)
        self.run(n, greedy=getattr(self, "_burst_greedy", getattr(self, "_captured_greedy", True)))

    def token_log(self):
        """int32 view [max_ctx + 1] of the engine's token log: slot p = the greedy token of the step that fed position
        p. After `replay(k)` from position p0 the k new tokens are token_log()[p0 : p0 + k] — one host read."""
        return _device_view(L.lib().woq_engine_token_log_ptr(self._h), (self.cfg.max_ctx + 1,), self.device, "<i4")

    def kv_shift(self, n_keep, n_discard, n_cached, seq=0, move_pos=True):
        """Rolling KV cache (woq_engine_kv_shift): drop positions [n_keep, n_keep + n_discard) of sequence `seq`, whose
        cache holds `n_cached` rows, and move the later rows down in place, K rows rotated back by the angle of
        `n_discard`. `move_pos` (sequence 0): the device position and the `discarded` word follow, so the burst issued
        next feeds position n_cached - n_discard. Issued on the current stream, the one bursts run on: no
        synchronisation, no read-back. Every shift re-rounds the moved K rows to the cache type."""
        self._check_shiftable()
        L.check(L.lib().woq_engine_kv_shift(self._h, int(seq), int(n_keep), int(n_discard), int(n_cached),
                                            int(bool(move_pos)), L.stream_ptr()))

    def discarded(self):
        """Positions the rolling cache has dropped in the running request (one host synchronisation): the sampled
        tail's Philox counter is position + discarded."""
        return int(_device_view(L.lib().woq_engine_discarded_ptr(self._h), (1,), self.device, "<i4").item())

    def set_discarded(self, value=0):
        """discarded = value, stream-ordered (a request starts from 0)."""
        L.check(L.lib().woq_engine_discarded_set(self._h, int(value), L.stream_ptr()))

    def _check_shiftable(self):
        """The K re-rotation multiplies by a table row: right for any per-dimension frequency, wrong for tables scaled
        by an attention factor (yarn), whose rows are not rotations."""
        if getattr(self, "rope_attention_factor", 1.0) != 1.0:
            raise RuntimeError("QBits: the rolling KV cache does not combine with RoPE tables scaled by an attention "
                               "factor (%g: yarn rope scaling)" % self.rope_attention_factor)

    def _request_geometry(self, n_prompt, max_new_tokens, streaming):
        """(ctx_size, n_keep, n_discard) of a request with a rolling cache, (None, 0, 0) of one without, which has to
        fit the cache as a whole."""
        if streaming is not None:
            self._check_shiftable()
            return streaming.resolve(self.cfg.max_ctx, n_prompt)
        if n_prompt + max_new_tokens > self.cfg.max_ctx:  # the kernels index the KV cache by position, unchecked
            raise RuntimeError("QBits: prompt (%d) + max_new_tokens (%d) exceeds the engine's max_ctx (%d)"
                               % (n_prompt, max_new_tokens, self.cfg.max_ctx))
        return None, 0, 0

    def uses_xq(self):
        """True when the decode step's kernels hand activations over as XQ limb blocks (csrc/woq_xq.h)."""
        return bool(L.lib().woq_engine_uses_xq(self._h))

    def phase(self, layer, phase, greedy=True):
        L.check(L.lib().woq_engine_phase(self._h, int(layer), int(phase), int(greedy), L.stream_ptr()))

    def _on_own_stream(self, fn):
        """Run `fn` with the engine's own stream current (captures are not allowed on the legacy default stream)."""
        cur = torch.cuda.current_stream(self.device)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            out = fn()
        cur.wait_stream(self._stream)
        return out

    def set_time_eager(self, on=True):
        """time_gemv / time_twin: passes issued eagerly back to back on the current stream (default) or as a replayed
        graph on the engine's own stream (round 3's measure; that stream sits behind a `wait_stream`, which costs every
        kernel boundary ~1 us — see LAUNCH)."""
        L.check(L.lib().woq_engine_set_time_eager(self._h, int(bool(on))))
        self._time_eager = bool(on)

    def _timed_call(self, fn):
        """Timing helpers: eagerly issued passes need no stream of their own and must not sit behind a cross-stream wait;
        captured ones cannot run on the legacy default stream."""
        return fn() if getattr(self, "_time_eager", True) else self._on_own_stream(fn)

    def time_gemv(self, reps=1, mask=15):
        """(total ms, algorithmic bytes per pass, launches per pass) of `reps` replays of a captured pass over every
        layer's GEMV launches in the decode step's own forms; mask picks projections (bit 0 qkv, 1 o, 2 gate/up, 3 down)."""
        ms, by, n = ctypes.c_float(), ctypes.c_double(), ctypes.c_int()
        self._timed_call(lambda: L.check(L.lib().woq_engine_time_gemv_mask(
            self._h, int(mask), reps, L.stream_ptr(), ctypes.byref(ms), ctypes.byref(by), ctypes.byref(n))))
        return ms.value, by.value, n.value

    def time_twin(self, mode, reps=1):
        """Total ms of `reps` replays of a captured pass over every layer's 4 GEMV launches with the arithmetic taken
        out: mode 0 = load-only twins over the engine's own blobs, mode 1 = empty kernels on the same grids (bench.py
        roofline.ceiling)."""
        ms = ctypes.c_float()
        self._timed_call(lambda: L.check(L.lib().woq_engine_time_twin(
            self._h, int(mode), int(reps), L.stream_ptr(), ctypes.byref(ms))))
        return ms.value

    def time_prefill_gemm(self, layer, n_rows, reps=3):
        """(gemm_ms, call_ms) of the engine's own gate/up GEMM call over the `n_rows` rows a preceding prefill left in
        the residual stream: the MFMA GEMM kernel alone, and pack pass + GEMM (bench.py prefill.dominant_gemm)."""
        g, c = ctypes.c_float(), ctypes.c_float()
        L.check(L.lib().woq_engine_time_prefill_gemm(self._h, int(layer), int(n_rows), int(reps), L.stream_ptr(),
                                                     ctypes.byref(g), ctypes.byref(c)))
        return g.value, c.value

    # ---- tensor parallel: host-driven collectives between sub-blocks (RCCL via torch.distributed) ----
    def step_tp(self, group=None, greedy=True):
        """One token with the row-parallel partial sums all-reduced after o_proj and down_proj.
        One RCCL all-reduce (sum, fp32 [hidden]) per sub-block — SURVEY.md §8(e)."""
        import torch.distributed as dist

        for l in range(self.cfg.layers):
            self.phase(l, 0, greedy)
            dist.all_reduce(self.hidden, group=group)
            self.phase(l, 1, greedy)
            dist.all_reduce(self.hidden, group=group)
        self.phase(0, 2, greedy)

    def prefill(self, tokens, start_pos=0, greedy=True):
        """Prompt pass: `tokens` int [T] or [n_seq, T] at positions start_pos.. of each sequence's KV cache (all
        linears as MFMA GEMMs over n_seq*T rows, causal attention over the cache). Returns the last-position logits
        fp32 [n_seq, vocab] (a view of engine memory, valid until the next prefill). Sequence 0 is the one
        step()/replay() continue: with greedy its next token and position are already in place."""
        t = torch.as_tensor(tokens, dtype=torch.int32, device=self.device)
        if t.dim() == 1:
            t = t.unsqueeze(0)
        t = t.contiguous()
        n_seq, T = t.shape
        L.check(L.lib().woq_engine_prefill(self._h, t.data_ptr(), int(n_seq), int(T), int(start_pos), int(greedy),
                                           L.stream_ptr()))
        ptr = L.lib().woq_engine_prefill_logits_ptr(self._h)
        return _device_view(ptr, (n_seq, self.cfg.vocab), self.device)

    # ---- decode attention regime -----------------------------------------------------------------------------
    LONG_CTX = 480  # cached positions beyond which the sliced decode attention wins (r04l, V runs double-buffered: 448 -> 0.617 vs 0.631, 512 -> 0.635 vs 0.634, 640 -> 0.661 vs 0.634). Round 4 (eager bursts, V rows of two runs prefetched; Llama-2-7B shape, 16 layers, ms per token, one workgroup per head inside the fused launch vs context slices + combine: 256 -> 0.593 vs 0.618, 384 -> 0.615 vs 0.621, 512 -> 0.644 vs 0.635; profiles/r04k_*). Round 1 had measured the crossover near 256 on the two-launch form

    FUSED_SLICED_CTX = 192  # ... and where slices INSIDE the fused launch (self-merging, round 6) start to pay: 7B shape,
    # 16 layers, ms per token, 1 vs 4 slices (profiles/r06t_*): 96 -> 0.544-0.549 vs 0.558, 160 -> 0.557-0.562 vs
    # 0.561, 224 -> 0.570-0.574 vs 0.564, 320 -> 0.588 vs 0.570, 512 -> 0.625 vs 0.580

    def set_attn_splits(self, n):
        """1 = one workgroup per head, n > 1 = n context slices per head + combine. Invalidates a captured graph."""
        if int(n) != L.lib().woq_engine_attn_splits(self._h):
            L.check(L.lib().woq_engine_set_attn_splits(self._h, int(n)))
            self.captured = False

    GROUPED_CTX = 10240  # cached positions from which the grouped-query (matrix-core) slices are used where they apply
    # (a launch of their own: 186-247 registers, they cannot share a kernel with the strips). Round 6, Mistral-7B shape,
    # fp8 cache, 16 layers, ms per token, 16 per-head slices inside the fused launch vs grouped slices (both forms
    # merge among themselves; profiles/r06t_*): 4096 -> 0.644 vs 0.707, 8192 -> 0.720 vs 0.745, 16384 -> 0.850 vs 0.789

    def set_attn_grouped(self, on):
        """Sliced regime only: one workgroup per (kv head, slice) for all the query heads of the group (head_dim 128,
        2 / 4 / 8 query heads per kv head, fp16 / fp8 cache; ignored elsewhere). Invalidates a captured graph."""
        if bool(on) != bool(L.lib().woq_engine_attn_grouped(self._h)):
            L.check(L.lib().woq_engine_set_attn_grouped(self._h, int(bool(on))))
            self.captured = False

    GROUPED_CHUNK = 256  # positions per slice of the grouped form's position-independent geometry (two 32-position sub-tiles per wave, both requested before the position is read)

    def set_attn_chunk(self, chunk):
        """Grouped form: `chunk` > 0 = slice s owns the absolute positions [s * chunk, (s + 1) * chunk) whatever the
        current position is (K / V requested before it is read); 0 = slices cut evenly from the current span.
        Invalidates a captured graph."""
        if int(chunk) != L.lib().woq_engine_attn_chunk(self._h):
            L.check(L.lib().woq_engine_set_attn_chunk(self._h, int(chunk)))
            self.captured = False

    def set_tp_options(self, xq=True, fused_push=True):
        """Tensor-parallel decode with a device communicator: `xq` = the XQ decode kernels with an XQ-emitting
        all-reduce kernel (off: the fp32-activation kernels), `fused_push` = o_proj / down_proj push their partial sums
        into the peers' inboxes from their own epilogue (off: the all-reduce kernel pushes; bit-identical results).
        Invalidates a captured graph."""
        L.check(L.lib().woq_engine_set_tp_options(self._h, int(bool(xq)), int(bool(fused_push))))
        self.captured = False

    def set_fuse_attn(self, on):
        """Decode step: qkv GEMV + attention as one launch where the shape allows (csrc/woq_gemv_attn.hip; default
        on). Invalidates a captured graph."""
        L.check(L.lib().woq_engine_set_fuse_attn(self._h, int(bool(on))))
        self.captured = False

    def uses_fused_attn(self):
        """True when the next step / capture runs the fused qkv + attention launch."""
        return bool(L.lib().woq_engine_fuse_attn(self._h))

    def status(self):
        """Sticky device-side status of the decode step, 0 = fine. bit 0: an attention workgroup of the fused launch
        gave up waiting for its head's q / k / v; bit 1: a step found its position at or beyond max_ctx and ran at
        max_ctx - 1 instead (its outputs are meaningless, memory was not touched out of bounds)."""
        return int(L.lib().woq_engine_status(self._h, L.stream_ptr()))

    def clear_status(self):
        """Reset the sticky status (after the caller dealt with what it reported)."""
        L.check(L.lib().woq_engine_clear_status(self._h, L.stream_ptr()))

    def attn_plan(self, splits=0, grouped=-1):
        """How the next step / capture runs its attention (layer 0): a dict of form (L.ATTN_*), merge (L.ATTN_MERGE_*),
        slices, chunk_fixed, ... (L.engine_attn_plan); `splits` > 0 / `grouped` >= 0 ask about another slice count /
        grouped request without changing the engine."""
        return L.engine_attn_plan(self._h, splits, grouped)

    def _grouped_applies(self):
        """True when a sliced context asked to run grouped would run the grouped-query matrix-core form."""
        return self.attn_plan(splits=2, grouped=1)["form"] == L.ATTN_GROUPED

    def tune_attn_for(self, positions):
        """Pick the regime for a context of `positions` cached tokens (host-side hint: the position lives on the
        device): slices = enough workgroups to fill the chip, each at least 64 positions; from GROUPED_CTX on,
        grouped-query shapes take 256-position slices of the matrix-core form."""
        grouped = positions >= self.GROUPED_CTX and self._grouped_applies()
        self.set_attn_grouped(grouped)
        # position-independent slices: not with a sliding window (the slices move with the position), and only for
        # the fp8 cache, whose kernel keeps raw bytes in registers and fits two workgroups on a CU — the fp16 form
        # holds one (272 registers), and ceil(positions / 256) x kv_heads workgroups would then run a second round
        # measured slower (+2.5 us per layer, profiles/r04d_*): opt-in through WOQ_ATTN_FIXED_CHUNK=1 (parity:
        # test_grouped_attention_fixed_chunk_slices_vs_oracle drives the same geometry through set_attn_chunk)
        fixed = (os.environ.get("WOQ_ATTN_FIXED_CHUNK", "0") not in ("", "0") and grouped and not self.cfg.reserved[2]
                 and self.cfg.kv_dtype == L.FP8_E4M3)
        self.set_attn_chunk(self.GROUPED_CHUNK if fixed else 0)
        fused_sliced = not grouped and self.uses_fused_attn_sliced()
        if positions <= (self.FUSED_SLICED_CTX if fused_sliced else self.LONG_CTX):
            self.set_attn_splits(1)
        elif fixed:  # enough fixed slices to cover `positions`; the last one takes what lies beyond
            self.set_attn_splits(max(2, min(64, -(-positions // self.GROUPED_CHUNK))))
        elif grouped:  # (round 6, slices merging among themselves: 8k -> 0.765 / 0.732 / 0.739 ms for 16 / 24 / 32 slices)
            self.set_attn_splits(max(2, min(32, positions // 320)))
        elif fused_sliced:
            # slices as attention workgroups of the fused qkv launch, merging among themselves (round 6): fewer, longer
            # slices than launches of their own want (profiles/r06t_*, 16 layers, ms per token) — 7B shape 512: 0.580 /
            # 0.577 for 4 / 8 (0.594 for 2), 2048: 0.657 / 0.659 / 0.668 for 8 / 12 / 16 (0.707 for 4); Mistral shape
            # 2048: 0.633 / 0.628 for 8 / 16, 4096: 0.689 / 0.670, 8192: 0.785 / 0.751 for 12 / 16
            self.set_attn_splits(4 if positions < 1024 else 8 if positions < 3072 else 16)
        else:
            self.set_attn_splits(max(2, min(32, 1024 // max(1, self.cfg.heads), positions // 64)))

    def uses_fused_attn_sliced(self):
        """True when a sliced context would ride in the fused qkv launch (the engine's plan at two slices)."""
        return self.attn_plan(splits=2)["form"] == L.ATTN_FUSED

    def kv_cache(self, which="k"):
        """The engine's K or V cache as a torch view [max_batch, layers, max_ctx, kv_heads, head_dim] (no copy)."""
        c = self.cfg
        shape = (self.max_batch, c.layers, c.max_ctx, c.kv_heads, c.head_dim)
        ptr = L.lib().woq_engine_kv_cache_ptr(self._h, 0 if which == "k" else 1)
        code = c.kv_dtype
        if code == L.FP8_E4M3:
            return _device_view(ptr, shape, self.device, "|u1").view(torch.float8_e4m3fn)
        t = _device_view(ptr, shape, self.device, "<f2")
        return t if code == L.F16 else t.view(torch.bfloat16)

    # ---- tensor parallel through the engine's all-reduce seam (woq_engine_set_allreduce) --------------------------
    def bind_allreduce(self, group=None):
        """Let the NATIVE step / prompt pass call back into torch.distributed after o_proj and down_proj: the
        callback wraps the engine's fp32 buffer as a tensor view and issues `dist.all_reduce` (backend "nccl" = RCCL
        over xGMI) on the current stream. Needed for `prefill` under TP (the host-driven `step_tp` splits only the
        decode step); not graph-capturable."""
        import torch.distributed as dist

        def _cb(_user, buf, count, _stream):
            try:
                dist.all_reduce(_device_view(buf, (int(count),), self.device), group=group)
                return 0
            except Exception:  # pragma: no cover - surfaces as "all-reduce callback failed" from the C side
                return 1

        self._allreduce_cb = L.ALLREDUCE_FN(_cb)  # keep the ctypes thunk alive
        L.check(L.lib().woq_engine_set_allreduce(self._h, self._allreduce_cb, None))
        self.captured = False

    def bind_comm(self, comm, vocab_offset=0):
        """Tensor parallel with the exchange ON THE DEVICE (runtime/comm.py DeviceComm): the native step then issues
        the two all-reduce kernels per layer and the greedy-token exchange itself, so `capture()` / `replay()` cover a
        whole tensor-parallel token. `vocab_offset` = first vocabulary row of this rank's lm_head shard. The prompt
        pass keeps a bound RCCL callback when there is one (bandwidth-bound rows), else it uses the comm in pieces."""
        h = comm.handle if comm is not None else None
        L.check(L.lib().woq_engine_set_comm(self._h, h, int(vocab_offset)))
        self._comm = comm
        self.captured = False

    def unbind_allreduce(self):
        L.check(L.lib().woq_engine_set_allreduce(self._h, ctypes.cast(None, L.ALLREDUCE_FN), None))
        self._allreduce_cb = None

    # ---- native sampler: the next token of a chaining step chosen by csrc/woq_sample.hip ---------------------------
    NATIVE_TOP_K_MAX = 1024

    def native_sampler_supports(self, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0,
                                presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, logit_bias=None, guide=None):
        """True when `set_sampler` takes this request (the checks of csrc/woq_sample.hip `sampler_config_problem` and
        `sampler_controls_problem`): one GPU (a tensor-parallel head is vocab-sharded); a positive penalty alone;
        sampling with a positive finite temperature and 1 <= top_k <= 1024 with any top_p, or top_k = 0 with top_p = 1;
        finite presence / frequency penalties, min_p in [0, 1] (> 0 only when sampling), at most 1024 bias entries
        inside the vocabulary, each finite or -inf; `guide` (a TokenGuide, `set_guide`) with a table over this
        vocabulary. Everything else keeps `iter_sampled` + `DeviceSampler`, which answers or raises as it always did
        (it has no guide)."""
        if self.cfg.tp_size > 1 or self._comm is not None or self._allreduce_cb is not None:
            return False
        if guide is not None and guide.table.shape[1] != self.cfg.vocab:
            return False
        if not float(1.0 if repetition_penalty is None else repetition_penalty) > 0.0:
            return False
        pres, freq, min_p, bias = _controls(presence_penalty, frequency_penalty, min_p, logit_bias)
        if not (math.isfinite(pres) and math.isfinite(freq) and 0.0 <= min_p <= 1.0):
            return False
        if len(bias) > L.SAMPLER_MAX_BIAS or any(not 0 <= k < self.cfg.vocab or v != v or v == float("inf")
                                                 for k, v in bias.items()):
            return False
        if not do_sample:
            return min_p == 0.0
        temperature = float(1.0 if temperature is None else temperature)
        if not (temperature > 0.0 and math.isfinite(temperature)):
            return False
        top_k, top_p = int(top_k or 0), float(1.0 if top_p is None else top_p)
        if top_k < 0 or top_k > self.NATIVE_TOP_K_MAX or not 0.0 <= top_p <= 1.0:
            return False
        return top_k > 0 or top_p >= 1.0

    def set_sampler(self, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seed=0,
                    presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, logit_bias=None):
        """Install (or re-parameterise) the native sampler: from now on every chaining step — the prompt pass's tail,
        `step`, `run`, `replay` — picks its token with Hugging Face's repetition penalty / temperature / top-k / top-p in
        HF's order and a Philox draw keyed by (`seed`, position). Installing drops a captured graph; changing the
        parameters of an installed sampler does not (the kernel reads them from device memory).
        `presence_penalty` / `frequency_penalty` (OpenAI's, over the tokens generated in this request), `min_p` (HF's
        MinPLogitsWarper) and `logit_bias` ({token id: value}, -inf = a ban, added ahead of the penalties): the sampler
        controls, installed only when one of them is not neutral — one more launch per step (a pre-pass over the
        vocabulary). Installing or removing them drops a captured graph; changing their values does not."""
        if do_sample and float(1.0 if temperature is None else temperature) <= 0:
            raise ValueError("`temperature` has to be a strictly positive float when sampling")
        cfg = L.sampler_config(do_sample, temperature, top_k, top_p, repetition_penalty, seed)
        L.check(L.lib().woq_engine_set_sampler(self._h, ctypes.byref(cfg)))
        self._guide_owns_sampler = False  # the caller's sampler from here on: clear_guide leaves it
        was_installed = self.sampler_installed
        if not self.sampler_installed:
            self.captured = False
        self.sampler_installed = True
        pres, freq, min_p, bias = _controls(presence_penalty, frequency_penalty, min_p, logit_bias)
        if pres != 0.0 or freq != 0.0 or min_p != 0.0 or bias:
            ctl, ids, vals = L.sampler_controls(pres, freq, min_p, bias)
            if L.lib().woq_engine_set_sampler_controls(self._h, ctypes.byref(ctl), ids, vals) != 0:
                why = L.lib().woq_last_error().decode()
                if not was_installed:  # refused controls leave no half-installed sampler behind
                    self.clear_sampler()
                raise RuntimeError(why)
            if not self.controls_installed:
                self.captured = False
            self.controls_installed = True
        elif self.controls_installed:
            L.check(L.lib().woq_engine_set_sampler_controls(self._h, None, None, None))
            self.captured = False
            self.controls_installed = False

    def clear_sampler(self):
        """Back to the plain greedy tail (drops a graph captured with the sampler; removes the controls and the guide
        too)."""
        L.check(L.lib().woq_engine_set_sampler(self._h, None))
        if self.sampler_installed:
            self.captured = False
        self.sampler_installed = self.controls_installed = self.guide_installed = False
        self._guide, self._guide_prefix, self._guide_owns_sampler = None, (), False

    # ---- token guide: constrained decoding (runtime/guide.py builds the tables) --------------------------------------
    def set_guide(self, guide, prefix_ids=()):
        """Install a `TokenGuide` (or replace the installed one): from now on every chaining step bans the ids its
        state's row bans before the pick and moves the state on the pick, on the device. Installs a greedy sampler when
        none is installed (`clear_guide` removes that one again). Installing drops a captured graph; replacing a guide
        by another, and `guide_reset`, do not (the kernels read table and state from device memory). The state starts
        at `guide.walk(prefix_ids)`; `iter_generate` starts every request at the guide's state after its prompt
        (`guide.prompt_state`) followed by `prefix_ids`."""
        if guide.table.shape[1] != self.cfg.vocab:
            raise RuntimeError("QBits: the guide's table is over %d ids, the engine's vocabulary has %d"
                               % (guide.table.shape[1], self.cfg.vocab))
        prefix = tuple(int(t) for t in prefix_ids)
        state = guide.walk(prefix)
        owns = not self.sampler_installed
        if owns:
            self.set_sampler()
        table = torch.from_numpy(guide.table.view(np.int16)).to(self.device)
        if L.lib().woq_engine_set_guide(self._h, table.data_ptr(), guide.n_states, state) != 0:  # (synchronises)
            why = L.lib().woq_last_error().decode()
            if owns:
                self.clear_sampler()
            raise RuntimeError(why)
        if not self.guide_installed:
            self.captured = False
        self.guide_installed = True
        self._guide, self._guide_prefix = guide, prefix
        self._guide_owns_sampler = owns or self._guide_owns_sampler

    def clear_guide(self):
        """Remove the guide (drops a graph captured with it), and the greedy sampler `set_guide` installed for it."""
        if self._guide_owns_sampler:
            self.clear_sampler()
            return
        L.check(L.lib().woq_engine_set_guide(self._h, None, 0, 0))
        if self.guide_installed:
            self.captured = False
        self.guide_installed = False
        self._guide, self._guide_prefix = None, ()

    def guide_reset(self, state=None):
        """The guide's state <- `state` (default: after `prefix_ids`), stream-ordered; a captured graph stays valid."""
        if state is None:
            state = self._guide.walk(self._guide_prefix)
        L.check(L.lib().woq_engine_guide_reset(self._h, int(state), L.stream_ptr()))

    def guide_state(self):
        """The guide's current state (one host synchronisation)."""
        ptr = L.lib().woq_engine_guide_state_ptr(self._h)
        if not ptr or not self.guide_installed:
            raise RuntimeError("QBits: no token guide installed")
        return int(_device_view(ptr, (1,), self.device, "<i4").item())

    def mark_counts(self, token_ids, clear=True):
        """The frequency / presence penalties' history: count `token_ids` (after zeroing the table when `clear`). The
        sampled tail counts every token it picks itself; `iter_generate` starts a request from zero."""
        t = torch.as_tensor(token_ids, dtype=torch.int32, device=self.device).reshape(-1).contiguous()
        L.check(L.lib().woq_engine_sampler_counts(self._h, t.data_ptr() if t.numel() else None, int(t.numel()),
                                                  int(bool(clear)), L.stream_ptr()))

    def token_counts(self):
        """uint32-as-int32 view [vocab] of how often each id was generated in this request."""
        return _device_view(L.lib().woq_engine_sampler_count_ptr(self._h), (self.cfg.vocab,), self.device, "<i4")

    def mark_seen(self, token_ids, clear=True):
        """The repetition penalty's history: set the bits of `token_ids` (after emptying the set when `clear`)."""
        t = torch.as_tensor(token_ids, dtype=torch.int32, device=self.device).reshape(-1).contiguous()
        L.check(L.lib().woq_engine_sampler_seen(self._h, t.data_ptr() if t.numel() else None, int(t.numel()),
                                                int(bool(clear)), L.stream_ptr()))

    def seen_bits(self):
        """uint32-as-int32 view [(vocab + 31) / 32] of the history bit set (bit i & 31 of word i >> 5 = id i)."""
        return _device_view(L.lib().woq_engine_sampler_seen_ptr(self._h), ((self.cfg.vocab + 31) // 32,), self.device,
                            "<i4")

    # ---- log-probability record: csrc/woq_logprob.hip after every chaining pick -------------------------------------
    LOGPROB_TOP = L.LOGPROB_TOP

    def set_logprobs(self, on=True):
        """Record, after every chaining pick (the prompt pass's tail, `step`, `run`, `replay`), the log-probability of
        the picked token and the 20 most likely ids under the RAW model distribution (log_softmax of the fp32 logits,
        before penalty / temperature / top-k / top-p) into `logprob_log()`. Switching on or off drops a captured graph.
        Raises on a tensor-parallel engine (the head is vocab-sharded)."""
        L.check(L.lib().woq_engine_set_logprobs(self._h, int(bool(on))))
        if bool(on) != self.logprobs_on:
            self.captured = False
        self.logprobs_on = bool(on)

    def clear_logprobs(self):
        """Recording off: the step is the one it was before `set_logprobs` (the logs keep their contents)."""
        self.set_logprobs(False)

    def logprob_log(self):
        """(chosen fp32 [max_ctx + 1], top_id int32 [max_ctx + 1, 20], top_lp fp32 [max_ctx + 1, 20]): views of the
        engine's logs, row p = the record of the step that fed position p (the index of `token_log`). Top ids are
        ordered by (logit descending, id ascending) and padded with -1 / -inf."""
        rows, get = self.cfg.max_ctx + 1, L.lib().woq_engine_logprob_ptr
        if not get(self._h, 0):
            raise RuntimeError("QBits: no log-probability log before the first set_logprobs()")
        return (_device_view(get(self._h, 0), (rows,), self.device),
                _device_view(get(self._h, 1), (rows, self.LOGPROB_TOP), self.device, "<i4"),
                _device_view(get(self._h, 2), (rows, self.LOGPROB_TOP), self.device))

    # ---- scoring a given text: csrc/woq_score.hip over the prompt pass's rows ----------------------------------------
    def prefill_scored(self, tokens, targets, start_pos=0, greedy=False):
        """`prefill` of one sequence that also writes rows start_pos .. of `logprob_log()`: row start_pos + t holds the
        raw distribution after position start_pos + t, `chosen` = the log-probability of targets[t] (the id at position
        start_pos + t + 1; an id outside the vocabulary gives NaN). greedy=True leaves the last row to the chaining tail.
        Needs the logs (a `set_logprobs(True)` at some earlier point); recording need not be on."""
        t = torch.as_tensor(tokens, dtype=torch.int32, device=self.device).reshape(-1).contiguous()
        g = torch.as_tensor(targets, dtype=torch.int32, device=self.device).reshape(-1).contiguous()
        if g.numel() != t.numel():
            raise RuntimeError("QBits: prefill_scored takes one target per token")
        L.check(L.lib().woq_engine_prefill_scored(self._h, t.data_ptr(), int(t.numel()), int(start_pos), g.data_ptr(),
                                                  int(greedy), L.stream_ptr()))
        ptr = L.lib().woq_engine_prefill_logits_ptr(self._h)
        return _device_view(ptr, (1, self.cfg.vocab), self.device)

    def prefill_rows(self, rows):
        """fp32 view [rows, hidden] of the residual stream the last prompt pass left (before the final norm); for tests."""
        return _device_view(L.lib().woq_engine_prefill_rows_ptr(self._h), (int(rows), self.cfg.hidden), self.device)

    def score(self, ids, chunk=2048, logprobs=0):
        """Log-probabilities the model assigns to a given text -> `(token_lps, top)`: token_lps[i] = log P(ids[i + 1] |
        ids[:i + 1]) (len(ids) - 1 floats), top[i] = `logprobs` (0..20) pairs `(id, log-probability)` of the most likely
        ids at that position. The text runs through `prefill_scored` in chunks of `chunk` tokens; one device-to-host
        copy at the end. Leaves `logprobs_on` and an installed sampler as they were."""
        ids = [int(t) for t in ids]
        n, n_top = len(ids), request._top_count(logprobs)
        if n < 2:
            raise RuntimeError("QBits: scoring needs at least 2 tokens (got %d)" % n)
        if n > self.cfg.max_ctx:
            raise RuntimeError("QBits: text (%d tokens) exceeds the engine's max_ctx (%d)" % (n, self.cfg.max_ctx))
        if not L.lib().woq_engine_logprob_ptr(self._h, 0):  # allocate the logs, leave recording as it was
            before = self.logprobs_on
            self.set_logprobs(True)
            self.set_logprobs(before)
        targets = ids[1:] + [-1]  # the last position has no next token: its row is dropped
        for s0 in range(0, n, int(chunk)):
            self.prefill_scored(ids[s0:s0 + chunk], targets[s0:s0 + chunk], start_pos=s0, greedy=False)
        _, lps, top = request._records(self, 0, n - 1, n_top)
        return lps, top

    def perplexity(self, ids, chunk=2048):
        """exp(-mean(log P(ids[i + 1] | ids[:i + 1]))) of a text, the mean taken on the host in float64."""
        lps, _ = self.score(ids, chunk=chunk)
        return math.exp(-math.fsum(lps) / len(lps))

    # ---- a whole request: runtime/request.py drives the engine --------------------------------------------------------
    def iter_generate(self, prompt_ids, max_new_tokens, chunk=2048, burst=16, eos=(), logprobs=None, streaming=None):
        """`request.iter_generate` over this engine: prompt pass + bursts of chained steps, yielding each burst's tokens."""
        return request.iter_generate(self, prompt_ids, max_new_tokens, chunk, burst, eos, logprobs, streaming)

    def generate(self, prompt_ids, max_new_tokens, chunk=2048, burst=16, sampler=None, logprobs=None, streaming=None):
        """`request.generate` over this engine: `iter_generate` to the end -> the new tokens."""
        return request.generate(self, prompt_ids, max_new_tokens, chunk, burst, sampler, logprobs, streaming)


def _device_view(ptr, shape, device, typestr="<f4"):
    """torch view of engine-owned device memory (no copy) through the CUDA array interface."""

    class _Raw:
        pass

    raw = _Raw()
    raw.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(raw, device=device)


def synth_llama_weights(engine, hidden, inter, heads, kv_heads, head_dim, layers, vocab, group=128, sym=True,
                        scale_dtype="fp16", seed=1234, model_dtype=torch.float16, embed_vocab=None,
                        shared_seed=None, weight_dtype="int4_clip", compute_dtype="fp32", act_order=False):
    """Synthetic random-init quantised Llama-shaped weights built directly on the device (no checkpoint, no
    network): int4 values uniform in [-8,7], scales ~ 0.02-ish/7 so dequantised weights look like N(0, 0.02^2),
    norms 1 + N(0, 0.02^2), embeddings N(0, 0.02^2). Returns the list of blobs (kept alive by the engine).
    Tensor-parallel shards: pass the PER-RANK heads / kv_heads / inter / vocab (what the engine was built with) and
    `embed_vocab` = the full vocabulary (the embedding table is replicated, lm_head is the rank's rows), and
    `shared_seed` = one seed for all ranks: the replicated tensors (norm weights, embedding) are drawn from it so
    that every rank holds the same copy, while `seed` (per rank) draws the shards.
    `weight_dtype` "nf4" / "fp4_e2m1" / "fp4_e2m1_bnb": uniform table codes 0..15 instead of int4 values (symmetric),
    scales sized so that the dequantised weights keep the same spread; `compute_dtype` is recorded in the blobs (nf4
    decodes with three digit planes at "fp32", two at "bf16" / "fp16" / "int8": csrc/woq_gemv_common.h)."""
    table = weight_dtype in TABLE_WEIGHT_DTYPES
    fp8 = weight_dtype in FP8_WEIGHT_DTYPES
    if (table or fp8) and not sym:
        raise RuntimeError("QBits: float weight types are symmetric")
    dev = engine.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    gs = g  # replicated tensors
    if shared_seed is not None:
        gs = torch.Generator(device=dev)
        gs.manual_seed(shared_seed)

    def rand_q(k, n):
        kg = (k + (k if group == -1 else group) - 1) // (k if group == -1 else group)
        if fp8:  # fp8 codes of N(0, 64^2) values (finite by construction), scales so that the weights look like N(0, 0.02^2)
            v = (64.0 * torch.randn(k, n, generator=g, device=dev)).clamp_(-400.0, 400.0)
            q = v.to(FP8_WEIGHT_DTYPES[weight_dtype]).view(torch.int8)
            s = (0.5 + torch.rand(kg, n, generator=g, device=dev)) * (0.02 / 64.0)
            return q, s, None
        q = torch.randint(0 if table else -8, 16 if table else 8, (k, n), generator=g, device=dev, dtype=torch.int8)
        s = (0.5 + torch.rand(kg, n, generator=g, device=dev)) * (0.02 / (TABLE_WEIGHT_DTYPES[weight_dtype] if table else 4.0))
        z = None if sym else torch.randint(-8, 8, (kg, n), generator=g, device=dev, dtype=torch.int8)
        return q, s, z

    def pack(q, s, z):
        # act_order: a GPTQ desc_act blob — every projection carries a random group assignment of its K rows (q / k / v and
        # gate / up are fused, so each fused blob has one, the way a GPTQ run leaves them); the rows are synthetic, so
        # "regrouped order" is whatever they are in
        k = q.shape[0]
        gsz = k if group == -1 else group
        g_idx = torch.empty(0, dtype=torch.int32)
        if act_order:
            g_idx = (torch.randperm(k, generator=g, device=dev) // gsz).to(torch.int32)
        return qbits.repack_quantized_weight(q, s, z if z is not None else torch.empty(0, dtype=torch.int8),
                                             g_idx, weight_dtype, scale_dtype, compute_dtype, z is not None, group)

    qkv_n = (heads + 2 * kv_heads) * head_dim
    for l in range(layers):
        q, s, z = rand_q(hidden, qkv_n)
        qkv_blob = pack(q, s, z)
        q, s, z = rand_q(heads * head_dim, hidden)
        o_blob = pack(q, s, z)
        gq, gsc, gz = rand_q(hidden, inter)
        uq, usc, uz = rand_q(hidden, inter)
        gu_blob = pack(fuse_gate_up(gq, uq), fuse_gate_up(gsc, usc), None if gz is None else fuse_gate_up(gz, uz))
        q, s, z = rand_q(inter, hidden)
        down_blob = pack(q, s, z)
        ln1 = 1 + 0.02 * torch.randn(hidden, generator=gs, device=dev)
        ln2 = 1 + 0.02 * torch.randn(hidden, generator=gs, device=dev)
        engine.set_layer(l, qkv_blob, o_blob, gu_blob, down_blob, ln1, ln2)
        del q, s, z, gq, gsc, gz, uq, usc, uz
    embed = (0.02 * torch.randn(embed_vocab or vocab, hidden, generator=gs, device=dev)).to(model_dtype)
    lm_head = (0.02 * torch.randn(vocab, hidden, generator=g, device=dev)).to(model_dtype)
    norm = 1 + 0.02 * torch.randn(hidden, generator=gs, device=dev)
    engine.set_head(embed, norm, lm_head)
    return engine


# ---- fused decode engine from a quantised HF model (the `ipex.optimize_transformers` analogue) ---------------------
# 4-bit table weight types the engine takes (round 4) -> the rms of their table over uniform codes (synthetic weights)
TABLE_WEIGHT_DTYPES = {"nf4": 0.5, "fp4_e2m1": 2.9, "fp4_e2m1_bnb": 0.47}
# 8-bit float weight types the engine takes (round 6; reference strings bestla_weightonly_dispatcher.hpp:62-72) -> torch dtype
FP8_WEIGHT_DTYPES = {"fp8_e4m3": torch.float8_e4m3fn, "fp8_e5m2": torch.float8_e5m2}
_TABLES = {
    "nf4": [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
            -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
            0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0],
    "fp4_e2m1": [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0],
    "fp4_e2m1_bnb": [0.0, 0.0625 / 12, 8.0 / 12, 1.0, 4.0 / 12, 0.5, 2.0 / 12, 0.25,
                     -0.0, -0.0625 / 12, -8.0 / 12, -1.0, -4.0 / 12, -0.5, -2.0 / 12, -0.25],
}


def _code_parts(mod):
    """QuantizedLinearQBits of a 4-bit table type -> (codes int8 [K,N] in 0..15, scales fp32 [G,N], None): the blob has
    no integer export (modules.py recover_qparms raises), so the codes are read back as the nearest table entry of
    dequantised / scale — exact, the entries are >= 5e-3 apart and the quotient is off by an fp32 rounding."""
    w = mod.weight.data
    info = lambda t: qbits.acquire_packed_weight_info(w, t)  # noqa: E731
    k, n = int(info(2)[0]), int(info(3)[0])
    if int(info(4)[0]):
        raise RuntimeError("QBits: the fused decode engine does not take act-order (g_idx) layers")
    scales = info(9)
    deq = torch.empty(k, n, dtype=torch.float32, device=w.device)
    qbits.dequantize_packed_weight(w, deq, False, mod.compute_dtype, mod.weight_dtype, mod.scale_dtype)
    s = scales[torch.arange(k, device=w.device) // int(info(1)[0])]
    x = deq / torch.where(s == 0, torch.ones_like(s), s)
    tab = torch.tensor(_TABLES[mod.weight_dtype], dtype=torch.float32, device=w.device)
    vals, order = torch.sort(tab, stable=True)
    pos = torch.bucketize(x, (vals[1:] + vals[:-1]) * 0.5)
    return order[pos].to(torch.int8), scales, None


def _fp8_parts(mod):
    """QuantizedLinearQBits of an fp8 weight type -> (code bytes int8 [K,N], scales fp32 [G,N], None): dequantised / scale
    IS an fp8 value up to an fp32 rounding of the quotient, so casting it to the torch fp8 dtype returns the code."""
    w = mod.weight.data
    info = lambda t: qbits.acquire_packed_weight_info(w, t)  # noqa: E731
    k, n = int(info(2)[0]), int(info(3)[0])
    if int(info(4)[0]):
        raise RuntimeError("QBits: the fused decode engine does not take act-order (g_idx) layers")
    scales = info(9)
    deq = torch.empty(k, n, dtype=torch.float32, device=w.device)
    qbits.dequantize_packed_weight(w, deq, False, mod.compute_dtype, mod.weight_dtype, mod.scale_dtype)
    s = scales[torch.arange(k, device=w.device) // int(info(1)[0])]
    x = deq / torch.where(s == 0, torch.ones_like(s), s)
    return x.to(FP8_WEIGHT_DTYPES[mod.weight_dtype]).view(torch.int8), scales, None


def _signed_parts(mod):
    """QuantizedLinearQBits -> (q int8 [K,N] in [-8,7], scales fp32 [G,N], zp int8 [G,N] signed or None, g_idx int32 [K]
    or None). Act-order (GPTQ desc_act) modules: rows in the regrouped order the blob holds, plus the raw g_idx that
    `repack_quantized_weight` turns into the activation shuffle (reference nn/modules.py:205-224)."""
    if getattr(mod, "weight_dtype", "int4_clip") in TABLE_WEIGHT_DTYPES:
        return _code_parts(mod) + (None,)
    if getattr(mod, "weight_dtype", "int4_clip") in FP8_WEIGHT_DTYPES:
        return _fp8_parts(mod) + (None,)
    int_w, scales, zeros, g_idx = mod.recover_qparms_kn()
    if g_idx is not None:
        # recover_qparms_kn hands the rows back in the CHECKPOINT's order; the blob wants them regrouped (group g owns
        # rows [g * group, (g + 1) * group), in order of appearance) exactly as set_weights_bias does before it repacks
        order = torch.argsort(g_idx.to(torch.int64), stable=True)
        int_w = int_w[order.to(int_w.device)].contiguous()
    return (int_w - 8).to(torch.int8), scales, None if zeros is None else (zeros - 8).to(torch.int8), g_idx


def _same_order(parts, what):
    """Projections fused along N share ONE activation shuffle: q / k / v (and gate / up) of a GPTQ act-order checkpoint
    see the same inputs, hence the same Hessian diagonal, hence the same permutation — checked, not assumed."""
    idx = [p[3] for p in parts]
    if all(i is None for i in idx):
        return None
    if any(i is None for i in idx) or any(not torch.equal(idx[0], i) for i in idx[1:]):
        raise RuntimeError("QBits: %s carry different act-order permutations; the fused decode engine needs one per fused "
                           "projection (the model keeps the module path)" % what)
    return idx[0]


def optimize_transformers(model, max_ctx=2048, kv_dtype=torch.float16, adapters=None):
    """Post-pass over a model returned by `AutoModelForCausalLM.from_pretrained(..., quantization_config=...)`:
    builds the native batch-1 decode engine over the SAME quantised weights (q/k/v fused along N, gate/up
    interleaved per 16-column tile for the fused SiLU*mul epilogue). Mirrors the two-step shape of the reference's
    Intel-GPU flow, `ipex.optimize_transformers(qmodel, ...)` after `from_pretrained`
    (docs/weightonlyquant.md:199-202). Llama-class decoders (RMSNorm, RoPE, gated SiLU MLP): Llama-2 / 3.x, Mistral,
    Qwen2 (q / k / v biases) and Qwen3 (per-head q / k norm), with HF's default, linear, llama3 or yarn RoPE.

    A model that holds unmerged LoRA adapters (`get_peft_model`, `load_peft_adapter`) is refused unless
    `adapters="unmerged"`: the engine is then built over the adopted blobs and the model's adapter installed on it
    (`WoqDecoderEngine.set_lora`: a copy — after training the adapter further, call `model.woq_engine.set_lora(model)`
    again), and `model.generate` runs on the engine from then on."""
    if adapters not in (None, "unmerged"):
        raise ValueError("QBits: optimize_transformers(adapters=%r): None or \"unmerged\"" % (adapters,))
    cfg = model.config
    # anything the engine's kernels do not implement keeps the model on the module path instead of changing its maths
    ok, reason = engine_supports(cfg)
    if not ok:
        raise RuntimeError(reason)
    has_adapters = any(hasattr(m, "lora_A") for m in model.modules())
    if has_adapters and adapters is None:
        raise RuntimeError("QBits: the fused decode engine does not run unmerged LoRA adapters by default (the model keeps "
                           "the module path); fold them into the blobs with model.merge_and_unload() first (lossy: RTN), "
                           "or pass optimize_transformers(model, adapters=\"unmerged\") to serve them as they are")
    rtype, rs = rope_scaling_of(cfg)
    layers = model.model.layers
    first = layers[0].self_attn.q_proj
    wdt = getattr(first, "weight_dtype", "int4_clip")
    fp8 = wdt in FP8_WEIGHT_DTYPES
    if not fp8 and (getattr(first, "bits", 4) != 4 or (wdt != "int4_clip" and wdt not in TABLE_WEIGHT_DTYPES)):
        raise RuntimeError("QBits: the fused decode engine takes int4_clip / nf4 / fp4 / fp8 layers (int8 models run "
                           "on the module path)")
    hidden, inter = cfg.hidden_size, cfg.intermediate_size
    heads = cfg.num_attention_heads
    kv_heads = getattr(cfg, "num_key_value_heads", heads) or heads
    head_dim = getattr(cfg, "head_dim", None) or hidden // heads
    theta = getattr(cfg, "rope_theta", None)
    if theta is None:
        theta = (getattr(cfg, "rope_parameters", None) or {}).get("rope_theta", 10000.0)
    dev = first.weight.device
    window = engine_window(cfg)
    eng = WoqDecoderEngine(hidden, inter, heads, kv_heads, head_dim, len(layers), cfg.vocab_size, max_ctx=max_ctx,
                           rms_eps=cfg.rms_norm_eps, rope_theta=float(theta), kv_dtype=kv_dtype, device=dev,
                           sliding_window=int(window))
    # every projection of every layer is repacked under ONE (weight type, compute type, group, scale type, scheme): a
    # model whose modules differ would be repacked under layer 0's q_proj's and decode silently wrong —
    # refuse it here; such models keep the module path
    def _sig(m):
        return (getattr(m, "weight_dtype", "int4_clip"), getattr(m, "bits", 4), m.blocksize, m.scale_dtype, m.scheme,
                getattr(m, "compute_dtype", "fp32"))

    for l, layer in enumerate(layers):
        at, mlp = layer.self_attn, layer.mlp
        for name, m in (("q_proj", at.q_proj), ("k_proj", at.k_proj), ("v_proj", at.v_proj), ("o_proj", at.o_proj),
                        ("gate_proj", mlp.gate_proj), ("up_proj", mlp.up_proj), ("down_proj", mlp.down_proj)):
            if not hasattr(m, "blocksize") or _sig(m) != _sig(first):
                raise RuntimeError("QBits: the fused decode engine needs one quantisation recipe for every projection; "
                                   "layers.%d.%s is %r, layers.0.q_proj is %r" %
                                   (l, name, _sig(m) if hasattr(m, "blocksize") else type(m).__name__, _sig(first)))
    if (wdt in TABLE_WEIGHT_DTYPES or fp8) and first.scheme == "asym":
        raise RuntimeError("QBits: the float weight types are symmetric only (reference utils/config.py:360-370)")
    asym = first.scheme == "asym" and wdt not in TABLE_WEIGHT_DTYPES and not fp8
    group, sdt = first.blocksize, first.scale_dtype
    # the blobs' compute type picks nf4's digit-plane count (three at fp32, two otherwise); int4 kernels do not read it
    cdt = getattr(first, "compute_dtype", "fp32") if wdt in TABLE_WEIGHT_DTYPES else "fp32"

    def pack(q, s, z, g_idx=None):
        return qbits.repack_quantized_weight(q.contiguous(), s.contiguous(),
                                             z.contiguous() if z is not None else torch.empty(0, dtype=torch.int8),
                                             g_idx.to(torch.int32).contiguous() if g_idx is not None
                                             else torch.empty(0, dtype=torch.int32), wdt, sdt, cdt, asym, group)

    def cat(parts, what):
        return (torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1),
                torch.cat([p[2] for p in parts], 1) if asym else None, _same_order(parts, what))

    for l, layer in enumerate(layers):
        at, mlp = layer.self_attn, layer.mlp
        for m in (at.o_proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj):
            if m.bias is not None:
                raise RuntimeError("QBits: the fused decode engine does not take biased projections")
        # q / k / v biases (Qwen2) ride in the fused projection's epilogue: all three, or the model keeps the module path
        biases = [m.bias for m in (at.q_proj, at.k_proj, at.v_proj)]
        if any(b is not None for b in biases) and any(b is None for b in biases):
            state = ", ".join("%s_proj.bias %s" % (n, "missing" if b is None else "set") for n, b in zip("qkv", biases))
            raise RuntimeError("QBits: the fused decode engine takes q_proj / k_proj / v_proj biases only together "
                               "(layers.%d has %s)" % (l, state))
        qkv_bias = torch.cat([b.detach().float().reshape(-1) for b in biases]) if biases[0] is not None else None
        q_norm, k_norm = getattr(at, "q_norm", None), getattr(at, "k_norm", None)
        if (q_norm is None) != (k_norm is None):
            raise RuntimeError("QBits: the fused decode engine takes q_norm and k_norm only together (layers.%d)" % l)
        qkv = pack(*cat([_signed_parts(at.q_proj), _signed_parts(at.k_proj), _signed_parts(at.v_proj)],
                        "layers.%d q_proj / k_proj / v_proj" % l))
        g, u = _signed_parts(mlp.gate_proj), _signed_parts(mlp.up_proj)
        gu = pack(fuse_gate_up(g[0], u[0]), fuse_gate_up(g[1], u[1]), fuse_gate_up(g[2], u[2]) if asym else None,
                  _same_order([g, u], "layers.%d gate_proj / up_proj" % l))
        eng.set_layer(l, qkv, at.o_proj.weight.data, gu, mlp.down_proj.weight.data, layer.input_layernorm.weight,
                      layer.post_attention_layernorm.weight)
        if qkv_bias is not None or q_norm is not None:
            eng.set_layer_extras(l, qkv_bias=qkv_bias, q_norm=None if q_norm is None else q_norm.weight,
                                 k_norm=None if k_norm is None else k_norm.weight)
    head_dtype = kv_dtype if kv_dtype in (torch.float16, torch.bfloat16) else torch.float16  # fp8 is cache-only
    cos = sin = None
    att = 1.0
    if rtype != "default":  # (the default tables are set_head's own)
        mpe = getattr(cfg, "max_position_embeddings", None)
        att = rope_inv_freq(head_dim, float(theta), rs, mpe)[1]
        cos, sin = build_rope_tables(max_ctx, head_dim, float(theta), dev, rope_scaling=rs, max_position_embeddings=mpe)
    eng.set_head(model.model.embed_tokens.weight.detach().to(head_dtype), model.model.norm.weight,
                 model.lm_head.weight.detach().to(head_dtype), cos, sin, attention_factor=att)
    if has_adapters:
        eng.set_lora(model)  # raises what the engine cannot carry (fp8 layers, ranks beyond 64): no engine then
        model._woq_adapters = "unmerged"  # `generate` rebuilds a longer engine the same way
        model._woq_engine_off = False
    model.woq_engine = eng
    return eng
