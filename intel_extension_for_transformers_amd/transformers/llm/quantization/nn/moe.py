"""`QuantizedMoEExpertsQBits` — the module `_replace_linear` swaps in for the expert collection of a sparse
mixture-of-experts block (HF `MixtralExperts`, `Qwen3MoeExperts`: two 3-D parameters `gate_up_proj [E, 2I, H]` and
`down_proj [E, H, I]` and a SiLU `act_fn`). The reference quantises linears only and has no counterpart.

Same call as the module it replaces, `forward(hidden_states [T, H], top_k_index [T, k], top_k_weights [T, k]) -> [T, H]`,
so HF's `*SparseMoeBlock` and its router stay as they are. Every expert's two matrices are RTN-quantised by
`qbits.quantize_to_packed_weight` into WQH1 blobs, stacked at a uniform stride: `gate_up_blobs`, `down_blobs` uint8
[E, stride]. Two forms compute the same block:
  grouped  one `qbits.moe_forward` call (csrc/woq_moe.hip: plan, gate/up, down, combine — four launches, the routing never
           reaches the host), for T <= `grouped_max_tokens` (below `prompt_min_tokens`): int4 / int3 / int2, the 4-bit
           table types (nf4, fp4_e2m1, fp4_e2m1_bnb: digit planes on the same int8 MFMA), the int8 composite, and
           fp8_e4m3 / fp8_e5m2 (the code bytes as the B operand of the fp8 MFMA, the activation as six base-16 digits);
  prompt   the same call with form="prompt" (csrc/woq_moe_prompt.hip: 128-row blocks of one expert on the fp16 MFMA, six
           launches) from `prompt_min_tokens` rows up, in row chunks of at most `qbits.MOE_PROMPT_MAX_SLOTS` slots;
  loop     HF's per-expert loop with each `F.linear` a `qbits.woq_linear` on the expert's slice of the blob tensor: above
           that limit, and for shapes the grouped kernels do not take (`grouped_supported`).
A `hidden_states` or `top_k_weights` that requires grad takes the training form: the same forward under
`autograd.MoEExpertsKBit`, whose backward is one `qbits.moe_backward` (csrc/woq_moe_bwd.hip) through the frozen experts.
"""
import logging

import torch

from ..... import qbits
from ..autograd import MoEExpertsKBit, moe_experts_ref_impl, qbits_debug_enabled
from ..calibration import is_moe_experts  # noqa: F401  (the walker's test, re-exported beside the module it selects)
from .modules import QuantizedLinearQBits

logger = logging.getLogger(__name__)

# what the decode engine's sparse layer takes (runtime/engine.py _sparse_mlp)
_ENGINE_WEIGHT_TYPES = ("int4_clip", "int4", "int3_clip", "int2_clip")
_GROUPED_WEIGHT_TYPES = _ENGINE_WEIGHT_TYPES + ("nf4", "fp4_e2m1", "fp4_e2m1_bnb", "int8", "fp8_e4m3", "fp8_e5m2")
_KINDS = ("gate_up_proj", "down_proj")
_warned_act = False


def silu_act(act_fn):
    """is this HF activation SiLU (nn.SiLU, transformers' SiLUActivation, F.silu)?"""
    return act_fn is torch.nn.functional.silu or type(act_fn).__name__ in ("SiLU", "SiLUActivation")


def warn_other_activation(dotted, act_fn):
    global _warned_act
    if not _warned_act:
        logger.warning("QBits: the experts of %s use %s, not SiLU; expert collections with another activation are left "
                       "unquantised", dotted, type(act_fn).__name__)
        _warned_act = True


class PackedExpertsShell(torch.nn.Module):
    """Holder of a saved expert collection's optimum-format tensors between file and repack (modeling_auto._ShellLinear's
    role): `tensors["gate_up_proj.qweight"]` ... stacked over a leading expert dimension."""

    def __init__(self, num_experts, hidden_dim, intermediate_dim, tensors):
        super().__init__()
        self.num_experts, self.hidden_dim, self.intermediate_dim = num_experts, hidden_dim, intermediate_dim
        self.tensors = tensors


class QuantizedMoEExpertsQBits(torch.nn.Module):
    """E quantised expert MLPs behind one routed call."""

    # The largest T of tools/moe_rate.py's {1, 4, 16, 64, 256} at which the grouped form is not slower than the loop form
    # at both measured shapes (Mixtral-8x7B and Qwen3-30B-A3B, int4 g128): profiles/r22_moe_rate.txt.
    # int8 and nf4 experts: below the loop form at T = 256 at both shapes too (profiles/r25_moe_wtypes.txt L15, L24, L33,
    # L42), so one value serves every kind. fp8 experts inherit it: grouped is below the loop form at T = 1 and 16 at both
    # shapes and is not called from prompt_min_tokens up (profiles/r26_moe_fp8.txt; fp8_e4m3 g128 only, e5m2 unmeasured).
    grouped_max_tokens = 256
    # From this many rows the prompt form serves the call: the smallest T of tools/moe_rate.py's {64, 128, ..., 4096} from
    # which its median is below that of the form that served the T before (grouped up to 256, loop above), at both
    # measured shapes and by more than either's min-to-median spread (profiles/r23_moe_prompt_rate.txt). Not measured below.
    # int8 and nf4 experts: the prompt form is below the loop form at T = 64 / 256 / 1024 and passes the grouped form between
    # 16 and 64 (profiles/r25_moe_wtypes.txt L14-16, L23-25, L32-34, L41-43); the same value.
    # fp8_e4m3 experts: at T = 64 the prompt form is 3.2x / 2.2x below the grouped form and far below the loop, at T = 16
    # grouped leads the loop (profiles/r26_moe_fp8.txt); the inherited value stands, unmeasured between 16 and 64.
    prompt_min_tokens = 64

    def __init__(self, num_experts, hidden_dim, intermediate_dim, compute_dtype="fp32", weight_dtype="int4_clip", bits=4,
                 scale_dtype="fp32", blocksize=32, scheme="sym", device=None):
        super().__init__()
        self.num_experts, self.hidden_dim, self.intermediate_dim = int(num_experts), int(hidden_dim), int(intermediate_dim)
        self.compute_dtype, self.weight_dtype, self.bits = compute_dtype, weight_dtype, bits
        self.scale_dtype, self.blocksize, self.scheme, self.device = scale_dtype, blocksize, scheme, device
        self.register_buffer("gate_up_blobs", torch.empty(0, dtype=torch.uint8))
        self.register_buffer("down_blobs", torch.empty(0, dtype=torch.uint8))
        self._views = {}

    # ---- the hot call ---------------------------------------------------------------------------------------------
    def grouped_supported(self):
        return (self.weight_dtype in _GROUPED_WEIGHT_TYPES and self.intermediate_dim % 16 == 0
                and self.hidden_dim % 4 == 0 and self.num_experts <= qbits.MOE_MAX_EXPERTS)

    def forward(self, hidden_states, top_k_index, top_k_weights):
        """An input that asks for a gradient (in grad mode, hidden_states or top_k_weights requiring grad: the rule of
        QuantizedLinearQBits.forward) takes the training form, the same forward with a backward through the frozen
        experts: `MoEExpertsKBit` (qbits.moe_backward), or torch ops over dequantised experts for fp8 experts, shapes
        `grouped_supported()` refuses and under QBITS_DEBUG. Every other call is `inference_forward`."""
        if torch.is_grad_enabled() and (hidden_states.requires_grad or top_k_weights.requires_grad):
            if self.gate_up_blobs.numel() == 0:
                raise RuntimeError("QBits: QuantizedMoEExpertsQBits has no packed weights (call set_fp_weights first)")
            if qbits_debug_enabled() or self.weight_dtype.startswith("fp8") or not self.grouped_supported():
                return moe_experts_ref_impl(self, hidden_states, top_k_index, top_k_weights)
            return MoEExpertsKBit.apply(self, hidden_states, top_k_index, top_k_weights)
        return self.inference_forward(hidden_states, top_k_index, top_k_weights)

    def inference_forward(self, hidden_states, top_k_index, top_k_weights):
        if self.gate_up_blobs.numel() == 0:
            raise RuntimeError("QBits: QuantizedMoEExpertsQBits has no packed weights (call set_fp_weights first)")
        t, k = hidden_states.shape[0], top_k_index.shape[-1]
        if self.grouped_supported() and t >= self.prompt_min_tokens:
            return self.prompt_forward(hidden_states, top_k_index, top_k_weights, max(1, qbits.MOE_PROMPT_MAX_SLOTS // k))
        if (self.grouped_supported() and t <= self.grouped_max_tokens
                and t * top_k_index.shape[-1] <= qbits.MOE_MAX_SLOTS):
            return qbits.moe_forward(hidden_states, top_k_index, top_k_weights, self.gate_up_blobs, self.down_blobs)
        return self.loop_forward(hidden_states, top_k_index, top_k_weights)

    def prompt_forward(self, hidden_states, top_k_index, top_k_weights, chunk_tokens):
        """form="prompt" over row chunks of whole tokens (rows are independent, so chunking is exact)"""
        t = hidden_states.shape[0]
        if t <= chunk_tokens:
            return qbits.moe_forward(hidden_states, top_k_index, top_k_weights, self.gate_up_blobs, self.down_blobs,
                                     form="prompt")
        x = hidden_states if hidden_states.dtype in (torch.float32, torch.bfloat16, torch.float16) else hidden_states.float()
        out = torch.empty(t, self.hidden_dim, dtype=x.dtype, device=x.device)
        for r in range(0, t, chunk_tokens):
            s = slice(r, min(r + chunk_tokens, t))
            qbits.moe_forward(x[s], top_k_index[s], top_k_weights[s], self.gate_up_blobs, self.down_blobs, out=out[s],
                              form="prompt")
        return out

    def _expert_views(self, kind):
        """the E blobs of a kind as 1-D views that carry their header (qbits.header_of then never reads the device)"""
        blobs = self.gate_up_blobs if kind == "gate_up_proj" else self.down_blobs
        cached = self._views.get(kind)
        if cached is None or cached[0] != blobs.data_ptr():
            hdr = qbits.header_of(blobs)
            views = list(blobs.view(torch.int8).unbind(0))
            for v in views:
                v._woq_hdr = ((v.data_ptr(), v.numel()), hdr)
            cached = self._views[kind] = (blobs.data_ptr(), views)
        return cached[1]

    def _linear(self, x, blob, n):
        out = torch.empty(x.shape[0], n, dtype=x.dtype, device=x.device)
        qbits.woq_linear(x, blob, None, out, self.compute_dtype, self.weight_dtype, self.scale_dtype,
                         self.scheme == "asym")
        return out

    def loop_forward(self, hidden_states, top_k_index, top_k_weights):
        """HF's MixtralExperts.forward over the blobs; an id outside [0, E) drops its slot, as there."""
        e_n = self.num_experts
        x = hidden_states if hidden_states.dtype in (torch.float32, torch.bfloat16, torch.float16) else hidden_states.float()
        final = torch.zeros_like(x)
        gate_up, down = self._expert_views("gate_up_proj"), self._expert_views("down_proj")
        with torch.no_grad():
            ids = torch.where((top_k_index >= 0) & (top_k_index < e_n), top_k_index, e_n).long()
            mask = torch.nn.functional.one_hot(ids, num_classes=e_n + 1).permute(2, 1, 0)
            hit = torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero()
        for e in hit[:, 0].tolist():
            if e == e_n:
                continue
            top_k_pos, token_idx = torch.where(mask[e])
            gate, up = self._linear(x[token_idx], gate_up[e], 2 * self.intermediate_dim).chunk(2, dim=-1)
            cur = self._linear(torch.nn.functional.silu(gate) * up, down[e], self.hidden_dim)
            cur = cur * top_k_weights[token_idx, top_k_pos, None]
            final.index_add_(0, token_idx, cur.to(final.dtype))
        return final.to(hidden_states.dtype)

    # ---- load time ------------------------------------------------------------------------------------------------
    def _adopt(self, gate_up, down):
        self.gate_up_blobs = torch.stack(gate_up).view(torch.uint8)
        self.down_blobs = torch.stack(down).view(torch.uint8)
        self._views = {}

    def set_fp_weights(self, gate_up_proj, down_proj):
        """RTN of fp `gate_up_proj [E, 2I, H]` and `down_proj [E, H, I]` (nn.Linear layout per expert), one
        `qbits.quantize_to_packed_weight` per matrix; the stride is the blob size `woq_packed_weight_size` gives."""
        quant = lambda w: qbits.quantize_to_packed_weight(  # noqa: E731
            w.detach().to(self.device or w.device).float(), True, self.blocksize, self.compute_dtype, self.weight_dtype,
            self.scale_dtype, self.scheme == "asym")
        self._adopt([quant(w) for w in gate_up_proj], [quant(w) for w in down_proj])

    def _linear_shell(self, kind):
        k, n = ((self.hidden_dim, 2 * self.intermediate_dim) if kind == "gate_up_proj"
                else (self.intermediate_dim, self.hidden_dim))
        return QuantizedLinearQBits(k, n, False, compute_dtype=self.compute_dtype, compress_statistics=False,
                                    weight_dtype=self.weight_dtype, bits=self.bits, scale_dtype=self.scale_dtype,
                                    blocksize=self.blocksize, scheme=self.scheme, device=self.device,
                                    use_optimum_format=True)

    def set_packed_weights(self, tensors, q_config):
        """`export_tensors`'s dict back into blobs: per expert `unpack_weight` -> QuantizedLinearQBits.set_weights_bias
        -> `qbits.repack_quantized_weight`, the route a saved linear takes."""
        from ..utils import unpack_weight

        blobs = {}
        for kind in _KINDS:
            shell, blobs[kind] = self._linear_shell(kind), []
            qzeros = tensors.get(kind + ".qzeros")
            for e in range(self.num_experts):
                int_w, scales, zeros = unpack_weight(tensors[kind + ".qweight"][e], tensors[kind + ".scales"][e],
                                                     None if qzeros is None else qzeros[e], q_config)
                shell.set_weights_bias(int_w[:shell.in_features], scales, zeros, torch.empty(0, dtype=torch.int32),
                                       q_config)
                blobs[kind].append(shell.weight.data)
        self._adopt(blobs["gate_up_proj"], blobs["down_proj"])

    def export_tensors(self):
        """{"gate_up_proj.qweight" | ".scales" | ".qzeros", "down_proj. ...": tensor stacked over the experts} in the
        optimum format `pack_weight` writes for a linear (modeling_auto.save_low_bit)."""
        from ..utils import pack_weight

        out = {}
        for kind in _KINDS:
            shell, parts = self._linear_shell(kind), {"qweight": [], "scales": [], "qzeros": []}
            for blob in self._expert_views(kind):
                shell._adopt(blob, None)
                int_w, scales, zeros, _ = shell.recover_qparms_kn()
                if self.bits == 8:  # on disk 8-bit values live in the unsigned domain, q + 128
                    int_w = int_w.to(torch.int16) + 128
                    zeros = None if zeros is None else zeros.to(torch.int16) + 128
                qweight, sc16, qzeros = pack_weight(int_w, scales, zeros, bits=self.bits)
                parts["qweight"].append(qweight)
                parts["scales"].append(scales if self.scale_dtype == "fp32" else sc16)
                if qzeros is not None:
                    parts["qzeros"].append(qzeros)
            for suffix, ts in parts.items():
                if ts:
                    out[kind + "." + suffix] = torch.stack(ts).cpu().contiguous()
        return out
