"""ctypes binding of libwoq_hip.so (C ABI declared in include/woq_hip.h).

There is deliberately NO fallback: if the library is missing or a call fails, a RuntimeError with
the library's "QBits: ..." message is raised — the same exception type the reference's TORCH_CHECKs
surface as (qbits/dispatcher/src/bestla_weightonly_dispatcher.cpp:289,368).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WOQ_HIP_LIB") or os.path.join(_HERE, "libwoq_hip.so")  # env: A/B builds in development

F32, BF16, F16, FP8_E4M3 = 0, 1, 2, 3
W_INT4_CLIP, W_INT8, W_NF4, W_FP4_E2M1, W_FP4_E2M1_BNB, W_INT3_CLIP, W_INT2_CLIP = 0, 1, 2, 3, 4, 5, 6
W_FP8_E4M3, W_FP8_E5M2 = 7, 8
S_FP8_E8M0 = 4       # pack-time scale type for fp8 weights: stored as bf16, header flag FLAG_SCALE_E8M0
FLAG_SCALE_E8M0 = 4
C_FP32, C_BF16, C_INT8, C_FP16 = 0, 1, 2, 3
HEADER_BYTES = 256

WEIGHT_TYPES = {"int4_clip": W_INT4_CLIP, "int4": W_INT4_CLIP, "int8": W_INT8, "nf4": W_NF4, "fp4_e2m1": W_FP4_E2M1,
                "fp4": W_FP4_E2M1, "fp4_e2m1_bnb": W_FP4_E2M1_BNB, "int3_clip": W_INT3_CLIP, "int2_clip": W_INT2_CLIP,
                "fp8_e4m3": W_FP8_E4M3, "fp8": W_FP8_E4M3, "fp8_e5m2": W_FP8_E5M2}
SCALE_TYPES = {"fp32": F32, "bf16": BF16, "fp16": F16, "fp8_e8m0": S_FP8_E8M0}
COMPUTE_TYPES = {"fp32": C_FP32, "bf16": C_BF16, "int8": C_INT8, "fp16": C_FP16}
SCALE_NAMES = {F32: "fp32", BF16: "bf16", F16: "fp16"}
COMPUTE_NAMES = {v: k for k, v in COMPUTE_TYPES.items()}
WEIGHT_NAMES = {W_INT4_CLIP: "int4_clip", W_INT8: "int8", W_NF4: "nf4", W_FP4_E2M1: "fp4_e2m1",
                W_FP4_E2M1_BNB: "fp4_e2m1_bnb", W_FP8_E4M3: "fp8_e4m3", W_FP8_E5M2: "fp8_e5m2"}


class BlobHeader(ctypes.Structure):
    """struct woq_blob_header (include/woq_blob.h)."""

    _fields_ = [
        ("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("total_bytes", ctypes.c_uint64),
        ("K", ctypes.c_int32), ("N", ctypes.c_int32), ("group", ctypes.c_int32), ("Kpad", ctypes.c_int32),
        ("Npad", ctypes.c_int32), ("n_groups", ctypes.c_int32),
        ("weight_type", ctypes.c_uint32), ("scale_type", ctypes.c_uint32), ("compute_type", ctypes.c_uint32),
        ("flags", ctypes.c_uint32), ("scale_mode", ctypes.c_uint32), ("narrow_bits", ctypes.c_uint32),
        ("off_q", ctypes.c_uint64), ("off_scale", ctypes.c_uint64), ("off_zp", ctypes.c_uint64),
        ("off_shuffle", ctypes.c_uint64), ("pad", ctypes.c_uint8 * (HEADER_BYTES - 96)),
    ]


assert ctypes.sizeof(BlobHeader) == HEADER_BYTES


class EngineConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("hidden", "inter", "heads", "kv_heads", "head_dim", "layers", "vocab",
                                              "max_ctx")] + [("rms_eps", ctypes.c_float), ("rope_theta", ctypes.c_float),
                                                             ("tp_rank", ctypes.c_int32), ("tp_size", ctypes.c_int32),
                                                             ("kv_dtype", ctypes.c_int32),
                                                             ("reserved", ctypes.c_int32 * 3)]


class LayerWeights(ctypes.Structure):
    _fields_ = [("qkv_blob", ctypes.c_void_p), ("o_blob", ctypes.c_void_p), ("gate_up_blob", ctypes.c_void_p),
                ("down_blob", ctypes.c_void_p), ("ln1", ctypes.c_void_p), ("ln2", ctypes.c_void_p),
                ("qkv_hdr", BlobHeader), ("o_hdr", BlobHeader), ("gate_up_hdr", BlobHeader), ("down_hdr", BlobHeader)]


class SamplerConfig(ctypes.Structure):
    """struct woq_sampler_config (include/woq_hip.h)."""

    _fields_ = [("do_sample", ctypes.c_int32), ("top_k", ctypes.c_int32), ("temperature", ctypes.c_float),
                ("top_p", ctypes.c_float), ("repetition_penalty", ctypes.c_float), ("seed_lo", ctypes.c_uint32),
                ("seed_hi", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class SamplerControls(ctypes.Structure):
    """struct woq_sampler_controls (include/woq_hip.h)."""

    _fields_ = [("presence_penalty", ctypes.c_float), ("frequency_penalty", ctypes.c_float), ("min_p", ctypes.c_float),
                ("n_bias", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 4)]


SAMPLER_MAX_BIAS = 1024  # logit_bias entries the native sampler takes (csrc/woq_sample.hip SAMPLER_MAX_BIAS)

ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)

# every symbol include/woq_hip.h declares (tests check the .so exports all of them): ABI version 4, the frozen boundary
EXPORTS = [
    "woq_last_error", "woq_abi_version", "woq_device_count", "woq_packed_weight_size",
    "woq_repack_quantized_weight", "woq_quantize_to_packed_weight", "woq_dequantize_packed_weight",
    "woq_read_header", "woq_blob_extract", "woq_linear", "woq_rmsnorm", "woq_rope", "woq_silu_mul", "woq_gelu",
    "woq_engine_create", "woq_engine_destroy", "woq_engine_set_layer", "woq_engine_set_head",
    "woq_engine_bind_io", "woq_engine_token_ptr", "woq_engine_pos_ptr", "woq_engine_logits_ptr", "woq_engine_hidden_ptr",
    "woq_engine_step", "woq_engine_capture", "woq_engine_replay", "woq_engine_steps", "woq_engine_set_allreduce",
    "woq_engine_phase", "woq_engine_prefill", "woq_engine_prefill_logits_ptr", "woq_engine_kv_cache_ptr",
    "woq_engine_set_attn_splits", "woq_engine_attn_splits", "woq_engine_set_attn_grouped", "woq_engine_attn_grouped",
    "woq_engine_set_tp_options", "woq_engine_set_fuse_attn", "woq_engine_fuse_attn", "woq_engine_status",
    "woq_engine_clear_status", "woq_comm_create", "woq_comm_handle", "woq_comm_connect", "woq_comm_allreduce_f32",
    "woq_comm_status", "woq_comm_set_timeout_ms", "woq_comm_destroy", "woq_engine_set_comm", "woq_set_workspace",
    "woq_engine_uses_xq", "woq_engine_token_log_ptr", "woq_table_digit_planes",
    "woq_engine_set_sampler", "woq_engine_sampler_seen", "woq_engine_sampler_seen_ptr",
    "woq_engine_set_logprobs", "woq_engine_logprobs", "woq_engine_logprob_ptr", "woq_engine_prefill_scored",
    "woq_engine_set_sampler_controls", "woq_engine_sampler_counts", "woq_engine_sampler_count_ptr",
    "woq_engine_set_guide", "woq_engine_guide_reset", "woq_engine_guide_state_ptr",
    "woq_engine_kv_shift", "woq_engine_discarded_ptr", "woq_engine_discarded_set", "woq_gptq_sweep",
    "woq_engine_set_layer_extras", "woq_awq_scale_delta", "woq_awq_clip_search",
    "woq_autoround_forward", "woq_autoround_step", "woq_autoround_codes", "woq_teq_forward", "woq_teq_grad",
    "woq_linear_backward", "woq_linear_backward_workspace",
    "woq_engine_lora_reserve", "woq_engine_set_lora", "woq_engine_clear_lora", "woq_engine_lora_on",
]
# include/woq_hip_experimental.h: measurement hooks and lab switches, outside WOQ_ABI_VERSION
EXPERIMENTAL_EXPORTS = [
    "woq_engine_set_attn_chunk", "woq_engine_attn_chunk", "woq_engine_time_gemv", "woq_engine_time_gemv_mask",
    "woq_engine_time_twin", "woq_engine_set_time_eager", "woq_engine_time_prefill_gemm", "woq_gemm_form_log",
    "woq_probe_rope_append", "woq_probe_attn_prefill", "woq_probe_attn_decode", "woq_probe_sample",
    "woq_probe_logprobs", "woq_probe_score_rows", "woq_engine_prefill_rows_ptr",
    "woq_probe_xq_from_f32", "woq_probe_gemv_xq", "woq_probe_lm_head", "woq_probe_greedy_tail", "woq_probe_embed",
    "woq_probe_gemv_f32", "woq_probe_gemm_plan", "woq_probe_gemm_f16", "woq_probe_sample_controls",
    "woq_probe_attn_decode_plan", "woq_engine_attn_plan", "woq_probe_guide", "woq_probe_sample_stream",
    "woq_probe_rope_append_qknorm", "woq_probe_attn_decode_qknorm",
    "woq_probe_gemv_xq_tp", "woq_probe_comm_allreduce", "woq_probe_comm_greedy", "woq_probe_comm_set_seq",
    "woq_probe_lora_delta", "woq_probe_lora_shrink", "woq_probe_lora_expand",
]
# the engine's LoRA targets (include/woq_hip.h woq_engine_set_lora), by HF module name
LORA_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
LORA_MAX_RANK = 64
LORA_EXPAND_ADD_F32, LORA_EXPAND_ADD_F16, LORA_EXPAND_SILU = 0, 1, 2  # csrc/woq_host.h LoraExpandMode
# woq_gemm_form_log bits: which prefill-GEMM form a launch ran (csrc/woq_gemm_f16.hip GEMM_FORM_*)
GEMM_FORM_FRAG, GEMM_FORM_SPLITK, GEMM_FORM_FP32, GEMM_FORM_HANDSCHED = 1, 2, 4, 8
GEMM_FORM_RING, GEMM_FORM_TALL, GEMM_FORM_RAW = 16, 32, 64
# the decode attention plan (csrc/woq_host.h AttnForm / AttnMergeMode): how a step's attention runs, how its slices merge
ATTN_FUSED, ATTN_PER_HEAD, ATTN_GROUPED = 0, 1, 2
ATTN_MERGE_NONE, ATTN_MERGE_COMBINE, ATTN_MERGE_COUNTER, ATTN_MERGE_A2A = 0, 1, 2, 3
_ATTN_PLAN_FIELDS = ("form", "merge", "slices", "chunk_fixed", "span", "spw", "lds", "grid_x", "grid_y", "launches",
                     "refused")

_lib = None


def lib():
    """Load libwoq_hip.so or raise — never falls back to a CPU/eager path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "QBits: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback for the MI355X path." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, cs, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    L.woq_last_error.restype = ctypes.c_char_p
    L.woq_packed_weight_size.restype = cs
    L.woq_packed_weight_size.argtypes = [ci] * 7
    L.woq_table_digit_planes.restype = ci
    L.woq_table_digit_planes.argtypes = [ci, ci, vp, vp]
    L.woq_repack_quantized_weight.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, cs, vp]
    L.woq_quantize_to_packed_weight.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, cs, vp]
    L.woq_dequantize_packed_weight.argtypes = [vp, ctypes.POINTER(BlobHeader), vp, ci, vp]
    L.woq_gptq_sweep.argtypes = [vp, vp] + [ci] * 8 + [vp] * 6
    L.woq_awq_scale_delta.argtypes = [vp, vp] + [ci] * 5 + [vp, vp]
    L.woq_awq_clip_search.argtypes = [vp, vp] + [ci] * 8 + [vp] * 4
    L.woq_autoround_forward.argtypes = [vp] * 4 + [ci] * 5 + [vp, ci, vp]
    L.woq_autoround_step.argtypes = [vp] * 5 + [ci] * 6 + [cf, cf] + [vp] * 3
    L.woq_autoround_codes.argtypes = [vp] * 4 + [ci] * 5 + [vp] * 4
    L.woq_teq_forward.argtypes = [vp, vp] + [ci] * 5 + [vp, ci, vp]
    L.woq_teq_grad.argtypes = [vp, vp, vp] + [ci] * 6 + [vp, vp]
    L.woq_linear_backward.argtypes = [vp, ci, ci, vp, ctypes.POINTER(BlobHeader), vp, ci, ci, ci, vp]
    L.woq_linear_backward_workspace.restype = cs
    L.woq_linear_backward_workspace.argtypes = [ci, ctypes.POINTER(BlobHeader)]
    L.woq_read_header.argtypes = [vp, ctypes.POINTER(BlobHeader), vp]
    L.woq_blob_extract.argtypes = [vp, ctypes.POINTER(BlobHeader), ci, vp, vp]
    L.woq_linear.argtypes = [vp, ci, ci, vp, ctypes.POINTER(BlobHeader), vp, vp, ci, ci, ci, vp]
    L.woq_rmsnorm.argtypes = [vp, ci, vp, cf, ci, ci, vp, ci, vp]
    L.woq_rope.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, vp]
    L.woq_silu_mul.argtypes = [vp, vp, ci, cs, vp, vp]
    L.woq_gelu.argtypes = [vp, ci, cs, ci, vp, vp]
    L.woq_engine_create.argtypes = [ctypes.POINTER(EngineConfig), ctypes.POINTER(vp)]
    L.woq_engine_destroy.argtypes = [vp]
    L.woq_engine_destroy.restype = None
    L.woq_engine_set_layer.argtypes = [vp, ci, ctypes.POINTER(LayerWeights)]
    L.woq_engine_set_head.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp]
    L.woq_engine_set_layer_extras.argtypes = [vp, ci, vp, vp, vp]
    L.woq_engine_lora_reserve.argtypes = [vp, ci]
    L.woq_engine_set_lora.argtypes = [vp, ci, ci, vp, vp, ci, cf]
    L.woq_engine_clear_lora.argtypes = [vp]
    L.woq_engine_lora_on.argtypes = [vp]
    L.woq_probe_lora_delta.argtypes = [ci, vp, vp, vp, vp, cf, ci, ci, ci, ci] + [vp] * 8
    L.woq_probe_lora_shrink.argtypes = [vp, ci, ci, ci, ci, vp, cf, ci, vp, vp, vp, ci, vp]
    L.woq_probe_lora_expand.argtypes = [ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    for f in ("woq_engine_token_ptr", "woq_engine_pos_ptr", "woq_engine_logits_ptr", "woq_engine_hidden_ptr"):
        getattr(L, f).restype = vp
        getattr(L, f).argtypes = [vp]
    L.woq_engine_bind_io.argtypes = [vp, vp, vp, vp, vp]
    L.woq_engine_step.argtypes = [vp, ci, vp]
    L.woq_engine_capture.argtypes = [vp, ci, vp]
    L.woq_engine_replay.argtypes = [vp, ci, vp]
    L.woq_engine_steps.argtypes = [vp, ci, ci, vp]
    L.woq_engine_set_time_eager.argtypes = [vp, ci]
    L.woq_engine_set_allreduce.argtypes = [vp, ALLREDUCE_FN, vp]
    L.woq_engine_phase.argtypes = [vp, ci, ci, ci, vp]
    L.woq_engine_prefill.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    L.woq_engine_prefill_logits_ptr.restype = vp
    L.woq_engine_prefill_logits_ptr.argtypes = [vp]
    L.woq_engine_set_attn_splits.argtypes = [vp, ci]
    L.woq_engine_attn_splits.argtypes = [vp]
    L.woq_engine_set_attn_grouped.argtypes = [vp, ci]
    L.woq_engine_attn_grouped.argtypes = [vp]
    L.woq_engine_set_attn_chunk.argtypes = [vp, ci]
    L.woq_engine_attn_chunk.argtypes = [vp]
    L.woq_engine_set_fuse_attn.argtypes = [vp, ci]
    L.woq_engine_fuse_attn.argtypes = [vp]
    L.woq_engine_status.argtypes = [vp, vp]
    L.woq_engine_clear_status.argtypes = [vp, vp]
    L.woq_engine_kv_cache_ptr.restype = vp
    L.woq_engine_kv_cache_ptr.argtypes = [vp, ci]
    L.woq_engine_time_gemv.argtypes = [vp, ci, vp, ctypes.POINTER(cf), ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(ci)]
    L.woq_engine_time_gemv_mask.argtypes = [vp, ci, ci, vp, ctypes.POINTER(cf), ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ci)]
    L.woq_engine_time_twin.argtypes = [vp, ci, ci, vp, ctypes.POINTER(cf)]
    L.woq_engine_set_tp_options.argtypes = [vp, ci, ci]
    L.woq_engine_time_prefill_gemm.argtypes = [vp, ci, ci, ci, vp, ctypes.POINTER(cf), ctypes.POINTER(cf)]
    L.woq_gemm_form_log.argtypes = [ctypes.POINTER(ci), ci]
    L.woq_probe_gemm_plan.argtypes = [ci] * 16 + [ctypes.POINTER(ctypes.c_longlong)]
    L.woq_probe_rope_append.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, cs, vp]
    L.woq_probe_attn_prefill.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, ci, cs, vp, ci, vp]
    L.woq_probe_attn_decode.argtypes = [vp, vp, vp, ci, vp, vp, vp] + [ci] * 9 + [vp, vp]
    L.woq_probe_rope_append_qknorm.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, cs, vp, vp, cf, vp]
    L.woq_probe_attn_decode_qknorm.argtypes = [vp, vp, vp, ci, vp, vp, vp] + [ci] * 7 + [vp, vp, cf, vp, vp]
    L.woq_probe_attn_decode_plan.argtypes = [ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_longlong)]
    L.woq_engine_attn_plan.argtypes = [vp, ci, ci, ctypes.POINTER(ctypes.c_longlong)]
    L.woq_comm_create.argtypes = [ci, ci, cs, ctypes.POINTER(vp)]
    L.woq_comm_handle.argtypes = [vp, vp, cs]
    L.woq_comm_connect.argtypes = [vp, vp, ctypes.POINTER(ci)]
    L.woq_comm_allreduce_f32.argtypes = [vp, vp, cs, vp]
    L.woq_comm_status.argtypes = [vp, vp, ctypes.POINTER(ci)]
    L.woq_comm_set_timeout_ms.argtypes = [vp, ci]
    L.woq_comm_destroy.argtypes = [vp]
    L.woq_comm_destroy.restype = None
    L.woq_engine_set_comm.argtypes = [vp, vp, ci]
    L.woq_set_workspace.argtypes = [vp, cs]
    L.woq_engine_uses_xq.argtypes = [vp]
    L.woq_engine_token_log_ptr.restype = vp
    L.woq_engine_token_log_ptr.argtypes = [vp]
    L.woq_engine_set_sampler.argtypes = [vp, ctypes.POINTER(SamplerConfig)]
    L.woq_engine_sampler_seen.argtypes = [vp, vp, ci, ci, vp]
    L.woq_engine_sampler_seen_ptr.restype = vp
    L.woq_engine_sampler_seen_ptr.argtypes = [vp]
    L.woq_probe_sample.argtypes = [vp, ci, vp, ctypes.POINTER(SamplerConfig), vp, vp, vp, vp, vp, vp]
    L.woq_probe_sample_stream.argtypes = [vp, ci, vp, ctypes.POINTER(SamplerConfig), vp, vp, vp, vp, vp, vp, vp]
    L.woq_engine_kv_shift.argtypes = [vp, ci, ci, ci, ci, ci, vp]
    L.woq_engine_discarded_ptr.restype = vp
    L.woq_engine_discarded_ptr.argtypes = [vp]
    L.woq_engine_discarded_set.argtypes = [vp, ci, vp]
    L.woq_engine_set_sampler_controls.argtypes = [vp, ctypes.POINTER(SamplerControls), vp, vp]
    L.woq_engine_sampler_counts.argtypes = [vp, vp, ci, ci, vp]
    L.woq_engine_sampler_count_ptr.restype = vp
    L.woq_engine_sampler_count_ptr.argtypes = [vp]
    L.woq_probe_sample_controls.argtypes = [vp, ci, vp, vp, ctypes.POINTER(SamplerConfig),
                                            ctypes.POINTER(SamplerControls)] + [vp] * 9
    L.woq_engine_set_guide.argtypes = [vp, vp, ci, ci]
    L.woq_engine_guide_reset.argtypes = [vp, ci, vp]
    L.woq_engine_guide_state_ptr.restype = vp
    L.woq_engine_guide_state_ptr.argtypes = [vp]
    L.woq_probe_guide.argtypes = [vp, ci, vp, vp, ctypes.POINTER(SamplerConfig), ctypes.POINTER(SamplerControls), vp, vp,
                                  vp, ci, ci, ci] + [vp] * 7
    L.woq_engine_set_logprobs.argtypes = [vp, ci]
    L.woq_engine_logprobs.argtypes = [vp]
    L.woq_engine_logprob_ptr.restype = vp
    L.woq_engine_logprob_ptr.argtypes = [vp, ci]
    L.woq_probe_logprobs.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.woq_engine_prefill_scored.argtypes = [vp, vp, ci, ci, vp, ci, vp]
    L.woq_probe_score_rows.argtypes = [vp, vp, cf, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp]
    L.woq_engine_prefill_rows_ptr.restype = vp
    L.woq_engine_prefill_rows_ptr.argtypes = [vp]
    L.woq_probe_xq_from_f32.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp]
    L.woq_probe_gemv_xq.argtypes = [vp, vp, cf, vp, ci] + [vp] * 9
    L.woq_probe_gemv_xq_tp.argtypes = [vp, vp, cf, vp, ci] + [vp] * 10
    L.woq_probe_comm_allreduce.argtypes = [vp, vp, cs, ci] + [vp] * 6
    L.woq_probe_comm_greedy.argtypes = [vp, vp, vp, ci, ci] + [vp] * 5
    L.woq_probe_comm_set_seq.argtypes = [vp, ctypes.c_uint, vp]
    L.woq_probe_lm_head.argtypes = [vp, vp, cf, vp, ci, ci, ci, vp, vp, vp, vp]
    L.woq_probe_greedy_tail.argtypes = [ci, vp, ci] + [vp] * 6 + [ci, ci] + [vp] * 7 + [ci, vp, vp]
    L.woq_probe_embed.argtypes = [vp, ci, vp, ci] + [vp] * 8 + [ci, vp, vp]
    L.woq_probe_gemv_f32.argtypes = [vp, ci, ci, ci, vp, vp, cf, ci, vp, vp, ci, vp, ci, ci, vp, ctypes.POINTER(ci), vp]
    L.woq_probe_gemm_f16.argtypes = [vp, ci, ci, ci, vp, vp, cf, ci, vp, vp, ci, vp, ci, ci, ci, vp, cs, vp]
    _lib = L
    return L


def gemm_form_log():
    """The forms (GEMM_FORM_* bit sets) of the prefill-GEMM launches since the last call, oldest first (at most 64
    kept); empties the log."""
    buf = (ctypes.c_int * 64)()
    n = lib().woq_gemm_form_log(buf, 64)
    return list(buf[:min(n, 64)])


def probe_gemm_plan(K, N, group, weight_type, scale_type, compute_type, asym, act_shuffle, M, act_dtype, lda,
                    aligned=True, has_norm=False, fp8=False, tall=True, tall_raw=False):
    """What the prefill GEMM's plan decides for one call (woq_probe_gemm_plan; host arithmetic, no device): a dict of
    form (GEMM_FORM_* bits), nz, half_tiles, row_blocks, ws_total, ws_sized (what the sizing function answers for the
    call), part_bytes and splitk_ws."""
    out = (ctypes.c_longlong * 8)()
    check(lib().woq_probe_gemm_plan(K, N, group, weight_type, scale_type, compute_type, int(asym), int(act_shuffle), M,
                                    act_dtype, lda, int(aligned), int(has_norm), int(fp8), int(tall), int(tall_raw), out))
    return dict(zip(("form", "nz", "half_tiles", "row_blocks", "ws_total", "ws_sized", "part_bytes", "splitk_ws"),
                    (int(v) for v in out)))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def probe_rope_append(qkv, n_seq, T, start, heads, kv_heads, head_dim, cos, sin, kcache, vcache, kv_dtype, seq_stride):
    """rope_append_kernel alone (woq_probe_rope_append): torch tensors on the device, the current stream."""
    rc = lib().woq_probe_rope_append(_ptr(qkv), n_seq, T, start, heads, kv_heads, head_dim, _ptr(cos), _ptr(sin),
                                     _ptr(kcache), _ptr(vcache), kv_dtype, seq_stride, stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def probe_attn_prefill(qkv, n_seq, T, start, heads, kv_heads, head_dim, kcache, vcache, kv_dtype, seq_stride, out,
                       window):
    """attn_prefill_kernel alone (woq_probe_attn_prefill)."""
    rc = lib().woq_probe_attn_prefill(_ptr(qkv), n_seq, T, start, heads, kv_heads, head_dim, _ptr(kcache), _ptr(vcache),
                                      kv_dtype, seq_stride, _ptr(out), window, stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def probe_attn_decode(qkv, kcache, vcache, kv_dtype, pos, cos, sin, heads, kv_heads, head_dim, max_ctx, window, splits,
                      grouped, merge, chunk_fixed, out):
    """the decode attention launches alone (woq_probe_attn_decode); `pos` is a device int32 tensor."""
    rc = lib().woq_probe_attn_decode(_ptr(qkv), _ptr(kcache), _ptr(vcache), kv_dtype, _ptr(pos), _ptr(cos), _ptr(sin),
                                     heads, kv_heads, head_dim, max_ctx, window, splits, grouped, merge, chunk_fixed,
                                     _ptr(out), stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def probe_rope_append_qknorm(qkv, n_seq, T, start, heads, kv_heads, head_dim, cos, sin, kcache, vcache, kv_dtype,
                             seq_stride, q_norm, k_norm, eps):
    """rope_append with the per-head q / k RMSNorm in front of the rotation (woq_probe_rope_append_qknorm); q_norm /
    k_norm: fp32 [head_dim] on the device."""
    rc = lib().woq_probe_rope_append_qknorm(_ptr(qkv), n_seq, T, start, heads, kv_heads, head_dim, _ptr(cos), _ptr(sin),
                                            _ptr(kcache), _ptr(vcache), kv_dtype, seq_stride, _ptr(q_norm),
                                            _ptr(k_norm), eps, stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def probe_attn_decode_qknorm(qkv, kcache, vcache, kv_dtype, pos, cos, sin, heads, kv_heads, head_dim, max_ctx, window,
                             splits, merge, q_norm, k_norm, eps, out):
    """the per-query-head decode attention with the q / k RMSNorm (woq_probe_attn_decode_qknorm)."""
    rc = lib().woq_probe_attn_decode_qknorm(_ptr(qkv), _ptr(kcache), _ptr(vcache), kv_dtype, _ptr(pos), _ptr(cos),
                                            _ptr(sin), heads, kv_heads, head_dim, max_ctx, window, splits, merge,
                                            _ptr(q_norm), _ptr(k_norm), eps, _ptr(out), stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def probe_attn_decode_plan(heads, kv_heads, head_dim, kv_dtype, max_ctx, window=0, splits=1, grouped=False, fold=False,
                           chunk_fixed=0, fuse_attn=True, fuse_sliced=True, grouped_a2a=True, xq=True, granules=True,
                           layers=32, slots=0, qkv_k=0, group=128, weight_type=W_INT4_CLIP, scale_type=F16, asym=False,
                           act_shuffle=False):
    """What the decode attention's plan decides for one step (woq_probe_attn_decode_plan; host arithmetic, no device): a
    dict of form (ATTN_*), merge (ATTN_MERGE_*), slices, chunk_fixed, span, spw, lds, grid_x, grid_y, launches, refused.
    qkv_k > 0: the qkv blob is [(heads + 2 kv_heads) * head_dim, qkv_k] packed with the options that follow; 0 = none.
    Raises RuntimeError with the launcher's message where the launch would fail."""
    args = (ctypes.c_int * 23)(heads, kv_heads, head_dim, kv_dtype, max_ctx, window, splits, int(grouped), int(fold),
                               chunk_fixed, int(fuse_attn), int(fuse_sliced), int(grouped_a2a), int(xq), int(granules),
                               layers, slots, qkv_k, group, weight_type, scale_type, int(asym), int(act_shuffle))
    out = (ctypes.c_longlong * 11)()
    check(lib().woq_probe_attn_decode_plan(args, out))
    return dict(zip(_ATTN_PLAN_FIELDS, (int(v) for v in out)))


def engine_attn_plan(handle, splits=0, grouped=-1):
    """The plan the engine's next step would follow for layer 0 (woq_engine_attn_plan), as probe_attn_decode_plan's dict;
    splits > 0 / grouped >= 0 evaluate it at that slice count / grouped request. The engine is not changed. A plan the
    launch would refuse (a per-head workgroup beyond its LDS, ...) does not raise here: refused = 1, form as tried."""
    out = (ctypes.c_longlong * 11)()
    check(lib().woq_engine_attn_plan(handle, int(splits), int(grouped), out))
    return dict(zip(_ATTN_PLAN_FIELDS, (int(v) for v in out)))


def sampler_config(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seed=0):
    """woq_sampler_config from Hugging Face's option names (None = HF's neutral value); `seed` is one 64-bit value."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return SamplerConfig(do_sample=int(bool(do_sample)), top_k=int(top_k or 0),
                         temperature=float(1.0 if temperature is None else temperature),
                         top_p=float(1.0 if top_p is None else top_p),
                         repetition_penalty=float(1.0 if repetition_penalty is None else repetition_penalty),
                         seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32, reserved=0)


def probe_sample(logits, seen, cfg, pos, token_out, u=None, philox_out=None, status=None):
    """the sampled token tail alone (woq_probe_sample): device tensors, `cfg` a SamplerConfig, the current stream."""
    opt = lambda t: _ptr(t) if t is not None else None  # noqa: E731
    rc = lib().woq_probe_sample(_ptr(logits), int(logits.numel()), _ptr(seen), ctypes.byref(cfg), opt(u), _ptr(pos),
                                _ptr(token_out), opt(philox_out), opt(status), stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def probe_sample_stream(logits, seen, cfg, pos, discarded, token_out, u=None, philox_out=None, status=None):
    """`probe_sample` with the rolling cache's word (woq_probe_sample_stream): `discarded` = an int32 device tensor or a
    raw device pointer (`woq_engine_discarded_ptr`), None = 0; the Philox counter is position + discarded."""
    opt = lambda t: _ptr(t) if t is not None else None  # noqa: E731
    disc = discarded if discarded is None or isinstance(discarded, int) else _ptr(discarded)
    rc = lib().woq_probe_sample_stream(_ptr(logits), int(logits.numel()), _ptr(seen), ctypes.byref(cfg), opt(u), _ptr(pos),
                                       disc, _ptr(token_out), opt(philox_out), opt(status), stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def sampler_controls(presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, logit_bias=None):
    """(woq_sampler_controls, int32 id array, float value array) from the OpenAI / HF option names (None = neutral);
    `logit_bias` maps token ids to fp32 values (-inf = a ban). The arrays are ctypes arrays (None when empty)."""
    items = sorted((int(k), float(v)) for k, v in dict(logit_bias or {}).items())
    n = len(items)
    ids = (ctypes.c_int32 * n)(*[k for k, _ in items]) if n else None
    vals = (ctypes.c_float * n)(*[v for _, v in items]) if n else None
    ctl = SamplerControls(presence_penalty=float(presence_penalty or 0.0), frequency_penalty=float(frequency_penalty or 0.0),
                          min_p=float(min_p or 0.0), n_bias=n)
    return ctl, ids, vals


def probe_sample_controls(logits, seen, counts, cfg, controls, pos, token_out, adjusted_out, u=None, status=None,
                          kept_out=None):
    """the token tail with sampler controls alone (woq_probe_sample_controls): device tensors, `cfg` a SamplerConfig,
    `controls` what `sampler_controls` returns, `kept_out` a device int32 [1] for the size of the drawn-from set, the
    current stream."""
    ctl, ids, vals = controls
    rc = lib().woq_probe_sample_controls(_ptr(logits), int(logits.numel()), _ptr(seen), _ptr(counts), ctypes.byref(cfg),
                                         ctypes.byref(ctl), ids, vals, _opt(u), _ptr(pos), _ptr(token_out),
                                         _ptr(adjusted_out), _opt(kept_out), _opt(status), stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


GUIDE_BANNED = 0xFFFF  # a token guide's table entry for a banned id (csrc/woq_host.h GUIDE_BANNED)
STATUS_GUIDE_BANNED_PICK = 16  # woq_engine_status bit 4


def probe_guide(logits, seen, counts, cfg, controls, table, state, pos, token_out, adjusted_out, state_out,
                advance_state=-1, u=None, status=None):
    """the token tail with a token guide alone (woq_probe_guide): as `probe_sample_controls`, `table` a device int16 /
    uint16 tensor [n_states, vocab], `state` the row that masks, `advance_state` the row the advance reads (< 0: the
    same), `state_out` a device int32 [1]."""
    ctl, ids, vals = controls
    check(lib().woq_probe_guide(_ptr(logits), int(logits.numel()), _ptr(seen), _ptr(counts), ctypes.byref(cfg),
                                ctypes.byref(ctl), ids, vals, _ptr(table), int(table.shape[0]), int(state),
                                int(advance_state), _opt(u), _ptr(pos), _ptr(token_out), _ptr(adjusted_out),
                                _ptr(state_out), _opt(status), stream_ptr()))


LOGPROB_TOP = 20  # ids a log-probability record lists per position (csrc/woq_logprob.hip LP_TOP)


def probe_logprobs(logits, token, chosen_out, top_id_out, top_lp_out):
    """the log-probability record alone (woq_probe_logprobs): device tensors, the current stream."""
    rc = lib().woq_probe_logprobs(_ptr(logits), int(logits.numel()), _ptr(token), _ptr(chosen_out), _ptr(top_id_out),
                                  _ptr(top_lp_out), stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def probe_score_rows(hidden_rows, norm_w, eps, W, targets, chosen_out, top_id_out, top_lp_out):
    """the scored head alone (woq_probe_score_rows): hidden_rows fp32 [M, hidden], W fp16 / bf16 [vocab, hidden], targets
    int32 [M]; device tensors, the current stream."""
    M, hidden = hidden_rows.shape
    rc = lib().woq_probe_score_rows(_ptr(hidden_rows), _ptr(norm_w), float(eps), _ptr(W), torch_dtype_code(W.dtype),
                                    int(hidden), int(W.shape[0]), _ptr(targets), int(M), _ptr(chosen_out),
                                    _ptr(top_id_out), _ptr(top_lp_out), stream_ptr())
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def xq_limb_bytes(K):
    """bytes of the limb buffer of an XQ vector of K values (csrc/woq_xq.h xq_limb_bytes)"""
    return ((K // 16 * 48 + 1023) // 1024) * 1024 + 1024


def _opt(t):
    return _ptr(t) if t is not None else None


def _xq_ptrs(xo):
    """xo = (limbs, u, sx) device tensors, or None"""
    return (None, None, None) if xo is None else tuple(_ptr(t) for t in xo)


def probe_xq_from_f32(x, norm_w, limbs_out, u_out, sx_out, ssq_out=None):
    """the fp32 -> XQ conversion alone (woq_probe_xq_from_f32): device tensors, the current stream."""
    check(lib().woq_probe_xq_from_f32(_ptr(x), _opt(norm_w), int(x.numel()), _ptr(limbs_out), _ptr(u_out), _ptr(sx_out),
                                      _opt(ssq_out), stream_ptr()))


def probe_gemv_xq(x, blob, epi=0, in_norm_w=None, eps=0.0, bias=None, residual=None, next_norm_w=None, out=None, xo=None,
                  ssq_out=None):
    """one batch-1 projection of the XQ GEMV (woq_probe_gemv_xq): x fp32 [K], blob a packed weight on the device,
    xo = (limbs, u, sx) or None."""
    check(lib().woq_probe_gemv_xq(_ptr(x), _opt(in_norm_w), float(eps), _ptr(blob), int(epi), _opt(bias), _opt(residual),
                                  _opt(next_norm_w), _opt(out), *_xq_ptrs(xo), _opt(ssq_out), stream_ptr()))


def probe_gemv_xq_tp(comm, x, blob, epi=0, in_norm_w=None, eps=0.0, bias=None, residual=None, next_norm_w=None, out=None,
                     xo=None, ssq_out=None):
    """`probe_gemv_xq` whose epilogue also pushes the outputs into the peers' inboxes (woq_probe_gemv_xq_tp): `comm` a
    connected runtime.comm.DeviceComm; the all-reduce that follows runs with pushed=True."""
    check(lib().woq_probe_gemv_xq_tp(_ptr(x), _opt(in_norm_w), float(eps), _ptr(blob), int(epi), _opt(bias),
                                     _opt(residual), _opt(next_norm_w), _opt(out), *_xq_ptrs(xo), _opt(ssq_out),
                                     stream_ptr(), comm.handle))


def probe_comm_allreduce(comm, buf, n=None, pushed=False, norm_w=None, xo=None, ssq_out=None):
    """the engine's all-reduce launch alone (woq_probe_comm_allreduce): in-place sum over ranks of buf[:n] (fp32 device
    tensor; n defaults to its size), xo = (limbs, u, sx) or None, the current stream."""
    check(lib().woq_probe_comm_allreduce(comm.handle, _ptr(buf), int(buf.numel() if n is None else n), int(bool(pushed)),
                                         _opt(norm_w), *_xq_ptrs(xo), _opt(ssq_out), stream_ptr()))


def probe_comm_greedy(comm, pmax, pidx, vocab_offset, token, pos, log=None, status=None, n_pairs=None):
    """the tensor-parallel greedy pick alone (woq_probe_comm_greedy): pmax fp32 / pidx int32 device tensors of this rank's
    pairs, token / pos / status device int32 [1], log device int32."""
    n = int(pmax.numel() if n_pairs is None else n_pairs)
    check(lib().woq_probe_comm_greedy(comm.handle, _ptr(pmax), _ptr(pidx), n, int(vocab_offset), _ptr(token), _ptr(pos),
                                      _opt(log), _opt(status), stream_ptr()))


def probe_comm_set_seq(comm, seq):
    """test only (woq_probe_comm_set_seq): the sequence number of the communicator's next collective; every rank, the
    same value, with no collective in flight."""
    check(lib().woq_probe_comm_set_seq(comm.handle, int(seq), stream_ptr()))


def probe_lm_head(hidden_in, norm_w, eps, W, logits, pmax=None, pidx=None):
    """lm_head_kernel alone (woq_probe_lm_head): W fp16 / bf16 [vocab, hidden]."""
    check(lib().woq_probe_lm_head(_ptr(hidden_in), _ptr(norm_w), float(eps), _ptr(W), torch_dtype_code(W.dtype),
                                  int(W.shape[1]), int(W.shape[0]), _ptr(logits), _opt(pmax), _opt(pidx), stream_ptr()))


def probe_greedy_tail(mode, vocab, token, pos, logits=None, pmax=None, pidx=None, log=None, embed=None, out=None,
                      norm_w=None, xo=None, ssq_out=None, step_seq=None, max_ctx=0, status=None):
    """one greedy tail (woq_probe_greedy_tail): mode 0 argmax over logits, 1 argmax over the lm_head's pairs, 2 the same
    fused with the next step's embedding (embed [rows, hidden] fp16 / bf16 / fp32)."""
    dt, hidden = (torch_dtype_code(embed.dtype), int(embed.shape[1])) if embed is not None else (0, 0)
    check(lib().woq_probe_greedy_tail(int(mode), _opt(logits), int(vocab), _opt(pmax), _opt(pidx), _ptr(token), _ptr(pos),
                                      _opt(log), _opt(embed), dt, hidden, _opt(out), _opt(norm_w), *_xq_ptrs(xo),
                                      _opt(ssq_out), _opt(step_seq), int(max_ctx), _opt(status), stream_ptr()))


def probe_embed(embed, token, out, norm_w=None, xo=None, ssq_out=None, step_seq=None, pos=None, max_ctx=0, status=None):
    """embed_kernel alone (woq_probe_embed)."""
    check(lib().woq_probe_embed(_ptr(embed), torch_dtype_code(embed.dtype), _ptr(token), int(embed.shape[1]), _ptr(out),
                                _opt(norm_w), *_xq_ptrs(xo), _opt(ssq_out), _opt(step_seq), _opt(pos), int(max_ctx),
                                _opt(status), stream_ptr()))


def probe_gemv_f32(x, blob, out, M=1, lda=None, ldo=None, norm_w=None, eps=0.0, epi=0, bias=None, residual=None,
                   ld_res=None, gu_tmp=None):
    """one projection of the fp32-activation decode step (woq_probe_gemv_f32): x / out / residual device tensors whose
    data pointers are row 0 (views are fine), leading dimensions in elements; -> (kernel, chunks, waves, tiles per wave)
    with kernel 0 = generic, 1 = tile, 2 = fp8 matrix-core."""
    form = (ctypes.c_int * 4)()
    lda = int(x.numel() // M if lda is None else lda)
    ldo = int(out.numel() // M if ldo is None else ldo)
    check(lib().woq_probe_gemv_f32(_ptr(x), torch_dtype_code(x.dtype), lda, int(M), _ptr(blob), _opt(norm_w), float(eps),
                                   int(epi), _opt(bias), _opt(residual), int(ldo if ld_res is None else ld_res), _ptr(out),
                                   torch_dtype_code(out.dtype), ldo, _opt(gu_tmp), form, stream_ptr()))
    return tuple(form)


def probe_gemm_f16(x, blob, out, M, lda=None, ldo=None, norm_w=None, eps=0.0, epi=0, bias=None, residual=None,
                   ld_res=None, fp32_class=False, ws=None, ws_bytes=0):
    """one prompt-pass projection through launch_gemm_f16 (woq_probe_gemm_f16): x / out / residual device tensors whose
    data pointers are row 0 (views are fine), leading dimensions in elements; ws = a device workspace of ws_bytes (or
    None: per-call scratch). woq_gemm_form_log reports the form."""
    lda = int(x.numel() // M if lda is None else lda)
    ldo = int(out.numel() // M if ldo is None else ldo)
    check(lib().woq_probe_gemm_f16(_ptr(x), torch_dtype_code(x.dtype), lda, int(M), _ptr(blob), _opt(norm_w), float(eps),
                                   int(epi), _opt(bias), _opt(residual), int(ldo if ld_res is None else ld_res), _ptr(out),
                                   torch_dtype_code(out.dtype), ldo, int(bool(fp32_class)), _opt(ws), int(ws_bytes),
                                   stream_ptr()))


def _lora_parts(parts, want_a, want_b):
    """parts = [(A or None, B or None, scaling), ...] device fp32 tensors A [r, K] / B [n, r] (None = the part has no
    adapter: give (None, n_cols, 0.0) there) -> the host arrays the LoRA probes take. Keeps nothing alive: the caller's
    tensors must outlive the call."""
    n = len(parts)
    a, b = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
    r, cols, s = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_float * n)()
    for i, (A, B, sc) in enumerate(parts):
        if A is None and not hasattr(B, "data_ptr"):  # (None, n_cols, _): an absent part
            r[i], cols[i], s[i] = 0, int(B or 16), 0.0
            continue
        r[i] = int(A.shape[0] if A is not None else B.shape[1])
        cols[i] = int(B.shape[0]) if B is not None else 16
        s[i] = float(sc)
        a[i] = A.data_ptr() if A is not None else None
        b[i] = B.data_ptr() if B is not None else None
        if (want_a and A is None) or (want_b and B is None):
            raise ValueError("this probe reads the part's %s table" % ("A" if want_a and A is None else "B"))
    return n, a, b, r, cols, s


def probe_lora_delta(parts, out, x=None, xq=None, ssq=None, norm_w=None, eps=0.0, base_bias=None, interleave=False):
    """the decode step's LoRA delta launch alone (woq_probe_lora_delta). Input: `xq` = (limbs, u, sx) of K values with
    `ssq` (its K / 16 sums of squares, or None = no norm), or `x` fp32 [K] with `norm_w` (or None). out fp32 [N]."""
    n, a, b, r, cols, s = _lora_parts(parts, True, True)
    if xq is not None:
        K = int(xq[1].numel()) * 16
        check(lib().woq_probe_lora_delta(0, _ptr(xq[0]), _ptr(xq[1]), _ptr(xq[2]), _opt(ssq), float(eps), K,
                                         int(out.numel()), n, int(bool(interleave)), a, b, r, cols, s, _opt(base_bias),
                                         _ptr(out), stream_ptr()))
    else:
        check(lib().woq_probe_lora_delta(1, _ptr(x), None, None, _opt(norm_w), float(eps), int(x.numel()),
                                         int(out.numel()), n, int(bool(interleave)), a, b, r, cols, s, _opt(base_bias),
                                         _ptr(out), stream_ptr()))


def probe_lora_shrink(X, M, K, a_parts, T, ldx=None, ldt=None, norm_w=None, eps=0.0):
    """the prompt pass's LoRA shrink alone (woq_probe_lora_shrink): X fp32 / fp16 rows (data pointer = row 0), a_parts =
    the parts' A tables fp32 [r, K], T fp32 [>= M, ldt]."""
    n, a, _, r, _, _ = _lora_parts([(A, None, 1.0) for A in a_parts], True, False)
    check(lib().woq_probe_lora_shrink(_ptr(X), torch_dtype_code(X.dtype), int(K if ldx is None else ldx), int(M), int(K),
                                      _opt(norm_w), float(eps), n, a, r, _ptr(T), int(T.shape[-1] if ldt is None else ldt),
                                      stream_ptr()))


def probe_lora_expand(mode, T, M, N, parts, out, ldo, ldt=None, gu=None, ld_gu=0):
    """the prompt pass's LoRA expand alone (woq_probe_lora_expand): parts = [(None, B, scaling) | (None, n_cols, 0.0)],
    mode LORA_EXPAND_*; out is updated in place (modes 0, 1) or written (mode 2, from the fp16 gate/up rows `gu`)."""
    n, _, b, r, cols, s = _lora_parts(parts, False, True)
    check(lib().woq_probe_lora_expand(int(mode), _ptr(T), int(T.shape[-1] if ldt is None else ldt), int(M), int(N), n, b, r,
                                      cols, s, _ptr(out), int(ldo), _opt(gu), int(ld_gu), stream_ptr()))


def check(rc):
    if rc != 0:
        raise RuntimeError(lib().woq_last_error().decode())


def require_gpu():
    """The product path needs a real device: fail loudly instead of silently doing something else."""
    import torch

    if not torch.cuda.is_available() or lib().woq_device_count() == 0:
        raise RuntimeError("QBits: no MI355X/HIP device visible; the gfx950 WOQ path has no CPU fallback")


def torch_dtype_code(dt):
    import torch

    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:
        return F16
    raise RuntimeError("QBits: unsupported qbits data type.")  # text of qbits.cpp:35


def stream_ptr():
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
