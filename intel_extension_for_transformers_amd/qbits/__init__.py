"""`qbits` operator module for MI355X — same function names, argument order and meaning as the
reference's pybind module `qbits_py` (intel_extension_for_transformers/qbits/qbits.cpp:192-206,
re-exported by qbits/__init__.py:19-21), implemented as thin ctypes calls into libwoq_hip.so.

All tensors are torch CUDA(=HIP) tensors; launches go on torch.cuda.current_stream(); nothing here
allocates on the hot call (`woq_linear` writes the caller's pre-allocated `output` in place exactly like
qbits.cpp:113-140). Errors raise RuntimeError with the library's "QBits: ..." text.
"""
import ctypes

import torch

from .. import _lib as L

__all__ = [
    "woq_linear", "repack_quantized_weight", "quantize_to_packed_weight", "dequantize_packed_weight",
    "acquire_packed_weight_info", "get_packed_weight_size", "set_woq_workspace", "set_qbits_threads",
    "check_isa_supported", "check_torch_compatibility", "rmsnorm", "rope", "silu_mul", "gelu", "gptq_sweep",
    "awq_scale_delta", "awq_clip_search", "autoround_forward", "autoround_step", "autoround_codes",
    "teq_forward", "teq_grad", "woq_linear_backward", "woq_linear_backward_workspace",
]


import os as _os

_VERBOSE = _os.environ.get("QBITS_VERBOSE") is not None  # dispatcher_utils.hpp:51-58


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _blocksize_ok(k, blocksize):
    return blocksize == -1 or blocksize >= k or blocksize % 32 == 0


def _wtype(weight_type):
    if weight_type not in L.WEIGHT_TYPES:
        # reference text: bestla_packq_impl.cpp "unsupported bestla packq config"
        raise RuntimeError("Qbits: unsupported bestla packq config, weight_type: %s (MI355X path: int4_clip, int3_clip, int2_clip, int8, nf4, fp4_e2m1, fp4_e2m1_bnb, fp8_e4m3, fp8_e5m2)"
                           % weight_type)
    return L.WEIGHT_TYPES[weight_type]


def _stype(scale_type):
    if scale_type not in L.SCALE_TYPES:
        raise RuntimeError("QBits: unsupported scale_type %s (fp32 | bf16 | fp16; fp8_e8m0 with fp8 weights)" % scale_type)
    return L.SCALE_TYPES[scale_type]


def _ctype(compute_type):
    if compute_type not in L.COMPUTE_TYPES:
        raise RuntimeError("Qbits: unsupported bestla_config, compute_type: %s" % compute_type)
    return L.COMPUTE_TYPES[compute_type]


def header_of(packed):
    """Cached host copy of the blob header (the reference re-parses it on every call,
    bestla_weightonly_dispatcher.cpp:335; here it is read once per tensor storage)."""
    key = (packed.data_ptr(), packed.numel())
    cached = getattr(packed, "_woq_hdr", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    if not packed.is_cuda:
        raise RuntimeError("QBits: packed weight must live on the HIP device")
    hdr = L.BlobHeader()
    L.check(L.lib().woq_read_header(_ptr(packed), ctypes.byref(hdr), L.stream_ptr()))
    try:
        packed._woq_hdr = (key, hdr)
    except Exception:  # pragma: no cover
        pass
    return hdr


def get_packed_weight_size(k, n, weight_type, scale_type, compute_type, asym, blocksize, act_shuf):
    """qbits.cpp:79-88."""
    wt = _wtype(weight_type)
    if asym and wt in (L.W_NF4, L.W_FP4_E2M1, L.W_FP4_E2M1_BNB, L.W_FP8_E4M3, L.W_FP8_E5M2):
        raise RuntimeError("QBits: float weight types (nf4 / fp4 / fp8) are symmetric: asym is not supported")
    if _stype(scale_type) == L.S_FP8_E8M0 and wt not in (L.W_FP8_E4M3, L.W_FP8_E5M2):
        # the reference's validity matrix: qbits_ut/test_weightonly.py:24-25
        raise RuntimeError("QBits: fp8_e8m0 scales are only used with fp8_e4m3 / fp8_e5m2 weights")
    size = L.lib().woq_packed_weight_size(k, n, blocksize, _wtype(weight_type), _stype(scale_type), int(asym),
                                          int(act_shuf))
    if size == 0:
        raise RuntimeError("QBits: unsupported blocksize %d (must be -1 or a multiple of 32)" % blocksize)
    return size


def repack_quantized_weight(qweight, scale, zp, g_idx, weight_type, scale_type, compute_type, asym, blocksize):
    """qbits.cpp:61-77: int8 [K,N] (signed int4 values, or full int8 for weight_type "int8") + fp32 scales [G,N] +
    int8 zp [G,N] + int32 g_idx -> blob.
    Empty `zp` / `g_idx` tensors mean "absent", as in the reference (qbits.cpp:67, modules.py:233-237)."""
    L.require_gpu()
    dev = qweight.device if qweight.is_cuda else torch.device("cuda", torch.cuda.current_device())
    qweight = qweight.to(dev, torch.int8).contiguous()
    scale = scale.to(dev, torch.float32).contiguous()
    k, n = qweight.shape
    has_zp = bool(asym) and zp is not None and zp.numel() != 0
    has_idx = g_idx is not None and g_idx.numel() != 0
    zp_d = zp.to(dev, torch.int8).contiguous() if has_zp else None
    idx_d = g_idx.to(dev, torch.int32).contiguous() if has_idx else None
    size = get_packed_weight_size(k, n, weight_type, scale_type, compute_type, has_zp, blocksize, has_idx)
    out = torch.empty(size, dtype=torch.int8, device=dev)
    L.check(L.lib().woq_repack_quantized_weight(_ptr(qweight), _ptr(scale), _ptr(zp_d), _ptr(idx_d), k, n, blocksize,
                                                _wtype(weight_type), _stype(scale_type), _ctype(compute_type),
                                                _ptr(out), size, L.stream_ptr()))
    header_of(out)
    return out


def quantize_to_packed_weight(fp32_weight, transpose, blocksize, compute_type, weight_type, scale_type, asym):
    """qbits.cpp:90-100: RTN of an fp32 weight ([N,K] when transpose) into a blob."""
    L.require_gpu()
    dev = fp32_weight.device if fp32_weight.is_cuda else torch.device("cuda", torch.cuda.current_device())
    w = fp32_weight.to(dev, torch.float32).contiguous()
    k, n = (w.shape[1], w.shape[0]) if transpose else (w.shape[0], w.shape[1])
    size = get_packed_weight_size(k, n, weight_type, scale_type, compute_type, asym, blocksize, False)
    out = torch.empty(size, dtype=torch.int8, device=dev)
    L.check(L.lib().woq_quantize_to_packed_weight(_ptr(w), int(transpose), k, n, blocksize, _wtype(weight_type),
                                                  _stype(scale_type), _ctype(compute_type), int(asym), _ptr(out),
                                                  size, L.stream_ptr()))
    header_of(out)
    return out


def rtn_groups(k, group):
    """csrc/woq_rtn.h's rtn_group / rtn_group_count for K = k: (the group size as the kernels take it: <= 0 or > K means
    one group per column; the number of groups, the last may be short)"""
    g = k if group <= 0 or group > k else group
    return g, (k + g - 1) // g


def gptq_sweep(w, u, c0, rows, group, bits, asym, q, scale, zp, err, params_given=False, col_group=None):
    """The sequential sweep of GPTQ over one block of `rows` <= 128 input features starting at c0 (woq_gptq_sweep,
    csrc/woq_gptq.hip; no reference counterpart). In place on the caller's device tensors: w fp32 [K, N] (working order,
    Linear.weight.T), u fp32 [K, K] upper with H^-1 = U^T U, q int8 [K, N], scale fp32 [G, N], zp int8 [G, N] or None
    (sym), err fp32 [>= rows, N]; q / scale / zp in the domain `repack_quantized_weight` takes. params_given: scale / zp
    are read (static groups); col_group int32 [K]: the group of every working row, None = row // group."""
    k, n = w.shape
    n_groups = rtn_groups(k, group)[1]

    def ok(t, dtype, shape):
        return t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape

    if not (ok(w, torch.float32, (k, n)) and ok(u, torch.float32, (k, k)) and ok(q, torch.int8, (k, n))
            and ok(scale, torch.float32, (n_groups, n)) and (zp is None or ok(zp, torch.int8, (n_groups, n)))
            and err.is_cuda and err.dtype == torch.float32 and err.is_contiguous() and err.dim() == 2
            and err.shape[0] >= rows and err.shape[1] == n
            and (col_group is None or ok(col_group, torch.int32, (k,)))):
        raise RuntimeError("QBits: gptq_sweep takes contiguous device tensors w fp32 [K,N], u fp32 [K,K], q int8 [K,N], "
                           "scale fp32 [G,N], zp int8 [G,N], err fp32 [rows,N], col_group int32 [K]")
    L.check(L.lib().woq_gptq_sweep(_ptr(w), _ptr(u), k, n, int(c0), int(rows), int(group), int(bits), int(bool(asym)),
                                   int(bool(params_given)), _ptr(col_group), _ptr(q), _ptr(scale), _ptr(zp), _ptr(err),
                                   L.stream_ptr()))


def _f32_dev(t, shape):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape


def awq_scale_delta(w, s, group, bits, asym, out=None):
    """D = diag(1 / s) Q(diag(s) W) - W for one candidate of AWQ's scale search (woq_awq_scale_delta, csrc/woq_awq.hip;
    no reference counterpart): w fp32 [K, N] (working order, Linear.weight.T), s fp32 [K] (nonzero), Q the RTN rule of
    `quantize_to_packed_weight` at (bits, group, asym). Returns `out` fp32 [K, N] (allocated when None)."""
    k, n = w.shape
    if out is None:
        out = torch.empty_like(w)
    if not (_f32_dev(w, (k, n)) and _f32_dev(s, (k,)) and _f32_dev(out, (k, n))):
        raise RuntimeError("QBits: awq_scale_delta takes contiguous fp32 device tensors w [K,N], s [K], out [K,N]")
    L.check(L.lib().woq_awq_scale_delta(_ptr(w), _ptr(s), k, n, int(group), int(bits), int(bool(asym)), _ptr(out),
                                        L.stream_ptr()))
    return out


def awq_clip_search(w, h, group, bits, asym, n_grid=20, n_cand=10, w_out=None, losses=None):
    """AWQ's clip search over every (group, column) cell of w fp32 [K, N] (woq_awq_clip_search, csrc/woq_awq.hip; no
    reference counterpart): candidates c_j = 1 - j / n_grid, j < n_cand; the loss of a cell is d^T G d with
    d = Q(clamped) - w and G the group's diagonal block of h fp32 [K, K] (symmetric; a view with unit column stride is fine).
    group: 32, 64 or 128. -> (best int32 [G, N], losses fp32 [n_cand, G, N], w_out fp32 [K, N] = w clamped by best)."""
    k, n = w.shape
    g = rtn_groups(k, group)[1]
    if w_out is None:
        w_out = torch.empty_like(w)
    if not (_f32_dev(w, (k, n)) and _f32_dev(w_out, (k, n)) and h.is_cuda and h.dtype == torch.float32
            and tuple(h.shape) == (k, k) and h.stride(1) == 1 and h.stride(0) >= k):
        raise RuntimeError("QBits: awq_clip_search takes fp32 device tensors w [K,N] and w_out [K,N] (contiguous) and "
                           "h [K,K] (unit column stride)")
    best = torch.empty(g, n, dtype=torch.int32, device=w.device)
    if losses is None:
        losses = torch.empty(int(n_cand), g, n, dtype=torch.float32, device=w.device)
    elif not _f32_dev(losses, (int(n_cand), g, n)):
        raise RuntimeError("QBits: awq_clip_search: losses must be a contiguous fp32 device tensor [n_cand,G,N]")
    L.check(L.lib().woq_awq_clip_search(_ptr(w), _ptr(h), int(h.stride(0)), k, n, int(group), int(bits),
                                        int(bool(asym)), int(n_grid), int(n_cand), _ptr(best), _ptr(losses),
                                        _ptr(w_out), L.stream_ptr()))
    return best, losses, w_out


def _autoround_args(name, w, v, alpha, beta, group):
    """the argument checks the three AutoRound calls share -> (K, N, G)"""
    if w.dim() != 2:
        raise RuntimeError("QBits: %s: w must be [K,N]" % name)
    k, n = w.shape
    n_groups = rtn_groups(k, group)[1]
    if not (_f32_dev(w, (k, n)) and _f32_dev(v, (k, n)) and _f32_dev(alpha, (n_groups, n))
            and _f32_dev(beta, (n_groups, n))):
        raise RuntimeError("QBits: %s takes contiguous fp32 device tensors w [K,N], v [K,N], alpha [G,N], beta [G,N]"
                           % name)
    return k, n, n_groups


_FAKE_QUANT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)  # of a W~ and of its gradient


def autoround_forward(w, v, alpha, beta, group, bits, asym, out=None, dtype=None):
    """AutoRound's fake-quantised weight W~ [K, N] (woq_autoround_forward, csrc/woq_autoround.hip; no reference
    counterpart): w fp32 [K, N] (working order, Linear.weight.T), v fp32 [K, N] the rounding offset, alpha / beta fp32
    [G, N] the range factors; v = 0, alpha = beta = 1 is the RTN rule of `quantize_to_packed_weight` at (bits, group,
    asym). Returns `out` (fp32, fp16 or bf16; allocated as `dtype`, default fp32, when None)."""
    k, n, _ = _autoround_args("autoround_forward", w, v, alpha, beta, group)
    if out is None:
        out = torch.empty(k, n, dtype=dtype or torch.float32, device=w.device)
    if not (out.is_cuda and out.dtype in _FAKE_QUANT_DTYPES and out.is_contiguous() and tuple(out.shape) == (k, n)):
        raise RuntimeError("QBits: autoround_forward: out must be a contiguous fp32 / fp16 / bf16 device tensor [K,N]")
    L.check(L.lib().woq_autoround_forward(_ptr(w), _ptr(v), _ptr(alpha), _ptr(beta), k, n, int(group), int(bits),
                                          int(bool(asym)), _ptr(out), L.torch_dtype_code(out.dtype), L.stream_ptr()))
    return out


def autoround_step(w, v, alpha, beta, g, group, bits, asym, lr_v, lr_minmax, dalpha=None, dbeta=None):
    """One SignSGD step of AutoRound on one linear (woq_autoround_step, csrc/woq_autoround.hip): from g = dL/dW~ [K, N]
    (fp32, fp16 or bf16) the forward is recomputed, the gradients of v, alpha and beta formed (rounding straight-through)
    and p <- clamp(p - lr sign(grad)) applied in place to v (lr_v, kept in [-0.5, 0.5]) and alpha / beta (lr_minmax, kept
    in [0, 1]). dalpha / dbeta: optional fp32 [G, N] outputs for the raw gradients."""
    k, n, n_groups = _autoround_args("autoround_step", w, v, alpha, beta, group)
    if not (g.is_cuda and g.dtype in _FAKE_QUANT_DTYPES and g.is_contiguous() and tuple(g.shape) == (k, n)):
        raise RuntimeError("QBits: autoround_step: g must be a contiguous fp32 / fp16 / bf16 device tensor [K,N]")
    for t in (dalpha, dbeta):
        if t is not None and not _f32_dev(t, (n_groups, n)):
            raise RuntimeError("QBits: autoround_step: dalpha / dbeta must be contiguous fp32 device tensors [G,N]")
    L.check(L.lib().woq_autoround_step(_ptr(w), _ptr(v), _ptr(alpha), _ptr(beta), _ptr(g), L.torch_dtype_code(g.dtype),
                                       k, n, int(group), int(bits), int(bool(asym)), float(lr_v), float(lr_minmax),
                                       _ptr(dalpha), _ptr(dbeta), L.stream_ptr()))


def autoround_codes(w, v, alpha, beta, group, bits, asym):
    """The codes of AutoRound's quantiser at (v, alpha, beta) (woq_autoround_codes, csrc/woq_autoround.hip) ->
    (q int8 [K, N], scale fp32 [G, N], zp int8 [G, N] or None (sym)) in the signed domain `repack_quantized_weight`
    takes, as `gptq_quantize_weight` returns them."""
    k, n, n_groups = _autoround_args("autoround_codes", w, v, alpha, beta, group)
    q = torch.empty(k, n, dtype=torch.int8, device=w.device)
    scale = torch.empty(n_groups, n, dtype=torch.float32, device=w.device)
    zp = torch.empty(n_groups, n, dtype=torch.int8, device=w.device) if asym else None
    L.check(L.lib().woq_autoround_codes(_ptr(w), _ptr(v), _ptr(alpha), _ptr(beta), k, n, int(group), int(bits),
                                        int(bool(asym)), _ptr(q), _ptr(scale), _ptr(zp), L.stream_ptr()))
    return q, scale, zp


def _teq_args(name, w, a):
    """the argument checks the two TEQ calls share -> (K, N)"""
    if w.dim() != 2:
        raise RuntimeError("QBits: %s: w must be [K,N]" % name)
    k, n = w.shape
    if not (_f32_dev(w, (k, n)) and _f32_dev(a, (k,))):
        raise RuntimeError("QBits: %s takes contiguous fp32 device tensors w [K,N], a [K]" % name)
    return k, n


def teq_forward(w, a, group, bits, asym, out=None, dtype=None):
    """TEQ's fake-quantised weight W~ = Q(diag(a) w) / a [K, N] (woq_teq_forward, csrc/woq_teq.hip; no reference
    counterpart): w fp32 [K, N] (working order, Linear.weight.T), a fp32 [K] the per-input-channel scale (positive); Q
    the RTN rule of `quantize_to_packed_weight` at (bits, group, asym), so a = 1 is that rule. Returns `out` (fp32, fp16
    or bf16; allocated as `dtype`, default fp32, when None)."""
    k, n = _teq_args("teq_forward", w, a)
    if out is None:
        out = torch.empty(k, n, dtype=dtype or torch.float32, device=w.device)
    if not (out.is_cuda and out.dtype in _FAKE_QUANT_DTYPES and out.is_contiguous() and tuple(out.shape) == (k, n)):
        raise RuntimeError("QBits: teq_forward: out must be a contiguous fp32 / fp16 / bf16 device tensor [K,N]")
    L.check(L.lib().woq_teq_forward(_ptr(w), _ptr(a), k, n, int(group), int(bits), int(bool(asym)), _ptr(out),
                                    L.torch_dtype_code(out.dtype), L.stream_ptr()))
    return out


def teq_grad(w, a, g, group, bits, asym, out=None):
    """dL/da fp32 [K] of TEQ's quantiser from g = dL/dW~ [K, N] (fp32, fp16 or bf16) (woq_teq_grad, csrc/woq_teq.hip):
    the forward is recomputed, rounding is straight-through, a group's max / min pass to the row that attains them.
    Deterministic: the same inputs give the same bytes. Returns `out` (overwritten; allocated when None)."""
    k, n = _teq_args("teq_grad", w, a)
    if not (g.is_cuda and g.dtype in _FAKE_QUANT_DTYPES and g.is_contiguous() and tuple(g.shape) == (k, n)):
        raise RuntimeError("QBits: teq_grad: g must be a contiguous fp32 / fp16 / bf16 device tensor [K,N]")
    if out is None:
        out = torch.empty(k, dtype=torch.float32, device=w.device)
    if not _f32_dev(out, (k,)):
        raise RuntimeError("QBits: teq_grad: out must be a contiguous fp32 device tensor [K]")
    L.check(L.lib().woq_teq_grad(_ptr(w), _ptr(a), _ptr(g), L.torch_dtype_code(g.dtype), k, n, int(group), int(bits),
                                 int(bool(asym)), _ptr(out), L.stream_ptr()))
    return out


def dequantize_packed_weight(compressed_weight, dequantize_weight, transpose, compute_type, weight_type, scale_type):
    """qbits.cpp:102-111: in place into the caller-allocated fp32 tensor."""
    hdr = header_of(compressed_weight)
    want = (hdr.N, hdr.K) if transpose else (hdr.K, hdr.N)
    if (tuple(dequantize_weight.shape) != want or dequantize_weight.dtype != torch.float32
            or not dequantize_weight.is_contiguous()):
        raise RuntimeError("QBits: dequantize output must be contiguous fp32 of shape %s" % (want,))
    L.check(L.lib().woq_dequantize_packed_weight(_ptr(compressed_weight), ctypes.byref(hdr), _ptr(dequantize_weight),
                                                 int(transpose), L.stream_ptr()))


def woq_linear(activation, weight, bias, output, compute_type, weight_type, scale_type, asym):
    """qbits.cpp:113-140: output[M,N] = activation[M,K] @ W_deq (+ bias), written in place.
    `bias` empty tensor = none; a non-fp32 bias is converted like qbits.cpp:119-123."""
    hdr = header_of(weight)
    if activation.dim() != 2 or output.dim() != 2:
        raise RuntimeError("QBits: woq_linear expects 2-D activation and output")
    if activation.stride(1) != 1 or activation.stride(0) < activation.shape[1]:  # row-strided views go down as is
        activation = activation.contiguous()
    m, k = activation.shape
    if k != hdr.K or output.shape[0] != m or output.shape[1] != hdr.N:
        raise RuntimeError("QBits: woq_linear shape mismatch: act %s, weight K=%d N=%d, out %s"
                           % (tuple(activation.shape), hdr.K, hdr.N, tuple(output.shape)))
    b = None
    if bias is not None and bias.numel() != 0:
        b = bias if bias.dtype == torch.float32 else bias.float()
        b = b.to(activation.device).contiguous()
    verbose = _VERBOSE  # QBITS_VERBOSE, read once at import like the reference's static env_initer
    if verbose:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
    L.check(L.lib().woq_linear(_ptr(activation), L.torch_dtype_code(activation.dtype), activation.stride(0),
                               _ptr(weight), ctypes.byref(hdr), _ptr(b), _ptr(output),
                               L.torch_dtype_code(output.dtype), output.stride(0), m, L.stream_ptr()))
    if verbose:  # the reference's per-call line (bestla_weightonly_dispatcher.cpp:180-188); the time is the DEVICE time
        t1.record()  # of this call between two events on its stream (the call itself is asynchronous)
        t1.synchronize()
        print("QBits linear verbose\nm:%d n:%d k:%d weight_type:%s compute_type:%s blocksize:%d src_type:%s dst_type:%s "
              "execute time:%.4fms" % (m, hdr.N, hdr.K, weight_type, compute_type, hdr.group,
                                       str(activation.dtype).replace("torch.", ""),
                                       str(output.dtype).replace("torch.", ""), t0.elapsed_time(t1)), flush=True)


_own_workspace = None  # the workspace woq_linear_backward keeps when the caller has set none (grown on demand)


def woq_linear_backward_workspace(m, weight):
    """Bytes of workspace `woq_linear_backward` takes for `m` rows of gradient against this blob
    (woq_linear_backward_workspace, include/woq_hip.h): the fp16 image of dY and its row scales, never an image of W."""
    hdr = header_of(weight)
    return int(L.lib().woq_linear_backward_workspace(int(m), ctypes.byref(hdr)))


def _rows_ok(t, cols):
    return t.dim() == 2 and t.shape[1] == cols and t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= cols)


def woq_linear_backward(grad_output, weight, grad_input=None, dtype=None):
    """grad_input[M,K] = grad_output[M,N] @ W_deq^T straight from the blob (woq_linear_backward, csrc/woq_linear_bwd.hip;
    the reference's statement is autograd/functions.py:163-179, which dequantises the whole weight first). For an
    act-order blob the result is in the caller's (un-shuffled) column order. grad_output / grad_input: fp32, bf16 or
    fp16 device tensors with unit column stride (row-strided views go down as they are); grad_input is allocated as
    `dtype` (default: grad_output's) when None. Deterministic: the same inputs give the same bytes. fp8 weights raise.

    Scratch comes from the workspace (`set_woq_workspace`) and nowhere else: with one set, a call it has no room for
    raises with the size it needs; with none set, this module keeps one of its own, grown when a call needs more, so
    that a steady training loop allocates nothing."""
    global _own_workspace
    hdr = header_of(weight)
    if not (grad_output.is_cuda and grad_output.device == weight.device):
        raise RuntimeError("QBits: woq_linear_backward: grad_output must be on the packed weight's HIP device")
    if not _rows_ok(grad_output, hdr.N):
        raise RuntimeError("QBits: woq_linear_backward takes grad_output [M, N=%d] with unit column stride, got shape %s "
                           "stride %s" % (hdr.N, tuple(grad_output.shape), tuple(grad_output.stride())))
    gcode = L.torch_dtype_code(grad_output.dtype)
    m = grad_output.shape[0]
    if grad_input is None:
        grad_input = torch.empty(m, hdr.K, dtype=dtype or grad_output.dtype, device=grad_output.device)
    elif dtype is not None and grad_input.dtype != dtype:
        raise RuntimeError("QBits: woq_linear_backward: grad_input is %s, dtype asks for %s" % (grad_input.dtype, dtype))
    if not (grad_input.is_cuda and grad_input.device == weight.device):
        raise RuntimeError("QBits: woq_linear_backward: grad_input must be on the packed weight's HIP device")
    if not (_rows_ok(grad_input, hdr.K) and grad_input.shape[0] == m):
        raise RuntimeError("QBits: woq_linear_backward takes grad_input [M=%d, K=%d] with unit column stride, got shape "
                           "%s stride %s" % (m, hdr.K, tuple(grad_input.shape), tuple(grad_input.stride())))
    ocode = L.torch_dtype_code(grad_input.dtype)
    if m == 0:
        return grad_input
    if _workspace is None or _workspace is _own_workspace:
        need = int(L.lib().woq_linear_backward_workspace(m, ctypes.byref(hdr)))
        fits = (_own_workspace is not None and _own_workspace.numel() >= need
                and _own_workspace.device == weight.device)
        if not fits:
            _own_workspace = torch.empty(need, dtype=torch.uint8, device=weight.device)
        if not fits or _workspace is None:
            set_woq_workspace(_own_workspace)
    ldg = grad_output.stride(0) if m > 1 else max(grad_output.stride(0), hdr.N)
    ldo = grad_input.stride(0) if m > 1 else max(grad_input.stride(0), hdr.K)
    L.check(L.lib().woq_linear_backward(_ptr(grad_output), gcode, ldg, _ptr(weight), ctypes.byref(hdr), _ptr(grad_input),
                                        ocode, ldo, m, L.stream_ptr()))
    return grad_input


def _ascii(s):
    return torch.tensor([ord(c) for c in s], dtype=torch.int32)


def acquire_packed_weight_info(packw, acquire_type):
    """qbits.cpp:165-167 -> bestla_packq_impl.cpp:152-204. Scalars come back as int64[1], strings as int32
    ASCII arrays, tensors as dense copies — the reference's conventions (:176-198)."""
    hdr = header_of(packw)
    t = int(acquire_type)
    one = lambda v: torch.tensor([int(v)], dtype=torch.int64)  # noqa: E731
    if t == 0:
        return one(hdr.total_bytes)
    if t == 1:
        return one(hdr.group)
    if t == 2:
        return one(hdr.K)
    if t == 3:
        return one(hdr.N)
    if t == 4:
        return one(1 if hdr.off_shuffle else 0)
    if t == 11:
        return one(1 if hdr.off_zp else 0)
    if t == 6:
        # int3_clip / int2_clip blobs are int4 storage with a tag (include/woq_blob.h narrow_bits)
        return _ascii({3: "int3_clip", 2: "int2_clip"}.get(hdr.narrow_bits) or L.WEIGHT_NAMES[hdr.weight_type])
    if t == 7:
        return _ascii(L.COMPUTE_NAMES[hdr.compute_type])
    if t == 8:
        return _ascii("fp8_e8m0" if hdr.flags & L.FLAG_SCALE_E8M0 else L.SCALE_NAMES[hdr.scale_type])
    if t == 5:
        if not hdr.off_shuffle:
            raise RuntimeError("QBits: not pack g_idx tensor.")
        out = torch.empty(hdr.K, dtype=torch.int32, device=packw.device)
    elif t == 9:
        out = torch.empty(hdr.n_groups, hdr.N, dtype=torch.float32, device=packw.device)
    elif t == 10:
        if not hdr.off_zp:
            raise RuntimeError("QBits: not pack zero-point tensor.")
        out = torch.empty(hdr.n_groups, hdr.N, dtype=torch.int8, device=packw.device)
    else:
        raise RuntimeError("QBits: unsupported acquire_type")
    L.check(L.lib().woq_blob_extract(_ptr(packw), ctypes.byref(hdr), t, _ptr(out), L.stream_ptr()))
    return out


_workspace = None  # the tensor whose memory the library points into (it must outlive every call: kept here)


def set_woq_workspace(workspace):
    """qbits.cpp:142-144 -> bestla_weightonly_dispatcher.cpp:394-397: a caller-owned tensor whose memory the library
    uses as scratch from now on (a raw pointer; this module keeps the tensor alive). With it, the calls that need
    scratch — int8 weights, 16-bit activations at M <= 8, the M > 8 GEMM's packed activations — allocate nothing and
    can be captured into a graph; without it (or when it is too small for a call) they use stream-ordered allocation.
    `None` or an empty tensor removes it. Like the reference's, one process-wide workspace: not for concurrent use
    from several threads."""
    global _workspace
    if workspace is None or workspace.numel() == 0:
        L.check(L.lib().woq_set_workspace(None, 0))
        _workspace = None
        return None
    if not workspace.is_cuda or not workspace.is_contiguous():
        raise RuntimeError("QBits: the workspace must be a contiguous tensor on the HIP device")
    L.check(L.lib().woq_set_workspace(_ptr(workspace), workspace.numel() * workspace.element_size()))
    _workspace = workspace
    return None


def set_qbits_threads(thread_num):
    """qbits.cpp:146. CPU thread-pool size has no meaning on the GPU path."""
    return None


def check_isa_supported(isa):
    """qbits.cpp:173-180 answered for this device: the x86 ISA names are all False; 'GFX950'/'MFMA' True on MI355X."""
    if isa in ("GFX950", "MFMA", "CDNA4"):
        return torch.cuda.is_available() and L.lib().woq_device_count() > 0
    return False


def check_torch_compatibility(version):
    """qbits.cpp:182-190. The C ABI carries no torch types, so any torch that can hand out device pointers works."""
    return True


# ---- ops between the linears (no reference boundary exists for these: they replace HF module forwards) ----
# The kernels index by the sizes handed down and nothing else, so every tensor is checked here: a wrong dtype, length or
# device would be an out-of-bounds access, not an error. Inputs may be strided (they are copied); outputs may not.
def _elem_dev(t, like, numel=None, shape=None):
    """t: a contiguous fp32 / fp16 / bf16 tensor on `like`'s device, of this numel / shape when given"""
    return (t.is_cuda and t.device == like.device and t.is_contiguous() and L.torch_dtype_code(t.dtype) is not None
            and (numel is None or t.numel() == numel) and (shape is None or tuple(t.shape) == tuple(shape)))


def rmsnorm(x, weight, eps, out=None):
    """out = x / sqrt(mean(x^2) + eps) * weight over the last dimension of x [..., d] (fp32 / fp16 / bf16, device);
    weight [d] on the device (a 16-bit weight is widened to fp32); out (allocated when None): x's shape, any of the
    three types, contiguous."""
    code = L.torch_dtype_code(x.dtype)
    if not (x.is_cuda and x.dim() >= 1 and x.shape[-1] > 0):
        raise RuntimeError("QBits: rmsnorm takes a device tensor x [..., d] with d > 0")
    d = x.shape[-1]
    if not (_elem_dev(weight.contiguous(), x, shape=(d,))):
        raise RuntimeError("QBits: rmsnorm takes a device weight [d] (fp32, fp16 or bf16)")
    x = x.contiguous()
    out = torch.empty_like(x) if out is None else out
    if not _elem_dev(out, x, shape=x.shape):
        raise RuntimeError("QBits: rmsnorm: out must be a contiguous device tensor of x's shape (fp32, fp16 or bf16)")
    L.check(L.lib().woq_rmsnorm(_ptr(x), code, _ptr(weight.float().contiguous()), float(eps), x.numel() // d, d,
                                _ptr(out), L.torch_dtype_code(out.dtype), L.stream_ptr()))
    return out


def rope(x, pos, cos, sin):
    """In place on x [tokens, heads, D] (fp32 / fp16 / bf16, contiguous, D even); cos/sin fp32 [max_pos, D/2]; pos int32
    [tokens] (device). Every pos[t] must lie in [0, max_pos): the values live on the device and are not read here."""
    code = L.torch_dtype_code(x.dtype)
    if not (x.dim() == 3 and _elem_dev(x, x)):
        raise RuntimeError("QBits: rope needs a contiguous [tokens, heads, D] device tensor")
    t, h, d = x.shape
    if d % 2 != 0:
        raise RuntimeError("QBits: rope head_dim must be even")
    if not (pos.is_cuda and pos.device == x.device and pos.dtype == torch.int32 and pos.is_contiguous()
            and tuple(pos.shape) == (t,)):
        raise RuntimeError("QBits: rope takes a contiguous int32 device tensor pos [tokens]")
    if not (cos.dim() == 2 and cos.device == x.device and _f32_dev(cos, (cos.shape[0], d // 2))
            and sin.device == x.device and _f32_dev(sin, tuple(cos.shape)) and (cos.shape[0] > 0 or x.numel() == 0)):
        raise RuntimeError("QBits: rope takes contiguous fp32 device tables cos, sin [max_pos, D/2]")
    L.check(L.lib().woq_rope(_ptr(x), code, _ptr(pos), _ptr(cos), _ptr(sin), t, h, d, L.stream_ptr()))
    return x


def silu_mul(gate, up, out=None):
    """out = gate / (1 + exp(-gate)) * up, element by element; gate, up, out of one type (fp32 / fp16 / bf16) and numel
    on the device. out may be gate or up."""
    code = L.torch_dtype_code(gate.dtype)
    gate, up = gate.contiguous(), up.contiguous()
    if not (_elem_dev(gate, gate) and up.dtype == gate.dtype and _elem_dev(up, gate, numel=gate.numel())):
        raise RuntimeError("QBits: silu_mul takes device tensors gate, up of one dtype and numel")
    out = torch.empty_like(gate) if out is None else out
    if not (out.dtype == gate.dtype and _elem_dev(out, gate, numel=gate.numel())):
        raise RuntimeError("QBits: silu_mul: out must be a contiguous device tensor of gate's dtype and numel")
    L.check(L.lib().woq_silu_mul(_ptr(gate), _ptr(up), code, gate.numel(), _ptr(out), L.stream_ptr()))
    return out


def gelu(x, approximate="tanh", out=None):
    """GeLU element by element: approximate "tanh" (gelu_new) or "erf" / "none" (the exact form); x, out of one type
    (fp32 / fp16 / bf16) and numel on the device."""
    code = L.torch_dtype_code(x.dtype)
    if approximate not in ("tanh", "erf", "none"):
        raise RuntimeError("QBits: gelu: approximate is \"tanh\" or \"erf\" / \"none\", not %r" % (approximate,))
    x = x.contiguous()
    if not _elem_dev(x, x):
        raise RuntimeError("QBits: gelu takes a device tensor x")
    out = torch.empty_like(x) if out is None else out
    if not (out.dtype == x.dtype and _elem_dev(out, x, numel=x.numel())):
        raise RuntimeError("QBits: gelu: out must be a contiguous device tensor of x's dtype and numel")
    L.check(L.lib().woq_gelu(_ptr(x), code, x.numel(), 1 if approximate == "tanh" else 0, _ptr(out), L.stream_ptr()))
    return out
