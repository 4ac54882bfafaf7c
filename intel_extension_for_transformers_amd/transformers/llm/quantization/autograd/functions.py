"""`matmul_kbit` — the seam between `QuantizedLinearQBits.forward` and the operator module, under the reference's
names (intel_extension_for_transformers/transformers/llm/quantization/autograd/functions.py).

  * `matmul_kbit(A, B, bias, out, compute_dtype, weight_dtype, scale_dtype, scheme, do_dequant=False)` (:184-217):
    inference form = one `qbits.woq_linear` call writing `out` in place;
  * `QBITS_DEBUG` (:108, :203): any value other than unset / "NULL" routes the SAME call through
    `qbits_woq_linear_ref_impl` — dequantise the blob, optional g_idx gather, fp32 matmul, + bias (:41-63) — which is
    the reference's own definition of the result and gives an in-product A/B of the fused kernels at any size.
    Both arms run on the GPU (`dequantize_packed_weight` is a HIP kernel, the matmul is torch's rocBLAS call);
  * `qbits_acquire_type` (:29-38) — selector enum of `acquire_packed_weight_info`.

  * `MatMulKBit` (:70-181), the training form behind `do_dequant=True`: the same forward for any M, saving the blob
    and never the activations; the backward hands `dX = dY @ W_deq^T` to `qbits.woq_linear_backward`, which reads the
    blob as it lies (csrc/woq_linear_bwd.hip) where the reference dequantises the whole weight (:163-179). Under
    `QBITS_DEBUG`, and for fp8 weights (not built in the fused kernel), the backward is the reference's own statement.
    No gradient reaches the blob: the weights are frozen, as in QLoRA.
"""
import os
from enum import Enum

import torch

from ..... import qbits


class qbits_acquire_type(Enum):
    SIZE = 0
    BLOCKSIZE = 1
    K = 2
    N = 3
    ACT_SHUFFLE = 4
    G_IDX = 5
    WEI_TYPE = 6
    CMPT_TYPE = 7
    SCALE_TYPE = 8
    SCALE_TENSOR = 9
    ZP_TENSOR = 10
    IS_ASYM = 11


def qbits_woq_linear_ref_impl(activation, packw, bias, compute_type, weight_type, scale_type):
    """functions.py:41-63: W = dequantize_packed_weight(packw) [K, N] fp32; x = index_select(x, 1, g_idx) when the
    blob carries a shuffle; x.float() @ W (+ bias). Returns a new fp32 tensor [M, N]."""
    activation = activation.to(torch.float32)
    n = int(qbits.acquire_packed_weight_info(packw, qbits_acquire_type.N.value)[0])
    k = activation.shape[1]
    revert_wei = torch.empty(k, n, dtype=torch.float32, device=packw.device)
    qbits.dequantize_packed_weight(packw, revert_wei, False, compute_type, weight_type, "fp32")
    if int(qbits.acquire_packed_weight_info(packw, qbits_acquire_type.ACT_SHUFFLE.value)[0]) != 0:
        g_idx = qbits.acquire_packed_weight_info(packw, qbits_acquire_type.G_IDX.value)
        activation = torch.index_select(activation, 1, g_idx.to(activation.device, torch.int64))
    out = torch.matmul(activation, revert_wei)
    if bias is not None and bias.numel() != 0:
        assert bias.is_contiguous()
        assert bias.dtype == torch.float32
        out += bias
    return out


def qbits_debug_enabled():
    """The reference reads the variable on every call (functions.py:108,203), so flipping it mid-run works."""
    return os.getenv("QBITS_DEBUG", "NULL") != "NULL"


def matmul_kbit(A, B, bias, out, compute_dtype, weight_dtype, scale_dtype, scheme, do_dequant=False):
    """functions.py:184-217. Returns `out` (written in place on the fused arm; the reference arm returns its own
    fp32 result cast to `out`'s dtype so that callers see one dtype either way).

    do_dequant=True is the training form: it exists to carry a gradient to A (or to a bias). It is taken where one can
    flow, i.e. in grad mode with an A or a bias that requires grad — what `QuantizedLinearQBits.forward` asks before it
    passes the flag. A call that sets the flag with nothing to differentiate keeps the answer it had before the
    training form was built, NotImplementedError: the form it needs is the inference one, do_dequant=False."""
    if do_dequant:
        if not (torch.is_grad_enabled() and (A.requires_grad or (bias is not None and bias.requires_grad))):
            raise NotImplementedError("QBits: matmul_kbit(do_dequant=True) is the training form (MatMulKBit) and needs "
                                      "grad mode and an activation or bias that requires grad; with nothing to "
                                      "differentiate, call the inference form (do_dequant=False)")
        return MatMulKBit.apply(A, B, out, bias, compute_dtype, weight_dtype, scale_dtype, scheme)
    return _matmul_kbit_forward(A, B, bias, out, compute_dtype, weight_dtype, scale_dtype, scheme)


def _matmul_kbit_forward(A, B, bias, out, compute_dtype, weight_dtype, scale_dtype, scheme):
    packw = B.data if isinstance(B, torch.nn.Parameter) else B
    if not qbits_debug_enabled():
        qbits.woq_linear(A, packw, bias if bias is not None else _EMPTY_F32, out, compute_dtype, weight_dtype,
                         scale_dtype, False if scheme == "sym" else True)
        return out
    ref = qbits_woq_linear_ref_impl(A, packw, bias, compute_dtype, weight_dtype, scale_dtype)
    if out is not None and out.shape == ref.shape:
        out.copy_(ref)
        return out
    return ref


_EMPTY_F32 = torch.empty(0, dtype=torch.float32)
_FP8_WEIGHTS = ("fp8_e4m3", "fp8_e5m2", "fp8")


def qbits_woq_linear_backward_ref_impl(grad_output, packw, compute_type, weight_type, scale_type):
    """The reference's backward (functions.py:163-179): W = dequantize_packed_weight(packw) [K, N] fp32,
    grad.float() @ W.t(), and for a blob that carries a shuffle the columns put back where the forward's index_select
    took them from. Returns a new fp32 tensor [M, K]."""
    info = lambda t: qbits.acquire_packed_weight_info(packw, t)  # noqa: E731
    k, n = int(info(qbits_acquire_type.K.value)[0]), int(info(qbits_acquire_type.N.value)[0])
    revert_wei = torch.empty(k, n, dtype=torch.float32, device=packw.device)
    qbits.dequantize_packed_weight(packw, revert_wei, False, compute_type, weight_type, "fp32")
    grad = torch.matmul(grad_output.to(torch.float32), revert_wei.t())
    if int(info(qbits_acquire_type.ACT_SHUFFLE.value)[0]) != 0:
        g_idx = info(qbits_acquire_type.G_IDX.value).to(grad.device, torch.int64)
        out = torch.empty_like(grad)
        out[:, g_idx] = grad
        grad = out
    return grad


class MatMulKBit(torch.autograd.Function):
    """functions.py:70-181 under the reference's name: y = A @ W_deq (+ bias) with W a packed blob. Saves the blob,
    never A: dX needs only dY and W. backward -> (dX in A's dtype, None for the blob, None, dY.sum(0) for a bias that
    requires grad, None ...)."""

    @staticmethod
    def forward(ctx, A, B, out, bias, compute_dtype, weight_dtype, scale_dtype, scheme):
        packw = B.data if isinstance(B, torch.nn.Parameter) else B
        ctx.packw = packw  # not a differentiable tensor: nothing for save_for_backward to track
        ctx.a_dtype = A.dtype
        ctx.types = (compute_dtype, weight_dtype, scale_dtype)
        if out is None:
            out = torch.empty(A.shape[0], int(qbits.acquire_packed_weight_info(packw, qbits_acquire_type.N.value)[0]),
                              dtype=A.dtype, device=A.device)
        res = _matmul_kbit_forward(A, packw, bias, out, compute_dtype, weight_dtype, scale_dtype, scheme)
        if res is out:
            ctx.mark_dirty(out)
        return res

    @staticmethod
    def backward(ctx, grad_output):
        compute_dtype, weight_dtype, scale_dtype = ctx.types
        grad_a = grad_bias = None
        if ctx.needs_input_grad[0]:
            if qbits_debug_enabled() or weight_dtype in _FP8_WEIGHTS:
                grad_a = qbits_woq_linear_backward_ref_impl(grad_output, ctx.packw, compute_dtype, weight_dtype,
                                                            scale_dtype).to(ctx.a_dtype)
            else:
                g = grad_output
                if g.stride(1) != 1 or (g.shape[0] > 1 and g.stride(0) < g.shape[1]):
                    g = g.contiguous()
                grad_a = qbits.woq_linear_backward(g, ctx.packw, dtype=ctx.a_dtype)
        if ctx.needs_input_grad[3]:
            grad_bias = grad_output.sum(0)
        return grad_a, None, None, grad_bias, None, None, None, None
