"""GPTQ calibration on the device: `from_pretrained(fp_model, quantization_config=GPTQConfig(...))`.

The reference hands this step to neural_compressor (external, CPU; reference utils.py:531-702); here the algorithm
(Frantar et al. 2022, as in AutoGPTQ's `fasterquant`) is restated — tests/gptq_reference.py is its float64 statement:

  gptq_quantize_weight  one linear: Hessian -> damped, (act-order) permuted, inverted in float64 -> U with
                        H^-1 = U^T U -> per block of 128 input features the sweep kernel (qbits.gptq_sweep,
                        csrc/woq_gptq.hip: quantise a row, push its error into the block's later rows) and one GEMM
                        that pushes the block's errors into every row after it
  gptq_quantize_model   the calibration loop: decoder block by decoder block, Hessians from forward hooks, every
                        linear swapped for a QuantizedLinearQBits through `set_weights_bias` (the walk, the hooks and
                        the swap are calibration.py's, shared with awq.py and autoround.py)

torch does the GEMM-shaped parts (H += X^T X, the trailing update) through rocBLAS and the factorisations through
rocSOLVER on purpose; the column-by-column sweep, a chain of tiny dependent steps that torch would issue as about six
launches per input feature, is the HIP kernel.
"""
import logging

import torch

from .... import qbits
from .calibration import (BITS, WNAME, block_linears, calibration_batches, capture_block_inputs, check_request,
                          collect_input_stats, decoder_blocks, fp32_matmul, install_quantized, is_conv1d, next_inputs,
                          run_block)

logger = logging.getLogger(__name__)

SWEEP_ROWS = 128  # the most rows one sweep launch takes (csrc/woq_gptq.hip GPTQ_BLOCK)


def upper_factor(hessian):
    """fp32 U, upper triangular, with H^-1 = U^T U ("Cholesky of the inverse, upper"). The factorisation, the inverse
    and the second factorisation run in float64: an fp32 Cholesky of a Hessian as wide as Llama's down_proj (11008)
    is the step that fails ("not positive definite") in fp32 implementations, and float64 costs little on this chip."""
    h = hessian.double()
    low = torch.linalg.cholesky(h)
    eye = torch.eye(h.shape[0], dtype=h.dtype, device=h.device)
    low_inv = torch.linalg.solve_triangular(low, eye, upper=False)
    return torch.linalg.cholesky(low_inv.t() @ low_inv, upper=True).float().contiguous()


def gptq_quantize_weight(weight_kn, hessian, bits=4, group_size=128, sym=True, blocksize=128, damp_percent=0.01,
                         desc_act=False, static_groups=False):
    """weight_kn [K, N] (Linear.weight.T; a Conv1D weight as it is), hessian [K, K] = 2 / tokens * X^T X ->
    (codes int8 [K, N], scales fp32 [G, N], zeros int8 [G, N] or None (sym), g_idx int32 [K] or None, loss): codes and
    zeros in the signed domain `qbits.repack_quantized_weight` takes, rows in the ORIGINAL order. g_idx (act-order
    without static groups, AutoGPTQ's convention) = the group of every original row, each group exactly `group_size`
    rows; with static_groups the groups are the regular ones of the original order and g_idx is None.
    loss = sum err^2 / 2, AutoGPTQ's figure. Neither input is modified."""
    if bits not in WNAME:
        raise NotImplementedError("GPTQ: bits must be 2, 3, 4 or 8, got %s" % bits)
    if not 32 <= blocksize <= SWEEP_ROWS or blocksize % 32:
        raise ValueError("GPTQ: blocksize must be 32, 64, 96 or 128")
    dev = weight_kn.device if weight_kn.is_cuda else torch.device("cuda", torch.cuda.current_device())
    w = weight_kn.detach().to(dev, torch.float32).clone(memory_format=torch.contiguous_format)
    h = hessian.detach().to(dev, torch.float32).clone(memory_format=torch.contiguous_format)
    k, n = w.shape
    group = k if group_size <= 0 or group_size > k else group_size
    if group != k and group % 32:
        raise ValueError("GPTQ: group_size must be -1 or a multiple of 32")
    n_groups = (k + group - 1) // group
    asym = not sym

    diag = torch.diagonal(h)
    dead = diag == 0  # a feature the calibration data never drove: nothing to fit, keep H invertible
    diag[dead] = 1.0
    w[dead] = 0.0

    scale = zp = None
    if static_groups:  # the RTN parameters of the weight as it came, groups in the original order
        blob = qbits.quantize_to_packed_weight(w, False, group_size, "fp32", WNAME[bits], "fp32", asym)
        scale = qbits.acquire_packed_weight_info(blob, 9).contiguous()
        zp = qbits.acquire_packed_weight_info(blob, 10).contiguous() if asym else None
    perm = None
    if desc_act:
        perm = torch.argsort(torch.diagonal(h), descending=True, stable=True)
        w = w[perm].contiguous()
        h = h[perm][:, perm].contiguous()
    diag = torch.diagonal(h)
    diag += damp_percent * diag.mean()
    u = upper_factor(h)
    del h

    if scale is None:
        scale = torch.empty(n_groups, n, dtype=torch.float32, device=dev)
        zp = torch.empty(n_groups, n, dtype=torch.int8, device=dev) if asym else None
    col_group = (perm // group).to(torch.int32).contiguous() if (static_groups and desc_act) else None
    q = torch.empty(k, n, dtype=torch.int8, device=dev)
    err = torch.empty(min(blocksize, k), n, dtype=torch.float32, device=dev)
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    with fp32_matmul():  # the trailing update is an fp32 GEMM
        for c0 in range(0, k, blocksize):
            rows = min(blocksize, k - c0)
            c1 = c0 + rows
            qbits.gptq_sweep(w, u, c0, rows, group_size, bits, asym, q, scale, zp, err, static_groups, col_group)
            e = err[:rows]
            if c1 < k:
                w[c1:].addmm_(u[c0:c1, c1:].t(), e, alpha=-1.0)
            loss += e.double().square().sum()
    g_idx = None
    if desc_act:
        inv = torch.argsort(perm)
        q = q[inv].contiguous()
        if not static_groups:
            g_idx = (torch.arange(k, device=dev) // group)[inv].to(torch.int32)
    return q, scale, zp, g_idx, float(loss) / 2


# ---- the calibration loop ----------------------------------------------------------------------------------------
def validate_gptq_request(model, config):
    """Everything about a request that can be refused without touching a device."""
    check_request(model, config, "GPTQ", ("use_mse_search", "true_sequential", "use_double_quant", "layer_wise"))


@torch.no_grad()
def gptq_quantize_model(model, config, device="cuda"):
    """Quantise every eligible linear of every decoder block of an fp model with GPTQ, in place. Block by block: forward
    hooks on the block's linears accumulate H = 2 / tokens * X^T X (fp32, on the device) while the block runs over the
    calibration samples; each linear is quantised and replaced; the block runs again, quantised, to produce the next
    block's inputs. One block's Hessians live at a time. lm_head and whatever else `llm_int8_skip_modules` names stay."""
    validate_gptq_request(model, config)
    batches = calibration_batches(config)
    path, blocks = decoder_blocks(model)
    skip = list(getattr(config, "llm_int8_skip_modules", None) or [])
    model.to(device)
    model.eval()
    inputs = capture_block_inputs(model, blocks, batches, device)
    for li, block in enumerate(blocks):
        linears = block_linears(block, "%s.%d" % (path, li), skip)
        hess, _, count = collect_input_stats(block, linears, inputs)
        for name, m in linears:
            h = hess.pop(name).mul_(2.0 / max(1, count[name]))
            w_kn = m.weight.data if is_conv1d(m) else m.weight.data.t()  # a view: gptq_quantize_weight makes the copy
            q, scales, zeros, g_idx, loss = gptq_quantize_weight(
                w_kn, h, BITS[config.weight_dtype], config.group_size, bool(config.sym),
                getattr(config, "blocksize", SWEEP_ROWS) or SWEEP_ROWS, config.damp_percent, bool(config.desc_act),
                bool(config.static_groups))
            del h
            logger.info("GPTQ %s.%d.%s: loss %.6g", path, li, name, loss)
            install_quantized(block, name, m, config, device, codes=q, scales=scales, zeros=zeros, g_idx=g_idx)
        inputs = next_inputs(inputs, run_block(block, inputs))
    return model
