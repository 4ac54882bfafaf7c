"""GPTQ calibration on the device: `from_pretrained(fp_model, quantization_config=GPTQConfig(...))`.

The reference hands this step to neural_compressor (external, CPU; reference utils.py:531-702); here the algorithm
(Frantar et al. 2022, as in AutoGPTQ's `fasterquant`) is restated — tests/gptq_reference.py is its float64 statement:

  gptq_quantize_weight  one linear: Hessian -> damped, (act-order) permuted, inverted in float64 -> U with
                        H^-1 = U^T U -> per block of 128 input features the sweep kernel (qbits.gptq_sweep,
                        csrc/woq_gptq.hip: quantise a row, push its error into the block's later rows) and one GEMM
                        that pushes the block's errors into every row after it
  gptq_quantize_model   the calibration loop: decoder block by decoder block, Hessians from forward hooks, every
                        linear swapped for a QuantizedLinearQBits through `set_weights_bias`

torch does the GEMM-shaped parts (H += X^T X, the trailing update) through rocBLAS and the factorisations through
rocSOLVER on purpose; the column-by-column sweep, a chain of tiny dependent steps that torch would issue as about six
launches per input feature, is the HIP kernel.
"""
import logging

import torch

from .... import qbits
from .nn.modules import QuantizedLinearQBits

logger = logging.getLogger(__name__)

_WNAME = {4: "int4_clip", 8: "int8", 3: "int3_clip", 2: "int2_clip"}
_BITS = {"int4_clip": 4, "int8": 8, "int3_clip": 3, "int2_clip": 2}
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
    if bits not in _WNAME:
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
        blob = qbits.quantize_to_packed_weight(w, False, group_size, "fp32", _WNAME[bits], "fp32", asym)
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
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False  # the trailing update is an fp32 GEMM
    try:
        for c0 in range(0, k, blocksize):
            rows = min(blocksize, k - c0)
            c1 = c0 + rows
            qbits.gptq_sweep(w, u, c0, rows, group_size, bits, asym, q, scale, zp, err, static_groups, col_group)
            e = err[:rows]
            if c1 < k:
                w[c1:].addmm_(u[c0:c1, c1:].t(), e, alpha=-1.0)
            loss += e.double().square().sum()
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
    g_idx = None
    if desc_act:
        inv = torch.argsort(perm)
        q = q[inv].contiguous()
        if not static_groups:
            g_idx = (torch.arange(k, device=dev) // group)[inv].to(torch.int32)
    return q, scale, zp, g_idx, float(loss) / 2


# ---- the calibration loop ----------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def _check_options(config):
    for opt in ("use_mse_search", "true_sequential", "use_double_quant", "layer_wise"):
        if getattr(config, opt, False):
            raise NotImplementedError("GPTQ on the MI355X path does not implement %s" % opt)
    if config.weight_dtype not in _BITS:
        raise NotImplementedError("GPTQ quantises to the integer weight types (int4_clip, int8), not weight_dtype=%s"
                                  % config.weight_dtype)


def _data_source(config):
    """where the calibration ids come from: 'loader' or 'texts'; a dataset given by its hub name is not fetched"""
    dataset = getattr(config, "dataset", None)
    if getattr(config, "calib_dataloader", None) is not None:
        return "loader"
    if isinstance(dataset, (list, tuple)) and dataset and all(isinstance(t, str) for t in dataset):
        return "texts"
    raise NotImplementedError("GPTQ calibration does not download datasets (dataset=%r): pass calib_dataloader= (an "
                              "iterable of input_ids tensors) or dataset=[texts] with tokenizer=" % (dataset,))


def validate_gptq_request(model, config):
    """Everything about a request that can be refused without touching a device."""
    _check_options(config)
    _data_source(config)
    _decoder_blocks(model)


def _rows(item):
    """input_ids of one dataloader item -> list of 1-D id tensors"""
    if isinstance(item, dict):
        item = item["input_ids"]
    elif isinstance(item, (tuple, list)) and len(item) and not isinstance(item[0], int):
        item = item[0]["input_ids"] if isinstance(item[0], dict) else item[0]
    ids = torch.as_tensor(item).long()
    return [ids] if ids.dim() == 1 else list(ids.reshape(-1, ids.shape[-1]))


def calibration_batches(config):
    """`config.calib_dataloader` (an iterable of input_ids tensors, or of dicts / tuples holding them) or
    `config.dataset` as a list of strings with `config.tokenizer` -> list of [b, t] id tensors: at most n_samples rows,
    each cut to seq_len, batch_size rows of equal length per batch. A dataset given by its hub name is not fetched."""
    n_samples, seq_len = int(config.n_samples), int(config.seq_len)
    batch_size = max(1, int(getattr(config, "batch_size", 1) or 1))
    rows = []
    if _data_source(config) == "loader":
        for item in config.calib_dataloader:
            rows.extend(r[:seq_len] for r in _rows(item))
            if len(rows) >= n_samples:
                break
    else:
        if config.tokenizer is None:
            raise ValueError("GPTQConfig(dataset=[texts]) needs tokenizer=")
        for text in config.dataset[:n_samples]:
            rows.append(torch.as_tensor(config.tokenizer(text)["input_ids"]).long().reshape(-1)[:seq_len])
    rows = [r for r in rows[:n_samples] if r.numel() > 0]
    if not rows:
        raise ValueError("GPTQ: the calibration data is empty")
    batches, cur = [], []
    for r in rows:
        if cur and (len(cur) == batch_size or cur[0].numel() != r.numel()):
            batches.append(torch.stack(cur))
            cur = []
        cur.append(r)
    batches.append(torch.stack(cur))
    return batches


def _decoder_blocks(model):
    for path in ("model.layers", "transformer.h"):
        obj = model
        for part in path.split("."):
            obj = getattr(obj, part, None)
            if obj is None:
                break
        if isinstance(obj, (torch.nn.ModuleList, torch.nn.Sequential)) and len(obj):
            return path, obj
    raise NotImplementedError("GPTQ calibration walks model.model.layers or model.transformer.h; model type %s has "
                              "neither" % (getattr(getattr(model, "config", None), "model_type", None)
                                           or type(model).__name__))


def _is_conv1d(m):
    return type(m).__name__ == "Conv1D" and hasattr(m, "nf")


def _block_linears(block, prefix, skip):
    out = []
    for name, m in block.named_modules():
        if isinstance(m, QuantizedLinearQBits) or not (isinstance(m, torch.nn.Linear) or _is_conv1d(m)):
            continue
        if any(s in prefix + "." + name for s in skip):
            continue
        out.append((name, m))
    return out


def _run_block(block, inputs):
    outs = []
    for args, kwargs in inputs:
        y = block(*args, **kwargs)
        outs.append(y[0] if isinstance(y, (tuple, list)) else y)
    return outs


@torch.no_grad()
def gptq_quantize_model(model, config, device="cuda"):
    """Quantise every eligible linear of every decoder block of an fp model with GPTQ, in place. Block by block: forward
    hooks on the block's linears accumulate H = 2 / tokens * X^T X (fp32, on the device) while the block runs over the
    calibration samples; each linear is quantised and replaced; the block runs again, quantised, to produce the next
    block's inputs. One block's Hessians live at a time. lm_head and whatever else `llm_int8_skip_modules` names stay."""
    _check_options(config)
    batches = calibration_batches(config)
    path, blocks = _decoder_blocks(model)
    skip = list(getattr(config, "llm_int8_skip_modules", None) or [])
    bits = _BITS[config.weight_dtype]
    sym = bool(config.sym)
    model.to(device)
    model.eval()

    # the first block's inputs, as the model itself calls it
    inputs = []

    def grab(_module, args, kwargs):
        inputs.append((args, kwargs))
        raise _Stop()

    handle = blocks[0].register_forward_pre_hook(grab, with_kwargs=True)
    use_cache = getattr(model.config, "use_cache", None) if hasattr(model, "config") else None
    try:
        if use_cache is not None:
            model.config.use_cache = False
        for ids in batches:
            try:
                model(input_ids=ids.to(device))
            except _Stop:
                pass
    finally:
        handle.remove()
        if use_cache is not None:
            model.config.use_cache = use_cache

    for li, block in enumerate(blocks):
        linears = _block_linears(block, "%s.%d" % (path, li), skip)
        hess, count, hooks = {}, {}, []
        for name, m in linears:
            kdim = m.weight.shape[0] if _is_conv1d(m) else m.in_features
            hess[name] = torch.zeros(kdim, kdim, dtype=torch.float32, device=device)
            count[name] = 0

            def accumulate(_m, args, _out, name=name):
                x = args[0].reshape(-1, args[0].shape[-1]).float()
                hess[name].addmm_(x.t(), x)
                count[name] += x.shape[0]

            hooks.append(m.register_forward_hook(accumulate))
        _run_block(block, inputs)
        for hk in hooks:
            hk.remove()
        for name, m in linears:
            conv = _is_conv1d(m)
            w_kn = m.weight.data if conv else m.weight.data.t()
            h = hess.pop(name).mul_(2.0 / max(1, count[name]))
            q, scales, zeros, g_idx, loss = gptq_quantize_weight(
                w_kn, h, bits, config.group_size, sym, getattr(config, "blocksize", SWEEP_ROWS) or SWEEP_ROWS,
                config.damp_percent, bool(config.desc_act), bool(config.static_groups))
            del h
            logger.info("GPTQ %s.%d.%s: loss %.6g", path, li, name, loss)
            k, n = q.shape
            new = QuantizedLinearQBits(k, n, m.bias is not None, compute_dtype=config.compute_dtype,
                                       compress_statistics=False, weight_dtype=config.weight_dtype, bits=config.bits,
                                       scale_dtype=config.scale_dtype, blocksize=config.group_size, scheme=config.scheme,
                                       device=device)
            if bits == 4:  # set_weights_bias takes 4-bit values unsigned, as the checkpoint formats store them
                q = q + 8
                zeros = zeros + 8 if zeros is not None else None
            new.set_weights_bias(q, scales, zeros, g_idx if g_idx is not None else torch.empty(0, dtype=torch.int32),
                                 config, m.bias.data if m.bias is not None else None)
            new.source_cls = type(m)
            new.requires_grad_(False)
            parent_name, _, leaf = name.rpartition(".")
            parent = block.get_submodule(parent_name) if parent_name else block
            parent._modules[leaf] = new
        outs = _run_block(block, inputs)
        inputs = [((y,) + tuple(args[1:]), kwargs) if args else ((), dict(kwargs, hidden_states=y))
                  for (args, kwargs), y in zip(inputs, outs)]
    return model
