"""AWQ calibration on the device: `from_pretrained(fp_model, quantization_config=AwqConfig(...))`.

The reference hands this step to neural_compressor (external, CPU; reference utils.py:531-702); here the algorithm
(Lin et al. 2023, as in llm-awq / AutoAWQ, with the linear-output objective) is restated — tests/awq_reference.py is its
float64 statement. The loss is the squared output error of the linears, so a block's activations enter only through
H = X^T X / T and a = mean |x| per distinct input tensor (q / k / v share one, gate / up share one); none are kept.

  auto_scale   per absorb group (the linears that share an input, and the op that produces it): 20 candidates
               s = a^(i / 20), normalised; loss = sum over the linears of tr(D^T H D), D = diag(1 / s) Q(diag(s) W) - W
               from qbits.awq_scale_delta (csrc/woq_awq.hip), the trace one GEMM; every group of a block is searched
               against the fp weights, then the scales are folded in: the linears' input columns * s, the producing op
               / s (Llama-class layouts only)
  auto_clip    per linear (q_proj / k_proj leaves skipped, AutoAWQ's rule) under H' = diag(1 / s) H diag(1 / s):
               qbits.awq_clip_search picks each (group, column) cell's clamp out of 10 candidates and clamps the weight
  quantise     the scaled, clamped weight goes through QuantizedLinearQBits.set_fp_weights_bias, the device RTN: the
               result is a plain RTN blob plus changed norm / projection weights, nothing new for save / load or the
               engine

torch does the GEMM-shaped parts (H += X^T X, H @ D) through rocBLAS on purpose, as in gptq.py.
"""
import logging

import torch

from .... import qbits
from .calibration import (ABSORB_GROUPS, BITS, SCALE_MODEL_TYPES, absorb_groups, block_linears, calibration_batches,
                          capture_block_inputs, check_request, collect_input_stats, decoder_blocks, fp32_matmul,
                          install_quantized, model_type, next_inputs, run_block, weight_kn)

logger = logging.getLogger(__name__)

N_GRID = 20  # candidates of the scale search, r_i = i / N_GRID; the clip search's c_j = 1 - j / N_GRID
N_CLIP = 10  # candidates of the clip search
CLIP_GROUPS = (32, 64, 128)  # the group sizes whose Gram block the clip kernel keeps in LDS
_NO_CLIP = ("q_proj", "k_proj")

# linears of such a block that see the same input tensor as another: the statistics are taken once
_SAME_INPUT = {"self_attn.k_proj": "self_attn.q_proj", "self_attn.v_proj": "self_attn.q_proj",
               "mlp.up_proj": "mlp.gate_proj"}


def validate_awq_request(model, config):
    """Everything about a request that can be refused without touching a device."""
    check_request(model, config, "AWQ", ("use_double_quant", "layer_wise"))
    if config.auto_scale and model_type(model) not in SCALE_MODEL_TYPES:
        raise NotImplementedError("AWQ auto_scale folds scales into Llama-class blocks (model_type %s), not model type "
                                  "%s: use auto_scale=False" % (" / ".join(SCALE_MODEL_TYPES), model_type(model)))
    if config.auto_clip and config.group_size not in CLIP_GROUPS:
        raise NotImplementedError("AWQ auto_clip keeps a group's Gram block on chip and takes group_size 32, 64 or 128, "
                                  "not group_size=%s: use auto_clip=False" % config.group_size)


def normalised_scale(a, i, n_grid=N_GRID):
    """candidate i of the scale search from a = mean |x| [K]: clamp(a^(i / n_grid), 1e-4) / sqrt(max min)"""
    s = a.pow(i / n_grid).clamp_(min=1e-4)
    return s / (s.max() * s.min()).sqrt()


def search_scale(weights_kn, h, a, group, bits, asym):
    """the scale search of one absorb group: weights_kn = the fp32 [K, N] weights of its linears, h [K, K], a [K] ->
    (best index, s [K], losses list)"""
    losses = []
    d = [torch.empty_like(w) for w in weights_kn]
    for i in range(N_GRID):
        s = normalised_scale(a, i).contiguous()
        loss = 0.0
        for w, di in zip(weights_kn, d):
            qbits.awq_scale_delta(w, s, group, bits, asym, out=di)
            loss += float((di * (h @ di)).sum(dtype=torch.float64))
        losses.append(loss)
    best = min(range(N_GRID), key=lambda i: (losses[i], i))  # the first minimum
    return best, normalised_scale(a, best), losses


def fold_scale(block, names, prev, s):
    """Fold s [K] into the block, function-preserving: the input columns of the linears `names` * s, the op `prev` that
    produces their input / s (a norm's weight; a linear's output rows and bias)."""
    for name in names:
        m = block.get_submodule(name)
        m.weight.data.mul_(s.to(m.weight.dtype)[None, :])
    p = block.get_submodule(prev)
    sp = s.to(p.weight.dtype)
    if isinstance(p, torch.nn.Linear):
        p.weight.data.div_(sp[:, None])
        if p.bias is not None:
            p.bias.data.div_(s.to(p.bias.dtype))
    else:
        p.weight.data.div_(sp)


def apply_scales(block, scales):
    """`scales` {group index: s}: fold every searched scale of a block in (see ABSORB_GROUPS)"""
    for gi, s in scales.items():
        names, prev = ABSORB_GROUPS[gi]
        fold_scale(block, names, prev, s)


@torch.no_grad()
def awq_quantize_model(model, config, device="cuda"):
    """Quantise every eligible linear of every decoder block of an fp model with AWQ, in place. Block by block: forward
    hooks accumulate X^T X and sum |x| per distinct input (fp32, on the device) while the block runs over the calibration
    samples; scales are searched and folded in, clamps searched and applied, every linear replaced by its RTN blob; the
    block runs again, quantised, to produce the next block's inputs. lm_head and whatever else `llm_int8_skip_modules`
    names stay."""
    validate_awq_request(model, config)
    batches = calibration_batches(config)
    path, blocks = decoder_blocks(model)
    skip = list(getattr(config, "llm_int8_skip_modules", None) or [])
    bits = BITS[config.weight_dtype]
    asym = not bool(config.sym)
    group = config.group_size
    llama = model_type(model) in SCALE_MODEL_TYPES
    model.to(device)
    model.eval()
    inputs = capture_block_inputs(model, blocks, batches, device)
    with fp32_matmul():  # H += X^T X and the loss H @ D are fp32 GEMMs
        for li, block in enumerate(blocks):
            where = "%s.%d" % (path, li)
            linears = block_linears(block, where, skip)
            have = {name for name, _ in linears}
            source = {name: (_SAME_INPUT.get(name, name) if llama else name) for name in have}
            source = {name: (src if src in have else name) for name, src in source.items()}
            gram, asum, count = collect_input_stats(block, linears, inputs, source, abs_sum=True)
            for name in gram:
                gram[name].div_(max(1, count[name]))
                asum[name].div_(max(1, count[name]))

            # auto_scale: every group against the fp weights, then all of them folded in
            in_scale = {}
            if config.auto_scale:
                scales = {}
                for gi in absorb_groups(block, linears, where, "AWQ"):
                    names = ABSORB_GROUPS[gi][0]
                    src = source[names[0]]
                    best, s, losses = search_scale([weight_kn(block.get_submodule(n)) for n in names], gram[src],
                                                   asum[src], group, bits, asym)
                    logger.info("AWQ %s %s: scale exponent %.2f, loss %.6g (RTN %.6g)", where, "/".join(names),
                                best / N_GRID, losses[best], losses[0])
                    scales[gi] = s
                    for n in names:
                        in_scale[n] = s
                apply_scales(block, scales)

            for name, m in linears:
                w_kn = weight_kn(m)
                if config.auto_clip and name.rpartition(".")[2] not in _NO_CLIP:
                    h = gram[source[name]]
                    if name in in_scale:
                        s = in_scale[name]
                        h = h / torch.outer(s, s)
                    best, losses, w_kn = qbits.awq_clip_search(w_kn, h, group, bits, asym, N_GRID, N_CLIP)
                    picked = losses.gather(0, best.long()[None]).sum(dtype=torch.float64)
                    logger.info("AWQ %s.%s: clip loss %.6g (RTN %.6g), %.0f%% of the cells clipped", where, name,
                                float(picked), float(losses[0].sum(dtype=torch.float64)),
                                100.0 * float((best > 0).float().mean()))
                install_quantized(block, name, m, config, device, fp_weight_kn=w_kn)
            del gram, asum
            inputs = next_inputs(inputs, run_block(block, inputs))
    return model
