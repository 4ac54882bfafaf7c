"""TEQ calibration on the device: `from_pretrained(fp_model, quantization_config=TeqConfig(...))`.

The reference hands this step to neural_compressor's TEQuantizer (external); here the method (Cheng et al. 2023, "TEQ:
Trainable Equivalent Transformation for Quantization of LLMs") is restated — tests/teq_reference.py is the float64
statement of its quantiser and of the quantiser's gradient. Every absorb group of a Llama-class decoder block
(calibration.py ABSORB_GROUPS: the linears that share an input, and the op that produces it) has one trainable scale a [K], positive,
initially 1. The group's linears see diag(a) W, the producing op is divided by a: in real arithmetic the block computes
the same function, and a is trained so that RTN of the scaled weights loses less.

  forward    every eligible linear computes x.matmul(W~) + bias with W~ = Q(diag(a) W) / a = qbits.teq_forward(w, a)
             (csrc/woq_teq.hip), one launch per linear per step; a linear in no trained group has a = 1 and no gradient
  backward   autograd gives dL/dW~ (the block's own ops, torch); qbits.teq_grad turns it into dL/da, one launch per
             linear; a group's gradient is the sum over its linears in ABSORB_GROUPS order
  update     torch's Adam on the [K] vectors, betas (0.9, 0.9), eps 1e-8, no weight decay (neural_compressor's values);
             the learning rate warms up linearly over the first 5 % of the steps and decays linearly to 0; a >= 1e-4
  keep       the scales at the lowest loss seen (step 0 is RTN), folded in on fp32 working copies: a group's linears
             w * a[k], then a producing linear's columns / a[n] (and its bias), a producing norm's weight / a; every
             linear then goes through the device RTN: a plain RTN blob plus changed norm / projection weights, as with
             AWQ, nothing new for save / load or the engine

Two decisions differ from neural_compressor's training against the whole model's language-model loss:

  1. Training is block by block against the fp block's outputs (mean squared error), as autoround.py does: it fits
     calibration.py's walk, never holds more than one block's autograd graph and needs no labels. The next block
     trains on the fp stream.
  2. A column scale is left out of training. Where a group's producer is itself a quantised linear (v_proj for o_proj,
     up_proj for down_proj), that linear's output columns are divided by the consumer's a. A positive factor on a whole
     column commutes with the RTN rule in real arithmetic (the group scale takes the factor, the codes stay), so it
     changes nothing in that linear's quantisation error and gets no gradient from it; it enters only at the fold.

The loop and its minibatch draw are calibration.py's train_block, shared with autoround.py. torch does the GEMM-shaped parts, the
block's backward and Adam on purpose.
"""
import logging

import torch

from .... import qbits
from .calibration import (ABSORB_GROUPS, BITS, DEFAULT_BATCH, SCALE_MODEL_TYPES, SEED, absorb_groups, block_linears,
                          calibration_batches, capture_block_inputs, check_request, decoder_blocks, fake_quant_dtype,
                          fake_quant_forward, fp32_matmul, install_quantized, model_type, next_inputs, run_block,
                          train_block, weight_kn)

logger = logging.getLogger(__name__)

BETAS, EPS = (0.9, 0.9), 1e-8  # Adam, neural_compressor's TEQ values
WARMUP = 0.05                  # of the steps
FLOOR = 1e-4                   # of a, AWQ's floor


def validate_teq_request(model, config):
    """Everything about a request that can be refused without touching a device."""
    check_request(model, config, "TEQ", ("use_double_quant", "layer_wise", "absorb_to_layer"))
    if model_type(model) not in SCALE_MODEL_TYPES:
        raise NotImplementedError("TEQ folds its scales into Llama-class blocks (model_type %s), not model type %s"
                                  % (" / ".join(SCALE_MODEL_TYPES), model_type(model)))


def schedule(lr, t, steps):
    """the learning rate of step t: linear warm-up over the first WARMUP of the steps, then linear decay to zero at
    `steps`"""
    warm = int(WARMUP * steps)
    if t < warm:
        return lr * (t + 1) / warm
    return lr * (steps - t) / (steps - warm)


def fold_scales(block, weights, scales):
    """Fold `scales` {group index: a [K]} into the block, function-preserving: `weights` {name: [K, N] working copy}
    is changed in place (a group's linears w * a[k], then a producing linear's columns / a[n]); a producing linear's
    bias and a producing norm's weight are divided in the module, in their own dtype."""
    for gi, a in scales.items():
        for name in ABSORB_GROUPS[gi][0]:
            weights[name].mul_(a.to(weights[name].dtype)[:, None])
    for gi, a in scales.items():
        prev = ABSORB_GROUPS[gi][1]
        p = block.get_submodule(prev)
        if prev in weights:
            weights[prev].div_(a.to(weights[prev].dtype)[None, :])
            if p.bias is not None:
                p.bias.data.div_(a.to(p.bias.dtype))
        else:
            p.weight.data.div_(a.to(p.weight.dtype))


class _Quantiser:
    """one linear: its fp32 weight, the scale it sees and what the two launches need"""

    def __init__(self, module, a, group, bits, asym, dtype):
        self.w = weight_kn(module)
        self.a = a  # the group's trainable [K], or ones without grad
        self.group, self.bits, self.asym, self.dtype = group, bits, asym, dtype
        self.bias = module.bias.data if module.bias is not None else None
        self.wq = None
        self.da = None


class FakeQuant(torch.autograd.Function):
    """W~ of one linear: the forward is qbits.teq_forward, the backward qbits.teq_grad. The gradient is left on the
    quantiser, not returned: the group's sum is taken in ABSORB_GROUPS order by the training loop."""

    @staticmethod
    def forward(ctx, a, q):
        ctx.q = q
        return qbits.teq_forward(q.w, a.detach(), q.group, q.bits, q.asym, dtype=q.dtype)

    @staticmethod
    def backward(ctx, g):
        q = ctx.q
        q.da = qbits.teq_grad(q.w, q.a.detach(), g.contiguous(), q.group, q.bits, q.asym)
        return None, None


def block_trainer(quantisers, groups, steps, lr):
    """what calibration.train_block runs around its loss -> (begin_step, after_backward, snapshot). A quantiser in no
    trained group keeps one W~ for the whole loop, built here; begin_step builds the others'. after_backward sums every
    group's gradient in ABSORB_GROUPS order, takes the Adam step at the step's rate and keeps a at FLOOR or above."""
    params = [a for a, _ in groups.values()]
    opt = torch.optim.Adam(params, lr=lr, betas=BETAS, eps=EPS, weight_decay=0.0)
    trained = [q for q in quantisers if q.a.requires_grad]
    for q in quantisers:
        if not q.a.requires_grad:
            q.wq = FakeQuant.apply(q.a, q)

    def begin_step(t):
        for q in trained:
            q.wq = FakeQuant.apply(q.a, q)
        return trained

    def after_backward(t):
        for a, members in groups.values():
            grad = members[0].da
            for q in members[1:]:
                grad = grad + q.da
            a.grad = grad
        for pg in opt.param_groups:
            pg["lr"] = schedule(lr, t, steps)
        opt.step()
        with torch.no_grad():
            for a in params:
                a.clamp_(min=FLOOR)
        for q in quantisers:
            q.da = None

    return begin_step, after_backward, lambda: {gi: a.detach().clone() for gi, (a, _) in groups.items()}


def block_quantisers(linears, trained, group, bits, asym, dtype, device):
    """One trainable a [K] per group of `trained` (indices into ABSORB_GROUPS), one quantiser per linear -> (quantisers
    in `linears` order, {group index: (a, the group's quantisers in ABSORB_GROUPS order)}).
    A linear in no trained group sees a = 1 without grad."""
    modules, by_name, groups = dict(linears), {}, {}
    for gi in trained:
        names = ABSORB_GROUPS[gi][0]
        a = torch.ones(modules[names[0]].in_features, dtype=torch.float32, device=device).requires_grad_(True)
        for name in names:
            by_name[name] = _Quantiser(modules[name], a, group, bits, asym, dtype)
        groups[gi] = (a, [by_name[name] for name in names])
    for name, m in linears:
        if name not in by_name:
            ones = torch.ones(m.in_features, dtype=torch.float32, device=device)
            by_name[name] = _Quantiser(m, ones, group, bits, asym, dtype)
    return [by_name[name] for name, _ in linears], groups


@torch.no_grad()
def teq_quantize_model(model, config, device="cuda"):
    """Quantise every eligible linear of every decoder block of an fp model with TEQ, in place. Block by block: the fp
    block's outputs on the fp inputs are the targets; the block's linears run with the fake quantiser while the scales
    of its absorb groups take `config.train_steps` Adam steps; the best scales are folded in and every linear becomes
    its RTN blob. The next block trains on the fp outputs. `train_steps=0` is RTN through this path. lm_head and whatever
    else `llm_int8_skip_modules` names stay. model._teq_log: (rtn_loss, best_loss, best_step) per block;
    model._teq_scales: {group index: a} per block."""
    validate_teq_request(model, config)
    batch_size = int(getattr(config, "batch_size", DEFAULT_BATCH) or DEFAULT_BATCH)
    batches = calibration_batches(config, batch_size)
    path, blocks = decoder_blocks(model)
    skip = list(getattr(config, "llm_int8_skip_modules", None) or [])
    bits = BITS[config.weight_dtype]
    asym = not bool(config.sym)
    steps = max(0, int(getattr(config, "train_steps", 0)))
    lr = float(getattr(config, "lr", 1e-3))
    model.to(device)
    model.eval()
    inputs = capture_block_inputs(model, blocks, batches, device)
    gen = torch.Generator().manual_seed(SEED)
    model._teq_log, model._teq_scales = [], []
    with fp32_matmul():
        for li, block in enumerate(blocks):
            where = "%s.%d" % (path, li)
            linears = block_linears(block, where, skip)
            targets = run_block(block, inputs)
            entry, best = (None, None, -1), {}
            trained = absorb_groups(block, linears, where, "TEQ") if steps > 0 else []
            if trained:
                quantisers, groups = block_quantisers(linears, trained, config.group_size, bits, asym,
                                                      fake_quant_dtype(targets), device)
                with fake_quant_forward(linears, quantisers):
                    rtn_loss, best_loss, best_step, best = train_block(
                        block, inputs, targets, steps, batch_size, gen, *block_trainer(quantisers, groups, steps, lr))
                entry = (rtn_loss, best_loss, best_step)
                logger.info("TEQ %s: loss %.6g at step %d (RTN %.6g)", where, best_loss, best_step, rtn_loss)
                del quantisers, groups
            model._teq_log.append(entry)
            model._teq_scales.append(best)

            weights = {name: weight_kn(m) for name, m in linears}
            fold_scales(block, weights, best)
            for name, m in linears:
                install_quantized(block, name, m, config, device, fp_weight_kn=weights[name])
            del weights
            inputs = next_inputs(inputs, targets)
    return model
