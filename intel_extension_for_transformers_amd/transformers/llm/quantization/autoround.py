"""AutoRound calibration on the device: `from_pretrained(fp_model, quantization_config=AutoRoundConfig(...))`.

The reference hands this step to neural_compressor / auto-round (external; reference utils.py:531-702); here the method
(Cheng et al. 2023, "Optimize Weight Rounding via Signed Gradient Descent") is restated — tests/autoround_reference.py
is the float64 statement of its quantiser. Per linear the trainables are a rounding offset V [K, N] in [-0.5, 0.5]
(initially 0) and two range factors alpha, beta [G, N] in [0, 1] (initially 1); V = 0, alpha = beta = 1 is the
package's RTN. They are trained decoder block by decoder block with SignSGD against the fp block's outputs:

  forward    every eligible linear computes x.matmul(W~) + bias with W~ = qbits.autoround_forward(w, V, alpha, beta)
             (csrc/woq_autoround.hip), one launch per linear per iteration
  backward   autograd gives dL/dW~ (the block's own ops, torch); qbits.autoround_step turns it into the three gradients
             and applies p <- clamp(p - lr_t sign(grad)) in place, one launch per linear; lr_t = lr (1 - t / iters)
  keep       the parameters at the lowest loss seen (iteration 0 is RTN), then qbits.autoround_codes ->
             QuantizedLinearQBits.set_weights_bias, as gptq.py finishes: a plain blob, nothing new for save / load or
             the engine

A minibatch is drawn from the calibration batches (`calibration_batches`: rows of equal length, `batch_size` of them,
default 8): whole batches in a random order until `batch_size` samples are reached, from a torch.Generator seeded
with 42. torch does the GEMM-shaped parts and the block's backward on purpose, as in gptq.py.
"""
import logging

import torch

from .... import qbits
from .calibration import (BITS, DEFAULT_BATCH, SEED, block_linears, calibration_batches, capture_block_inputs,
                          check_request, decoder_blocks, fake_quant_dtype, fake_quant_forward, fp32_matmul,
                          install_quantized, next_inputs, run_block, train_block, weight_kn)

logger = logging.getLogger(__name__)


def validate_autoround_request(model, config):
    """Everything about a request that can be refused without touching a device."""
    check_request(model, config, "AutoRound", ("use_double_quant", "layer_wise", "quant_lm_head"), blocks_first=True)


def learning_rates(config):
    """(iters, lr, minmax_lr): lr defaults to 1 / iters, minmax_lr to lr"""
    iters = max(0, int(config.iters))
    lr = getattr(config, "lr", None)
    lr = (1.0 / iters if iters else 0.0) if lr is None else float(lr)
    mm = getattr(config, "minmax_lr", None)
    return iters, lr, (lr if mm is None else float(mm))


def schedule(lr, t, iters):
    """the learning rate of iteration t: linear decay to zero at `iters`"""
    return lr * (1.0 - t / iters)


class _Quantiser:
    """the trainables of one linear and what the two launches need"""

    def __init__(self, module, group, bits, asym, dtype):
        self.w = w = weight_kn(module)
        k, n = w.shape
        self.group, self.bits, self.asym, self.dtype = group, bits, asym, dtype
        # V is the tensor autograd sees (FakeQuant needs an input that requires grad); it never receives one
        self.v = torch.zeros(k, n, dtype=torch.float32, device=w.device).requires_grad_(True)
        self.alpha = torch.ones(qbits.rtn_groups(k, group)[1], n, dtype=torch.float32, device=w.device)
        self.beta = torch.ones_like(self.alpha)
        self.bias = module.bias.data if module.bias is not None else None
        self.lr_v = self.lr_mm = 0.0
        self.wq = None

    def params(self):
        return self.v.detach().clone(), self.alpha.clone(), self.beta.clone()


class FakeQuant(torch.autograd.Function):
    """W~ of one linear: the forward is qbits.autoround_forward, the backward the fused gradient + SignSGD step
    (qbits.autoround_step) on the quantiser's own tensors; no gradient is returned."""

    @staticmethod
    def forward(ctx, v, q):
        ctx.q = q
        return qbits.autoround_forward(q.w, v.detach(), q.alpha, q.beta, q.group, q.bits, q.asym, dtype=q.dtype)

    @staticmethod
    def backward(ctx, g):
        q = ctx.q
        qbits.autoround_step(q.w, q.v.detach(), q.alpha, q.beta, g.contiguous(), q.group, q.bits, q.asym, q.lr_v,
                             q.lr_mm)
        return None, None


def block_trainer(quantisers, iters, lr, minmax_lr):
    """what calibration.train_block runs around its loss -> (begin_step, after_backward, snapshot). begin_step sets the
    iteration's rates and builds every W~; the SignSGD step itself is FakeQuant's backward, nothing is left for after."""
    def begin_step(t):
        for q in quantisers:
            q.lr_v, q.lr_mm = schedule(lr, t, iters), schedule(minmax_lr, t, iters)
            q.wq = FakeQuant.apply(q.v, q)
        return quantisers

    return begin_step, lambda t: None, lambda: [q.params() for q in quantisers]


@torch.no_grad()
def autoround_quantize_model(model, config, device="cuda"):
    """Quantise every eligible linear of every decoder block of an fp model with AutoRound, in place. Block by block:
    the fp block's outputs on the fp inputs are the targets; the block's linears run with the fake quantiser while V,
    alpha and beta take `config.iters` SignSGD steps; the best parameters become the blob. With
    `disable_quanted_input=True` (the default) the next block trains on the fp outputs, otherwise on the outputs of the
    blocks quantised so far (two input lists), the targets still from the fp stream. `iters=0` is RTN through this path.
    lm_head and whatever else `llm_int8_skip_modules` names stay. model._autoround_log: (rtn_loss, best_loss, best_iter)
    per block."""
    validate_autoround_request(model, config)
    batch_size = int(getattr(config, "batch_size", DEFAULT_BATCH) or DEFAULT_BATCH)
    batches = calibration_batches(config, batch_size)
    path, blocks = decoder_blocks(model)
    skip = list(getattr(config, "llm_int8_skip_modules", None) or [])
    bits = BITS[config.weight_dtype]
    asym = not bool(config.sym)
    iters, lr, minmax_lr = learning_rates(config)
    fp_stream_only = bool(getattr(config, "disable_quanted_input", True))
    model.to(device)
    model.eval()
    inputs = capture_block_inputs(model, blocks, batches, device)
    gen = torch.Generator().manual_seed(SEED)
    q_inputs = inputs  # what the block trains on; the fp stream itself unless disable_quanted_input=False
    model._autoround_log = []
    with fp32_matmul():
        for li, block in enumerate(blocks):
            where = "%s.%d" % (path, li)
            linears = block_linears(block, where, skip)
            targets = run_block(block, inputs)
            dtype = fake_quant_dtype(targets)
            quantisers = [_Quantiser(m, config.group_size, bits, asym, dtype) for _, m in linears]
            entry = (None, None, -1)
            if iters > 0 and quantisers:
                with fake_quant_forward(linears, quantisers):
                    rtn_loss, best_loss, best_iter, best = train_block(
                        block, q_inputs, targets, iters, batch_size, gen,
                        *block_trainer(quantisers, iters, lr, minmax_lr))
                entry = (rtn_loss, best_loss, best_iter)
                logger.info("AutoRound %s: loss %.6g at iteration %d (RTN %.6g)", where, best_loss, best_iter, rtn_loss)
            else:
                best = [q.params() for q in quantisers]
            model._autoround_log.append(entry)

            for (name, m), q, (v, alpha, beta) in zip(linears, quantisers, best):
                codes, scales, zeros = qbits.autoround_codes(q.w, v, alpha, beta, config.group_size, bits, asym)
                install_quantized(block, name, m, config, device, codes=codes, scales=scales, zeros=zeros)
            del quantisers, best
            if not fp_stream_only:
                q_inputs = next_inputs(q_inputs, run_block(block, q_inputs))
            inputs = next_inputs(inputs, targets)
            if fp_stream_only:
                q_inputs = inputs
    return model
