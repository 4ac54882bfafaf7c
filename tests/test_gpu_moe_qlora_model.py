"""Gradient through the frozen experts of a quantised sparse layer: a two-layer Mixtral-type model
(tests/test_gpu_moe_model.py's config: H 128, I 96, E 4, k 2) quantised with RtnConfig(bits=4, group_size=32). The expert
weights of the random-init model are multiplied by EXPERT_GAIN before quantisation, so that the expert branch of a layer
carries a share of the gradient comparable to the residual branch's (at the initialiser's 0.02 it is a few per cent).
Reference and bound of the expert block: tests/moe_backward_reference.py (float64 autograd over the dequantised experts).
Before the backward existed the module's output had no grad_fn: the module test failed at `backward()`, and the whole-model
test at its allowance, which is what its last assertion shows.
"""
import copy

import numpy as np
import pytest
import torch

from tests import moe_backward_reference as BR
from tests import test_gpu_moe_model as M
from tests import test_gpu_qlora_model as QL

pytestmark = pytest.mark.gpu
EXPERT_GAIN = 8.0
_MODEL = []


def _deq(blob, transposed):
    from intel_extension_for_transformers_amd import qbits

    hdr = qbits.header_of(blob)
    out = torch.empty((hdr.N, hdr.K) if transposed else (hdr.K, hdr.N), dtype=torch.float32, device=blob.device)
    qbits.dequantize_packed_weight(blob, out, transposed, "fp32", "int4_clip", "fp32")
    return out.double().cpu()


def _model():
    """(fp model, its quantised copy with q_proj / v_proj adapters and gradient checkpointing, layer 0's expert module and
    that module's dequantised weights E x [H, 2I], E x [I, H] float64)"""
    from transformers import AutoModelForCausalLM as HF

    from intel_extension_for_transformers_amd.transformers import (AutoModelForCausalLM, LoraConfig, RtnConfig,
                                                                   get_peft_model, prepare_model_for_kbit_training)

    if not _MODEL:
        torch.manual_seed(17)
        fp = HF.from_config(M._config("mixtral")).float()
        with torch.no_grad():
            for p in fp.parameters():
                if p.dim() == 3:
                    p.mul_(EXPERT_GAIN)
        q = AutoModelForCausalLM.from_pretrained(copy.deepcopy(fp), quantization_config=RtnConfig(bits=4, group_size=32))
        q = get_peft_model(prepare_model_for_kbit_training(q, use_gradient_checkpointing=True),
                           LoraConfig(r=4, lora_alpha=8, target_modules=["q_proj", "v_proj"]))
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            for _, m in QL._lora(q):
                m.lora_B["default"].weight.copy_(0.05 * torch.randn(m.lora_B["default"].weight.shape, generator=g))
        q.train()  # HF checkpoints the layers in training mode only; the config has no dropout
        mod = sorted(M._experts_of(q).items())[0][1]
        _MODEL.append((fp, q, mod, [_deq(b, False).numpy() for b in mod.gate_up_blobs.view(torch.int8)],
                       [_deq(b, False).numpy() for b in mod.down_blobs.view(torch.int8)]))
    return _MODEL[0]


def _inputs(T, seed=5):
    g = torch.Generator().manual_seed(seed)
    x, dout = torch.randn(T, 128, generator=g), torch.randn(T, 128, generator=g)
    idx = torch.rand(T, 4, generator=g).argsort(1)[:, :2].contiguous()
    w = torch.rand(T, 2, generator=g)
    return x, idx, w, dout


def _module_reference(T):
    _, _, _, Wgu, Wdn = _model()
    x, idx, w, dout = (t.numpy() for t in _inputs(T))
    rx, rw = BR.reference(x, idx, w, dout, Wgu, Wdn)
    return (rx, rw) + BR.bound(x, idx, w, dout, Wgu, Wdn, rx)


# T = 9: the grouped form's forward; 80: the prompt form's; debug: the dequantise-and-torch arm (moe_experts_ref_impl)
@pytest.mark.parametrize("T,arm", [(9, "fused"), (80, "fused"), (9, "debug")])
def test_module_gradients_against_float64_autograd(T, arm, monkeypatch):
    if arm == "debug":
        monkeypatch.setenv("QBITS_DEBUG", "1")
    mod = _model()[2]
    x, idx, w, dout = _inputs(T)
    xd, wd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    out = mod(xd, idx.cuda(), wd)
    out.backward(dout.cuda())  # no grad_fn before the backward was built
    rx, rw, bx, bw = _module_reference(T)
    assert xd.grad.dtype == torch.float32 and wd.grad.dtype == torch.float32
    ex = np.abs(xd.grad.cpu().numpy().astype(np.float64) - rx) / bx
    ew = np.abs(wd.grad.cpu().numpy().astype(np.float64) - rw) / bw
    print("\nexperts module T=%d %s: worst |grad - ref| / bound dX %.3f dw %.3f" % (T, arm, ex.max(), ew.max()))
    assert ex.max() <= 1.0 and ew.max() <= 1.0


def test_without_grad_the_module_is_the_inference_call():
    from intel_extension_for_transformers_amd import qbits

    mod = _model()[2]
    x, idx, w, _ = _inputs(9)
    x, idx, w = x.cuda().requires_grad_(True), idx.cuda(), w.cuda()
    with torch.no_grad():
        got = mod(x, idx, w)
    ref = qbits.moe_forward(x.detach(), idx, w, mod.gate_up_blobs, mod.down_blobs)
    assert got.grad_fn is None and torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_a_call_above_the_chunk_size_equals_its_chunks():
    from intel_extension_for_transformers_amd import qbits

    mod = _model()[2]
    C = qbits.MOE_BACKWARD_CHUNK_TOKENS
    x, idx, w, dout = (t.cuda() for t in _inputs(C + 3))
    gx, gw = qbits.moe_backward(dout, x, idx, w, mod.gate_up_blobs, mod.down_blobs)
    parts = [qbits.moe_backward(dout[s], x[s], idx[s], w[s], mod.gate_up_blobs, mod.down_blobs)
             for s in (slice(0, C), slice(C, C + 3))]
    assert torch.equal(gx.view(torch.int32), torch.cat([p[0] for p in parts]).view(torch.int32))
    assert torch.equal(gw.view(torch.int32), torch.cat([p[1] for p in parts]).view(torch.int32))


def _twin(fp, q, dtype):
    """fp's architecture on the CPU in `dtype`: every quantised linear holds its dequantised weight (q_proj / v_proj with
    q's adapters, tests/test_gpu_qlora_model.py's _TwinLinear), the experts are HF's own module holding theirs"""
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    t = copy.deepcopy(fp).to(dtype).train()
    t.config._experts_implementation = "eager"
    for p in t.parameters():
        p.requires_grad_(False)
    for name, m in list(q.named_modules()):
        if isinstance(m, QuantizedLinearQBits) and hasattr(m, "lora_A"):
            lora = (m.lora_A["default"].weight.detach().cpu().to(dtype).clone(),
                    m.lora_B["default"].weight.detach().cpu().to(dtype).clone(), m.scaling)
            parent, _, leaf = name.rpartition(".")
            setattr(t.get_submodule(parent), leaf, QL._TwinLinear(_deq(m.weight.data, True).to(dtype), False, lora))
        elif isinstance(m, QuantizedLinearQBits):
            t.get_submodule(name).weight.data = _deq(m.weight.data, True).to(dtype)
    for name, m in M._experts_of(q).items():
        old = t.get_submodule(name)
        old.gate_up_proj.data = torch.stack([_deq(b, True) for b in m.gate_up_blobs.view(torch.int8)]).to(dtype)
        old.down_proj.data = torch.stack([_deq(b, True) for b in m.down_blobs.view(torch.int8)]).to(dtype)
    return t


def test_lora_gradients_of_the_whole_model_against_the_fp32_twin():
    """prepare_model_for_kbit_training (gradient checkpointing on) -> get_peft_model on q_proj / v_proj -> one
    loss.backward(); layer 0's lora A / B gradients against the fp32 twin. Allowance per tensor, nothing of it taken from
    the path under test: the spread |fp32 twin - float64 twin| of the reference itself, plus r max|ref| per sparse layer
    the gradient crosses (two), r = the expert block's derived bound over the largest reference gradient at this
    module (dX or dw, whichever is larger, tests/moe_backward_reference.py at T = 80).
    Measured (profiles/r27_moe_backward.txt): r = 0.123; spread 2e-9 .. 7e-8 against max|ref| 2.7e-3 .. 9.6e-2, so the
    allowance is 0.246 max|ref| per tensor; worst |got - ref| = 0.0053 of it (v_proj.A: 5.8e-5 against 1.09e-2); with the
    experts' gradient missing, as before the backward existed, every layer-0 tensor is off by 4.07 allowances (about
    max|ref| itself)."""
    fp, q, _, _, _ = _model()
    ids = QL._batch()
    rx, rw, bx, bw = _module_reference(80)
    r = max(bx.max() / np.abs(rx).max(), bw.max() / np.abs(rw).max())
    g32, g64 = (QL._lora_grads(_twin(fp, q, d), ids) for d in (torch.float32, torch.float64))
    got = QL._lora_grads(q, ids.cuda())
    experts = list(M._experts_of(q).values())
    for m in experts:  # the module as it was before the backward: no grad_fn, gradient through the residual branch only
        m.forward = m.inference_forward
    try:
        without = QL._lora_grads(q, ids.cuda())
    finally:
        for m in experts:
            del m.forward
    worst, worst_without = 0.0, 0.0
    for key in sorted(k for k in g32 if ".layers.0." in k):
        allow = float((g32[key] - g64[key]).abs().max() + 2 * r * g32[key].abs().max())
        err, miss = float((got[key] - g32[key]).abs().max()), float((without[key] - g32[key]).abs().max())
        print("%s: max|ref| %.3e spread %.3e allowance %.3e |got - ref| %.3e without the experts' gradient %.3e"
              % (key, g32[key].abs().max(), (g32[key] - g64[key]).abs().max(), allow, err, miss))
        worst, worst_without = max(worst, err / allow), max(worst_without, miss / allow)
    print("r %.4f; worst |got - ref| / allowance %.4f; without the experts' gradient %.2f" % (r, worst, worst_without))
    assert worst <= 1.0
    assert worst_without > 1.0  # else the comparison above would pass on a model whose experts pass no gradient
