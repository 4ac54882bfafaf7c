"""QLoRA end to end on the GPU: LoRA adapters over the blobs of a tiny random-init 2-layer Llama (no checkpoints, no
network), the gradient passing through every quantised projection by `qbits.woq_linear_backward`.

The twins: the same architecture with every quantised linear replaced by a dense one holding the dequantised weight,
(a) in float64 on the CPU: the reference; (b) the same with each such linear rounding the incoming gradient and the
weight to 11 significant bits in its backward: an emulation of the kernel's arithmetic written here, which says how
large an error that arithmetic alone produces; (c) in fp32 on the GPU, for the training comparison."""
import copy
import functools
import json
import os

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

VOCAB = 128
LORA = dict(r=4, lora_alpha=8)


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    # head_dim 64 is the decode engine's smallest: the merged model has to be one it takes
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=4, head_dim=64, vocab_size=VOCAB, max_position_embeddings=128,
                      rms_norm_eps=1e-5, tie_word_embeddings=False, attn_implementation="eager")
    return LlamaForCausalLM(cfg).float().eval()


def _quantised(fp=None):
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, RtnConfig

    return AutoModelForCausalLM.from_pretrained(copy.deepcopy(fp if fp is not None else _tiny_llama()),
                                                quantization_config=RtnConfig(bits=4, group_size=32))


def _batch():
    g = torch.Generator().manual_seed(3)
    return torch.randint(0, VOCAB, (2, 24), generator=g)


def _deq(module):
    from intel_extension_for_transformers_amd import qbits

    w = module.weight.data
    k, n = (int(qbits.acquire_packed_weight_info(w, t)[0]) for t in (2, 3))
    out = torch.empty(k, n, dtype=torch.float32, device=w.device)
    qbits.dequantize_packed_weight(w, out, False, module.compute_dtype, module.weight_dtype, module.scale_dtype)
    return out  # [K, N]


def _peft(q, seed=11, random_b=True):
    """adapters on q/k/v/o; random_b: lora_B drawn too, so that every adapter parameter has a gradient"""
    from intel_extension_for_transformers_amd.transformers import (LoraConfig, get_peft_model,
                                                                   prepare_model_for_kbit_training)

    q = get_peft_model(prepare_model_for_kbit_training(q), LoraConfig(**LORA))
    if random_b:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for _, m in _lora(q):
                m.lora_B["default"].weight.copy_(0.05 * torch.randn(m.lora_B["default"].weight.shape, generator=g))
    return q


def _lora(model):
    from intel_extension_for_transformers_amd.transformers import QuantizedLoraLinearQBits

    return [(n, m) for n, m in model.named_modules() if isinstance(m, QuantizedLoraLinearQBits)]


def _round11(x):
    """to 11 significant bits, round to nearest even: fp16's precision without its range"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)


class _EmulatedBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):  # w [N, K]
        ctx.save_for_backward(w)
        return x @ w.t()

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return _round11(g) @ _round11(w), None


class _TwinLinear(nn.Module):
    def __init__(self, w_nk, emulate, lora=None):
        super().__init__()
        self.register_buffer("w", w_nk)
        self.emulate = emulate
        self.scaling = 0.0
        if lora is not None:
            a, b, self.scaling = lora
            self.lora_a, self.lora_b = nn.Parameter(a), nn.Parameter(b)

    def forward(self, x):
        y = _EmulatedBackward.apply(x, self.w) if self.emulate else x @ self.w.t()
        if self.scaling:
            y = y + self.scaling * ((x @ self.lora_a.t()) @ self.lora_b.t())
        return y


def _twin(fp, q, dtype, device, emulate=False):
    """fp's architecture with every linear that q quantised holding q's dequantised weight (and q's adapters)"""
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    t = copy.deepcopy(fp).to(dtype=dtype, device=device)
    for p in t.parameters():
        p.requires_grad_(False)
    for name, m in list(q.named_modules()):
        if not isinstance(m, QuantizedLinearQBits):
            continue
        lora = None
        if hasattr(m, "lora_A"):
            lora = (m.lora_A["default"].weight.detach().to(dtype=dtype, device=device).clone(),
                    m.lora_B["default"].weight.detach().to(dtype=dtype, device=device).clone(), m.scaling)
        parent, _, leaf = name.rpartition(".")
        setattr(t.get_submodule(parent), leaf, _TwinLinear(_deq(m).t().to(dtype=dtype, device=device).contiguous(),
                                                           emulate, lora))
    t.get_input_embeddings().register_forward_hook(lambda mod, inp, out: out.requires_grad_(True))
    return t


def _loss(model, ids):
    return model(input_ids=ids, labels=ids).loss


def _lora_grads(model, ids):
    model.zero_grad(set_to_none=True)
    _loss(model, ids).backward()
    out = {}
    for n, p in model.named_parameters():
        if p.requires_grad:
            key = n.replace(".lora_A.default.weight", ".A").replace(".lora_B.default.weight", ".B")
            out[key.replace(".lora_a", ".A").replace(".lora_b", ".B")] = p.grad.detach().double().cpu()
    return out


@functools.lru_cache(maxsize=None)
def _setup():
    fp = _tiny_llama()
    q = _peft(_quantised(fp))
    return fp, q


def test_fresh_adapter_leaves_the_logits_bit_equal():
    fp = _tiny_llama()
    base = _quantised(fp)
    ids = _batch().cuda()
    with torch.no_grad():
        want = base(ids).logits.clone()
    q = _peft(base, random_b=False)
    with torch.no_grad():
        got = q(ids).logits
    assert torch.equal(got, want)
    with torch.enable_grad():  # the training form of the base projection runs the same forward
        got = q(ids).logits
    assert got.requires_grad and torch.equal(got.detach(), want)


def test_lora_gradients_vs_float64_twin():
    """relative Frobenius error of every adapter gradient against the float64 twin, held to 4x what the emulated
    arithmetic (gradient and weight rounded to 11 bits in every quantised linear's backward) gives, + 2^-20"""
    fp, q = _setup()
    ids = _batch()
    got = _lora_grads(q, ids.cuda())
    ref = _lora_grads(_twin(fp, q, torch.float64, "cpu"), ids)
    emu = _lora_grads(_twin(fp, q, torch.float64, "cpu", emulate=True), ids)
    assert set(got) == set(ref) == set(emu) and len(got) == 16
    worst = (0.0, 0.0, "")
    for k in sorted(ref):
        den = ref[k].norm().item()
        assert den > 0, k
        e_fused, e_emu = (got[k] - ref[k]).norm().item() / den, (emu[k] - ref[k]).norm().item() / den
        print("%-44s fused %.3e emulated %.3e" % (k, e_fused, e_emu))
        worst = max(worst, (e_fused, e_emu, k))
        assert e_fused <= 4 * e_emu + 2.0 ** -20, (k, e_fused, e_emu)
    print("worst fused %.3e (emulated %.3e) at %s" % worst)


def test_debug_backward_arm_agrees_with_the_fused_arm(monkeypatch):
    """one projection of the model, both arms of MatMulKBit's backward: the reference's dequantise-and-matmul statement
    (QBITS_DEBUG) against the kernel, within the kernel's bound plus the fp32 matmul's own N 2^-24 S"""
    from tests import woq_backward_reference as R

    _, q = _setup()
    m = q.model.layers[1].mlp.down_proj
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, m.in_features, generator=g).cuda().requires_grad_(True)
    G = torch.randn(37, m.out_features, generator=g).cuda()
    grads = {}
    for arm in ("fused", "debug"):
        if arm == "debug":
            monkeypatch.setenv("QBITS_DEBUG", "1")
        x.grad = None
        m(x).backward(G)
        grads[arm] = x.grad.detach().double().cpu().numpy()
    monkeypatch.delenv("QBITS_DEBUG")
    W = _deq(m).double().cpu().numpy()
    dY = G.double().cpu().numpy()
    ref, S = R.backward(dY, W)
    tol = R.bound(dY, W, S) + m.out_features * 2.0 ** -24 * S
    assert (abs(grads["fused"] - grads["debug"]) <= tol).all()
    assert (abs(grads["fused"] - ref) <= R.bound(dY, W, S)).all()


def test_ten_adam_steps_follow_the_fp32_twin():
    fp = _tiny_llama()
    q = _peft(_quantised(fp), random_b=False)
    twin = _twin(fp, q, torch.float32, "cuda")
    ids = _batch().cuda()
    losses = {}
    for name, model in (("fused", q), ("twin", twin)):
        model.train()
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
        first = None
        for _ in range(10):
            opt.zero_grad(set_to_none=True)
            loss = _loss(model, ids)
            first = loss.item() if first is None else first
            loss.backward()
            opt.step()
        with torch.no_grad():
            losses[name] = (first, _loss(model, ids).item())
    print("loss fused %.4f -> %.4f, fp32 twin %.4f -> %.4f" % (losses["fused"] + losses["twin"]))
    assert losses["fused"][1] < losses["fused"][0]
    assert abs(losses["fused"][1] - losses["twin"][1]) <= 0.05 * losses["twin"][1]


def test_save_and_load_adapter_in_pefts_format(tmp_path):
    from safetensors.torch import load_file

    fp, q = _setup()
    d = str(tmp_path / "adapter")
    q.save_adapter(d)
    cfg = json.load(open(os.path.join(d, "adapter_config.json")))
    assert cfg["peft_type"] == "LORA" and cfg["r"] == LORA["r"] and cfg["lora_alpha"] == LORA["lora_alpha"]
    assert cfg["target_modules"] == ["k_proj", "o_proj", "q_proj", "v_proj"] and cfg["lora_dropout"] == 0.0
    assert cfg["bias"] == "none" and cfg["task_type"] == "CAUSAL_LM" and "base_model_name_or_path" in cfg
    saved = load_file(os.path.join(d, "adapter_model.safetensors"))
    want = {"base_model.model.model.layers.%d.self_attn.%s.lora_%s.weight" % (l, p, ab)
            for l in range(2) for p in ("q_proj", "k_proj", "v_proj", "o_proj") for ab in "AB"}
    assert set(saved) == want
    other = _peft(_quantised(fp), seed=99)
    other.load_adapter(d)
    for (n, a), (_, b) in zip(_lora(q), _lora(other)):
        assert torch.equal(a.lora_A["default"].weight, b.lora_A["default"].weight), n
        assert torch.equal(a.lora_B["default"].weight, b.lora_B["default"].weight), n
    ids = _batch().cuda()
    with torch.no_grad():
        assert torch.equal(q(ids).logits, other(ids).logits)
    keys = [k for k in q.state_dict() if "lora_" in k]
    assert "model.layers.0.self_attn.q_proj.lora_A.default.weight" in keys


def test_merge_and_unload_engine_gate_and_generate():
    from intel_extension_for_transformers_amd import qbits
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    fp = _tiny_llama()
    q = _peft(_quantised(fp))
    with pytest.raises(RuntimeError, match=r"merge_and_unload\(\)"):
        optimize_transformers(q, max_ctx=64)
    ids = _batch()[:1, :6].cuda()
    with torch.no_grad():
        nxt = int(q(ids).logits[0, -1].argmax())
    out = q.generate(ids, max_new_tokens=3, do_sample=False)  # unmerged: the module path
    assert out.shape[1] == 9 and int(out[0, 6]) == nxt and getattr(q, "woq_engine", None) is None
    want = {}
    for n, m in _lora(q):
        w = _deq(m).t() + m.scaling * (m.lora_B["default"].weight @ m.lora_A["default"].weight)
        want[n] = qbits.quantize_to_packed_weight(w.contiguous(), True, m.blocksize, m.compute_dtype, m.weight_dtype,
                                                  m.scale_dtype, m.scheme == "asym")
    q.merge_and_unload()
    assert not _lora(q)
    for n, blob in want.items():
        m = q.get_submodule(n)
        assert type(m) is QuantizedLinearQBits and torch.equal(m.weight.data, blob), n
    eng = optimize_transformers(q, max_ctx=64)
    assert eng is not None


def test_merge_refuses_act_order_blobs_and_bad_configs():
    from intel_extension_for_transformers_amd.transformers import LoraConfig, QuantizedLoraLinearQBits
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits
    from tests import woq_backward_reference as R

    with pytest.raises(ValueError, match="bias"):
        LoraConfig(bias="all")
    d = R.weight(384, 200, 128, "int4_clip", False, True)
    base = QuantizedLinearQBits(384, 200, bias=False, blocksize=128, scale_dtype="fp32", compute_dtype="fp32")
    e8 = torch.empty(0, dtype=torch.int8)
    from intel_extension_for_transformers_amd import qbits

    base._adopt(qbits.repack_quantized_weight(torch.from_numpy(d["q"].copy()).cuda(), torch.from_numpy(d["s"].copy()).cuda(),
                                              e8, torch.from_numpy(d["g_idx"].copy()).cuda(), "int4_clip", "fp32", "fp32",
                                              False, 128), None)
    m = QuantizedLoraLinearQBits(base, r=2, lora_alpha=4)
    assert m.weight is base.weight  # adopted, not copied
    with pytest.raises(RuntimeError, match="act-order"):
        m.merge()
    # and its gradient still lands un-shuffled
    x = torch.randn(5, 384, device="cuda", requires_grad=True)
    G = torch.randn(5, 200, device="cuda")
    m(x).backward(G)
    ref, S = R.backward(G.double().cpu().numpy(), d["W"], d["shuffle"])
    # lora_B is zero: the adapter adds nothing to dX
    assert (abs(x.grad.double().cpu().numpy() - ref) <= R.bound(G.double().cpu().numpy(), d["W"], S)).all()


def test_gradient_checkpointing_gives_the_same_gradients():
    from intel_extension_for_transformers_amd.transformers import (LoraConfig, get_peft_model,
                                                                   prepare_model_for_kbit_training)

    fp, q = _setup()
    ids = _batch().cuda()
    q.train()
    plain = _lora_grads(q, ids)
    ck = get_peft_model(prepare_model_for_kbit_training(_quantised(fp), use_gradient_checkpointing=True),
                        LoraConfig(**LORA))
    with torch.no_grad():
        for (_, a), (_, b) in zip(_lora(q), _lora(ck)):
            b.lora_A["default"].weight.copy_(a.lora_A["default"].weight)
            b.lora_B["default"].weight.copy_(a.lora_B["default"].weight)
    ck.train()
    assert ck.is_gradient_checkpointing
    got = _lora_grads(ck, ids)
    q.eval()
    for k in plain:
        assert torch.equal(got[k], plain[k]), k


def test_neural_chat_loads_the_adapter_from_peft_path(tmp_path):
    from intel_extension_for_transformers_amd.neural_chat import PipelineConfig, build_chatbot
    from intel_extension_for_transformers_amd.neural_chat.config import LoadingModelConfig
    from intel_extension_for_transformers_amd.transformers import RtnConfig
    from tests.test_gpu_api import _tiny_tokenizer

    fp, q = _setup()
    d = tmp_path / "tiny-llama-chat"
    fp.save_pretrained(str(d))
    _tiny_tokenizer(d, VOCAB)
    q.save_adapter(str(tmp_path / "adapter"))
    bot = build_chatbot(PipelineConfig(model_name_or_path=str(d), device="cuda",
                                       optimization_config=RtnConfig(bits=4, group_size=32),
                                       loading_config=LoadingModelConfig(peft_path=str(tmp_path / "adapter"))))
    assert bot.engine is None and len(_lora(bot.model)) == 8
    # the same checkpoint loaded the way NeuralChat loads it, without and with the adapter
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM
    from intel_extension_for_transformers_amd.transformers.llm.quantization.lora import load_peft_adapter

    twin = AutoModelForCausalLM.from_pretrained(str(d), quantization_config=RtnConfig(bits=4, group_size=32),
                                                device_map="cuda").eval()
    ids = _batch().cuda()
    with torch.no_grad():
        got = bot.model(ids).logits
        base = twin(ids).logits.clone()
        want = load_peft_adapter(twin, str(tmp_path / "adapter"))(ids).logits
    assert torch.equal(got, want) and not torch.equal(got, base)
    for (n, a), (_, b) in zip(_lora(q), _lora(bot.model)):
        assert torch.equal(a.lora_B["default"].weight, b.lora_B["default"].weight), n
