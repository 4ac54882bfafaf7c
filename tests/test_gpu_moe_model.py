"""Sparse mixture-of-experts models through `from_pretrained(..., RtnConfig(bits=4, group_size=32))`: random-init
MixtralForCausalLM (H 128, I 96, E 4, k 2) and Qwen3MoeForCausalLM (E 8, k 3, norm_topk_prob=False), 2 layers, vocab 128,
4 heads, 2 kv heads. Logits of a 7-token prompt against a float64 twin of the HF model in which every quantised weight,
linears and experts alike, holds its dequantised values; the bound is tests/test_gpu_model_coverage.py's model-level
2e-3 * max|ref| + 1e-4.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEOM = dict(hidden_size=128, num_hidden_layers=2, vocab_size=128, num_attention_heads=4, num_key_value_heads=2,
            head_dim=32, max_position_embeddings=64, tie_word_embeddings=False)
PROMPT = [5, 99, 23, 64, 7, 120, 41]
_CASES = {}


def _config(kind):
    from transformers import MixtralConfig, Qwen3MoeConfig

    if kind == "mixtral":
        return MixtralConfig(**GEOM, intermediate_size=96, num_local_experts=4, num_experts_per_tok=2)
    return Qwen3MoeConfig(**GEOM, intermediate_size=96, moe_intermediate_size=96, num_experts=8, num_experts_per_tok=3,
                          norm_topk_prob=False)


def _experts_of(model):
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.moe import QuantizedMoEExpertsQBits

    return {n: m for n, m in model.named_modules() if isinstance(m, QuantizedMoEExpertsQBits)}


def _twin(path, qmodel):
    """the fp model of `path` in float64 (HF's own expert loop) with every quantised weight replaced by its dequantised values"""
    from transformers import AutoModelForCausalLM

    from intel_extension_for_transformers_amd import qbits
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    def deq(blob):
        hdr = qbits.header_of(blob)
        out = torch.empty(hdr.N, hdr.K, dtype=torch.float32, device=blob.device)
        qbits.dequantize_packed_weight(blob, out, True, "fp32", "int4_clip", "fp32")
        return out.double().cpu()

    twin = AutoModelForCausalLM.from_pretrained(path, torch_dtype=torch.float64).eval()
    twin.config._experts_implementation = "eager"
    for name, mod in qmodel.named_modules():
        if isinstance(mod, QuantizedLinearQBits):
            twin.get_submodule(name).weight.data = deq(mod.weight.data)
    for name, mod in _experts_of(qmodel).items():
        old = twin.get_submodule(name)
        old.gate_up_proj.data = torch.stack([deq(b) for b in mod.gate_up_blobs.view(torch.int8)])
        old.down_proj.data = torch.stack([deq(b) for b in mod.down_blobs.view(torch.int8)])
    return twin


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    def get(kind):
        from transformers import AutoModelForCausalLM as HF

        from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, RtnConfig

        if kind not in _CASES:
            path = str(tmp_path_factory.mktemp(kind))
            torch.manual_seed(17)
            HF.from_config(_config(kind)).float().save_pretrained(path)
            q = AutoModelForCausalLM.from_pretrained(path, quantization_config=RtnConfig(bits=4, group_size=32))
            with torch.no_grad():
                ref = _twin(path, q)(torch.tensor([PROMPT])).logits[0].numpy()
            ref.setflags(write=False)
            _CASES[kind] = (path, q, ref)
        return _CASES[kind]

    yield get
    _CASES.clear()


def _logits(q):
    with torch.no_grad():
        return q(torch.tensor([PROMPT], device="cuda")).logits[0].float().cpu().numpy()


def _within(got, ref, what):
    err, bound = float(np.abs(got - ref).max()), 2e-3 * float(np.abs(ref).max()) + 1e-4
    print("\n%s: err / bound %.4f" % (what, err / bound))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_experts_are_quantised_and_logits_match_the_twin(cases, kind):
    _, q, ref = cases(kind)
    experts = _experts_of(q)
    assert len(experts) == 2 and all(m.grouped_supported() for m in experts.values())
    assert not [n for n, p in q.named_parameters() if p.dim() == 3 and p.is_floating_point()]
    _within(_logits(q), ref, kind + " grouped form")
    for m in experts.values():  # the same prompt, longer than the limit: the loop form
        m.grouped_max_tokens = len(PROMPT) - 1
    try:
        _within(_logits(q), ref, kind + " loop form")
    finally:
        for m in experts.values():
            del m.grouped_max_tokens


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_save_and_load_give_the_same_blobs_and_logits(cases, kind, tmp_path):
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM

    _, q, _ = cases(kind)
    q.save_pretrained(str(tmp_path))
    q2 = AutoModelForCausalLM.from_pretrained(str(tmp_path))
    a, b = _experts_of(q), _experts_of(q2)
    assert sorted(a) == sorted(b) and len(b) == 2
    for name in a:
        assert torch.equal(a[name].gate_up_blobs, b[name].gate_up_blobs), name
        assert torch.equal(a[name].down_blobs, b[name].down_blobs), name
    assert np.array_equal(_logits(q).view(np.uint32), _logits(q2).view(np.uint32))


def test_calibrated_methods_refuse_expert_weights():
    from transformers import AutoModelForCausalLM as HF

    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, GPTQConfig

    with pytest.raises(NotImplementedError, match="mixture-of-experts"):
        AutoModelForCausalLM.from_pretrained(HF.from_config(_config("mixtral")), quantization_config=GPTQConfig(bits=4))
