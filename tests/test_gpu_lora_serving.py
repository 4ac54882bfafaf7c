"""Serving a fine-tuned int4 model with its LoRA adapter UNMERGED on the fused decode engine:
`optimize_transformers(model, adapters="unmerged")`, `model.generate`, `engine.set_lora(adapter_dir)`, NeuralChat's
`LoadingModelConfig(peft_on_engine=True)`. The models are the tiny random-init Llama of tests/test_gpu_qlora_model.py
with drawn adapters (tests/test_gpu_lora_engine.py `_wrapped`).

Greedy tokens. The engine's 8 tokens must equal the module path's. Equal tokens are only a fair demand where the
float64 twin (tests/lora_twin.py) separates its top two logits by more than twice the tolerance both paths are held to
(the prompt pass's 1e-2 max|logit| + 1e-3 for the first token, the decode step's 2e-3 max|logit| + 1e-4 afterwards, plus
the derived LoRA term); prompt and adapter seed were chosen on the CPU twin so that every one of the 8 steps does (the
smallest margin there is 7.5 times that), and the test asserts it on the twin of the weights it really runs.
"""
import numpy as np
import pytest
import torch

from tests import engine_stage_shadow as S
from tests import lora_twin as TW
from tests.test_gpu_lora_engine import ALL7, PROMPT, QV, _engine, _step_bytes, _wrapped

pytestmark = pytest.mark.gpu

N_NEW = 8


def _assert_margins(twin, prompt, what):
    toks, steps = twin.greedy(prompt, N_NEW)
    ratios = []
    for i, (margin, big, ltol) in enumerate(steps):
        tol = (1e-2 * big + 1e-3 if i == 0 else 2e-3 * big + 1e-4) + ltol
        ratios.append(margin / (2 * tol))
    print("\n%s: twin tokens %s, top-1 / top-2 margin over twice the tolerance per step: %s"
          % (what, toks, " ".join("%.1f" % r for r in ratios)))
    assert min(ratios) > 1.0, (what, ratios)
    return toks


@pytest.mark.parametrize("targets", [ALL7, QV], ids=["all-seven", "q-v"])
def test_generate_on_the_engine_equals_the_module_path(targets):
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from tests.test_gpu_qlora_model import _deq

    q, ad = _wrapped(targets)
    ids = torch.tensor([PROMPT], device="cuda")
    want_twin = _assert_margins(TW.twin_from_quantised(q, _deq, ad), PROMPT, "%d targets" % len(targets))
    module_path = q.generate(ids, max_new_tokens=N_NEW, do_sample=False)  # wrapped: the module path
    assert getattr(q, "woq_engine", None) is None and module_path.shape[1] == len(PROMPT) + N_NEW
    eng = optimize_transformers(q, max_ctx=64, adapters="unmerged")  # TypeError without the feature
    assert eng.lora_on and q.woq_engine is eng
    got = q.generate(ids, max_new_tokens=N_NEW, do_sample=False)
    assert q.woq_engine is eng and eng.lora_on, "generate left the engine"
    assert got[0].tolist() == module_path[0].tolist() == PROMPT + want_twin
    # the engine really produced them: its token log (slot p = the pick of the step that fed position p) holds the chain
    # from the second generated token on; the first is the prompt pass's pick
    assert eng.token_log()[len(PROMPT):len(PROMPT) + N_NEW - 1].tolist() == want_twin[1:]
    # without the adapter the chain is another one (the adapter is not decoration)
    eng.clear_lora()
    assert q.generate(ids, max_new_tokens=N_NEW, do_sample=False)[0].tolist() != got[0].tolist()


def test_default_still_refuses_and_names_both_ways():
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers

    q, _ = _wrapped(QV)
    with pytest.raises(RuntimeError, match=r"merge_and_unload\(\)") as e:
        optimize_transformers(q, max_ctx=64)
    assert 'adapters="unmerged"' in str(e.value)
    with pytest.raises(ValueError, match="adapters"):
        optimize_transformers(q, max_ctx=64, adapters="merged")
    assert getattr(q, "woq_engine", None) is None and q._woq_engine_off is True


def test_act_order_model_with_an_adapter_runs_on_the_engine():
    """a GPTQ act-order blob refuses `merge` ("Keep the adapter unmerged"): unmerged is its only way onto the engine"""
    from intel_extension_for_transformers_amd import qbits
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from intel_extension_for_transformers_amd.transformers import LoraConfig, get_peft_model
    from tests.test_gpu_qlora_model import _quantised, _tiny_llama

    q = _quantised(_tiny_llama())
    g = torch.Generator().manual_seed(4)
    # re-adopt every projection as an act-order blob: the module's own codes and scales under a drawn g_idx, one
    # permutation per group of projections that the engine fuses (q / k / v, gate / up)
    for layer in q.model.layers:
        perms = {}
        for name in TW.PROJ:
            m = getattr(layer.self_attn if name[0] in "qkvo" else layer.mlp, name)
            key = "qkv" if name in ("q_proj", "k_proj", "v_proj") else "gu" if name in ("gate_proj", "up_proj") else name
            K = m.in_features
            if key not in perms:
                perms[key] = (torch.randperm(K, generator=g) // m.blocksize).to(torch.int32)
            g_idx = perms[key]
            int_w, scales, zeros, _ = m.recover_qparms_kn()
            # rows regrouped in order of appearance, as set_weights_bias does before it repacks
            order = torch.argsort(g_idx.to(torch.int64), stable=True)
            blob = qbits.repack_quantized_weight((int_w - 8).to(torch.int8)[order.to(int_w.device)].contiguous(),
                                                 scales.contiguous(), torch.empty(0, dtype=torch.int8),
                                                 g_idx.to(int_w.device), m.weight_dtype, m.scale_dtype, m.compute_dtype,
                                                 False, m.blocksize)
            m._adopt(blob, None)
    q = get_peft_model(q, LoraConfig(r=4, lora_alpha=8, target_modules=["q_proj", "v_proj", "down_proj"]))
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for _, m in q.named_modules():
            if hasattr(m, "lora_B"):
                m.lora_B["default"].weight.copy_(0.1 * torch.randn(m.lora_B["default"].weight.shape, generator=gen))
    q.eval()
    with pytest.raises(RuntimeError, match="act-order"):
        q.model.layers[0].self_attn.q_proj.merge()
    eng = optimize_transformers(q, max_ctx=64, adapters="unmerged")
    assert eng.lora_on and not eng.uses_xq()  # act-order blobs take the fp32-activation step
    # Against the module path on the same blobs and adapters (fp32 modules with an fp32 head; the engine's head is fp16, a
    # relative 2^-11 per lm_head weight): the prompt-pass measure of tests/test_gpu_engine.py, 1e-2 max|ref| + 1e-3, for
    # the prompt pass's logits and for a decode step's. (The float64 twin is not used here: it multiplies by the
    # dequantised matrix as it lies in the blob, and an act-order blob holds its rows regrouped.)
    ids = torch.tensor([PROMPT], device="cuda")
    with torch.no_grad():
        ref = q(ids).logits[0, -1].double().cpu().numpy()
        nxt = int(ref.argmax())
        ref2 = q(torch.tensor([PROMPT + [nxt]], device="cuda")).logits[0, -1].double().cpu().numpy()
    got = eng.prefill(PROMPT, greedy=False)[0].double().cpu().numpy()
    eng.token.fill_(nxt)
    eng.pos.fill_(len(PROMPT))
    eng.step(greedy=False)
    got2 = eng.logits.double().cpu().numpy()
    r1 = float(np.abs(got - ref).max() / (1e-2 * np.abs(ref).max() + 1e-3))
    r2 = float(np.abs(got2 - ref2).max() / (1e-2 * np.abs(ref2).max() + 1e-3))
    eng.clear_lora()
    base = eng.prefill(PROMPT, greedy=False)[0].double().cpu().numpy()
    effect = float(np.abs(got - base).max() / (1e-2 * np.abs(ref).max() + 1e-3))
    print("\nact-order: err / tolerance prompt pass %.3f, decode step %.3f; adapter's effect / tolerance %.1f" % (r1, r2, effect))
    assert r1 <= 1.0 and r2 <= 1.0 and effect > 1.0


def test_adapter_directory_installs_the_same_bytes(tmp_path):
    q, eng, _ = _engine(ALL7)
    want = _step_bytes(eng)
    q.save_adapter(str(tmp_path / "adapter"))
    eng.clear_lora()
    assert S.first_difference(_step_bytes(eng), want) is not None
    eng.set_lora(str(tmp_path / "adapter"))
    assert eng.lora_on and S.first_difference(_step_bytes(eng), want) is None
    # the engine holds a copy: training on (here: zeroing lora_B) changes nothing until the next set_lora
    with torch.no_grad():
        for _, m in q.named_modules():
            if hasattr(m, "lora_B"):
                m.lora_B["default"].weight.zero_()
    assert S.first_difference(_step_bytes(eng), want) is None
    eng.set_lora(q)
    assert S.first_difference(_step_bytes(eng), want) is not None


def test_neural_chat_serves_the_adapter_on_the_engine(tmp_path):
    from intel_extension_for_transformers_amd.neural_chat import PipelineConfig, build_chatbot
    from intel_extension_for_transformers_amd.neural_chat.config import GenerationConfig, LoadingModelConfig
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from intel_extension_for_transformers_amd.transformers import RtnConfig
    from tests.test_gpu_api import _tiny_tokenizer
    from tests.test_gpu_qlora_model import VOCAB, _tiny_llama

    fp = _tiny_llama()
    q, _ = _wrapped(QV, fp=fp)
    d = tmp_path / "tiny-llama-chat"
    fp.save_pretrained(str(d))
    _tiny_tokenizer(d, VOCAB)
    q.save_adapter(str(tmp_path / "adapter"))

    def bot(**kw):
        return build_chatbot(PipelineConfig(model_name_or_path=str(d), device="cuda",
                                            optimization_config=RtnConfig(bits=4, group_size=32),
                                            loading_config=LoadingModelConfig(peft_path=str(tmp_path / "adapter"), **kw)))

    assert LoadingModelConfig().peft_on_engine is False
    off = bot()
    assert off.engine is None
    on = bot(peft_on_engine=True)
    assert on.engine is not None and on.engine.lora_on and on.model.woq_engine is on.engine
    pieces, _ = on.predict_stream("a b c", config=GenerationConfig(do_sample=False, max_new_tokens=6, repetition_penalty=1.0))
    text = "".join(pieces)
    assert text.strip() and on.engine.lora_on
    # the chatbot's engine carries exactly this adapter: its step leaves the bytes of an engine built here over the same
    # checkpoint's blobs with the same adapter installed from the wrapped model
    mine = optimize_transformers(q, max_ctx=on.engine.cfg.max_ctx, adapters="unmerged")
    assert S.first_difference(_step_bytes(on.engine), _step_bytes(mine)) is None
    on.engine.clear_lora()
    assert S.first_difference(_step_bytes(on.engine), _step_bytes(mine)) is not None
