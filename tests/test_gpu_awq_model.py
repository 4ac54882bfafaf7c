"""AWQ calibration end to end on the GPU: `from_pretrained(fp_model, quantization_config=AwqConfig(...))` on tiny
random-init models (no checkpoints, no network)."""
import copy
import math

import pytest
import torch

from tests import awq_reference as A

pytestmark = pytest.mark.gpu


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    # head_dim 64 (the decode engine's smallest) on 4 heads: q / k / v project 128 -> 256, o_proj 256 -> 128
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=4, head_dim=64, vocab_size=256, max_position_embeddings=128,
                      rms_norm_eps=1e-5, tie_word_embeddings=False)
    model = LlamaForCausalLM(cfg).float().eval()
    # norm weights spread log-uniformly over [0.25, 8]: some input channels of q / k / v and gate / up are salient
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for layer in model.model.layers:
            for norm in (layer.input_layernorm, layer.post_attention_layernorm):
                norm.weight.copy_(torch.exp(torch.empty(128).uniform_(math.log(0.25), math.log(8.0), generator=g)))
    return model


def _tiny_gpt2():
    from transformers import GPT2Config, GPT2LMHeadModel

    torch.manual_seed(0)
    return GPT2LMHeadModel(GPT2Config(n_embd=128, n_layer=2, n_head=4, vocab_size=256, n_positions=64)).float().eval()


def _calib():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, 256, (8, 32), generator=g)]  # 8 samples of 32 ids


def _convert(fp, cfg):
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM

    return AutoModelForCausalLM.from_pretrained(copy.deepcopy(fp), quantization_config=cfg)


def _applied_weight(module, k):
    """[K, N] float64: the weight a quantised linear applies, read off its own forward on the unit vectors"""
    with torch.no_grad():
        y = module(torch.eye(k, device="cuda"))
        if module.bias is not None:
            y = y - module.bias.float()
    return y.double().cpu().numpy()


def _loss(fp_module, q_module, H, s=None, s_out=None):
    """tr(D^T H D) in float64, D = the weight the quantised module applies to the ORIGINAL input (its own input is the
    original divided by s; its outputs were divided by s_out for the next linear to undo) minus the fp weight"""
    w = fp_module.weight.detach().double().cpu().numpy()
    w = w if type(fp_module).__name__ == "Conv1D" else w.T
    eff = _applied_weight(q_module, w.shape[0])
    if s is not None:
        eff = eff / s[:, None]
    if s_out is not None:
        eff = eff * s_out[None, :]
    return A.loss_from_h(eff - w, H)


@pytest.mark.parametrize("zero_point", [True, False])
def test_llama_from_pretrained_awq(tmp_path, monkeypatch, zero_point):
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, AwqConfig, RtnConfig
    from intel_extension_for_transformers_amd.transformers.llm.quantization import awq
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    folded = []  # per block, the scales the driver folds in: {absorb group index: s}
    fold = awq.apply_scales
    monkeypatch.setattr(awq, "apply_scales", lambda block, scales: (folded.append(dict(scales)), fold(block, scales))[1])
    fp = _tiny_llama()
    calib = _calib()
    qmodel = _convert(fp, AwqConfig(bits=4, group_size=32, zero_point=zero_point, calib_dataloader=calib, n_samples=8,
                                    seq_len=32))
    linears = [n for n, m in fp.named_modules() if isinstance(m, torch.nn.Linear) and n.startswith("model.layers.")]
    assert len(linears) == 14
    for n in linears:
        assert isinstance(qmodel.get_submodule(n), QuantizedLinearQBits), n
    assert type(qmodel.lm_head) is torch.nn.Linear

    # layer 0's q / k / v see input_layernorm(embed(ids)); the AWQ model feeds them that input divided by the scale it
    # folded into the norm, s = fp norm weight / AWQ norm weight. Under H of the fp inputs the summed output error of the
    # three is what the scale search minimised (candidate 0 being RTN), and v_proj is clipped on top. v_proj's OUTPUT
    # columns also carry 1 / (o_proj's scale), which o_proj's input columns undo: that one is taken from the driver
    # (no norm holds it) and multiplied back, so that v_proj is compared as the function it stands for.
    rtn = _convert(fp, RtnConfig(bits=4, group_size=32, sym=not zero_point))
    with torch.no_grad():
        x = fp.model.layers[0].input_layernorm(fp.model.embed_tokens(torch.cat(calib))).reshape(-1, 128)
    H, _ = A.stats(x.double().numpy())
    s = (fp.model.layers[0].input_layernorm.weight.detach().double()
         / qmodel.model.layers[0].input_layernorm.weight.detach().double().cpu()).numpy()
    assert s.max() / s.min() > 1.5  # a scale was found: the norm moved
    assert len(folded) == 2 and sorted(folded[0]) == [0, 1, 2, 3]
    assert abs(folded[0][0].double().cpu().numpy() / s - 1).max() <= 2.0 ** -22  # the norm took 1 / s, to fp32 rounding
    s_o = folded[0][1].double().cpu().numpy()
    loss_awq = loss_rtn = 0.0
    for leaf in ("q_proj", "k_proj", "v_proj"):
        name = "model.layers.0.self_attn." + leaf
        loss_awq += _loss(fp.get_submodule(name), qmodel.get_submodule(name), H, s, s_o if leaf == "v_proj" else None)
        loss_rtn += _loss(fp.get_submodule(name), rtn.get_submodule(name), H)
    print("llama layer 0 q+k+v zero_point=%d: loss awq %.6g rtn %.6g, scale spread %.2f" % (zero_point, loss_awq, loss_rtn,
                                                                                          s.max() / s.min()))
    assert loss_awq < loss_rtn

    # save -> load: the same logits
    probe = torch.tensor([[5, 17, 200, 3, 77, 9]], device="cuda")
    with torch.no_grad():
        logits = qmodel(probe).logits.float()
    qmodel.save_pretrained(str(tmp_path / "q"))
    back = AutoModelForCausalLM.from_pretrained(str(tmp_path / "q"))
    with torch.no_grad():
        assert torch.equal(back(probe).logits.float(), logits)

    # the decode engine builds on the result and agrees with the module path (the bound tests/test_gpu_gptq_model.py uses)
    eng = optimize_transformers(qmodel, max_ctx=64, kv_dtype=torch.float16)
    prompt = [5, 17, 200, 3, 77]
    pids = torch.tensor([prompt], device="cuda")
    with torch.no_grad():
        ref_logits = qmodel(pids).logits[0, -1].float()
        ref_out = qmodel._woq_hf_generate(pids, max_new_tokens=6, do_sample=False)[0, len(prompt):].tolist()
    for i, t in enumerate(prompt):
        eng.token.fill_(t)
        eng.pos.fill_(i)
        eng.step(greedy=False)
    got = eng.logits.float()
    assert (got - ref_logits).abs().max().item() <= 2e-3 * ref_logits.abs().max().item() + 1e-4
    assert eng.generate(prompt, 6) == ref_out


def test_gpt2_conv1d_from_pretrained_awq_clip_only():
    from intel_extension_for_transformers_amd.transformers import AwqConfig, RtnConfig
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    fp = _tiny_gpt2()
    calib = _calib()
    qmodel = _convert(fp, AwqConfig(bits=4, group_size=32, auto_scale=False, calib_dataloader=calib, n_samples=8,
                                    seq_len=32))
    convs = [n for n, m in fp.named_modules() if type(m).__name__ == "Conv1D"]
    assert len(convs) == 8
    for n in convs:
        assert isinstance(qmodel.get_submodule(n), QuantizedLinearQBits), n
    rtn = _convert(fp, RtnConfig(bits=4, group_size=32, sym=False))
    with torch.no_grad():
        ids = torch.cat(calib)
        pos = torch.arange(ids.shape[1])
        x = fp.transformer.h[0].ln_1(fp.transformer.wte(ids) + fp.transformer.wpe(pos)).reshape(-1, 128)
    H, _ = A.stats(x.double().numpy())
    name = "transformer.h.0.attn.c_attn"
    loss_awq = _loss(fp.get_submodule(name), qmodel.get_submodule(name), H)
    loss_rtn = _loss(fp.get_submodule(name), rtn.get_submodule(name), H)
    print("gpt2 c_attn: loss awq (clip only) %.6g rtn %.6g" % (loss_awq, loss_rtn))
    # the clip search keeps candidate 0 (RTN) in every cell unless another is better under this very H
    assert loss_awq <= loss_rtn
    with torch.no_grad():
        assert torch.isfinite(qmodel(torch.tensor([[5, 17, 200]], device="cuda")).logits).all()


def test_texts_with_a_tokenizer_calibrate_too():
    from intel_extension_for_transformers_amd.transformers import AwqConfig
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    class Tok:
        def __call__(self, text):
            return {"input_ids": [ord(c) % 256 for c in text]}

    texts = ["the quick brown fox jumps over the lazy dog " * 2, "pack my box with five dozen liquor jugs " * 2]
    qmodel = _convert(_tiny_llama(), AwqConfig(bits=4, group_size=32, dataset=texts, tokenizer=Tok(), n_samples=2,
                                               seq_len=48))
    assert isinstance(qmodel.model.layers[1].mlp.down_proj, QuantizedLinearQBits)
    with torch.no_grad():
        assert torch.isfinite(qmodel(torch.tensor([[5, 17, 200]], device="cuda")).logits).all()


def test_neural_chat_pipeline_with_an_awq_config(tmp_path):
    """PipelineConfig(optimization_config=AwqConfig(...)) -> build_chatbot: the model is calibrated at load time, the
    decode engine builds on it and a greedy request answers the same through the engine and the module path."""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    from intel_extension_for_transformers_amd.neural_chat import GenerationConfig, PipelineConfig, build_chatbot
    from intel_extension_for_transformers_amd.transformers import AwqConfig
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    d = tmp_path / "tiny-llama-chat"
    fp = _tiny_llama()
    fp.generation_config.eos_token_id = None  # random-init model: never stop early
    fp.save_pretrained(str(d))
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2}
    vocab.update({"w%d" % i: i for i in range(3, fp.config.vocab_size)})
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    PreTrainedTokenizerFast(tokenizer_object=tk, unk_token="<unk>", bos_token="<s>",
                            eos_token="</s>").save_pretrained(str(d))
    opt = AwqConfig(bits=4, group_size=32, calib_dataloader=_calib(), n_samples=8, seq_len=32, scale_dtype="fp16")
    bot = build_chatbot(PipelineConfig(model_name_or_path=str(d), device="cuda", optimization_config=opt))
    assert bot.engine is not None
    assert isinstance(bot.model.model.layers[0].mlp.down_proj, QuantizedLinearQBits)
    cfg = GenerationConfig(max_new_tokens=8, do_sample=False, repetition_penalty=1.0)
    text = bot.predict("w5 w17 w200 w3 w77", config=cfg)
    assert len(text.split()) == 8
    bot_engine, bot.engine = bot.engine, None
    bot.model._woq_engine_off = True
    try:
        assert bot.predict("w5 w17 w200 w3 w77", config=cfg) == text
    finally:
        bot.engine = bot_engine
        bot.model._woq_engine_off = False
