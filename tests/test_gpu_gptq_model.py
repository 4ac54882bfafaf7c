"""GPTQ calibration end to end on the GPU: `gptq_quantize_weight` on whole matrices against the float64 reference
(tests/gptq_reference.py), and `from_pretrained(fp_model, quantization_config=GPTQConfig(...))` on tiny random-init
models (no checkpoints, no network)."""
import numpy as np
import pytest
import torch

from tests import gptq_reference as G
from tests import quant_reference as Q

pytestmark = pytest.mark.gpu

# loss_dev / loss_ref over the weight-level cases below, measured on the MI355X (profiles/r13_gptq.txt; the codes came
# out identical to the float64 reference's in all twelve, what is left is the fp32 rounding of the scales, of U and of
# the errors): tr(D H D^T) within 1.7e-7 of 1, the sweep's own sum err^2 / 2 within 7.9e-7. Each bound is 1 + 16 x the
# largest measured |ratio - 1| (the cap of 1 + 1e-3 is not reached). A wrong element of U or a missing trailing update
# moves either by tens of percent.
LOSS_RATIO_MARGIN = 16 * 1.7e-7
SWEEP_LOSS_MARGIN = 16 * 7.9e-7


@pytest.mark.parametrize("desc_act,static_groups", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("K,N,sym", [(256, 96, True), (384, 200, True), (256, 96, False)])
def test_weight_level_loss(K, N, sym, desc_act, static_groups):
    from intel_extension_for_transformers_amd.transformers.llm.quantization.gptq import gptq_quantize_weight

    group, bits = 64, 4
    w, H = G.correlated(K, N, seed=K)
    if K == 384:
        H[5], H[:, 5] = 0.0, 0.0  # a dead feature: its row of the weight is dropped, H stays invertible
    ref = G.quantize_weight(w, H, bits, group, sym, damp_percent=0.01, desc_act=desc_act, static_groups=static_groups)
    q, scales, zeros, g_idx, loss = gptq_quantize_weight(torch.from_numpy(w).cuda(), torch.from_numpy(H).cuda(), bits,
                                                         group, sym, 128, 0.01, desc_act, static_groups)
    assert q.dtype == torch.int8 and tuple(q.shape) == (K, N) and tuple(scales.shape) == (K // group, N)
    assert (zeros is None) == sym
    gi = None
    if desc_act and not static_groups:
        gi = g_idx.cpu().numpy()
        assert gi.shape == (K,) and np.bincount(gi, minlength=K // group).tolist() == [group] * (K // group)
        assert np.array_equal(gi, ref["g_idx"])
    else:
        assert g_idx is None
    deq = G.dequantize(q.cpu().numpy(), scales.cpu().numpy(), zeros.cpu().numpy() if zeros is not None else None, group,
                       gi)
    w_used = np.array(w, np.float64)
    if K == 384:
        w_used[5] = 0.0
        assert (deq[5] == 0).all()
    Hd = ref["Hd"]
    loss_dev, loss_ref = G.hessian_loss(w_used, deq, Hd), G.hessian_loss(w_used, ref["deq"], Hd)
    loss_rtn = G.hessian_loss(w_used, Q.quantize(w_used, group, G.WNAME[bits], not sym)["deq"], Hd)
    ratio = loss_dev / loss_ref
    print("gptq weight K=%d N=%d sym=%d desc_act=%d static=%d: loss dev %.6f ref %.6f rtn %.6f dev/ref %.8f codes "
          "differing %d sum err^2 / 2 dev/ref %.8f" % (K, N, sym, desc_act, static_groups, loss_dev, loss_ref, loss_rtn,
                                                        ratio, int((q.cpu().numpy() + (0 if sym else 8) != ref["q"]).sum()),
                                                        loss / ref["loss"]))
    assert loss_dev < loss_rtn
    assert abs(ratio - 1) <= LOSS_RATIO_MARGIN
    assert abs(loss / ref["loss"] - 1) <= SWEEP_LOSS_MARGIN


# ---- model level -------------------------------------------------------------------------------------------------
def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    # head_dim 64 (the decode engine's smallest) on 4 heads: q / k / v project 128 -> 256, o_proj 256 -> 128
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=4, head_dim=64, vocab_size=256, max_position_embeddings=128,
                      rms_norm_eps=1e-5, tie_word_embeddings=False)
    return LlamaForCausalLM(cfg).float().eval()


def _tiny_gpt2():
    from transformers import GPT2Config, GPT2LMHeadModel

    torch.manual_seed(0)
    return GPT2LMHeadModel(GPT2Config(n_embd=128, n_layer=2, n_head=4, vocab_size=256, n_positions=64)).float().eval()


def _calib():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, 256, (4, 32), generator=g) for _ in range(2)]  # 8 samples of 32 ids


def _applied_weight(module, k):
    """[K, N] float64: the weight a quantised linear applies, read off its own forward on the unit vectors (whatever
    row order the blob keeps inside)"""
    with torch.no_grad():
        y = module(torch.eye(k, device="cuda"))
        if module.bias is not None:
            y = y - module.bias.float()
    return y.double().cpu().numpy()


def _first_linear_loss(fp, qmodel, x, name):
    """tr(D H D^T) of the named first-block linear under H = 2 / T X^T X of its own fp inputs x [T, K], in float64"""
    m_fp = fp.get_submodule(name)
    w = m_fp.weight.detach().double().cpu().numpy()
    w = w if type(m_fp).__name__ == "Conv1D" else w.T
    x = x.double().cpu().numpy()
    H = 2.0 / x.shape[0] * (x.T @ x)
    return G.hessian_loss(w, _applied_weight(qmodel.get_submodule(name), w.shape[0]), H)


def _convert(fp, cfg):
    import copy

    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM

    return AutoModelForCausalLM.from_pretrained(copy.deepcopy(fp), quantization_config=cfg)


@pytest.mark.parametrize("sym,desc_act", [(True, False), (True, True), (False, False), (False, True)])
def test_llama_from_pretrained_gptq(tmp_path, sym, desc_act):
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, GPTQConfig, RtnConfig
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    fp = _tiny_llama()
    calib = _calib()
    qmodel = _convert(fp, GPTQConfig(bits=4, group_size=32, sym=sym, desc_act=desc_act, damp_percent=0.01,
                                     calib_dataloader=calib, n_samples=8, seq_len=32, batch_size=4,
                                     scale_dtype="fp16"))
    linears = [n for n, m in fp.named_modules() if isinstance(m, torch.nn.Linear) and n.startswith("model.layers.")]
    assert len(linears) == 14
    for n in linears:
        assert isinstance(qmodel.get_submodule(n), QuantizedLinearQBits), n
    assert type(qmodel.lm_head) is torch.nn.Linear

    # layer 0's q_proj sees input_layernorm(embed(ids)): under that Hessian GPTQ beats round-to-nearest
    rtn = _convert(fp, RtnConfig(bits=4, group_size=32, sym=sym, scale_dtype="fp16"))
    with torch.no_grad():
        ids = torch.cat(calib)
        x = fp.model.layers[0].input_layernorm(fp.model.embed_tokens(ids)).reshape(-1, 128)
    name = "model.layers.0.self_attn.q_proj"
    loss_gptq, loss_rtn = _first_linear_loss(fp, qmodel, x, name), _first_linear_loss(fp, rtn, x, name)
    print("llama q_proj sym=%d desc_act=%d: loss gptq %.6g rtn %.6g" % (sym, desc_act, loss_gptq, loss_rtn))
    assert loss_gptq < loss_rtn

    # save -> load: the same logits
    probe = torch.tensor([[5, 17, 200, 3, 77, 9]], device="cuda")
    with torch.no_grad():
        logits = qmodel(probe).logits.float()
    qmodel.save_pretrained(str(tmp_path / "q"))
    back = AutoModelForCausalLM.from_pretrained(str(tmp_path / "q"))
    with torch.no_grad():
        assert torch.equal(back(probe).logits.float(), logits)

    # the decode engine builds on the result and agrees with the module path (as tests/test_gpu_api.py holds RTN models)
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


def test_gpt2_conv1d_from_pretrained_gptq():
    from intel_extension_for_transformers_amd.transformers import GPTQConfig, RtnConfig
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    fp = _tiny_gpt2()
    calib = _calib()
    qmodel = _convert(fp, GPTQConfig(bits=4, group_size=32, damp_percent=0.01, calib_dataloader=calib, n_samples=8,
                                     seq_len=32, batch_size=4))
    convs = [n for n, m in fp.named_modules() if type(m).__name__ == "Conv1D"]
    assert len(convs) == 8
    for n in convs:
        assert isinstance(qmodel.get_submodule(n), QuantizedLinearQBits), n
    rtn = _convert(fp, RtnConfig(bits=4, group_size=32))
    with torch.no_grad():
        ids = torch.cat(calib)
        pos = torch.arange(ids.shape[1])
        x = fp.transformer.h[0].ln_1(fp.transformer.wte(ids) + fp.transformer.wpe(pos)).reshape(-1, 128)
    name = "transformer.h.0.attn.c_attn"
    loss_gptq, loss_rtn = _first_linear_loss(fp, qmodel, x, name), _first_linear_loss(fp, rtn, x, name)
    print("gpt2 c_attn: loss gptq %.6g rtn %.6g" % (loss_gptq, loss_rtn))
    assert loss_gptq < loss_rtn
    with torch.no_grad():
        assert torch.isfinite(qmodel(torch.tensor([[5, 17, 200]], device="cuda")).logits).all()


def test_texts_with_a_tokenizer_calibrate_too():
    from intel_extension_for_transformers_amd.transformers import GPTQConfig
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    class Tok:
        def __call__(self, text):
            return {"input_ids": [ord(c) % 256 for c in text]}

    texts = ["the quick brown fox jumps over the lazy dog " * 2, "pack my box with five dozen liquor jugs " * 2]
    qmodel = _convert(_tiny_llama(), GPTQConfig(bits=4, group_size=32, dataset=texts, tokenizer=Tok(), n_samples=2,
                                                seq_len=48, batch_size=1))
    assert isinstance(qmodel.model.layers[1].mlp.down_proj, QuantizedLinearQBits)


def test_unsupported_options_raise_by_name():
    from intel_extension_for_transformers_amd.transformers import GPTQConfig

    for option in ("use_mse_search", "true_sequential", "use_double_quant", "layer_wise"):
        with pytest.raises(NotImplementedError, match=option):
            _convert(_tiny_llama(), GPTQConfig(bits=4, group_size=32, calib_dataloader=_calib(), **{option: True}))


def test_neural_chat_pipeline_with_a_gptq_config(tmp_path):
    """PipelineConfig(optimization_config=GPTQConfig(...)) -> build_chatbot: the model is calibrated at load time, the
    decode engine builds on it and a greedy request answers the same through the engine and the module path."""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    from intel_extension_for_transformers_amd.neural_chat import GenerationConfig, PipelineConfig, build_chatbot
    from intel_extension_for_transformers_amd.transformers import GPTQConfig
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
    opt = GPTQConfig(bits=4, group_size=32, desc_act=True, damp_percent=0.01, calib_dataloader=_calib(), n_samples=8,
                     seq_len=32, batch_size=4, scale_dtype="fp16")
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
