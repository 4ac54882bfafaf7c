"""AutoRound calibration end to end on the GPU: `from_pretrained(fp_model, quantization_config=AutoRoundConfig(...))`
on tiny random-init models (no checkpoints, no network): a 2-layer Llama-class model with grouped-query attention and
a 2-layer GPT-2 (Conv1D)."""
import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ITERS = 20


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    # head_dim 64 (the decode engine's smallest), 4 query heads on 2 kv heads: k / v project 128 -> 128
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=64, vocab_size=256, max_position_embeddings=128,
                      rms_norm_eps=1e-5, tie_word_embeddings=False)
    model = LlamaForCausalLM(cfg).float().eval()
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


def _config(**kw):
    from intel_extension_for_transformers_amd.transformers import AutoRoundConfig

    kw.setdefault("calib_dataloader", _calib())
    cfg = AutoRoundConfig(bits=4, group_size=32, n_samples=8, seq_len=32, **kw)
    cfg.batch_size = 8  # every step sees all samples
    return cfg


def _convert(fp, cfg):
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM

    return AutoModelForCausalLM.from_pretrained(copy.deepcopy(fp), quantization_config=cfg)


def _quantised(model):
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    return [(n, m) for n, m in model.named_modules() if isinstance(m, QuantizedLinearQBits)]


def _deq(module):
    from intel_extension_for_transformers_amd import qbits

    w = module.weight.data
    k, n = (int(qbits.acquire_packed_weight_info(w, t)[0]) for t in (2, 3))
    out = torch.empty(k, n, dtype=torch.float32, device=w.device)
    qbits.dequantize_packed_weight(w, out, False, module.compute_dtype, module.weight_dtype, module.scale_dtype)
    return out


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("make", [_tiny_llama, _tiny_gpt2])
def test_zero_iterations_are_rtn(make, sym):
    """iters=0: every quantised linear's dequantised weight and scales equal the RtnConfig model's, bit for bit"""
    from intel_extension_for_transformers_amd import qbits
    from intel_extension_for_transformers_amd.transformers import RtnConfig

    fp = make()
    ar = _convert(fp, _config(iters=0, sym=sym))
    rtn = _convert(fp, RtnConfig(bits=4, group_size=32, sym=sym))
    names = [n for n, _ in _quantised(ar)]
    assert len(names) == (14 if make is _tiny_llama else 8)
    assert "lm_head" not in names and ar._autoround_log == [(None, None, -1)] * 2
    for n in names:
        a, r = ar.get_submodule(n), rtn.get_submodule(n)
        assert torch.equal(_deq(a), _deq(r)), n
        assert torch.equal(qbits.acquire_packed_weight_info(a.weight.data, 9),
                           qbits.acquire_packed_weight_info(r.weight.data, 9)), n


@functools.lru_cache(maxsize=None)
def _trained(kind, sym):
    """one conversion at iters=20 with the parameters the driver kept, recorded at the call that makes the codes"""
    from intel_extension_for_transformers_amd import qbits

    kept = []
    codes = qbits.autoround_codes

    def record(w, v, alpha, beta, group, bits, asym):
        kept.append((w.clone(), v.clone(), alpha.clone(), beta.clone(), group, bits, asym))
        return codes(w, v, alpha, beta, group, bits, asym)

    fp = _tiny_llama() if kind == "llama" else _tiny_gpt2()
    qbits.autoround_codes = record
    try:
        model = _convert(fp, _config(iters=ITERS, sym=sym))
    finally:
        qbits.autoround_codes = codes
    return fp, model, kept


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_training_lowers_the_block_loss(kind, sym):
    from intel_extension_for_transformers_amd import qbits

    fp, model, kept = _trained(kind, sym)
    log = model._autoround_log
    print("%s sym=%d: (rtn loss, best loss, best iteration) per block: %s" % (kind, sym, log))
    assert len(log) == 2
    for rtn_loss, best_loss, best_iter in log:
        assert math.isfinite(rtn_loss) and math.isfinite(best_loss) and 0 <= best_iter < ITERS
        assert best_loss <= rtn_loss  # the same data every step, and iteration 0 is kept as the best so far
    assert any(best < rtn for rtn, best, _ in log)
    # every swapped-in blob is the quantiser at the kept parameters
    mods = _quantised(model)
    assert len(mods) == len(kept) == (14 if kind == "llama" else 8)
    moved = 0
    for (name, m), (w, v, alpha, beta, group, bits, asym) in zip(mods, kept):
        assert (group, bits, asym) == (32, 4, not sym)
        assert torch.equal(_deq(m), qbits.autoround_forward(w, v, alpha, beta, group, bits, asym)), name
        assert float(v.abs().max()) <= 0.5 and float(alpha.min()) >= 0 and float(alpha.max()) <= 1
        moved += int((v != 0).any())
    assert moved > 0
    assert type(model.lm_head).__name__ == "Linear"


def test_a_second_conversion_gives_the_same_bytes():
    fp, model, _ = _trained("llama", False)
    again = _convert(fp, _config(iters=ITERS, sym=False))
    assert again._autoround_log == model._autoround_log
    for (n, a), (_, b) in zip(_quantised(model), _quantised(again)):
        assert torch.equal(a.weight.data, b.weight.data), n


def test_training_on_the_quantised_stream():
    """disable_quanted_input=False: the second block trains on the first quantised block's outputs, the targets still
    from the fp stream; its loss at iteration 0 is therefore not the fp-stream run's"""
    fp, base, _ = _trained("llama", False)
    model = _convert(fp, _config(iters=ITERS, sym=False, disable_quanted_input=False))
    log = model._autoround_log
    print("quantised stream: %s (fp stream: %s)" % (log, base._autoround_log))
    for rtn_loss, best_loss, _ in log:
        assert math.isfinite(rtn_loss) and math.isfinite(best_loss) and best_loss <= rtn_loss
    assert log[0][0] == base._autoround_log[0][0] and log[1][0] != base._autoround_log[1][0]
    with torch.no_grad():
        assert torch.isfinite(model(torch.tensor([[5, 17, 200]], device="cuda")).logits).all()


def test_round_trip_and_the_decode_engine(tmp_path):
    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM

    _, qmodel, _ = _trained("llama", False)
    probe = torch.tensor([[5, 17, 200, 3, 77, 9]], device="cuda")
    with torch.no_grad():
        logits = qmodel(probe).logits.float()
    qmodel.save_pretrained(str(tmp_path / "q"))
    back = AutoModelForCausalLM.from_pretrained(str(tmp_path / "q"))
    with torch.no_grad():
        assert torch.equal(back(probe).logits.float(), logits)

    # the decode engine builds on the result and agrees with the module path (the bound tests/test_gpu_awq_model.py uses)
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


def test_texts_with_a_tokenizer_calibrate_too():
    class Tok:
        def __call__(self, text):
            return {"input_ids": [ord(c) % 256 for c in text]}

    texts = ["the quick brown fox jumps over the lazy dog " * 2, "pack my box with five dozen liquor jugs " * 2]
    from intel_extension_for_transformers_amd.transformers import AutoRoundConfig

    cfg = AutoRoundConfig(bits=4, group_size=32, dataset=texts, tokenizer=Tok(), n_samples=2, seq_len=48, iters=4)
    qmodel = _convert(_tiny_llama(), cfg)
    assert len(_quantised(qmodel)) == 14 and len(qmodel._autoround_log) == 2
    with torch.no_grad():
        assert torch.isfinite(qmodel(torch.tensor([[5, 17, 200]], device="cuda")).logits).all()


def test_neural_chat_pipeline_with_an_autoround_config(tmp_path):
    """PipelineConfig(optimization_config=AutoRoundConfig(...)) -> build_chatbot: the model is calibrated at load time,
    the decode engine builds on it and a greedy request answers the same through the engine and the module path."""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    from intel_extension_for_transformers_amd.neural_chat import GenerationConfig, PipelineConfig, build_chatbot
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
    opt = _config(iters=4, scale_dtype="fp16")
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
