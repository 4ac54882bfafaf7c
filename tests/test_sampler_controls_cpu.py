"""CPU checks of the sampler controls (logit bias, presence / frequency penalty, min_p): the torch restatement
(`runtime.engine.DeviceSampler`) against the installed transformers' own classes in HF's order and against the numpy
float32 restatement (tests/sampler_controls_reference.py) bit for bit; the reference's min_p cut against the torch one;
the C ABI's new entry points in the headers, the binding and INTEGRATION.md; how `model.generate`'s options map."""
import os
import re

import numpy as np
import pytest
import torch

from tests import sampler_controls_reference as C
from tests import sampler_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(rng, vocab, neg_inf=False):
    logits = (4 * rng.standard_normal(vocab)).astype(np.float32)
    if neg_inf:
        logits[rng.choice(vocab, vocab // 10, replace=False)] = -np.inf
    prompt = rng.choice(vocab, 40, replace=False)
    generated = rng.choice(vocab, 60, replace=True)
    generated[:12] = generated[12]          # one id generated 13 times
    generated[20:25] = prompt[:5]           # ids that are in the prompt too
    top = np.argsort(-logits)[:6]
    generated[30:33] = top[:3]              # the penalties bite among the best ids
    bias = {int(i): float(v) for i, v in zip(rng.choice(vocab, 30, replace=False), 3 * rng.standard_normal(30))}
    bias[int(top[3])] = float("-inf")
    bias[int(top[4])] = 4.0
    bias[int(generated[0])] = -0.5
    return logits, prompt, generated, bias


def _hf_chain(model, n_in, **options):
    """the processors and warpers the INSTALLED transformers builds for these generate options, in ITS order"""
    from transformers import GenerationConfig, LogitsProcessorList

    return model._get_logits_processor(generation_config=GenerationConfig(**options), input_ids_seq_length=n_in,
                                       encoder_input_ids=None, prefix_allowed_tokens_fn=None,
                                       logits_processor=LogitsProcessorList(), device="cpu")


def test_device_sampler_equals_the_transformers_classes_in_their_order():
    """The chain comes from transformers' own `_get_logits_processor`, so the order of the sequence bias, the repetition
    penalty and the warpers (min_p after top-k / top-p today) is the installed release's, not this file's."""
    from transformers import LlamaConfig, LlamaForCausalLM

    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler

    model = LlamaForCausalLM(LlamaConfig(hidden_size=16, intermediate_size=16, num_hidden_layers=1, num_attention_heads=2,
                                         num_key_value_heads=2, vocab_size=64))
    rng = np.random.default_rng(11)
    for vocab, kw in [(1000, dict(temperature=0.9, top_k=40, top_p=0.9, repetition_penalty=1.1, min_p=0.05)),
                      (3001, dict(temperature=0.7, top_k=0, top_p=1.0, repetition_penalty=1.2, min_p=0.1)),
                      (3001, dict(temperature=1.3, top_k=50, top_p=1.0, repetition_penalty=1.0, min_p=0.5)),
                      (777, dict(temperature=2.0, top_k=0, top_p=0.8, repetition_penalty=1.3, min_p=0.02)),
                      (500, dict(temperature=1.0, top_k=8, top_p=0.95, repetition_penalty=1.1, min_p=1.0))]:
        for trial in range(3):
            logits, prompt, generated, bias = _case(rng, vocab, neg_inf=bool(trial & 1))
            history = np.concatenate([prompt, generated])
            chain = _hf_chain(model, len(history), do_sample=True, sequence_bias={(i,): v for i, v in bias.items()}, **kw)
            names = [type(p).__name__ for p in chain]
            assert "SequenceBiasLogitsProcessor" in names and "MinPLogitsWarper" in names and len(names) >= 3, names
            want = chain(torch.from_numpy(history)[None], torch.from_numpy(logits)[None].clone())[0]
            got = DeviceSampler(do_sample=True, logit_bias=bias, **kw).processed(
                torch.from_numpy(logits), torch.from_numpy(history), torch.from_numpy(generated))
            assert torch.equal(got, want), (vocab, kw, trial)
            assert 1 <= int(torch.isfinite(got).sum()) < vocab
    # not sampling: the bias and the penalty alone, and the argmax of those
    logits, prompt, generated, bias = _case(rng, 2000)
    chain = _hf_chain(model, len(prompt), do_sample=False, repetition_penalty=1.3,
                      sequence_bias={(i,): v for i, v in bias.items()})
    assert len(chain) == 2
    want = chain(torch.from_numpy(prompt)[None], torch.from_numpy(logits)[None].clone())[0]
    got = DeviceSampler(do_sample=False, repetition_penalty=1.3, logit_bias=bias).processed(
        torch.from_numpy(logits), torch.from_numpy(prompt))
    assert torch.equal(got, want)


def test_device_sampler_penalties_equal_the_numpy_restatement_bit_for_bit():
    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler

    rng = np.random.default_rng(5)
    for vocab, rep, pres, freq, temp in [(1000, 1.1, 0.7, 0.35, 0.9), (3001, 0.8, -1.25, -0.15, 0.1),
                                         (50257, 1.0, 2.0, 2.0, 1.7), (777, 1.3, 0.0, 0.5, 1.0), (777, 1.3, 0.5, 0.0, 0.6)]:
        logits, prompt, generated, bias = _case(rng, vocab, neg_inf=vocab == 3001)
        logits[rng.choice(vocab, 3)] = np.nan
        history = np.concatenate([prompt, generated])
        counts = np.bincount(generated, minlength=vocab)
        for do_sample in (False, True):
            want = C.scores_f32(logits, history, counts, rep, temp, do_sample, pres, freq, bias)
            got = DeviceSampler(do_sample=do_sample, temperature=temp, repetition_penalty=rep, presence_penalty=pres,
                                frequency_penalty=freq, logit_bias=bias).processed(
                torch.from_numpy(logits), torch.from_numpy(history), torch.from_numpy(generated)).numpy()
            assert C.same_bits(got, want), (vocab, rep, pres, freq, do_sample)
        # the prompt does not count: without generated tokens only the bias and the repetition penalty act
        want = C.adjusted_f32(logits, history, np.zeros(vocab, np.int64), rep, pres, freq, bias)
        got = DeviceSampler(repetition_penalty=rep, presence_penalty=pres, frequency_penalty=freq, logit_bias=bias
                            ).processed(torch.from_numpy(logits), torch.from_numpy(history), torch.from_numpy(generated[:0]))
        assert C.same_bits(got.numpy(), want)
    # -0.0 survives where there is no entry, and a (+0.0) entry turns it into +0.0
    z = np.array([-0.0, -0.0, -0.0, 1.0], dtype=np.float32)
    out = C.adjusted_f32(z, [], np.zeros(4, np.int64), 1.0, 0.0, 0.0, {1: 0.0, 2: -0.0})
    assert np.signbit(out).tolist() == [True, False, True, False]


def test_reference_min_p_cut_keeps_what_the_torch_restatement_keeps():
    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler

    rng = np.random.default_rng(3)
    for vocab, kw in [(1000, dict(temperature=0.9, top_k=40, top_p=0.9, repetition_penalty=1.1)),
                      (3001, dict(temperature=0.8, top_k=0, top_p=1.0, repetition_penalty=1.1)),
                      (5000, dict(temperature=1.5, top_k=1024, top_p=1.0, repetition_penalty=1.0))]:
        for min_p in (0.0, 0.05, 0.5, 1.0):
            logits, prompt, generated, bias = _case(rng, vocab)
            history = np.concatenate([prompt, generated])
            counts = np.bincount(generated, minlength=vocab)
            s = C.scores_f32(logits, history, counts, kw["repetition_penalty"], kw["temperature"], True, 0.4, 0.1, bias)
            ref = C.choose(s, kw["top_k"], kw["top_p"], min_p, max_candidates=1 << 30)
            assert ref.boundary_margin > 1e-4 and ref.min_p_units > 1e3  # fp32 softmax vs float64: far from both cuts
            got = DeviceSampler(do_sample=True, presence_penalty=0.4, frequency_penalty=0.1, min_p=min_p, logit_bias=bias,
                                **kw).processed(torch.from_numpy(logits), torch.from_numpy(history),
                                                torch.from_numpy(generated))
            kept = set(torch.nonzero(torch.isfinite(got)).reshape(-1).tolist())
            mass = np.diff(np.concatenate([[0.0], ref.cdf])) > 0
            assert kept == set(int(i) for i in ref.ids[mass]), (vocab, min_p)
            assert len(kept) == ref.n_mass
            if min_p == 1.0:
                assert len(kept) == 1
    # the reference without min_p is sampler_reference.choose itself
    s = (4 * rng.standard_normal(2000)).astype(np.float32)
    a, b = C.choose(s, 40, 0.9), R.choose(s, 40, 0.9)
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.cdf, b.cdf)


def test_abi_and_binding_carry_the_controls_entry_points():
    import ctypes

    from intel_extension_for_transformers_amd import _lib

    header = open(os.path.join(ROOT, "include", "woq_hip.h")).read()
    declared = set(re.findall(r"WOQ_API[^;(]*?\b(woq_\w+)\s*\(", header))
    new = {"woq_engine_set_sampler_controls", "woq_engine_sampler_counts", "woq_engine_sampler_count_ptr"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    exp = open(os.path.join(ROOT, "include", "woq_hip_experimental.h")).read()
    assert re.search(r"WOQ_API int woq_probe_sample_controls\(", exp)
    assert "woq_probe_sample_controls" in _lib.EXPERIMENTAL_EXPORTS
    assert "#define WOQ_ABI_VERSION 4" in header
    body = re.search(r"typedef struct woq_sampler_controls \{(.*?)\} woq_sampler_controls;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(float|int32_t|uint32_t)\b", body) == ["float", "float", "int32_t", "uint32_t"]
    assert "presence_penalty, frequency_penalty" in body and "reserved[4]" in body
    assert ctypes.sizeof(_lib.SamplerControls) == 32 and ctypes.sizeof(_lib.SamplerConfig) == 32
    assert [n for n, _t in _lib.SamplerControls._fields_] == ["presence_penalty", "frequency_penalty", "min_p", "n_bias",
                                                              "reserved"]
    ctl, ids, vals = _lib.sampler_controls(0.5, -0.25, 0.05, {9: float("-inf"), 3: 1.5})
    assert (ctl.presence_penalty, ctl.frequency_penalty, ctl.n_bias) == (0.5, -0.25, 2) and abs(ctl.min_p - 0.05) < 1e-8
    assert list(ids) == [3, 9] and list(vals) == [1.5, float("-inf")]
    ctl, ids, vals = _lib.sampler_controls()
    assert ctl.n_bias == 0 and ids is None and vals is None
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in new | {"woq_sampler_controls", "woq_probe_sample_controls"}:
        assert name in integration, name


def test_a_bias_the_engine_cannot_take_keeps_the_module_loop_even_when_greedy():
    """A multi-token `sequence_bias` on a greedy request must reach HF's loop (which applies it), not the engine's plain
    greedy chain (which would ignore it)."""
    import types

    from intel_extension_for_transformers_amd.transformers.modeling import modeling_auto

    calls = []
    fake = types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=100, token_latency=False),
                                 generation_config=types.SimpleNamespace(), token_latency=False,
                                 _woq_hf_generate=lambda *a, **kw: calls.append(kw) or "hf")
    ids = torch.tensor([[1, 2, 3]])
    for bias in ({(7, 8): -5.0}, {(100,): -1.0}, {(7,): "x"}):
        assert modeling_auto._engine_generate(fake, ids, max_new_tokens=4, sequence_bias=bias) == "hf"
        assert calls[-1]["sequence_bias"] == bias
    assert len(calls) == 3


def test_generate_options_map_onto_the_logit_bias():
    from intel_extension_for_transformers_amd.transformers.modeling.modeling_auto import _single_token_bias as f

    inf = float("inf")
    assert f(None, None, 100) == {}
    assert f({(7,): -inf, (3,): 2.0}, None, 100) == {7: -inf, 3: 2.0}
    assert f([[[7], -1.5]], [4, 5], 100) == {7: -1.5, 4: -inf, 5: -inf}
    assert f({(7,): 1.0}, [7], 100) == {7: -inf}
    assert f({(7, 8): -1.0}, None, 100) is None        # several tokens: HF's loop
    assert f({(100,): -1.0}, None, 100) is None        # outside the vocabulary: HF's loop refuses it
    assert f({(7,): inf}, None, 100) is None
    assert f({(7,): "x"}, None, 100) is None


def test_device_sampler_refuses_a_min_p_outside_the_unit_interval():
    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler

    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            DeviceSampler(do_sample=True, min_p=bad)


def test_the_module_loop_fallback_refuses_what_it_cannot_apply():
    from intel_extension_for_transformers_amd.neural_chat import GenerationConfig
    from intel_extension_for_transformers_amd.neural_chat.models.base_model import BaseModel

    bot = BaseModel.__new__(BaseModel)
    for kw in (dict(presence_penalty=0.5), dict(frequency_penalty=-0.5), dict(logit_bias={3: -100.0})):
        with pytest.raises(RuntimeError, match="QBits:"):
            next(BaseModel._hf_stream(bot, None, GenerationConfig(**kw), [0]))
