"""build_rope_tables' scaled parameterisations and engine_supports, without a GPU.

The tables: `linear`, `llama3` and `yarn` against the float64 restatement of tests/rope_reference.py, head_dim 64 and
128, positions 0..511 with original_max_position_embeddings 64 (llama3's low / high frequency bands and its smooth
band, yarn's ramp and both of its ends are all hit). The bound is HF's own: the table's largest error against float64
must not exceed twice the error of HF's fp32 rotary module against the same reference at the same positions — both are
fp32 evaluations of one formula, only the operation order may differ. Measured (profiles/r14_model_coverage.txt): the
tables are bit-equal to HF's module in every case, so the two errors are the same number.
"""
import types

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd.runtime.engine import (ENGINE_MODEL_TYPES, build_rope_tables, engine_supports,
                                                                 engine_window, rope_inv_freq)
from intel_extension_for_transformers_amd.runtime.tp import tp_supports
from tests import rope_reference as RR

N_POS, ORIG, THETA = 512, 64, 10000.0
SCALINGS = {
    "linear": {"rope_type": "linear", "factor": 4.0},
    "llama3": {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
               "original_max_position_embeddings": ORIG},
    "yarn": {"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": ORIG},
}


def _hf_tables(head_dim, rs):
    """cos / sin [N_POS, head_dim / 2] of HF's LlamaRotaryEmbedding in fp32"""
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding

    cfg = LlamaConfig(hidden_size=4 * head_dim, num_attention_heads=4, num_key_value_heads=4, head_dim=head_dim,
                      num_hidden_layers=1, intermediate_size=64, vocab_size=32, max_position_embeddings=N_POS,
                      rope_parameters=dict(rs, rope_theta=THETA))
    rot = LlamaRotaryEmbedding(cfg)
    cos, sin = rot(torch.zeros(1, dtype=torch.float32), torch.arange(N_POS)[None, :])
    return cos[0, :, :head_dim // 2].numpy(), sin[0, :, :head_dim // 2].numpy()


@pytest.mark.parametrize("head_dim", [64, 128])
@pytest.mark.parametrize("kind", sorted(SCALINGS))
def test_scaled_tables_are_as_close_to_float64_as_hf(kind, head_dim):
    rs = SCALINGS[kind]
    cos, sin = build_rope_tables(N_POS, head_dim, THETA, "cpu", rope_scaling=rs, max_position_embeddings=N_POS)
    assert cos.dtype == torch.float32 and tuple(cos.shape) == (N_POS, head_dim // 2)
    rc, rsn = RR.tables(np.arange(N_POS), head_dim, THETA, rs, N_POS)
    hc, hs = _hf_tables(head_dim, rs)
    mine = max(np.abs(cos.numpy() - rc).max(), np.abs(sin.numpy() - rsn).max())
    hf = max(np.abs(hc - rc).max(), np.abs(hs - rsn).max())
    print("\nrope %s head_dim %d: table error vs float64 %.3e, HF fp32 module %.3e" % (kind, head_dim, mine, hf))
    assert mine <= 2 * hf, (mine, hf)
    # the bands: the reference's frequencies are not one scaling of the default ones (the ramp / smooth band is hit)
    f, att = RR.inv_freq(head_dim, THETA, rs, N_POS)
    ratio = f / RR.inv_freq(head_dim, THETA)[0]
    if kind == "linear":
        assert np.allclose(ratio, 0.25)
    else:
        assert ratio.max() == 1.0 and np.isclose(ratio.min(), 1 / rs["factor"]) and ((ratio < 1) & (ratio > ratio.min())).any()
    assert (att != 1.0) == (kind == "yarn")
    assert rope_inv_freq(head_dim, THETA, rs, N_POS)[1] == pytest.approx(att, rel=1e-12)


@pytest.mark.parametrize("head_dim", [64, 128])
def test_default_tables_are_bit_equal_to_the_plain_ones(head_dim):
    """what build_rope_tables returned before it took a rope_scaling argument"""
    inv = 1.0 / (THETA ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    ang = torch.arange(N_POS, dtype=torch.float32)[:, None] * inv[None, :]
    for rs in (None, {}, {"rope_type": "default"}, {"rope_type": "default", "rope_theta": THETA}):
        cos, sin = build_rope_tables(N_POS, head_dim, THETA, "cpu", rope_scaling=rs)
        assert torch.equal(cos, ang.cos()) and torch.equal(sin, ang.sin())
    cos, sin = build_rope_tables(N_POS, head_dim, THETA, "cpu")
    assert torch.equal(cos, ang.cos()) and torch.equal(sin, ang.sin())


@pytest.mark.parametrize("kind", ["dynamic", "longrope", "su", "made_up"])
def test_other_scalings_keep_raising_the_plain_rope_error(kind):
    with pytest.raises(RuntimeError, match="implements plain RoPE only .*%s" % kind):
        build_rope_tables(8, 64, THETA, "cpu", rope_scaling={"rope_type": kind, "factor": 2.0})
    ok, why = engine_supports(_cfg(rope_scaling={"type": kind, "factor": 2.0}))
    assert not ok and "rope scaling" in why and kind in why


def _cfg(**kw):
    base = dict(model_type="llama", hidden_act="silu", rope_scaling=None, sliding_window=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_engine_supports_accepts_the_four_families_and_the_three_scalings():
    assert ENGINE_MODEL_TYPES == ("llama", "mistral", "qwen2", "qwen3")
    for mt in ENGINE_MODEL_TYPES:
        assert engine_supports(_cfg(model_type=mt)) == (True, "")
    for rs in SCALINGS.values():
        assert engine_supports(_cfg(rope_scaling=rs))[0]
        assert engine_supports(_cfg(rope_scaling=None, rope_parameters=dict(rs, rope_theta=THETA)))[0]
    assert engine_supports(_cfg(rope_scaling={"type": "linear", "factor": 2.0}))[0]  # the older key


def test_engine_supports_takes_real_hf_configs():
    from transformers import LlamaConfig, MistralConfig, Qwen2Config, Qwen3Config

    for cls in (LlamaConfig, MistralConfig, Qwen2Config, Qwen3Config):
        ok, why = engine_supports(cls(hidden_size=64, num_attention_heads=4, num_hidden_layers=2, intermediate_size=64,
                                      vocab_size=32))
        assert ok, (cls.__name__, why)


@pytest.mark.parametrize("kw, names", [
    (dict(model_type="gemma"), ("model_type", "gemma")),
    (dict(model_type="phi3"), ("model_type", "phi3")),
    (dict(hidden_act="gelu"), ("hidden_act", "gelu")),
    (dict(attention_bias=True), ("attention_bias",)),
    (dict(model_type="qwen3", attention_bias=True), ("attention_bias",)),
    (dict(mlp_bias=True), ("mlp_bias",)),
    (dict(partial_rotary_factor=0.5), ("partial_rotary_factor",)),
    (dict(model_type="qwen2", sliding_window=32, layer_types=["full_attention", "sliding_attention"]), ("layer_types",)),
    (dict(model_type="qwen3", sliding_window=32, layer_types=["sliding_attention", "full_attention"]), ("layer_types",)),
])
def test_engine_supports_refusals_name_their_field(kw, names):
    ok, why = engine_supports(_cfg(**kw))
    assert not ok and why.startswith("QBits:")
    for n in names:
        assert n in why, why


def test_sliding_window_of_the_qwen_families_follows_layer_types():
    q = dict(model_type="qwen2", sliding_window=32)
    assert engine_window(_cfg(**q, layer_types=["full_attention"] * 2)) == 0
    assert engine_window(_cfg(**q, layer_types=["sliding_attention"] * 2)) == 32
    with pytest.raises(RuntimeError, match="layer_types"):
        engine_window(_cfg(**q, layer_types=["full_attention", "sliding_attention"]))
    # no layer_types: the window counts only under use_sliding_window
    assert engine_window(_cfg(**q)) == 0
    assert engine_window(_cfg(**q, use_sliding_window=False)) == 0
    assert engine_window(_cfg(**q, use_sliding_window=True)) == 32
    assert engine_window(_cfg(model_type="qwen3", sliding_window=None, use_sliding_window=True)) == 0
    # llama / mistral: as before, whatever else the config says
    assert engine_window(_cfg(model_type="mistral", sliding_window=4096)) == 4096
    assert engine_window(_cfg(model_type="mistral", sliding_window=None)) == 0
    assert engine_window(_cfg(model_type="llama", sliding_window=16, layer_types=["full_attention"])) == 16


def test_tensor_parallel_host_uses_the_same_rule_and_refuses_the_extras_by_name():
    assert tp_supports(_cfg()) == (True, "")
    assert tp_supports(_cfg(model_type="mistral", rope_scaling=SCALINGS["llama3"]))[0]
    ok, why = tp_supports(_cfg(model_type="qwen2"))
    assert not ok and "bias" in why and "tensor-parallel" in why
    ok, why = tp_supports(_cfg(model_type="qwen3"))
    assert not ok and "q_norm" in why and "tensor-parallel" in why
    assert tp_supports(_cfg(model_type="gemma")) == engine_supports(_cfg(model_type="gemma"))
