"""TEQ without a GPU: the float64 reference (tests/teq_reference.py) against torch autograd and the RTN reference, the
fold's function preservation, the request checks, the config and the ABI tables."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from tests import quant_reference as Q
from tests import teq_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 96, 32), (384, 200, 128), (200, 70, 64), (512, 20, -1)]
CASES = [(K, N, g, bits, asym) for (K, N, g) in SHAPES for bits, asym in ((4, False), (4, True), (8, True))]
WNAME = {4: "int4_clip", 8: "int8"}


# ---- the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_closed_form_is_autograd(K, N, group, bits, asym):
    """the closed form the kernel computes == torch autograd of the float64 statement, to 1e-12 relative; its fp32
    restatement with sequential sums stays inside the kernel test's bound 2^-20 * sum |terms|"""
    w, a, g = R.inputs(K, N, group, bits, asym, seed=K + bits)
    f = R.forward(w, a, group, bits, asym)
    da, mag = R.gradients(w, a, g, group, bits, asym, f)
    auto, W = R.autograd_gradients(w, a, g, group, bits, asym)
    assert np.array_equal(W, f["W"])
    assert np.abs(da - auto).max() <= 1e-12 * np.abs(auto).max()
    assert (mag > 0).all() and (np.abs(da) <= mag).all()
    d32, _ = R.gradients(w, a, g, group, bits, asym, dtype=np.float32)
    ratio = (np.abs(d32.astype(np.float64) - da) / (2.0 ** -20 * mag)).max()
    print("K=%d N=%d group=%d bits=%d asym=%d: fp32 restatement worst err / B %.4f" % (K, N, group, bits, asym, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_inputs_are_unambiguous_and_hold_the_zero_cell(K, N, group, bits, asym):
    w, a, g = R.inputs(K, N, group, bits, asym, seed=K + bits)
    assert w.dtype == a.dtype == g.dtype == np.float32 and (a > 0).all()
    assert R.ambiguous(w, a, group, bits, asym) == 0
    g0 = R.group_of(K, group)[0]
    f = R.forward(w, a, group, bits, asym)
    assert not w[:g0, 0].any() and f["dead"][0, 0] and f["s"][0, 0] == 1.0 and f["dead"].sum() == 1
    assert not f["W"][:g0, 0].any()
    w2, a2, g2 = R.inputs(K, N, group, bits, asym, seed=K + bits)
    assert np.array_equal(w, w2) and np.array_equal(a, a2) and np.array_equal(g, g2)


@pytest.mark.parametrize("K,N,group,bits,asym", CASES)
def test_unit_scale_is_rtn(K, N, group, bits, asym):
    w, _, _ = R.inputs(K, N, group, bits, asym, seed=K + bits)
    f = R.forward(w, np.ones(K), group, bits, asym)
    q = Q.quantize(w, group, WNAME[bits], asym)
    assert np.array_equal(f["W"], q["deq"]) and np.array_equal(f["s"], q["s"])
    if asym:
        assert np.array_equal(f["z"], q["z"])


def test_the_scatter_terms_matter():
    """leaving E out changes da on the rows E lands on by far more than the kernel test's bound"""
    K, N, group, bits, asym = 256, 96, 32, 4, True
    w, a, g = R.inputs(K, N, group, bits, asym, seed=K + bits)
    da, mag = R.gradients(w, a, g, group, bits, asym)
    bare, _ = R.gradients(w, a, g, group, bits, asym, scatter=False)
    assert (np.abs(da - bare) > 2.0 ** -20 * mag).sum() > 32


# ---- the fold ----------------------------------------------------------------------------------------------------
def _tiny_block(kv_heads=4):
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaDecoderLayer, LlamaRotaryEmbedding

    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=96, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=kv_heads, head_dim=16, vocab_size=32, max_position_embeddings=32,
                      attention_bias=True, mlp_bias=True)
    cfg._attn_implementation = "eager"
    block = LlamaDecoderLayer(cfg, 0).double().eval()
    with torch.no_grad():
        for p in block.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn_like(p) * 0.5 + 1.0)
    x = torch.randn(2, 8, 64, dtype=torch.float64)
    pos = torch.arange(8)[None]
    rot = LlamaRotaryEmbedding(cfg)(x, pos)

    def run(b):
        with torch.no_grad():
            y = b(x, position_embeddings=rot, position_ids=pos, attention_mask=None)
        return y[0] if isinstance(y, (tuple, list)) else y

    return block, run


def test_fold_preserves_the_block():
    """all four groups at once, on a float64 block with biases: the linears' working copies * a[k], the producing
    linears' columns and biases / a, the norms / a; outputs within 1e-10"""
    from intel_extension_for_transformers_amd.transformers.llm.quantization import teq
    from intel_extension_for_transformers_amd.transformers.llm.quantization.calibration import ABSORB_GROUPS

    block, run = _tiny_block()
    want = run(block)
    folded = copy.deepcopy(block)
    gen = torch.Generator().manual_seed(3)
    scales = {gi: torch.exp(0.5 * torch.randn(folded.get_submodule(names[0]).in_features, generator=gen,
                                              dtype=torch.float64)) for gi, (names, _) in enumerate(ABSORB_GROUPS)}
    linears = [(n, m) for n, m in folded.named_modules() if isinstance(m, torch.nn.Linear)]
    assert len(linears) == 7
    weights = {n: m.weight.data.t().clone() for n, m in linears}
    norm0 = folded.input_layernorm.weight.clone()
    teq.fold_scales(folded, weights, scales)
    assert not torch.equal(folded.input_layernorm.weight, norm0)
    for n, m in linears:
        m.weight.data.copy_(weights[n].t())
    got = run(folded)
    assert (got - want).abs().max().item() <= 1e-10 * max(1.0, want.abs().max().item())
    assert (got - want).abs().max().item() > 0  # something was folded


def test_schedule():
    from intel_extension_for_transformers_amd.transformers.llm.quantization import teq

    lrs = [teq.schedule(1e-3, t, 1000) for t in range(1000)]
    assert lrs[0] == pytest.approx(1e-3 / 50) and lrs[49] == pytest.approx(1e-3) and lrs[50] == pytest.approx(1e-3)
    assert all(b > a for a, b in zip(lrs[:49], lrs[1:50])) and all(b < a for a, b in zip(lrs[50:], lrs[51:]))
    assert lrs[-1] == pytest.approx(1e-3 / 950) and teq.schedule(1e-3, 1000, 1000) == 0.0
    assert [teq.schedule(1.0, t, 4) for t in range(4)] == [1.0, 0.75, 0.5, 0.25]  # too few steps for a warm-up


# ---- refusals, before a device is touched ------------------------------------------------------------------------------
class _Config:
    def __init__(self, model_type):
        self.model_type = model_type


class _Blocks(torch.nn.Module):
    def __init__(self, model_type="llama"):
        super().__init__()
        self.model = torch.nn.Module()
        self.model.layers = torch.nn.ModuleList([torch.nn.Linear(32, 32)])
        self.lm_head = torch.nn.Linear(32, 2)
        self.config = _Config(model_type)


class _Flat(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.linear = torch.nn.Linear(32, 2)


IDS = [torch.zeros(2, 8, dtype=torch.long)]


def _cfg(**kw):
    from intel_extension_for_transformers_amd.transformers import TeqConfig

    c = TeqConfig(**kw)
    c.post_init_hip()
    return c


def _convert(model, cfg):
    from intel_extension_for_transformers_amd.transformers.llm.quantization.utils import convert_to_quantized_model

    return convert_to_quantized_model(model, cfg, device="cuda")


@pytest.mark.parametrize("option,value", [("use_double_quant", True), ("layer_wise", True),
                                          ("absorb_to_layer", {"input_layernorm": ["q_proj"]})])
def test_unsupported_options_raise_by_name(option, value):
    with pytest.raises(NotImplementedError, match=option):
        _convert(_Blocks(), _cfg(calib_dataloader=IDS, **{option: value}))


def test_other_model_types_raise_by_name():
    with pytest.raises(NotImplementedError, match="gpt2"):
        _convert(_Blocks("gpt2"), _cfg(calib_dataloader=IDS))
    with pytest.raises(NotImplementedError, match="calibration is not part"):  # the data check comes first
        _convert(_Blocks("gpt2"), _cfg())


def test_model_without_decoder_blocks_is_named():
    with pytest.raises(NotImplementedError, match="_Flat"):
        _convert(_Flat(), _cfg(calib_dataloader=IDS))


def test_float_weight_types_raise():
    with pytest.raises(NotImplementedError, match="nf4"):
        _convert(_Blocks(), _cfg(calib_dataloader=IDS, bits=4, weight_dtype="nf4", sym=True))


def test_no_calibration_data_raises_as_awq_does():
    for kw in (dict(), dict(dataset="wikitext2")):
        with pytest.raises(NotImplementedError) as e:
            _convert(_Blocks(), _cfg(**kw))
        assert str(e.value).startswith("TeqConfig calibration is not part of the MI355X hot path without "
                                       "calibration data")
        assert "calib_dataloader" in str(e.value)


def test_calibration_data_and_knobs_are_not_serialised():
    from intel_extension_for_transformers_amd.transformers import TeqConfig

    c = _cfg(calib_dataloader=IDS, n_samples=3, seq_len=5, train_steps=7, lr=0.5, batch_size=2)
    assert c.calib_dataloader is IDS and (c.train_steps, c.lr, c.batch_size) == (7, 0.5, 2)
    d = c.to_dict()
    for name in ("calib_dataloader", "train_steps", "lr", "batch_size"):
        assert name not in d and name not in c.to_json_string(use_diff=False)
    assert set(d) == set(_cfg().to_dict())  # the schema is the one a config without them has
    back = TeqConfig.from_dict(d)
    assert back.calib_dataloader is None and back.n_samples == 3 and back.group_size == c.group_size
    default = TeqConfig()
    assert default.calib_dataloader is None and (default.train_steps, default.lr, default.batch_size) == (1000, 1e-3, 8)


def test_abi_and_binding_carry_the_teq_entry_points():
    """include/woq_hip.h, _lib.EXPORTS, qbits.__all__, INTEGRATION.md and the Makefile name the two entry points; the
    ABI version stays 4"""
    import ctypes

    from intel_extension_for_transformers_amd import _lib, qbits

    header = open(os.path.join(ROOT, "include", "woq_hip.h")).read()
    declared = set(re.findall(r"WOQ_API[^;(]*?\b(woq_\w+)\s*\(", header))
    new = {"woq_teq_forward", "woq_teq_grad"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert declared == set(_lib.EXPORTS)
    assert "#define WOQ_ABI_VERSION 4" in header
    assert {"teq_forward", "teq_grad"} <= set(qbits.__all__)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in new)
    makefile = open(os.path.join(ROOT, "intel_extension_for_transformers_amd", "csrc", "Makefile")).read()
    assert "woq_teq.hip" in makefile
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for n in new:
            getattr(lib, n)
