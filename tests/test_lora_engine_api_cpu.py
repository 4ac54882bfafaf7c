"""The public surface of the engine's unmerged LoRA adapters, without a GPU: the library exports and declares the new entry
points, `LoadingModelConfig` and `optimize_transformers` keep their defaults, and `WoqDecoderEngine.set_lora` reads an
adapter the way `save_adapter` writes it."""
import inspect
import os
import re

import pytest
import torch

from intel_extension_for_transformers_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = ("woq_engine_lora_reserve", "woq_engine_set_lora", "woq_engine_clear_lora", "woq_engine_lora_on")
PROBES = ("woq_probe_lora_delta", "woq_probe_lora_shrink", "woq_probe_lora_expand")


def test_library_exports_and_headers_declare_the_lora_entry_points():
    import ctypes

    header = open(os.path.join(ROOT, "include", "woq_hip.h")).read()
    exp = open(os.path.join(ROOT, "include", "woq_hip_experimental.h")).read()
    for n in ENGINE:
        assert re.search(r"WOQ_API int %s\(" % n, header) and n in _lib.EXPORTS and n not in exp
    for n in PROBES:
        assert re.search(r"WOQ_API int %s\(" % n, exp) and n in _lib.EXPERIMENTAL_EXPORTS and n not in header
    assert "#define WOQ_ABI_VERSION 4" in header  # new entry points only: the boundary's version stays
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libwoq_hip.so not built (python __graft_entry__.py)")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ENGINE + PROBES:
        assert hasattr(lib, n), n
    # the launchers are declared once, in woq_host.h, and the file is part of the build
    host = open(os.path.join(ROOT, "intel_extension_for_transformers_amd", "csrc", "woq_host.h")).read()
    for n in ("launch_lora_delta_xq", "launch_lora_delta_f32", "launch_lora_shrink", "launch_lora_expand"):
        assert len(re.findall(r"\bint %s\(" % n, host)) == 1, n
    assert "woq_lora.hip" in open(os.path.join(ROOT, "intel_extension_for_transformers_amd", "csrc", "Makefile")).read()
    assert _lib.LORA_TARGETS == ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def test_defaults_keep_adapters_off_the_engine():
    from intel_extension_for_transformers_amd.neural_chat.config import LoadingModelConfig
    from intel_extension_for_transformers_amd.runtime.engine import WoqDecoderEngine, optimize_transformers

    cfg = LoadingModelConfig(peft_path="x")
    assert cfg.peft_on_engine is False and LoadingModelConfig(peft_path="x", peft_on_engine=True).peft_on_engine is True
    assert inspect.signature(optimize_transformers).parameters["adapters"].default is None
    for name in ("set_lora", "clear_lora", "lora_on"):
        assert hasattr(WoqDecoderEngine, name)


def test_default_refusal_names_merge_and_the_keyword():
    """the refusal comes before anything touches a device: a CPU stand-in with a lora_A attribute is enough"""
    from transformers import LlamaConfig

    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.config = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                                      vocab_size=64)
            self.proj = torch.nn.Linear(4, 4)
            self.proj.lora_A = torch.nn.ModuleDict()

    with pytest.raises(RuntimeError, match=r"merge_and_unload\(\)") as e:
        optimize_transformers(Stub())
    assert 'adapters="unmerged"' in str(e.value)
    with pytest.raises(ValueError, match="adapters"):
        optimize_transformers(Stub(), adapters="yes")


def test_set_lora_reads_an_adapter_directory_as_save_adapter_writes_it(tmp_path):
    import json

    from safetensors.torch import save_file

    from intel_extension_for_transformers_amd.runtime.engine import WoqDecoderEngine

    g = torch.Generator().manual_seed(0)
    want = {}
    tensors = {}
    for layer in range(2):
        for target, (k, n) in (("q_proj", (128, 256)), ("down_proj", (256, 128))):
            a, b = torch.randn(4, k, generator=g), torch.randn(n, 4, generator=g)
            path = "model.layers.%d.%s.%s" % (layer, "self_attn" if target == "q_proj" else "mlp", target)
            tensors["base_model.model.%s.lora_A.weight" % path] = a
            tensors["base_model.model.%s.lora_B.weight" % path] = b
            want[(layer, target)] = (a, b)
    save_file(tensors, str(tmp_path / "adapter_model.safetensors"), metadata={"format": "pt"})
    json.dump({"peft_type": "LORA", "r": 4, "lora_alpha": 6, "target_modules": ["q_proj", "down_proj"]},
              open(tmp_path / "adapter_config.json", "w"))
    got = WoqDecoderEngine._lora_entries(str(tmp_path))
    assert sorted(got) == sorted(want)
    for key, (a, b, s) in got.items():
        assert torch.equal(a, want[key][0]) and torch.equal(b, want[key][1]) and s == 1.5
    # a dict passes through; a key outside the decoder layers' seven projections is refused
    assert WoqDecoderEngine._lora_entries({(1, "v_proj"): (1, 2, 3.0)}) == {(1, "v_proj"): (1, 2, 3.0)}
    with pytest.raises(RuntimeError, match="QBits"):
        WoqDecoderEngine._lora_entries({(0, "lm_head"): (1, 2, 3.0)})
    tensors["base_model.model.lm_head.lora_A.weight"] = torch.zeros(4, 128)
    save_file(tensors, str(tmp_path / "adapter_model.safetensors"), metadata={"format": "pt"})
    with pytest.raises(RuntimeError, match="QBits"):
        WoqDecoderEngine._lora_entries(str(tmp_path))
