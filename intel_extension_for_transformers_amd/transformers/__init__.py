"""`intel_extension_for_transformers.transformers` surface for the int4 weight-only path, MI355X backend
(reference exports: transformers/__init__.py:28-42)."""
from .utils.config import (AutoRoundConfig, AwqConfig, GPTQConfig, MixedPrecisionConfig, RtnConfig,  # noqa: F401
                           TeqConfig, WeightOnlyQuantConfig)


def __getattr__(name):  # the model classes import torch + HF transformers: load them on first use
    if name in ("AutoModelForCausalLM", "AutoModel", "AutoModelForSeq2SeqLM"):
        from .modeling import modeling_auto

        return getattr(modeling_auto, name)
    if name in _LORA:  # LoRA over blobs (llm/quantization/lora.py): torch only
        from .llm.quantization import lora

        return getattr(lora, name)
    raise AttributeError(name)


_LORA = ("LoraConfig", "QuantizedLoraLinearQBits", "prepare_model_for_kbit_training", "get_peft_model")


__all__ = ["AutoModelForCausalLM", "AutoModel", "AutoModelForSeq2SeqLM", "RtnConfig", "AwqConfig", "TeqConfig",
           "GPTQConfig", "AutoRoundConfig", "WeightOnlyQuantConfig", "MixedPrecisionConfig", "LoraConfig",
           "QuantizedLoraLinearQBits", "prepare_model_for_kbit_training", "get_peft_model"]
