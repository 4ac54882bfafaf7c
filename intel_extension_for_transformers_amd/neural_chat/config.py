"""Configuration objects of the chat pipeline — field names and defaults of the reference's neural_chat/config.py
(GenerationConfig :400-423, LoadingModelConfig :426-436, PipelineConfig :466-517) for the fields this path reads."""
from dataclasses import dataclass
from typing import Dict, List


@dataclass
class GenerationConfig:
    device: str = "cuda"
    temperature: float = 0.1
    top_k: int = 40
    top_p: float = 0.75
    repetition_penalty: float = 1.1
    num_beams: int = 1
    max_new_tokens: int = 256
    do_sample: bool = True
    num_return_sequences: int = 1
    bad_words_ids: List[int] = None
    force_words_ids: List[int] = None
    use_cache: bool = True
    return_stats: bool = False
    format_version: str = "v2"
    task: str = ""
    # OpenAI / vLLM sampling controls, applied on the device by the engine's sampler (runtime.engine set_sampler):
    presence_penalty: float = 0.0   # subtracted once from the score of every token generated so far
    frequency_penalty: float = 0.0  # subtracted once per time a token was generated so far
    min_p: float = 0.0              # sampling keeps tokens at least min_p times as likely as the likeliest
    logit_bias: Dict[int, float] = None  # token id -> value added to its logit ahead of the penalties (-inf = a ban)
    seed: int = None                # a sampled request with a seed is reproducible (None: torch's CPU generator)
    # structured output (vLLM's names): the generated text is one of the strings / fully matches the pattern. A token
    # automaton the engine follows on the device (runtime.guide.TokenGuide); one of the two at most
    guided_choice: List[str] = None
    guided_regex: str = None
    # rolling KV cache (StreamingLLM; Neural Speed's names, reference docs/streamingllm.md): with any of the three set a
    # request may be longer than the engine's cache — the first n_keep positions stay as attention sinks, n_discard
    # positions after them are dropped whenever ctx_size positions are cached (runtime.streaming.StreamingConfig:
    # ctx_size None = the engine's max_ctx, n_keep None = 4, n_discard None / -1 = half of what is not kept)
    ctx_size: int = None
    n_keep: int = None
    n_discard: int = None
    logprobs: int = None  # 0..20: fill BaseModel.last_logprobs with every emitted token's log-probability + alternatives


@dataclass
class LoadingModelConfig:
    peft_path: str = None
    # peft_path's adapter on the fused decode engine, unmerged (optimize_transformers(model, adapters="unmerged")); the
    # default keeps such a chatbot on the module path
    peft_on_engine: bool = False
    use_cache: bool = True
    world_size: int = 1
    use_neural_speed: bool = False  # accepted for signature parity; must stay False here
    gguf_model_path: str = None


def get_device_type():
    """Reference utils/common.py get_device_type picks cuda > xpu > hpu > cpu; here there is one backend."""
    import torch

    if torch.cuda.is_available():
        return "cuda"
    raise RuntimeError("QBits: no MI355X/HIP device visible; the gfx950 WOQ path has no CPU fallback")


class PipelineConfig:
    def __init__(self, model_name_or_path="Intel/neural-chat-7b-v3-1", tokenizer_name_or_path=None,
                 hf_endpoint_url=None, hf_access_token=None, device="auto", task="", plugins=None,
                 loading_config=None, optimization_config=None, assistant_model=None, serving_config=None,
                 openai_config=None):
        from ..transformers import (AutoRoundConfig, AwqConfig, GPTQConfig, MixedPrecisionConfig, RtnConfig,
                                    TeqConfig)

        if hf_endpoint_url or openai_config or serving_config:
            raise NotImplementedError("QBits: remote endpoints / OpenAI / vLLM serving are outside the MI355X path")
        self.model_name_or_path = model_name_or_path
        self.tokenizer_name_or_path = tokenizer_name_or_path
        self.hf_access_token = hf_access_token
        self.hf_endpoint_url = None
        self.device = get_device_type() if device == "auto" else device
        self.task = task
        self.plugins = plugins or {}
        self.loading_config = loading_config if loading_config is not None else LoadingModelConfig()
        # same default rule as the reference (:509-510): fp16 on a GPU
        self.optimization_config = optimization_config if optimization_config is not None else \
            MixedPrecisionConfig(dtype="float16")
        allowed = (MixedPrecisionConfig, RtnConfig, AwqConfig, TeqConfig, GPTQConfig, AutoRoundConfig)
        assert type(self.optimization_config) in allowed, \
            "Expect optimization_config be an object of MixedPrecisionConfig, RtnConfig, AwqConfig, TeqConfig, " \
            "GPTQConfig or AutoRoundConfig, got %s." % type(self.optimization_config)
        self.assistant_model = assistant_model
        self.serving_config = None
