from .engine import WoqDecoderEngine, build_rope_tables, engine_supports, fuse_gate_up, synth_llama_weights  # noqa: F401
from .guide import TokenGuide, token_bytes  # noqa: F401
from .streaming import StreamingConfig, plan_stream  # noqa: F401
