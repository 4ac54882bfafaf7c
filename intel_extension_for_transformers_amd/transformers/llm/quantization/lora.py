"""LoRA adapters over packed blobs ("QLoRA"): fine-tuning a weight-only-quantised model whose weights stay frozen in
their blobs, under PEFT's names and PEFT's on-disk format — without PEFT, which is not a dependency.

  * `LoraConfig`, `prepare_model_for_kbit_training`, `get_peft_model`: the three calls of a PEFT QLoRA script;
  * `QuantizedLoraLinearQBits` (reference nn/modules.py, the consumer of `quantize_to_packed_weight`): a
    `QuantizedLinearQBits` that adopts an existing module's blob and adds `scaling * lora_B(lora_A(dropout(x)))`.
    The base projection's backward is `qbits.woq_linear_backward` (autograd/functions.py MatMulKBit): the gradient
    passes through every quantised projection to the adapters in front of it;
  * adapters are saved as `adapter_config.json` + `adapter_model.safetensors` with keys
    `base_model.model.<module path>.lora_A.weight`, so they move to and from PEFT.

One adapter ("default") at a time; no DoRA, no rsLoRA, `bias="none"` only.

Serving. A wrapped model keeps the module path by default (`get_peft_model` switches the engine-backed `generate` off),
and `merge_and_unload()` is the lossy way onto the fused decode engine: it re-quantises W + scaling B A with RTN, and an
act-order blob refuses it. `optimize_transformers(model, adapters="unmerged")` is the other way: the engine is built over
the adopted blobs and carries the adapters as they are, x W_deq + scaling (x A^T) B^T in fp32 on q / k / v / o / gate /
up / down of the decoder layers, ranks 1..64 (runtime/engine.py `WoqDecoderEngine.set_lora`, csrc/woq_lora.hip). The
engine holds a COPY of lora_A / lora_B: it sees the values of the last `set_lora`, so after training further call
`model.woq_engine.set_lora(model)` again. Not on the engine: tensor-parallel engines, fp8-weight layers, adapters on
lm_head or the embeddings, several adapters in one step.
"""
import json
import math
import os
import types

import torch
from torch import nn

from .... import qbits
from .nn.modules import QuantizedLinearQBits

ADAPTER = "default"
DEFAULT_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj")  # the Llama-class attention projections
CONFIG_NAME, WEIGHTS_NAME = "adapter_config.json", "adapter_model.safetensors"


class LoraConfig:
    """PEFT's LoraConfig, the fields this path implements. target_modules None = q/k/v/o of the Llama-class families."""

    def __init__(self, r=8, lora_alpha=16, lora_dropout=0.0, target_modules=None, bias="none", task_type="CAUSAL_LM",
                 base_model_name_or_path=None, **unused):
        if bias != "none":
            raise ValueError("QBits: LoraConfig(bias=%r): only bias=\"none\" is implemented" % (bias,))
        if int(r) < 1:
            raise ValueError("QBits: LoraConfig(r=%r): the rank is a positive integer" % (r,))
        if isinstance(target_modules, str):
            target_modules = [target_modules]
        self.r, self.lora_alpha, self.lora_dropout = int(r), lora_alpha, float(lora_dropout)
        self.target_modules = sorted(target_modules if target_modules is not None else DEFAULT_TARGETS)
        self.bias, self.task_type, self.base_model_name_or_path = bias, task_type, base_model_name_or_path
        self.peft_type = "LORA"

    def to_dict(self):
        return {"peft_type": self.peft_type, "r": self.r, "lora_alpha": self.lora_alpha,
                "target_modules": list(self.target_modules), "lora_dropout": self.lora_dropout, "bias": self.bias,
                "task_type": self.task_type, "base_model_name_or_path": self.base_model_name_or_path,
                "inference_mode": False, "fan_in_fan_out": False, "init_lora_weights": True, "modules_to_save": None,
                "use_rslora": False, "use_dora": False}

    @classmethod
    def from_pretrained(cls, path):
        with open(os.path.join(path, CONFIG_NAME)) as f:
            d = json.load(f)
        if d.get("peft_type", "LORA") != "LORA":
            raise ValueError("QBits: %s holds a %r adapter; only LORA is implemented" % (path, d.get("peft_type")))
        if d.get("use_dora") or d.get("use_rslora"):
            raise ValueError("QBits: DoRA / rsLoRA adapters are not implemented")
        return cls(r=d["r"], lora_alpha=d["lora_alpha"], lora_dropout=d.get("lora_dropout", 0.0),
                   target_modules=d.get("target_modules"), bias=d.get("bias", "none"),
                   task_type=d.get("task_type", "CAUSAL_LM"), base_model_name_or_path=d.get("base_model_name_or_path"))


def _linear_kwargs(m):
    return dict(bias=m._wants_bias, compute_dtype=m.compute_dtype, compress_statistics=m.compress_statistics,
                weight_dtype=m.weight_dtype, bits=m.bits, scale_dtype=m.scale_dtype, blocksize=m.blocksize,
                scheme=m.scheme, device=m.device, double_quant_scale_dtype=m.double_quant_scale_dtype,
                compression_dtype=m.compression_dtype, compression_dim=m.compression_dim,
                use_optimum_format=m.use_optimum_format)


def _share_blob(dst, src):
    """dst takes src's packed weight and bias: the same Parameter objects, nothing is copied"""
    dst.weight, dst.bias, dst._bias32 = src.weight, src.bias, src._bias32
    dst.train(src.training)


class QuantizedLoraLinearQBits(QuantizedLinearQBits):
    """forward = base(x) + scaling * lora_B(lora_A(dropout(x))), scaling = lora_alpha / r, over the adopted blob.
    lora_A / lora_B are ModuleDicts of bias-free fp32 nn.Linear (state-dict keys `....lora_A.default.weight`), lora_A
    Kaiming-uniform, lora_B zero: a fresh adapter changes nothing."""

    def __init__(self, base, r=8, lora_alpha=16, lora_dropout=0.0, adapter_name=ADAPTER):
        if not isinstance(base, QuantizedLinearQBits) or base.weight.numel() == 0:
            raise RuntimeError("QBits: QuantizedLoraLinearQBits wraps a QuantizedLinearQBits that holds a packed weight")
        super().__init__(base.in_features, base.out_features, **_linear_kwargs(base))
        _share_blob(self, base)
        dev = base.weight.device
        self.r, self.lora_alpha, self.scaling = int(r), lora_alpha, float(lora_alpha) / int(r)
        self.active_adapter, self.merged = adapter_name, False
        self.lora_dropout = nn.ModuleDict({adapter_name: nn.Dropout(lora_dropout) if lora_dropout > 0 else nn.Identity()})
        self.lora_A = nn.ModuleDict({adapter_name: nn.Linear(base.in_features, self.r, bias=False, device=dev)})
        self.lora_B = nn.ModuleDict({adapter_name: nn.Linear(self.r, base.out_features, bias=False, device=dev)})
        nn.init.kaiming_uniform_(self.lora_A[adapter_name].weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B[adapter_name].weight)

    def forward(self, x):
        out = super().forward(x)
        if self.merged:
            return out
        tup = isinstance(out, tuple)  # the vLLM seam returns (output, None)
        y = out[0] if tup else out
        a, b = self.lora_A[self.active_adapter], self.lora_B[self.active_adapter]
        h = self.lora_dropout[self.active_adapter](x).to(a.weight.dtype)
        y = y + (self.scaling * b(a(h))).to(y.dtype)
        return (y, None) if tup else y

    # ---- merge / unmerge (reference nn/modules.py:477-485) ---------------------------------------------------------
    def _requantise(self, sign):
        w = self.weight.data
        info = lambda t: int(qbits.acquire_packed_weight_info(w, t)[0])  # noqa: E731
        if info(4):
            raise RuntimeError("QBits: this blob carries a GPTQ act-order shuffle; merging re-quantises with RTN, which "
                               "would lose the order and the calibrated codes. Keep the adapter unmerged")
        deq = torch.empty(info(2), info(3), dtype=torch.float32, device=w.device)
        qbits.dequantize_packed_weight(w, deq, False, self.compute_dtype, self.weight_dtype, self.scale_dtype)
        a, b = self.lora_A[self.active_adapter].weight, self.lora_B[self.active_adapter].weight
        with torch.no_grad():
            fp = deq.t() + sign * self.scaling * (b.float() @ a.float())  # nn.Linear layout [N, K]
        self.set_fp_weights_bias(fp, self.bias)

    def merge(self):
        """Folds the adapter into the blob: dequantise, add scaling * B A, re-quantise with RTN under the module's own
        recipe (`set_fp_weights_bias`). LOSSY, as in the reference: the merged blob is the nearest grid point to
        W + scaling B A, not that sum, and `unmerge` does not return the original bytes."""
        if not self.merged:
            self._requantise(1.0)
            self.merged = True

    def unmerge(self):
        if self.merged:
            self._requantise(-1.0)
            self.merged = False


def has_unmerged_adapters(model):
    return any(isinstance(m, QuantizedLoraLinearQBits) for m in model.modules())


def prepare_model_for_kbit_training(model, use_gradient_checkpointing=False, gradient_checkpointing_kwargs=None):
    """PEFT's call of the same name: freeze every parameter, hold the norm weights in fp32 (as PEFT does, every 16-bit
    parameter that is not a blob: a norm that answers in fp32 must not meet a 16-bit lm_head), make the embedding
    output require a gradient so that it reaches the first quantised projection, and optionally switch on gradient
    checkpointing."""
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.parameters():
        if p.dtype in (torch.float16, torch.bfloat16):
            p.data = p.data.to(torch.float32)
    if hasattr(model, "enable_input_require_grads"):
        model.enable_input_require_grads()
    else:
        model.get_input_embeddings().register_forward_hook(lambda mod, inp, out: out.requires_grad_(True))
    if use_gradient_checkpointing:
        kw = gradient_checkpointing_kwargs if gradient_checkpointing_kwargs is not None else {"use_reentrant": False}
        model.gradient_checkpointing_enable(gradient_checkpointing_kwargs=kw)
    return model


def _set_submodule(model, path, new):
    parent_path, _, leaf = path.rpartition(".")
    setattr(model.get_submodule(parent_path) if parent_path else model, leaf, new)


def _lora_modules(model):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, QuantizedLoraLinearQBits)]


def _engine_off(model, off):
    """a decode engine built over the blobs knows nothing of the adapters now on (or off) the model: drop it, and keep
    `generate` on the modules until `optimize_transformers(model, adapters="unmerged")` opts in again"""
    if getattr(model, "woq_engine", None) is not None:
        model.woq_engine = None
    model._woq_engine_off = bool(off)
    model._woq_adapters = None


def print_trainable_parameters(model):
    trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
    # a blob is int8 storage of packed nibbles and scales: count the weights it stands for
    total = 0
    for m in model.modules():
        for p in m.parameters(recurse=False):
            total += m.in_features * m.out_features if isinstance(m, QuantizedLinearQBits) and p is m.weight else p.numel()
    print("trainable params: %d || all params: %d || trainable%%: %.4f" % (trainable, total, 100.0 * trainable / total))
    return trainable, total


def save_adapter(model, save_directory):
    """adapter_config.json + adapter_model.safetensors, PEFT's names and keys"""
    from safetensors.torch import save_file

    os.makedirs(save_directory, exist_ok=True)
    cfg = model.peft_config[ADAPTER]
    with open(os.path.join(save_directory, CONFIG_NAME), "w") as f:
        json.dump(cfg.to_dict(), f, indent=2, sort_keys=True)
    tensors = {}
    for name, m in _lora_modules(model):
        tensors["base_model.model.%s.lora_A.weight" % name] = m.lora_A[ADAPTER].weight.detach().cpu().contiguous()
        tensors["base_model.model.%s.lora_B.weight" % name] = m.lora_B[ADAPTER].weight.detach().cpu().contiguous()
    save_file(tensors, os.path.join(save_directory, WEIGHTS_NAME), metadata={"format": "pt"})


def load_adapter(model, load_directory):
    """the weights of an adapter saved by `save_adapter` or by PEFT into this model's (already wrapped) targets"""
    from safetensors.torch import load_file

    cfg = LoraConfig.from_pretrained(load_directory)
    mine = model.peft_config[ADAPTER]
    if cfg.r != mine.r or sorted(cfg.target_modules) != sorted(mine.target_modules):
        raise RuntimeError("QBits: the adapter in %s has r=%d on %s; this model was wrapped with r=%d on %s"
                           % (load_directory, cfg.r, cfg.target_modules, mine.r, mine.target_modules))
    tensors = load_file(os.path.join(load_directory, WEIGHTS_NAME))
    mods = dict(_lora_modules(model))
    seen = set()
    for key, t in tensors.items():
        prefix, _, rest = key.partition("base_model.model.")
        path, _, which = rest.rpartition(".lora_")
        which = which.split(".")[0]
        if prefix or path not in mods or which not in ("A", "B"):
            raise RuntimeError("QBits: adapter key %r names no LoRA target of this model" % key)
        dst = (mods[path].lora_A if which == "A" else mods[path].lora_B)[ADAPTER].weight
        if tuple(dst.shape) != tuple(t.shape):
            raise RuntimeError("QBits: adapter key %r is %s, the model wants %s" % (key, tuple(t.shape), tuple(dst.shape)))
        with torch.no_grad():
            dst.copy_(t)
        seen.add((path, which))
    missing = [p for p in mods for w in "AB" if (p, w) not in seen]
    if missing:
        raise RuntimeError("QBits: the adapter holds no weights for %s" % sorted(set(missing)))
    mine.lora_alpha, mine.lora_dropout = cfg.lora_alpha, cfg.lora_dropout
    for m in mods.values():
        m.lora_alpha, m.scaling = cfg.lora_alpha, float(cfg.lora_alpha) / m.r
    return model


def merge_and_unload(model):
    """every adapter folded into its blob (`QuantizedLoraLinearQBits.merge`: RTN, lossy) and the wrappers replaced by
    plain `QuantizedLinearQBits` over the merged blobs: `optimize_transformers` and `save_pretrained` take the result"""
    for name, m in _lora_modules(model):
        m.merge()
        plain = QuantizedLinearQBits(m.in_features, m.out_features, **_linear_kwargs(m))
        _share_blob(plain, m)
        _set_submodule(model, name, plain)
    model.peft_config = {}
    _engine_off(model, False)
    return model


def get_peft_model(model, config):
    """Wraps every targeted `QuantizedLinearQBits` of `model` in place (the blobs are adopted, not copied), freezes
    everything but the adapters, and returns the model with `print_trainable_parameters`, `save_adapter(dir)`,
    `load_adapter(dir)` and `merge_and_unload()`."""
    if has_unmerged_adapters(model):
        raise RuntimeError("QBits: this model already holds an adapter (one at a time); merge_and_unload() it first")
    targets = set(config.target_modules)
    hit = [(n, m) for n, m in model.named_modules() if n.rpartition(".")[2] in targets]
    if not hit:
        raise RuntimeError("QBits: no module of the model is named %s" % sorted(targets))
    for n, m in hit:
        if not isinstance(m, QuantizedLinearQBits):
            raise RuntimeError("QBits: LoRA target %s is a %s; adapters go over QuantizedLinearQBits blobs"
                               % (n, type(m).__name__))
    for p in model.parameters():
        p.requires_grad_(False)
    for n, m in hit:
        _set_submodule(model, n, QuantizedLoraLinearQBits(m, config.r, config.lora_alpha, config.lora_dropout))
    if config.base_model_name_or_path is None:
        config.base_model_name_or_path = getattr(model.config, "_name_or_path", None) or None
    model.peft_config = {ADAPTER: config}
    model.active_adapter = ADAPTER
    for f in (print_trainable_parameters, save_adapter, load_adapter, merge_and_unload):
        setattr(model, f.__name__, types.MethodType(f, model))
    _engine_off(model, True)
    return model


def load_peft_adapter(model, path):
    """`PeftModel.from_pretrained(model, path)` for this path: wrap the targets the adapter's config names, load its
    weights, leave the model unmerged on the module path."""
    cfg = LoraConfig.from_pretrained(path)
    return get_peft_model(model, cfg).load_adapter(path)
