"""What the calibrated methods (gptq.py, awq.py, autoround.py, teq.py) share: the request checks, the calibration
batches, the walk down the decoder blocks (the first block's inputs as the model itself calls it, a block run over them, the next
block's inputs), the per-linear input statistics from forward hooks, the absorb groups of a Llama-class block (AWQ, TEQ),
the block-by-block training of a fake quantiser (AutoRound, TEQ: the minibatch draw, the wrap of the linears, the loop)
and the swap of a linear for its QuantizedLinearQBits. Plain functions; every method keeps its own loop over the blocks,
and no method file imports from another.
"""
import contextlib
import logging

import torch

from .nn.modules import QuantizedLinearQBits

WNAME = {4: "int4_clip", 8: "int8", 3: "int3_clip", 2: "int2_clip"}
BITS = {name: bits for bits, name in WNAME.items()}

_log = logging.getLogger(__name__)

_NOT_PART = " calibration is not part of the MI355X hot path without calibration data (dataset=%r is not downloaded)"
_NO_DATA = {"GPTQ": "GPTQ calibration does not download datasets (dataset=%r)", "AWQ": "AwqConfig" + _NOT_PART,
            "AutoRound": "AutoRoundConfig" + _NOT_PART, "TEQ": "TeqConfig" + _NOT_PART}


# ---- the request ---------------------------------------------------------------------------------------------------
def data_source(config, method="GPTQ"):
    """where the calibration ids come from: 'loader' or 'texts'; a dataset given by its hub name is not fetched"""
    dataset = getattr(config, "dataset", None)
    if getattr(config, "calib_dataloader", None) is not None:
        return "loader"
    if isinstance(dataset, (list, tuple)) and dataset and all(isinstance(t, str) for t in dataset):
        return "texts"
    raise NotImplementedError(_NO_DATA[method] % (dataset,) + ": pass calib_dataloader= (an iterable of input_ids "
                              "tensors) or dataset=[texts] with tokenizer=")


def check_request(model, config, method, unsupported_options, blocks_first=False):
    """Everything about a request that can be refused without touching a device; `method` is GPTQ, AWQ, AutoRound or TEQ.
    `blocks_first`: a model without decoder blocks is named before missing data (AutoRound's order)."""
    for opt in unsupported_options:
        if getattr(config, opt, False):
            raise NotImplementedError("%s on the MI355X path does not implement %s" % (method, opt))
    if config.weight_dtype not in BITS:
        raise NotImplementedError("%s quantises to the integer weight types (int4_clip, int8), not weight_dtype=%s"
                                  % (method, config.weight_dtype))
    if blocks_first:
        decoder_blocks(model)
        data_source(config, method)
    else:
        data_source(config, method)
        decoder_blocks(model)


def _rows(item):
    """input_ids of one dataloader item -> list of 1-D id tensors"""
    if isinstance(item, dict):
        item = item["input_ids"]
    elif isinstance(item, (tuple, list)) and len(item) and not isinstance(item[0], int):
        item = item[0]["input_ids"] if isinstance(item[0], dict) else item[0]
    ids = torch.as_tensor(item).long()
    return [ids] if ids.dim() == 1 else list(ids.reshape(-1, ids.shape[-1]))


def calibration_batches(config, batch_size=None):
    """`config.calib_dataloader` (an iterable of input_ids tensors, or of dicts / tuples holding them) or
    `config.dataset` as a list of strings with `config.tokenizer` -> list of [b, t] id tensors: at most n_samples rows,
    each cut to seq_len, batch_size rows of equal length per batch (`batch_size` if given, else the config's, else 1).
    A dataset given by its hub name is not fetched."""
    n_samples, seq_len = int(config.n_samples), int(config.seq_len)
    batch_size = max(1, int(batch_size or getattr(config, "batch_size", 1) or 1))
    rows = []
    if data_source(config) == "loader":
        for item in config.calib_dataloader:
            rows.extend(r[:seq_len] for r in _rows(item))
            if len(rows) >= n_samples:
                break
    else:
        if config.tokenizer is None:
            raise ValueError("GPTQConfig(dataset=[texts]) needs tokenizer=")
        for text in config.dataset[:n_samples]:
            rows.append(torch.as_tensor(config.tokenizer(text)["input_ids"]).long().reshape(-1)[:seq_len])
    rows = [r for r in rows[:n_samples] if r.numel() > 0]
    if not rows:
        raise ValueError("GPTQ: the calibration data is empty")
    batches, cur = [], []
    for r in rows:
        if cur and (len(cur) == batch_size or cur[0].numel() != r.numel()):
            batches.append(torch.stack(cur))
            cur = []
        cur.append(r)
    batches.append(torch.stack(cur))
    return batches


# ---- the model's blocks and their linears ----------------------------------------------------------------------------
def decoder_blocks(model):
    for path in ("model.layers", "transformer.h"):
        obj = model
        for part in path.split("."):
            obj = getattr(obj, part, None)
            if obj is None:
                break
        if isinstance(obj, (torch.nn.ModuleList, torch.nn.Sequential)) and len(obj):
            return path, obj
    raise NotImplementedError("GPTQ calibration walks model.model.layers or model.transformer.h; model type %s has "
                              "neither" % (getattr(getattr(model, "config", None), "model_type", None)
                                           or type(model).__name__))


def is_conv1d(m):
    return type(m).__name__ == "Conv1D" and hasattr(m, "nf")  # HF GPT-2 projection: weight already [K, N] (F10)


def in_features(m):
    return m.weight.shape[0] if is_conv1d(m) else m.in_features


def weight_kn(m):
    """the linear's weight as fp32 [K, N], a fresh contiguous tensor"""
    w = m.weight.data if is_conv1d(m) else m.weight.data.t()
    return w.to(torch.float32).clone(memory_format=torch.contiguous_format)


def block_linears(block, prefix, skip):
    out = []
    for name, m in block.named_modules():
        if isinstance(m, QuantizedLinearQBits) or not (isinstance(m, torch.nn.Linear) or is_conv1d(m)):
            continue
        if any(s in prefix + "." + name for s in skip):
            continue
        out.append((name, m))
    return out


# ---- the stream of block inputs --------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def capture_block_inputs(model, blocks, batches, device):
    """the first block's inputs, as the model itself calls it: one (args, kwargs) per batch"""
    inputs = []

    def grab(_module, args, kwargs):
        inputs.append((args, kwargs))
        raise _Stop()

    handle = blocks[0].register_forward_pre_hook(grab, with_kwargs=True)
    use_cache = getattr(model.config, "use_cache", None) if hasattr(model, "config") else None
    try:
        if use_cache is not None:
            model.config.use_cache = False
        for ids in batches:
            try:
                model(input_ids=ids.to(device))
            except _Stop:
                pass
    finally:
        handle.remove()
        if use_cache is not None:
            model.config.use_cache = use_cache
    return inputs


def run_block(block, inputs):
    outs = []
    for args, kwargs in inputs:
        y = block(*args, **kwargs)
        outs.append(y[0] if isinstance(y, (tuple, list)) else y)
    return outs


def next_inputs(inputs, outs):
    """the next block's inputs: this block's, with its outputs as the hidden states"""
    return [((y,) + tuple(args[1:]), kwargs) if args else ((), dict(kwargs, hidden_states=y))
            for (args, kwargs), y in zip(inputs, outs)]


def collect_input_stats(block, linears, inputs, source=None, abs_sum=False):
    """Runs `block` over `inputs` with forward hooks on `linears` -> ({name: X^T X [K, K]}, {name: sum |x| [K]} (empty
    without abs_sum), {name: tokens}): raw fp32 sums over every token the linear saw, on its own device. `source`
    {name: name} names the linear whose statistics a linear shares (they see the same tensor); only the sources get an
    entry."""
    xtx, asum, count, hooks = {}, {}, {}, []
    try:
        for name, m in linears:
            if source is not None and source[name] != name:
                continue
            k = in_features(m)
            xtx[name] = torch.zeros(k, k, dtype=torch.float32, device=m.weight.device)
            if abs_sum:
                asum[name] = torch.zeros(k, dtype=torch.float32, device=m.weight.device)
            count[name] = 0

            def accumulate(_m, args, _out, name=name):
                x = args[0].reshape(-1, args[0].shape[-1]).float()
                xtx[name].addmm_(x.t(), x)
                if abs_sum:
                    asum[name].add_(x.abs().sum(0))
                count[name] += x.shape[0]

            hooks.append(m.register_forward_hook(accumulate))
        run_block(block, inputs)
    finally:
        for hk in hooks:
            hk.remove()
    return xtx, asum, count


# ---- the absorb groups of a Llama-class block (AWQ's scales, TEQ's trainable scales) ----------------------------------
SCALE_MODEL_TYPES = ("llama", "mistral", "qwen2", "qwen3")  # the attribute layout the scale folding knows

# (the scaled linears: they share an input; the op that produces it and absorbs 1 / s)
ABSORB_GROUPS = (
    (("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "input_layernorm"),
    (("self_attn.o_proj",), "self_attn.v_proj"),
    (("mlp.gate_proj", "mlp.up_proj"), "post_attention_layernorm"),
    (("mlp.down_proj",), "mlp.up_proj"),
)


def model_type(model):
    return getattr(getattr(model, "config", None), "model_type", None) or type(model).__name__


def absorb_groups(block, linears, where, method):
    """the absorb groups of this block that can take a scale (indices into ABSORB_GROUPS): every member among `linears`;
    a group whose producing op is a linear only where that linear's outputs are the group's inputs one to one (o_proj
    after v_proj: not under grouped-query attention, AutoAWQ's rule). `method` (AWQ, TEQ) names the caller in the log
    lines, which go to its file's logger."""
    logger = logging.getLogger("%s.%s" % (__package__, method.lower()))
    have = {name for name, _ in linears}
    out = []
    for gi, (names, prev) in enumerate(ABSORB_GROUPS):
        if not all(n in have for n in names):
            logger.info("%s %s: absorb group %s skipped (not every linear is quantised)", method, where,
                        "/".join(names))
            continue
        p = block.get_submodule(prev)
        if isinstance(p, torch.nn.Linear):
            if prev not in have:
                logger.info("%s %s: absorb group %s skipped (%s is not quantised)", method, where, names[0], prev)
                continue
            if p.out_features != block.get_submodule(names[0]).in_features:
                # AutoAWQ compares the two weights' shapes, the same test wherever heads * head_dim = hidden
                logger.info("%s %s: %s scale skipped (grouped-query attention: %s has %d outputs for %d inputs)",
                            method, where, names[0], prev, p.out_features, block.get_submodule(names[0]).in_features)
                continue
        out.append(gi)
    return out


# ---- training a fake quantiser block by block (AutoRound, TEQ) --------------------------------------------------------
SEED = 42  # of the minibatch draw
DEFAULT_BATCH = 8


def _samples(unit):
    args, kwargs = unit
    x = args[0] if args else kwargs["hidden_states"]
    return int(x.shape[0])


def draw_minibatch(inputs, batch_size, gen):
    """the indices of one minibatch: whole batches in a random order until `batch_size` samples are reached"""
    picked, count = [], 0
    for i in torch.randperm(len(inputs), generator=gen).tolist():
        picked.append(i)
        count += _samples(inputs[i])
        if count >= batch_size:
            break
    return picked


def fake_quant_dtype(outs):
    """the dtype of a W~: the block output's where that is fp16 or bf16, else fp32"""
    return outs[0].dtype if outs[0].dtype in (torch.float16, torch.bfloat16) else torch.float32


@contextlib.contextmanager
def fake_quant_forward(linears, quantisers):
    """Inside, every linear of `linears` [(name, module)] computes x.matmul(q.wq) + q.bias with its quantiser q (same
    order): an instance `forward`, removed on any exit."""
    for (_, m), q in zip(linears, quantisers):
        m.forward = lambda x, q=q: x.matmul(q.wq) if q.bias is None else x.matmul(q.wq) + q.bias
    try:
        yield
    finally:
        for _, m in linears:
            del m.forward


def train_block(block, inputs, targets, steps, batch_size, gen, begin_step, after_backward, snapshot):
    """`steps` training steps of one block's fake quantisers (its linears inside fake_quant_forward) against `targets`,
    the fp block's outputs -> (first_loss, best_loss, best_step, best_snapshot). Per step t: one draw_minibatch;
    begin_step(t) sets the rates, builds the W~ (q.wq) of the trained quantisers and returns them; the mean squared error
    over the picked batches; snapshot() is kept at the lowest loss so far (before the update: these parameters gave this
    loss; a tie keeps the earlier step); backward(); after_backward(t) does what the quantisers' own backward left of the
    update; the W~ built this step are dropped. The block's parameters are frozen inside and restored on any exit."""
    best, best_loss, best_step, first_loss = None, None, -1, None
    flags = [(p, p.requires_grad) for p in block.parameters()]
    for p, _ in flags:
        p.requires_grad_(False)
    try:
        with torch.enable_grad():
            for t in range(steps):
                picked = draw_minibatch(inputs, batch_size, gen)
                rebuilt = begin_step(t)
                total = sum(targets[i].numel() for i in picked)
                loss = 0.0
                for i in picked:
                    y = run_block(block, [inputs[i]])[0]
                    loss = loss + (y.float() - targets[i].float()).square().sum()
                loss = loss / total
                value = float(loss.detach())
                _log.debug("step %d: batches %s, loss %.9g", t, picked, value)
                if t == 0:
                    first_loss = value
                if best_loss is None or value < best_loss:
                    best_loss, best_step = value, t
                    best = snapshot()
                loss.backward()
                after_backward(t)
                for q in rebuilt:
                    q.wq = None
    finally:
        for p, flag in flags:
            p.requires_grad_(flag)
    return first_loss, best_loss, best_step, best


# ---- the result -------------------------------------------------------------------------------------------------------
def install_quantized(block, name, m, config, device, *, codes=None, scales=None, zeros=None, g_idx=None,
                      fp_weight_kn=None):
    """Replaces the linear `m` = block.<name> by its QuantizedLinearQBits: from `codes` int8 [K, N], `scales`, `zeros`
    (signed domain, as the kernels give them) and `g_idx` through set_weights_bias, or from `fp_weight_kn` fp32 [K, N]
    through set_fp_weights_bias, the device RTN."""
    k, n = (codes if codes is not None else fp_weight_kn).shape
    new = QuantizedLinearQBits(k, n, m.bias is not None, compute_dtype=config.compute_dtype, compress_statistics=False,
                               weight_dtype=config.weight_dtype, bits=config.bits, scale_dtype=config.scale_dtype,
                               blocksize=config.group_size, scheme=config.scheme, device=device)
    bias = m.bias.data if m.bias is not None else None
    if codes is None:
        new.set_fp_weights_bias(fp_weight_kn.t(), bias)
    else:
        if BITS[config.weight_dtype] == 4:  # set_weights_bias takes 4-bit values unsigned, as the checkpoint formats do
            codes = codes + 8
            zeros = zeros + 8 if zeros is not None else None
        new.set_weights_bias(codes, scales, zeros, g_idx if g_idx is not None else torch.empty(0, dtype=torch.int32),
                             config, bias)
    new.source_cls = type(m)
    new.requires_grad_(False)
    parent_name, _, leaf = name.rpartition(".")
    parent = block.get_submodule(parent_name) if parent_name else block
    parent._modules[leaf] = new


@contextlib.contextmanager
def fp32_matmul():
    """torch's fp32 GEMMs (X^T X, the losses, the trailing updates) in full fp32 inside the block"""
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
