"""What unmerged LoRA adapters cost on the fused decode engine, at the Llama-2-7B shape (int4 sym, group 128, synthetic
weights as `synth_llama_weights`), 32 prompt tokens + 256 generated:

  decode   tokens/s of greedy bursts with no adapter installed (before anything was reserved, and again after
           `clear_lora()`), with an r = 16 adapter on q_proj / v_proj, and on all seven targets
  delta    us per delta launch of each projection kind (qkv, o, gate/up, down) at r = 16: the step with that kind
           alone targeted against the adapter-less step, per layer (the launch inside the step, boundary included)
  prefill  ms of a 2048-row prompt pass without an adapter, with q / v targeted, and with all seven (gate / up
           included: the base GEMM then stores plain gate / up rows and the expand applies SiLU * mul)

The arms alternate inside one process, `--reps` rounds after untimed ones; every figure is the median with the spread
(max - min) / median of its own rounds beside it. Times are device events around each burst / pass. The module path of
the same model (`model.generate` over QuantizedLoraLinearQBits modules) is not timed here: it needs a Hugging Face model of
the shape, which tools/woq_backward_rate.py's block arm builds for one layer only. One JSON line per figure; --out
appends them to a file. A run without a GPU fails.

  python tools/lora_engine_rate.py [--reps 5] [--layers 32] [--new 256] [--prompt 32] [--rows 2048] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from intel_extension_for_transformers_amd import _lib as L  # noqa: E402
from intel_extension_for_transformers_amd.runtime.engine import WoqDecoderEngine, synth_llama_weights  # noqa: E402

H, I, NH, KV, D, VOCAB = 4096, 11008, 32, 32, 128, 32000
ALL7, QV = L.LORA_TARGETS, ("q_proj", "v_proj")


def med(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return (max(xs) - min(xs)) / med(xs)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def adapters(eng, layers, targets, r=16, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = {}
    for l in range(layers):
        for t in targets:
            K, N = eng._lora_shape(t)
            out[(l, t)] = ((torch.rand(r, K, device="cuda", generator=g) * 2 - 1) / K ** 0.5,
                           0.01 * torch.randn(N, r, device="cuda", generator=g), 2.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_engine_rate: needs the GPU (no CPU timing is meaningful)")
    lines = []

    def emit(rec):
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()})
        print(line, flush=True)
        lines.append(line)

    eng = WoqDecoderEngine(H, I, NH, KV, D, args.layers, VOCAB, max_ctx=max(4096, args.rows))
    synth_llama_weights(eng, H, I, NH, KV, D, args.layers, VOCAB, group=128)
    prompt = torch.randint(0, VOCAB, (args.prompt,)).tolist()
    rows = torch.randint(0, VOCAB, (args.rows,)).tolist()

    def burst():
        eng.prefill(prompt, greedy=True)
        eng.prepare_decode(greedy=True)
        return timed(lambda: eng.replay(args.new))

    def install(which):
        if which is None:
            eng.clear_lora()
        else:
            eng.set_lora(adapters(eng, args.layers, which))

    # 1. decode: the arms alternate; "never reserved" can only come first
    res = {"no adapter (nothing reserved)": [burst() for _ in range(args.reps + 1)][1:]}
    arms = {"no adapter (after clear_lora)": None, "r16 on q/v": QV, "r16 on all seven": ALL7}
    for name in arms:
        res[name] = []
    for i in range(args.reps + 1):
        for name, which in arms.items():
            install(which)
            t = burst()
            if i > 0:
                res[name].append(t)
    base = med(res["no adapter (nothing reserved)"])
    for name, ms in res.items():
        emit(dict(kind="decode", arm=name, layers=args.layers, prompt=args.prompt, new=args.new, reps=len(ms),
                  tokens_per_s=1e3 * args.new / med(ms), ms_per_token=med(ms) / args.new, spread=spread(ms),
                  vs_no_adapter=base / med(ms)))

    # 2. one projection kind at a time: a step then holds ONE more launch per layer, and the difference to the
    # adapter-less step divided by the layers is what that launch costs inside the step, boundary included
    kinds = {"qkv": ("q_proj", "k_proj", "v_proj"), "o": ("o_proj",), "gate_up": ("gate_proj", "up_proj"),
             "down": ("down_proj",)}
    res = {k: [] for k in kinds}
    res["none"] = []
    for i in range(args.reps + 1):
        for name in res:
            install(kinds.get(name))
            t = burst()
            if i > 0:
                res[name].append(t)
    none = med(res["none"]) / args.new
    for name, parts_t in kinds.items():
        per_token = med(res[name]) / args.new
        emit(dict(kind="delta", projection=name, parts=len(parts_t), r_per_part=16, K=eng._lora_shape(parts_t[0])[0],
                  N=sum(eng._lora_shape(t)[1] for t in parts_t), reps=len(res[name]), ms_per_token=per_token,
                  ms_per_token_no_adapter=none, us_per_delta_launch=1e3 * (per_token - none) / args.layers,
                  spread=spread(res[name]), spread_no_adapter=spread(res["none"])))

    # 3. prompt pass
    res = {"no adapter": [], "r16 on q/v": [], "r16 on all seven": []}
    arms = {"no adapter": None, "r16 on q/v": QV, "r16 on all seven": ALL7}
    for i in range(args.reps + 1):
        for name, which in arms.items():
            install(which)
            t = timed(lambda: eng.prefill(rows, greedy=False))
            if i > 0:
                res[name].append(t)
    base = med(res["no adapter"])
    for name, ms in res.items():
        emit(dict(kind="prefill", arm=name, layers=args.layers, rows=args.rows, reps=len(ms), ms=med(ms),
                  tokens_per_s=1e3 * args.rows / med(ms), spread=spread(ms), vs_no_adapter=med(ms) / base))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
