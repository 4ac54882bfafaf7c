"""What H2O eviction costs at the Llama-2-7B shape (fp16 cache, max_ctx 2048, n_keep 4, n_discard 512, recent 256):

 1. the per-step score launches: a logits-only decode step at the last cache position with H2O on against the same step
    with it off, both in the separate qkv | attention form, between stream events; the difference is `layers` launches;
 2. the prompt score: a prompt pass of `--prompt` tokens with H2O on against off; the difference is 2 * `layers` launches;
 3. one eviction (`WoqDecoderEngine.h2o_evict`: select + compact) of a full cache over random scores, which are written
    again before every call.

min / median / max over the repeats after warm-up calls. Prints one JSON line; `--layers N` runs a reduced model (marked
in the output).

    python tools/h2o_rate.py [--repeats 20] [--layers 0]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="override the layer count (marks the result REDUCED)")
    ap.add_argument("--max-ctx", type=int, default=2048)
    ap.add_argument("--prompt", type=int, default=1024)
    ap.add_argument("--n-keep", type=int, default=4)
    ap.add_argument("--n-discard", type=int, default=512)
    ap.add_argument("--recent", type=int, default=256)
    args = ap.parse_args()

    import torch

    import bench

    cfg = bench.LLAMA2_7B
    layers = args.layers or cfg["layers"]
    eng = bench.build_engine(cfg, group=128, sym=True, max_ctx=args.max_ctx, layers=args.layers or None)
    eng.launch = "eager"
    eng.set_fuse_attn(False)  # the form an engine with H2O runs, for both sides of every comparison
    for which in ("k", "v"):
        eng.kv_cache(which).normal_()
    ctx = args.max_ctx
    prompt = torch.randint(0, cfg["vocab"], (args.prompt,), generator=torch.Generator().manual_seed(1)).tolist()

    def timed(body, before=None):
        ms = []
        for i in range(args.warmup + args.repeats):
            if before is not None:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            body()
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        return {"ms_min": round(min(ms), 4), "ms_median": round(statistics.median(ms), 4), "ms_max": round(max(ms), 4)}

    def step():
        eng.step(greedy=False)

    def at_last_position():
        eng.token.fill_(1)
        eng.pos.fill_(ctx - 1)

    def prompt_pass():
        eng.prefill(prompt, start_pos=0, greedy=False)

    res = {"tool": "h2o_rate", "model": cfg["name"], "layers": layers, "REDUCED": bool(args.layers), "kv_dtype": "fp16",
           "max_ctx": ctx, "device": torch.cuda.get_device_name(0)}
    off = {"step": timed(step, at_last_position), "prompt": timed(prompt_pass)}
    eng.set_h2o(True)
    on = {"step": timed(step, at_last_position), "prompt": timed(prompt_pass)}
    res["step_at_position_%d" % (ctx - 1)] = {"h2o_off": off["step"], "h2o_on": on["step"], "score_us_per_layer": round(
        1e3 * (on["step"]["ms_median"] - off["step"]["ms_median"]) / layers, 3)}
    res["prompt_pass_%d_tokens" % args.prompt] = {"h2o_off": off["prompt"], "h2o_on": on["prompt"], "score_us_per_layer": round(
        1e3 * (on["prompt"]["ms_median"] - off["prompt"]["ms_median"]) / layers, 3)}
    res["eviction"] = dict(n_keep=args.n_keep, n_discard=args.n_discard, recent=args.recent, n_cached=ctx,
                           **timed(lambda: eng.h2o_evict(args.n_keep, args.n_discard, args.recent, ctx, move_pos=False),
                                   lambda: eng.h2o_scores().uniform_()))
    eng.set_h2o(False)
    assert eng.status() == 0
    print(json.dumps(res, separators=(",", ":")))


if __name__ == "__main__":
    main()
