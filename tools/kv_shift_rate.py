"""What the rolling KV cache costs at the Llama-2-7B shape (fp16 cache, max_ctx 2048, n_keep 4, n_discard 1022):

 1. the time of one shift (`WoqDecoderEngine.kv_shift`), between stream events around each call, after warm-up calls,
    as min / median / max over the repeats, with the bytes it reads and writes;
 2. tokens/s of a 32 + 4096-token greedy request over the rolling cache against a 32 + 2000-token request without it,
    alternating in one session (host clock around `generate`, which ends on a device-to-host read).

The two requests do not attend over the same contexts (the rolling one refills 1026 .. 2048 positions again and again, the
plain one grows from 32 to 2032), so their rates differ by more than the shifts; the shifts' own share is reported from
(1) and the plan's shift count. Prints one JSON line; `--layers N` runs a reduced model (marked in the output).

    python tools/kv_shift_rate.py [--repeats 20] [--requests 2] [--layers 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20, help="timed shifts per geometry")
    ap.add_argument("--warmup", type=int, default=3, help="untimed shifts per geometry")
    ap.add_argument("--requests", type=int, default=2, help="timed requests of each kind, alternating")
    ap.add_argument("--layers", type=int, default=0, help="override the layer count (marks the result REDUCED)")
    ap.add_argument("--max-ctx", type=int, default=2048)
    ap.add_argument("--n-keep", type=int, default=4)
    ap.add_argument("--n-discard", type=int, default=1022)
    ap.add_argument("--stream-new", type=int, default=4096)
    ap.add_argument("--plain-new", type=int, default=2000)
    args = ap.parse_args()

    import torch

    import bench
    from intel_extension_for_transformers_amd.runtime.engine import StreamingConfig, plan_stream

    cfg = bench.LLAMA2_7B
    layers = args.layers or cfg["layers"]
    eng = bench.build_engine(cfg, group=128, sym=True, max_ctx=args.max_ctx, layers=args.layers or None)
    ctx, keep, disc = args.max_ctx, args.n_keep, args.n_discard
    row_bytes = cfg["kv_heads"] * cfg["head_dim"] * 2  # fp16
    for which in ("k", "v"):  # rows a real request would hold: finite values everywhere
        eng.kv_cache(which).normal_()

    def time_shift(n_keep, n_discard, n_cached):
        for _ in range(args.warmup):
            eng.kv_shift(n_keep, n_discard, n_cached, move_pos=False)
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.kv_shift(n_keep, n_discard, n_cached, move_pos=False)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        moved = (n_cached - n_keep - n_discard) * layers * row_bytes * 2  # K and V rows, each read once, written once
        med = statistics.median(ms)
        return {"n_keep": n_keep, "n_discard": n_discard, "n_cached": n_cached, "ms_min": round(min(ms), 4),
                "ms_median": round(med, 4), "ms_max": round(max(ms), 4), "bytes_read": moved, "bytes_written": moved,
                "read_plus_write_GB_per_s": round(2 * moved / (med * 1e-3) / 1e9, 1)}

    shifts = [time_shift(keep, disc, ctx), time_shift(0, 1, ctx)]  # the request's shift, and the largest move

    prompt = torch.randint(0, cfg["vocab"], (32,), generator=torch.Generator().manual_seed(1)).tolist()
    streaming = StreamingConfig(ctx_size=ctx, n_keep=keep, n_discard=disc)

    def request(kind):
        n_new = args.stream_new if kind == "streaming" else args.plain_new
        torch.cuda.synchronize()
        tic = time.time()
        out = eng.generate(prompt, n_new, streaming=streaming if kind == "streaming" else None)
        dt = time.time() - tic  # generate's last act is a device-to-host read of the last burst
        assert len(out) == n_new and eng.status() == 0
        return n_new / dt

    request("streaming"), request("plain")  # warm-up: captures, code objects, the tuner's choice at both lengths
    rates = {"streaming": [], "plain": []}
    for _ in range(args.requests):
        for kind in ("streaming", "plain"):
            rates[kind].append(request(kind))
    n_shifts = sum(1 for ev in plan_stream(len(prompt), args.stream_new, ctx, keep, disc, 16) if ev[0] == "shift")
    stream_s = args.stream_new / statistics.median(rates["streaming"])
    res = {
        "tool": "kv_shift_rate", "model": cfg["name"], "layers": layers, "REDUCED": bool(args.layers), "kv_dtype": "fp16",
        "max_ctx": ctx, "device": torch.cuda.get_device_name(0), "shift": shifts,
        "streaming_request": {"prompt": len(prompt), "new_tokens": args.stream_new, "shifts": n_shifts,
                              "tokens_per_s": [round(r, 1) for r in rates["streaming"]]},
        "plain_request": {"prompt": len(prompt), "new_tokens": args.plain_new,
                          "tokens_per_s": [round(r, 1) for r in rates["plain"]]},
        "shift_share_of_streaming_request": round(n_shifts * shifts[0]["ms_median"] * 1e-3 / stream_s, 5),
        "shift_ms_per_discarded_token": round(shifts[0]["ms_median"] / disc, 6),
    }
    print(json.dumps(res, separators=(",", ":")))


if __name__ == "__main__":
    main()
