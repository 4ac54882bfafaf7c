"""What one routed expert block costs at the Mixtral-8x7B shape (H 4096, I 14336, E 8, k 2) and the Qwen3-30B-A3B shape
(H 2048, I 768, E 128, k 8), g128 symmetric weights of `--weight` (int4 by default; int8, nf4, fp4_e2m1, fp4_e2m1_bnb, fp8_e4m3, fp8_e5m2),
fp16 activations, T in {1, 4, 16, 64, 128, 256, 512, 1024, 2048, 4096} or `--tokens`
(a shape whose k admits no more than 8192 tokens in one prompt-form call also runs that T and one chunked T beyond it),
uniform random routing (k distinct experts per token, softmax weights):

  grouped  QuantizedMoEExpertsQBits' one `qbits.moe_forward` call (csrc/woq_moe.hip: four launches, no host round trip)
  prompt   the same call with form="prompt" (csrc/woq_moe_prompt.hip: six launches, 128-row blocks on the fp16 MFMA), from
           T = `--prompt-from` (64) up; beyond `qbits.MOE_PROMPT_MAX_SLOTS` slots through the module's row chunks
  loop     its per-expert loop form (`qbits.woq_linear` on the expert's blobs, a host round trip for the experts hit)
  hf_fp16  the fp16 `MixtralExperts.forward` it replaces (HF's own loop, `_experts_implementation = "eager"`); `--no-hf`
           leaves it out

Microseconds per call between stream events around `--inner` back-to-back calls (the loop forms synchronise inside, so the
host's share is part of their figure, as it is in a decode step); min / median over `--repeats` after warm-up. Every
repeat takes the next of `--routings` routing sets, so the experts hit change from call to call as they do between
tokens. `grouped GB/s` = blob bytes of the distinct experts hit (both kinds), averaged over the routing sets, over the
grouped median: what a perfect stream of exactly those blobs would have to sustain.

    python tools/moe_rate.py [--shape mixtral-8x7b | qwen3-30b-a3b | all] [--weight int4_clip] [--tokens 1,16,64] [--repeats 20]

Prints a table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"mixtral-8x7b": (4096, 14336, 8, 2), "qwen3-30b-a3b": (2048, 768, 128, 8)}
TOKENS = (1, 4, 16, 64, 128, 256, 512, 1024, 2048, 4096)
PROMPT_FROM = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--routings", type=int, default=8)
    ap.add_argument("--weight", default="int4_clip", choices=["int4_clip", "int8", "nf4", "fp4_e2m1", "fp4_e2m1_bnb", "fp8_e4m3", "fp8_e5m2"])
    ap.add_argument("--tokens", default="", help="comma-separated T instead of the default ladder")
    ap.add_argument("--prompt-from", type=int, default=PROMPT_FROM)
    ap.add_argument("--no-hf", action="store_true")
    args = ap.parse_args()

    import torch
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from intel_extension_for_transformers_amd import qbits
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.moe import QuantizedMoEExpertsQBits

    def timed(body):
        us = []
        for i in range(args.warmup + args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for j in range(args.inner):
                body(i * args.inner + j)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                us.append(1e3 * a.elapsed_time(b) / args.inner)
        return round(min(us), 1), round(statistics.median(us), 1)

    res = {"tool": "moe_rate", "device": torch.cuda.get_device_name(0), "weights": "%s g128 sym, fp16 scales" % args.weight,
           "activations": "fp16", "shapes": {}}
    names = list(SHAPES) if args.shape == "all" else [args.shape]
    for name in names:
        H, I, E, k = SHAPES[name]
        gen = torch.Generator(device="cuda").manual_seed(0)
        with torch.device("cuda"):
            hf = MixtralExperts(MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E,
                                              num_experts_per_tok=k, num_hidden_layers=1)).half()
        hf.config._experts_implementation = "eager"
        with torch.no_grad():
            hf.gate_up_proj.normal_(std=0.02, generator=gen)
            hf.down_proj.normal_(std=0.02, generator=gen)
        mod = QuantizedMoEExpertsQBits(E, H, I, weight_dtype=args.weight, bits=8 if args.weight in ("int8", "fp8_e4m3", "fp8_e5m2") else 4,
                                       scale_dtype="fp16", blocksize=128, device="cuda")
        mod.set_fp_weights(hf.gate_up_proj.data, hf.down_proj.data)
        blob_bytes = mod.gate_up_blobs.shape[1] + mod.down_blobs.shape[1]
        rows = {}
        one_call = qbits.MOE_PROMPT_MAX_SLOTS // k
        ladder = TOKENS + ((one_call, one_call + one_call // 2) if one_call <= 8192 else ())
        for T in [int(t) for t in args.tokens.split(",")] if args.tokens else ladder:
            x = torch.randn(T, H, generator=gen, device="cuda", dtype=torch.float16)
            sets = []
            for _ in range(args.routings):
                score = torch.rand(T, E, generator=gen, device="cuda")
                w, idx = torch.topk(score, k, dim=-1)
                sets.append((idx, torch.softmax(w, dim=-1)))
            hit = statistics.mean(len(torch.unique(idx)) for idx, _ in sets)
            g = p = h = (float("nan"), float("nan"))
            with torch.no_grad():
                if T * k <= qbits.MOE_MAX_SLOTS:
                    g = timed(lambda i: qbits.moe_forward(x, *sets[i % len(sets)], mod.gate_up_blobs, mod.down_blobs))
                if T >= args.prompt_from:
                    p = timed(lambda i: mod.prompt_forward(x, *sets[i % len(sets)], one_call))
                lp = timed(lambda i: mod.loop_forward(x, *sets[i % len(sets)]))
                if not args.no_hf:
                    h = timed(lambda i: hf(x, sets[i % len(sets)][0], sets[i % len(sets)][1].half()))
            rows[T] = {"grouped_us": g, "prompt_us": p, "loop_us": lp, "hf_fp16_us": h, "experts_hit": round(hit, 2),
                       "grouped_GBps": round(hit * blob_bytes / g[1] / 1e3, 1)}
        res["shapes"][name] = {"H": H, "I": I, "E": E, "k": k, "blob_bytes_per_expert": blob_bytes, "T": rows}
        del hf, mod
        torch.cuda.empty_cache()

    print("us per call: min / median")
    for name, s in res["shapes"].items():
        print("%s (H %d, I %d, E %d, k %d; %d blob bytes an expert)" % (name, s["H"], s["I"], s["E"], s["k"],
                                                                       s["blob_bytes_per_expert"]))
        print("  %5s %21s %21s %21s %21s %12s %13s" % ("T", "grouped", "prompt", "loop", "hf fp16", "experts hit",
                                                        "grouped GB/s"))
        for T, r in s["T"].items():
            print("  %5d %10.1f /%9.1f %10.1f /%9.1f %10.1f /%9.1f %10.1f /%9.1f %12.2f %13.1f" % (
                T, *r["grouped_us"], *r["prompt_us"], *r["loop_us"], *r["hf_fp16_us"], r["experts_hit"],
                r["grouped_GBps"]))
    print(json.dumps(res, separators=(",", ":")))


if __name__ == "__main__":
    main()
