"""What routing one sparse layer costs at the Mixtral-8x7B shape (H 4096, E 8, k 2) and the Qwen3-30B-A3B shape (H 2048,
E 128, k 8), for one row (the decode form) and 2048 rows (the MFMA form), bf16 router weights, RMSNorm in front:

  route  one `qbits.moe_route` call on the fp32 rows (csrc/woq_moe_route.hip: norm, logits, soft-max, top-k, one launch)
  torch  what HF's decoder layer + TopKRouter launch for the same: RMSNorm in float, cast to bf16, F.linear, soft-max in
         float, topk, sum, divide

Microseconds per call between stream events around `--inner` back-to-back calls, the two alternating repeat by repeat;
min / median / max over `--repeats` after warm-up. Both are issued from Python, so at one row the figures hold the host's
enqueue cost of one launch against about ten; a kernel trace in a run of its own gives the launches' device time.

    python tools/moe_route_rate.py [--repeats 30]

Prints a table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"mixtral-8x7b": (4096, 8, 2), "qwen3-30b-a3b": (2048, 128, 8)}
EPS = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F

    from intel_extension_for_transformers_amd import qbits

    assert torch.cuda.is_available(), "moe_route_rate needs a GPU"
    res = {"tool": "moe_route_rate", "device": torch.cuda.get_device_name(0), "router": "bf16", "rows": {}}
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, (H, E, k) in SHAPES.items():
        W = (0.02 * torch.randn(E, H, generator=gen, device="cuda")).bfloat16()
        g = 1.0 + 0.1 * torch.randn(H, generator=gen, device="cuda")
        for T in (1, 2048):
            x = torch.randn(T, H, generator=gen, device="cuda")

            def route():
                return qbits.moe_route(x, W, k, True, g, EPS)

            def hf():
                xn = (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * g).bfloat16()
                p = torch.softmax(F.linear(xn, W), dtype=torch.float, dim=-1)
                w, idx = torch.topk(p, k, dim=-1)
                return xn, idx, (w / w.sum(-1, keepdim=True)).bfloat16()

            agree = float((route()[1].long().sort(-1).values == hf()[1].sort(-1).values).all(-1).float().mean())
            forms = (("route", route), ("torch", hf))
            us = {what: [] for what, _ in forms}
            for i in range(args.warmup + args.repeats):
                for what, body in forms:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.inner):
                        body()
                    b.record()
                    b.synchronize()
                    if i >= args.warmup:
                        us[what].append(1e3 * a.elapsed_time(b) / args.inner)
            res["rows"]["%s T=%d" % (name, T)] = {
                "H": H, "E": E, "k": k, "T": T, "rows_with_the_same_expert_set_as_bf16_torch": round(agree, 4),
                **{w + "_us": [round(min(v), 2), round(statistics.median(v), 2), round(max(v), 2)] for w, v in us.items()}}
    print("us per call: min / median / max")
    for name, r in res["rows"].items():
        print("  %-22s route %8.2f /%8.2f /%8.2f   torch %8.2f /%8.2f /%8.2f" % (name, *r["route_us"], *r["torch_us"]))
    print(json.dumps(res, separators=(",", ":")))


if __name__ == "__main__":
    main()
