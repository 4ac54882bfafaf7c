"""What the backward of the routed expert block costs at the Mixtral-8x7B (H 4096, I 14336, E 8, k 2) and Qwen3-30B-A3B
(H 2048, I 768, E 128, k 8) expert shapes, int4 sym group 128, bf16 gradients and activations:

  fused   qbits.moe_backward (csrc/woq_moe_bwd.hip): nine launches and a memset, g and u recomputed, in chunks of
          qbits.MOE_BACKWARD_CHUNK_TOKENS rows; scratch = moe_backward_workspace of a chunk
  torch   the arm fp8 experts and QBITS_DEBUG take: per expert that has rows, dequantize_packed_weight to fp32, a cast to
          bf16, the block in torch ops, torch.autograd.grad for dX and dw (forward included: it saves what the fused arm
          recomputes); it materialises K N 6 bytes per expert and kind

Every expert holds the same blob (the time does not depend on the values), routing is uniform random. Times are device
events around each call after untimed runs of the same calls; the arms alternate inside one process, `--reps` rounds, and
every figure is the median with the spread (max - min) / median of its own rounds. `fused_us_per_launch` is the whole
call over its launches (ten a chunk), not a per-kernel measurement. One JSON line per (shape, T); --out appends them to a
file. A run without a GPU fails.

  python tools/moe_backward_rate.py [--reps 7] [--shapes mixtral,qwen3] [--rows 256,1024,4096] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from intel_extension_for_transformers_amd import qbits  # noqa: E402
from tools.woq_backward_rate import alternate, med, spread  # noqa: E402

SHAPES = {"mixtral": (4096, 14336, 8, 2), "qwen3": (2048, 768, 128, 8)}


def _blobs(n, k, E, gen):
    w = 0.02 * torch.randn(n, k, device="cuda", generator=gen)
    blob = qbits.quantize_to_packed_weight(w, True, 128, "bf16", "int4_clip", "fp16", False)
    return blob.view(torch.uint8).unsqueeze(0).repeat(E, 1).contiguous()


def rate(name, T, reps):
    H, I, E, k = SHAPES[name]
    gen = torch.Generator(device="cuda").manual_seed(H + T)
    gu, dn = _blobs(2 * I, H, E, gen), _blobs(H, I, E, gen)
    x = torch.randn(T, H, device="cuda", generator=gen).to(torch.bfloat16)
    dout = torch.randn(T, H, device="cuda", generator=gen).to(torch.bfloat16)
    idx = torch.rand(T, E, device="cuda", generator=gen).argsort(1)[:, :k].contiguous()
    w = torch.rand(T, k, device="cuda", generator=gen)
    gx = torch.empty_like(x)
    res = {}

    def fused():
        res["fused"] = qbits.moe_backward(dout, x, idx, w, gu, dn, grad_hidden=gx)

    def deq(blob, kk, n):
        out = torch.empty(kk, n, dtype=torch.float32, device="cuda")
        qbits.dequantize_packed_weight(blob, out, False, "bf16", "int4_clip", "fp16")
        return out.to(torch.bfloat16)

    def torch_arm():
        xr, wr = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
        out = torch.zeros(T, H, dtype=torch.bfloat16, device="cuda")
        for e in range(E):
            tok, pos = torch.where(idx == e)
            if tok.numel() == 0:
                continue
            g, u = (xr[tok] @ deq(gu[e].view(torch.int8), H, 2 * I)).chunk(2, dim=-1)
            y = (torch.nn.functional.silu(g) * u) @ deq(dn[e].view(torch.int8), I, H)
            out = out.index_add(0, tok, y * wr[tok, pos, None].to(y.dtype))
        res["torch"] = torch.autograd.grad(out, (xr, wr), dout)

    t = alternate({"fused": fused, "torch": torch_arm}, reps)
    torch.cuda.synchronize()
    chunk = min(T, qbits.MOE_BACKWARD_CHUNK_TOKENS)
    launches = 10 * ((T + chunk - 1) // chunk)
    rx = res["torch"][0].float()
    f, g = med(t["fused"]), med(t["torch"])
    return dict(shape=name, H=H, I=I, E=E, top_k=k, T=T, reps=reps, fused_us=1e3 * f, fused_spread=spread(t["fused"]),
                fused_launches=launches, fused_us_per_launch=1e3 * f / launches, torch_us=1e3 * g,
                torch_spread=spread(t["torch"]), torch_over_fused=g / f,
                fused_scratch_bytes=qbits.moe_backward_workspace(chunk, k, E, H, I),
                torch_bytes_per_expert=(H * 2 * I + I * H) * 6,
                rel_diff_dx_vs_torch=((gx.float() - rx).norm() / rx.norm()).item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="mixtral,qwen3")
    ap.add_argument("--rows", default="256,1024,4096")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_backward_rate: needs the GPU (no CPU timing is meaningful)")
    lines = []
    for name in [s for s in args.shapes.split(",") if s]:
        for T in [int(m) for m in args.rows.split(",") if m]:
            rec = rate(name, T, args.reps)
            lines.append(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()}))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
