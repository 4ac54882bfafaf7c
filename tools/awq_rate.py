"""What AWQ calibration of one linear costs on the device, per part, at the Llama-2-7B shapes:

  clip         the HIP clip search (qbits.awq_clip_search): 10 candidates for every (group, column) cell, one launch
  torch_clip   a plain torch statement of the same search (kept here as the baseline: the project had no AWQ before):
               per candidate clamp -> group RTN -> d -> one batched [G, g, g] x [G, g, N] product -> cell losses
  delta        the 20 launches of qbits.awq_scale_delta of one scale search of this linear
  delta_loss   the same with each candidate's loss (D * (H @ D)).sum(), an fp32 GEMM, as quantization/awq.py runs it

Times are device events around each part after one untimed run of the same calls, the median of `--reps` runs; the
weights are N(0, 0.02), the Gram matrix is that of correlated random inputs with a few channels 16 times larger (the
time of every part is independent of the values). One JSON line per shape; --out also writes them to a file.

  python tools/awq_rate.py [--reps 3] [--shapes 4096x4096,...] [--group 128] [--out FILE] [--skip-torch]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from intel_extension_for_transformers_amd import qbits  # noqa: E402
from intel_extension_for_transformers_amd.transformers.llm.quantization.awq import (N_CLIP, N_GRID,  # noqa: E402
                                                                                     normalised_scale)

SHAPES = "4096x12288,4096x4096,4096x22016,11008x4096"
TOKENS = 4096


def timed(fn, reps):
    """median device milliseconds of fn() over reps runs, after one untimed run"""
    out = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2]


def torch_clip(w, h, group, bits):
    """the clip search in torch, sym, K a multiple of the group: -> (best [G, N], losses [N_CLIP, G, N])"""
    K, N = w.shape
    G = K // group
    qmax, off = 2 ** (bits - 1) - 1, 2 ** (bits - 1)
    wg = w.view(G, group, N)
    blocks = torch.stack([h[g * group:(g + 1) * group, g * group:(g + 1) * group] for g in range(G)])
    amax = wg.abs().amax(1, keepdim=True)
    losses = []
    for j in range(N_CLIP):
        m = (1.0 - j / N_GRID) * amax
        s = m / qmax
        s = torch.where(s == 0, torch.ones_like(s), s)
        d = torch.clamp(torch.round(torch.clamp(wg, -m, m) / s), -off, qmax) * s - wg
        losses.append((d * torch.bmm(blocks, d)).sum(1))
    losses = torch.stack(losses)
    return losses.argmin(0), losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--out")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("awq_rate: needs the GPU (no CPU timing is meaningful)")
    torch.backends.cuda.matmul.allow_tf32 = False
    dev, group, bits = "cuda", args.group, 4
    lines, grams = [], {}
    for shape in args.shapes.split(","):
        K, N = (int(v) for v in shape.split("x"))
        rec = dict(K=K, N=N, group=group, bits=bits, reps=args.reps, n_clip=N_CLIP, n_grid=N_GRID)
        g = torch.Generator(device=dev).manual_seed(K)
        if K not in grams:
            load = torch.randn(8, K, device=dev, generator=g)
            x = torch.randn(TOKENS, 8, device=dev, generator=g) @ load + 0.5 * torch.randn(TOKENS, K, device=dev,
                                                                                          generator=g)
            x[:, torch.randperm(K, device=dev, generator=g)[:K // 64]] *= 16.0
            grams[K] = ((x.t() @ x) / TOKENS, x.abs().mean(0))
            del x
        h, a = grams[K]
        w = 0.02 * torch.randn(K, N, device=dev, generator=g)
        w_out, d = torch.empty_like(w), torch.empty_like(w)
        keep = {}

        def clip():
            keep["dev"] = qbits.awq_clip_search(w, h, group, bits, False, N_GRID, N_CLIP, w_out=w_out)

        rec["clip_ms"] = timed(clip, args.reps)
        rec["clip_gfma_per_s"] = N * K * group * N_CLIP / rec["clip_ms"] / 1e6
        scales = [normalised_scale(a, i).contiguous() for i in range(N_GRID)]

        def deltas():
            for s in scales:
                qbits.awq_scale_delta(w, s, group, bits, False, out=d)

        def deltas_and_losses():
            for s in scales:
                qbits.awq_scale_delta(w, s, group, bits, False, out=d)
                keep["loss"] = (d * (h @ d)).sum(dtype=torch.float64)

        rec["delta_ms"] = timed(deltas, args.reps)
        rec["delta_us_per_launch"] = 1e3 * rec["delta_ms"] / N_GRID
        rec["delta_loss_ms"] = timed(deltas_and_losses, args.reps)
        if not args.skip_torch:
            rec["torch_clip_ms"] = timed(lambda: keep.__setitem__("torch", torch_clip(w, h, group, bits)), 1)
            rec["torch_over_kernel"] = rec["torch_clip_ms"] / rec["clip_ms"]
            # the same search on the same inputs: the choices agree but where two candidates' fp32 losses nearly tie
            rec["choices_equal_fraction"] = float((keep["dev"][0] == keep["torch"][0]).float().mean())
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()})
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
