"""What GPTQ calibration of one linear costs on the device, per part, at the Llama-2-7B shapes:

  sweep      the HIP sweep (qbits.gptq_sweep), all K / 128 launches of one linear
  torch      a straight torch port of the same column loop (kept here as the baseline: the project had no GPTQ before)
  trailing   the fp32 GEMMs that push each block's errors into the rows after it
  hessian    H += X^T X over 128 x 2048 calibration tokens (fp32 addmm, 2048 tokens a call)
  inverse    float64 Cholesky -> inverse -> upper Cholesky, rounded to fp32

Times are device events around each part after a warm-up of the same calls, the median of `--reps` runs; the weights
are N(0, 0.02), the Hessian is that of correlated random inputs (the time of every part is independent of the values).
One JSON line per shape; --out also writes them to a file.

  python tools/gptq_rate.py [--reps 3] [--shapes 4096x4096,...] [--out FILE] [--skip-torch]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from intel_extension_for_transformers_amd import qbits  # noqa: E402
from intel_extension_for_transformers_amd.transformers.llm.quantization.gptq import upper_factor  # noqa: E402

SHAPES = "4096x12288,4096x4096,4096x22016,11008x4096"
TOKENS, CHUNK = 128 * 2048, 2048


def timed(fn, reps, setup=None):
    """median device milliseconds of fn() over reps runs, after one untimed run"""
    out = []
    for i in range(reps + 1):
        if setup:
            setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2]


def torch_sweep(w, u, group, bits, q, scale, err_all):
    """the column loop in torch, sym: about eight launches per input feature"""
    K = w.shape[0]
    qmax, off = 2 ** (bits - 1) - 1, 2 ** (bits - 1)
    s = None
    for c0 in range(0, K, 128):
        c1 = min(c0 + 128, K)
        for j in range(c0, c1):
            if j % group == 0:
                s = w[j:j + group].abs().amax(0) / qmax
                s = torch.where(s == 0, torch.ones_like(s), s)
                scale[j // group] = s
            v = w[j]
            code = torch.clamp(torch.round(v / s), -off, qmax)
            d = code * s
            e = (v - d) / u[j, j]
            w[j + 1:c1].addr_(u[j, j + 1:c1], e, alpha=-1.0)
            w[j] = d
            q[j] = code
            err_all[j] = e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--out")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gptq_rate: needs the GPU (no CPU timing is meaningful)")
    torch.backends.cuda.matmul.allow_tf32 = False
    dev, group, bits = "cuda", args.group, 4
    lines, factors = [], {}
    for shape in args.shapes.split(","):
        K, N = (int(v) for v in shape.split("x"))
        rec = dict(K=K, N=N, group=group, bits=bits, reps=args.reps)
        g = torch.Generator(device=dev).manual_seed(K)
        if K not in factors:
            load = torch.randn(8, K, device=dev, generator=g)
            x = torch.randn(CHUNK, 8, device=dev, generator=g) @ load + 0.5 * torch.randn(CHUNK, K, device=dev, generator=g)
            h = torch.zeros(K, K, device=dev)

            def accumulate():
                for _ in range(TOKENS // CHUNK):
                    h.addmm_(x.t(), x)

            t_h = timed(accumulate, args.reps, setup=h.zero_)
            h.mul_(2.0 / TOKENS)
            d = torch.diagonal(h)
            d += 0.01 * d.mean()
            keep = {}
            t_inv = timed(lambda: keep.__setitem__("u", upper_factor(h)), args.reps)
            factors[K] = (keep["u"], t_h, t_inv)
            del h, x
        u, rec["hessian_ms"], rec["inverse_ms"] = factors[K]
        w0 = 0.02 * torch.randn(K, N, device=dev, generator=g)
        w = w0.clone()
        q = torch.empty(K, N, dtype=torch.int8, device=dev)
        scale = torch.empty((K + group - 1) // group, N, device=dev)
        err = torch.empty(128, N, device=dev)
        blocks = [(c0, min(128, K - c0)) for c0 in range(0, K, 128)]

        def sweeps():
            for c0, rows in blocks:
                qbits.gptq_sweep(w, u, c0, rows, group, bits, False, q, scale, None, err)

        def trailing():
            for c0, rows in blocks:
                if c0 + rows < K:
                    w[c0 + rows:].addmm_(u[c0:c0 + rows, c0 + rows:].t(), err[:rows], alpha=-1.0)

        def whole():
            for c0, rows in blocks:
                qbits.gptq_sweep(w, u, c0, rows, group, bits, False, q, scale, None, err)
                if c0 + rows < K:
                    w[c0 + rows:].addmm_(u[c0:c0 + rows, c0 + rows:].t(), err[:rows], alpha=-1.0)

        reset = lambda: w.copy_(w0)  # noqa: E731
        rec["sweep_ms"] = timed(sweeps, args.reps, setup=reset)
        rec["sweep_us_per_launch"] = 1e3 * rec["sweep_ms"] / len(blocks)
        rec["trailing_ms"] = timed(trailing, args.reps, setup=reset)
        rec["sweep_and_trailing_ms"] = timed(whole, args.reps, setup=reset)
        if not args.skip_torch:
            err_all = torch.empty(K, N, device=dev)
            qt = torch.empty(K, N, dtype=torch.float32, device=dev)

            def torch_whole():
                torch_sweep(w, u, group, bits, qt, scale, err_all)

            rec["torch_sweep_ms"] = timed(torch_whole, 1, setup=reset)
            rec["torch_over_kernel"] = rec["torch_sweep_ms"] / rec["sweep_ms"]
            # both swept every block without the trailing GEMMs: the same problem, so the codes should agree but for
            # fp32 ties and the port's unfused update
            w.copy_(w0)
            sweeps()
            rec["codes_equal_fraction"] = float((q.float() == qt).float().mean())
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()})
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
