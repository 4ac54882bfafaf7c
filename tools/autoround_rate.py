"""What AutoRound's quantiser costs on the device at the Llama-2-7B linear shapes (group 128, 4 bits, asym):

  forward      qbits.autoround_forward: W~ in bf16 from w, V, alpha, beta, one launch
  step         qbits.autoround_step: from dL/dW~ (bf16) the three gradients and the clamped sign step, one launch
  torch        a plain torch statement of the same fake quantiser (straight-through rounding), its autograd backward
               and the sign step on V, alpha, beta (kept here as the baseline: the project had no AutoRound before)
  block        one whole training iteration of a 7B-shaped decoder block (hidden 4096, intermediate 11008, 32 heads,
               bf16, `--batch` samples of `--seq` tokens) as quantization/autoround.py runs it, and the share of it
               that the fourteen quantiser launches take

Bytes are the algorithm's: forward K N (4 + 4 + 2) (w and V read once, W~ written; the range pass reads w a second time,
from L2 at this group size), step K N (4 + 4 + 4 + 2) (w, V, g read, V written), against 8 TB/s. Times are device events
around each part after untimed runs of the same calls, the median of `--reps` runs. One JSON line per shape and one for
the block; --out also writes them to a file.

  python tools/autoround_rate.py [--reps 5] [--shapes 4096x4096,...] [--group 128] [--out FILE] [--skip-torch]
                                 [--skip-block] [--batch 8] [--seq 2048]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from intel_extension_for_transformers_amd import qbits  # noqa: E402
from intel_extension_for_transformers_amd.transformers.llm.quantization import autoround, calibration  # noqa: E402

SHAPES = "4096x12288,4096x4096,4096x22016,11008x4096"
PEAK = 8.0e12  # bytes / s


def timed(fn, reps, warm=2):
    """median device milliseconds of fn() over reps runs, after `warm` untimed runs"""
    out = []
    for i in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2]


def _ste(x):
    return (torch.round(x) - x).detach() + x


def torch_iteration(w, v, alpha, beta, g, group, bits, lr):
    """forward, backward and sign step of the asym fake quantiser in torch; K a multiple of the group"""
    K, N = w.shape
    G, L = K // group, 2 ** bits - 1
    v.grad = alpha.grad = beta.grad = None
    wg = w.view(G, group, N)
    mn = wg.amin(1, keepdim=True).clamp(max=0.0)
    mx = wg.amax(1, keepdim=True).clamp(min=0.0)
    lo, hi = alpha.view(G, 1, N) * mn, beta.view(G, 1, N) * mx
    s = (hi - lo) / L
    s = torch.where(s == 0, torch.ones_like(s), s)
    z = torch.clamp(_ste(-lo / s), 0, L)
    c = torch.clamp(_ste(wg / s + v.view(G, group, N)) + z, 0, L)
    wq = ((c - z) * s).view(K, N).to(g.dtype)
    wq.backward(g)
    with torch.no_grad():
        v.sub_(lr * v.grad.sign()).clamp_(-0.5, 0.5)
        alpha.sub_(lr * alpha.grad.sign()).clamp_(0.0, 1.0)
        beta.sub_(lr * beta.grad.sign()).clamp_(0.0, 1.0)
    return wq


def rate_shape(K, N, group, bits, reps, skip_torch):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(K + N)
    w = 0.02 * torch.randn(K, N, device=dev, generator=gen)
    G = (K + group - 1) // group
    v = torch.zeros(K, N, device=dev)
    alpha, beta = torch.ones(G, N, device=dev), torch.ones(G, N, device=dev)
    g = torch.randn(K, N, device=dev, generator=gen).to(torch.bfloat16)
    out = torch.empty(K, N, dtype=torch.bfloat16, device=dev)
    rec = dict(K=K, N=N, group=group, bits=bits, reps=reps)
    ms = timed(lambda: qbits.autoround_forward(w, v, alpha, beta, group, bits, True, out=out), reps)
    fbytes = K * N * 10
    rec.update(forward_us=1e3 * ms, forward_GBps=fbytes / ms / 1e6, forward_of_peak=fbytes / (ms * 1e-3) / PEAK)
    ms2 = timed(lambda: qbits.autoround_step(w, v, alpha, beta, g, group, bits, True, 1e-3, 1e-3), reps)
    sbytes = K * N * 14
    rec.update(step_us=1e3 * ms2, step_GBps=sbytes / ms2 / 1e6, step_of_peak=sbytes / (ms2 * 1e-3) / PEAK)
    rec["forward_plus_step_us"] = rec["forward_us"] + rec["step_us"]
    if not skip_torch:
        tv = torch.zeros(K, N, device=dev, requires_grad=True)
        ta = torch.ones(G, N, device=dev, requires_grad=True)
        tb = torch.ones(G, N, device=dev, requires_grad=True)
        with torch.enable_grad():
            tms = timed(lambda: torch_iteration(w, tv, ta, tb, g, group, bits, 1e-3), max(1, reps // 2), warm=1)
        rec.update(torch_us=1e3 * tms, torch_over_kernels=1e3 * tms / rec["forward_plus_step_us"])
    return rec


def rate_block(group, bits, reps, batch, seq):
    """one iteration of a 7B-shaped block through the driver's own loop"""
    from transformers import LlamaConfig, LlamaForCausalLM

    dev = "cuda"
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=1, num_attention_heads=32,
                      num_key_value_heads=32, vocab_size=1024, max_position_embeddings=seq, tie_word_embeddings=False)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev).eval()
    block = model.model.layers[0]
    with torch.no_grad():
        ids = torch.randint(0, 1024, (batch, seq), device=dev)
        inputs = calibration.capture_block_inputs(model, [block], [ids], dev)
        targets = calibration.run_block(block, inputs)
    linears = calibration.block_linears(block, "model.layers.0", [])
    quantisers = [autoround._Quantiser(m, group, bits, True, torch.bfloat16) for _, m in linears]
    gen = torch.Generator().manual_seed(calibration.SEED)
    n = 4

    def run():
        calibration.train_block(block, inputs, targets, n, batch, gen,
                                *autoround.block_trainer(quantisers, n, 1e-3, 1e-3))

    with calibration.fake_quant_forward(linears, quantisers):
        ms = timed(run, reps, warm=1) / n
    gs = [torch.randn_like(q.w).to(torch.bfloat16) for q in quantisers]

    def launches():
        for q, g in zip(quantisers, gs):
            qbits.autoround_forward(q.w, q.v.detach(), q.alpha, q.beta, group, bits, True, dtype=torch.bfloat16)
            qbits.autoround_step(q.w, q.v.detach(), q.alpha, q.beta, g, group, bits, True, 1e-3, 1e-3)

    qms = timed(launches, reps)
    return dict(block="llama-2-7b", batch=batch, seq=seq, group=group, bits=bits, linears=len(quantisers),
                iteration_ms=ms, quantiser_launches_ms=qms, everything_else_ms=ms - qms, quantiser_share=qms / ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--out")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("autoround_rate: needs the GPU (no CPU timing is meaningful)")
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = []

    def emit(rec):
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()})
        print(line, flush=True)
        lines.append(line)

    for shape in args.shapes.split(","):
        K, N = (int(x) for x in shape.split("x"))
        emit(rate_shape(K, N, args.group, 4, args.reps, args.skip_torch))
    if not args.skip_block:
        emit(rate_block(args.group, 4, max(1, args.reps // 2), args.batch, args.seq))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
