"""What TEQ's quantiser costs on the device at the Llama-2-7B linear shapes (group 128, 4 bits):

  forward      qbits.teq_forward: W~ = Q(diag(a) w) / a in bf16 from w and a, one launch
  grad         qbits.teq_grad: from dL/dW~ (bf16) the gradient of a [K], two launches (the partial sums per column
               block, then their sum)
  torch        a plain torch statement of the same fake quantiser (straight-through rounding, amax / amin) and its
               autograd backward to a (kept here as the baseline: the project had no TEQ before)
  block        one whole training step of a 7B-shaped decoder block (hidden 4096, intermediate 11008, 32 heads, bf16,
               `--batch` samples of `--seq` tokens) as quantization/teq.py runs it, and the share of it that the
               quantiser launches of its seven linears take

Bytes are the algorithm's: forward K N (4 + 2) (w read once, W~ written; the range pass reads w a second time, from L2 at
this group size), grad K N (4 + 2) (w and g read), against 8 TB/s. Times are device events around each part after
untimed runs of the same calls, the median of `--reps` runs. One JSON line per shape and one for the block; --out also
writes them to a file.

  python tools/teq_rate.py [--reps 5] [--shapes 4096x4096,...] [--group 128] [--sym] [--out FILE] [--skip-torch]
                           [--skip-block] [--batch 8] [--seq 2048]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from intel_extension_for_transformers_amd import qbits  # noqa: E402
from intel_extension_for_transformers_amd.transformers.llm.quantization import calibration, teq  # noqa: E402

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


def torch_step(w, a, g, group, bits, asym):
    """forward and backward of the fake quantiser in torch; K a multiple of the group"""
    K, N = w.shape
    G = K // group
    L, qmax, off = 2 ** bits - 1, 2 ** (bits - 1) - 1, 2 ** (bits - 1)
    a.grad = None
    u = (w * a[:, None]).view(G, group, N)
    if asym:
        lo = u.amin(1, keepdim=True).clamp(max=0.0)
        hi = u.amax(1, keepdim=True).clamp(min=0.0)
        s = (hi - lo) / L
        s = torch.where(s == 0, torch.ones_like(s), s)
        z = torch.clamp(_ste(-lo / s), 0, L)
        deq = (torch.clamp(_ste(u / s) + z, 0, L) - z) * s
    else:
        s = u.abs().amax(1, keepdim=True) / qmax
        s = torch.where(s == 0, torch.ones_like(s), s)
        deq = torch.clamp(_ste(u / s), -off, qmax) * s
    wq = (deq.view(K, N) / a[:, None]).to(g.dtype)
    wq.backward(g)
    return wq


def rate_shape(K, N, group, bits, asym, reps, skip_torch):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(K + N)
    w = 0.02 * torch.randn(K, N, device=dev, generator=gen)
    a = torch.exp(0.5 * torch.randn(K, device=dev, generator=gen))
    g = torch.randn(K, N, device=dev, generator=gen).to(torch.bfloat16)
    out = torch.empty(K, N, dtype=torch.bfloat16, device=dev)
    da = torch.empty(K, device=dev)
    rec = dict(K=K, N=N, group=group, bits=bits, asym=int(asym), reps=reps)
    ms = timed(lambda: qbits.teq_forward(w, a, group, bits, asym, out=out), reps)
    nbytes = K * N * 6
    rec.update(forward_us=1e3 * ms, forward_GBps=nbytes / ms / 1e6, forward_of_peak=nbytes / (ms * 1e-3) / PEAK)
    ms2 = timed(lambda: qbits.teq_grad(w, a, g, group, bits, asym, out=da), reps)
    rec.update(grad_us=1e3 * ms2, grad_GBps=nbytes / ms2 / 1e6, grad_of_peak=nbytes / (ms2 * 1e-3) / PEAK)
    # the same call with the partial sums in a caller-owned workspace (qbits.set_woq_workspace) instead of a
    # stream-ordered allocation per call
    ws = torch.empty(((N + 63) // 64) * K * 4 + 4096, dtype=torch.int8, device=dev)
    qbits.set_woq_workspace(ws)
    try:
        ms3 = timed(lambda: qbits.teq_grad(w, a, g, group, bits, asym, out=da), reps)
    finally:
        qbits.set_woq_workspace(None)
    rec.update(grad_workspace_us=1e3 * ms3, grad_workspace_GBps=nbytes / ms3 / 1e6)
    rec["forward_plus_grad_us"] = rec["forward_us"] + rec["grad_us"]
    if not skip_torch:
        ta = a.clone().requires_grad_(True)
        with torch.enable_grad():
            tms = timed(lambda: torch_step(w, ta, g, group, bits, asym), max(1, reps // 2), warm=1)
        rec.update(torch_us=1e3 * tms, torch_over_kernels=1e3 * tms / rec["forward_plus_grad_us"])
    return rec


def rate_block(group, bits, asym, reps, batch, seq):
    """one training step of a 7B-shaped block through the driver's own loop"""
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
    quantisers, groups = teq.block_quantisers(linears, [0, 1, 2, 3], group, bits, asym, torch.bfloat16, dev)
    gen = torch.Generator().manual_seed(calibration.SEED)
    n = 4

    def run():
        calibration.train_block(block, inputs, targets, n, batch, gen, *teq.block_trainer(quantisers, groups, n, 1e-3))

    with calibration.fake_quant_forward(linears, quantisers):
        ms = timed(run, reps, warm=1) / n
    gs = [torch.randn_like(q.w).to(torch.bfloat16) for q in quantisers]

    def launches():
        for q, g in zip(quantisers, gs):
            qbits.teq_forward(q.w, q.a.detach(), group, bits, asym, dtype=torch.bfloat16)
            qbits.teq_grad(q.w, q.a.detach(), g, group, bits, asym)

    qms = timed(launches, reps)
    return dict(block="llama-2-7b", batch=batch, seq=seq, group=group, bits=bits, asym=int(asym),
                linears=len(quantisers), step_ms=ms, quantiser_launches_ms=qms, everything_else_ms=ms - qms,
                quantiser_share=qms / ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--sym", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("teq_rate: needs the GPU (no CPU timing is meaningful)")
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = []

    def emit(rec):
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()})
        print(line, flush=True)
        lines.append(line)

    for shape in args.shapes.split(","):
        K, N = (int(x) for x in shape.split("x"))
        emit(rate_shape(K, N, args.group, 4, not args.sym, args.reps, args.skip_torch))
    if not args.skip_block:
        emit(rate_block(args.group, 4, not args.sym, max(1, args.reps // 2), args.batch, args.seq))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
