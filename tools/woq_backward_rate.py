"""What the backward of a quantised projection costs at the Llama-2-7B shapes (int4 sym, group 128, bf16 gradients):

  fused   qbits.woq_linear_backward: dX = dY W_deq^T straight from the blob (csrc/woq_linear_bwd.hip), two launches
          (the pack pass over dY, the product); scratch = woq_linear_backward_workspace(M, blob)
  torch   the only way the project had before: qbits.dequantize_packed_weight to fp32 [K, N], a cast to the gradient's
          dtype, torch.matmul(dY, W.t()); scratch = K N (4 + 2) bytes
  block   one training step (forward + backward under bf16 autocast, no optimiser) of a 7B-shaped decoder block (hidden 4096, intermediate
          11008, 32 heads) over RTN blobs with r = 16 adapters on q/k/v/o, and the share of it that the seven
          woq_linear_backward calls take

FLOPs are the algorithm's, 2 M K N. Times are device events around each call after untimed runs of the same calls; the
two arms alternate inside one process, `--reps` rounds, and every figure is the median with the spread
(max - min) / median of its own rounds beside it. The outputs of the two arms are compared at the timed sizes. One JSON
line per (shape, M) and one for the block; --out also appends them to a file. A run without a GPU fails.

  python tools/woq_backward_rate.py [--reps 7] [--shapes 4096x12288,...] [--rows 512,2048,8192] [--group 128]
                                    [--skip-block] [--block-rows 2048] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from intel_extension_for_transformers_amd import qbits  # noqa: E402

SHAPES = "4096x12288,4096x4096,4096x22016,11008x4096"  # K x N: qkv, o, gate/up, down


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def alternate(fns, reps, warm=2):
    """{name: [ms, ...]}: every round runs each arm once, in turn; `warm` untimed rounds first"""
    out = {k: [] for k in fns}
    for i in range(reps + warm):
        for name, fn in fns.items():
            a, b = _events()
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warm:
                out[name].append(a.elapsed_time(b))
    return out


def med(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return (max(xs) - min(xs)) / med(xs)


def rate_shape(K, N, M, group, reps):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(K + N)
    w = 0.02 * torch.randn(N, K, device=dev, generator=gen)
    blob = qbits.quantize_to_packed_weight(w, True, group, "bf16", "int4_clip", "fp16", False)
    del w
    dY = torch.randn(M, N, device=dev, generator=gen).to(torch.bfloat16)
    out = torch.empty(M, K, dtype=torch.bfloat16, device=dev)
    need = qbits.woq_linear_backward_workspace(M, blob)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    res = {}

    def fused():
        qbits.woq_linear_backward(dY, blob, grad_input=out)

    def torch_arm():
        deq = torch.empty(K, N, dtype=torch.float32, device=dev)
        qbits.dequantize_packed_weight(blob, deq, False, "bf16", "int4_clip", "fp16")
        res["torch"] = torch.matmul(dY, deq.to(dY.dtype).t())

    qbits.set_woq_workspace(ws)
    try:
        t = alternate({"fused": fused, "torch": torch_arm}, reps)
    finally:
        torch.cuda.synchronize()
        qbits.set_woq_workspace(None)
    flops = 2.0 * M * K * N
    ref = res["torch"].float()
    diff = (out.float() - ref).norm().item() / ref.norm().item()
    f, g = med(t["fused"]), med(t["torch"])
    return dict(K=K, N=N, M=M, group=group, reps=reps, fused_us=1e3 * f, fused_spread=spread(t["fused"]),
                fused_TFLOPs=flops / f / 1e9, torch_us=1e3 * g, torch_spread=spread(t["torch"]),
                torch_TFLOPs=flops / g / 1e9, torch_over_fused=g / f, fused_scratch_bytes=need,
                torch_scratch_bytes=K * N * 6, rel_diff_vs_torch=diff)


def rate_block(M, group, reps):
    from transformers import LlamaConfig, LlamaForCausalLM

    from intel_extension_for_transformers_amd.transformers import (AutoModelForCausalLM, LoraConfig, RtnConfig,
                                                                   get_peft_model, prepare_model_for_kbit_training)
    from intel_extension_for_transformers_amd.transformers.llm.quantization.nn.modules import QuantizedLinearQBits

    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=1, num_attention_heads=32,
                      num_key_value_heads=32, vocab_size=1024, max_position_embeddings=max(M, 2048),
                      tie_word_embeddings=False)
    fp = LlamaForCausalLM(cfg).to(torch.bfloat16)
    q = AutoModelForCausalLM.from_pretrained(fp, quantization_config=RtnConfig(bits=4, group_size=group,
                                                                               compute_dtype="bf16", scale_dtype="fp16"))
    q = get_peft_model(prepare_model_for_kbit_training(q), LoraConfig(r=16, lora_alpha=32))
    q.train()
    ids = torch.randint(0, 1024, (1, M), device="cuda")

    def step():
        q.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = q(input_ids=ids, labels=ids).loss
        loss.backward()

    blobs = [m.weight.data for m in q.modules() if isinstance(m, QuantizedLinearQBits)]
    grads = [torch.randn(M, qbits.header_of(b).N, device="cuda").to(torch.bfloat16) for b in blobs]

    def kernels():
        for b, g in zip(blobs, grads):
            qbits.woq_linear_backward(g, b)

    t = alternate({"step": step, "kernels": kernels}, reps, warm=2)
    s, k = med(t["step"]), med(t["kernels"])
    return dict(block="llama-2-7b", rows=M, group=group, lora_r=16, projections=len(blobs), step_ms=s,
                step_spread=spread(t["step"]), backward_kernels_ms=k, backward_kernels_spread=spread(t["kernels"]),
                backward_share=k / s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--rows", default="512,2048,8192")
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--block-rows", type=int, default=2048)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("woq_backward_rate: needs the GPU (no CPU timing is meaningful)")
    lines = []

    def emit(rec):
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()})
        print(line, flush=True)
        lines.append(line)

    for shape in [s for s in args.shapes.split(",") if s]:
        K, N = (int(x) for x in shape.split("x"))
        for M in [int(m) for m in args.rows.split(",") if m]:
            emit(rate_shape(K, N, M, args.group, args.reps))
    if not args.skip_block:
        emit(rate_block(args.block_rows, args.group, max(3, args.reps // 2)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
