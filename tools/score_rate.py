"""What scoring a given text costs on the decode engine: `score()` (the scored prompt pass, csrc/woq_score.hip) against
`prefill()` of the same ids (the same pass with lm_head over the last row only) and against the text teacher-forced one
token at a time through `step(greedy=False)` with a torch `log_softmax` per token (the only way to get these numbers out
of the engine without the scored pass). Llama-2-7B geometry over synthetic int4 weights (`synth_llama_weights`), a
2048-token text, one process. The paths alternate; every path is warmed up once, then `--rounds` timed rounds each, host
clock around work that ends in a synchronise. The head stage alone (hi + lo pack, head GEMM, the record, over the rows
the prompt pass left) is timed with device events through `woq_probe_score_rows`. Prints medians and min - max in
milliseconds and writes them to `--out`.

    python tools/score_rate.py --out profiles/r09_prompt_scoring.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from intel_extension_for_transformers_amd import _lib as L  # noqa: E402
from intel_extension_for_transformers_amd.runtime.engine import WoqDecoderEngine, synth_llama_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--forced-rounds", type=int, default=2, help="timed rounds of the teacher-forced loop (seconds each)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    geom = dict(hidden=4096, inter=11008, heads=32, kv_heads=32, head_dim=128, layers=a.layers, vocab=32000)
    eng = WoqDecoderEngine(max_ctx=a.tokens, **geom)
    synth_llama_weights(eng, **geom)
    n = a.tokens
    ids = torch.randint(3, geom["vocab"], (n,), generator=torch.Generator().manual_seed(1)).tolist()
    ids_dev = torch.tensor(ids, dtype=torch.int32, device=eng.device)
    pos_dev = torch.arange(n, dtype=torch.int32, device=eng.device)
    nxt = ids_dev[1:].long()
    eng.tune_attn_for(n)  # the decode attention regime `generate` would pick for this context (the teacher-forced steps)

    def forced():
        """the text one token at a time: logits of every position, log_softmax in torch, one host read at the end"""
        out = torch.empty(n - 1, dtype=torch.float32, device=eng.device)
        for i in range(n - 1):
            eng.token.copy_(ids_dev[i:i + 1])
            eng.pos.copy_(pos_dev[i:i + 1])
            eng.step(greedy=False)
            out[i] = torch.log_softmax(eng.logits, -1)[nxt[i]]
        return out.tolist()

    paths = {"score": lambda: eng.score(ids)[0], "prefill": lambda: eng.prefill(ids, greedy=False)[0, :1].tolist(),
             "forced": forced}
    rounds = {"score": a.rounds, "prefill": a.rounds, "forced": a.forced_rounds}
    times = {k: [] for k in paths}
    results = {}
    for r in range(max(rounds.values()) + 1):  # round 0 warms every path up
        for name, fn in paths.items():
            if r > rounds[name]:
                continue
            torch.cuda.synchronize()
            tic = time.perf_counter()
            results[name] = fn()
            torch.cuda.synchronize()
            if r > 0:
                times[name].append(1e3 * (time.perf_counter() - tic))
    assert eng.status() == 0
    # the head stage alone over the rows the last prompt pass left
    eng.prefill(ids, greedy=False)
    rows, head = eng.prefill_rows(n), eng.head_tensors
    chosen = torch.empty(n, dtype=torch.float32, device=eng.device)
    top_id = torch.empty(n, 20, dtype=torch.int32, device=eng.device)
    top_lp = torch.empty(n, 20, dtype=torch.float32, device=eng.device)
    tg = torch.cat([ids_dev[1:], ids_dev[:1]])
    head_ms = []
    for r in range(a.rounds + 1):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        L.probe_score_rows(rows, head["norm"], eng.cfg.rms_eps, head["lm_head"], tg, chosen, top_id, top_lp)
        ev1.record()
        torch.cuda.synchronize()
        if r > 0:
            head_ms.append(ev0.elapsed_time(ev1))
    times["head_stage"] = head_ms
    med = {k: statistics.median(v) for k, v in times.items()}
    s, f = results["score"], results["forced"]
    worst = max(abs(x - y) for x, y in zip(s, f))
    ppl = torch.tensor(s, dtype=torch.float64).mean().neg().exp().item()
    lines = ["# Llama-2-7B geometry (%d layers), int4 g128, fp16 lm_head, a %d-token text; milliseconds, alternating rounds "
             "after one warm-up round of every path" % (a.layers, n),
             "# path: median (min - max) [rounds]"]
    for k in ("score", "prefill", "forced", "head_stage"):
        lines.append("%-11s %10.2f (%.2f - %.2f) [%d]" % (k, med[k], min(times[k]), max(times[k]), len(times[k])))
    lines += ["score() over prefill(): +%.2f ms = +%.1f %%" % (med["score"] - med["prefill"],
                                                               100 * (med["score"] / med["prefill"] - 1)),
              "head stage (pack + head GEMM + record, device events) as a share of score(): %.1f %%"
              % (100 * med["head_stage"] / med["score"]),
              "score() against the teacher-forced loop: %.1f x faster" % (med["forced"] / med["score"]),
              "largest |score() - teacher-forced| over the %d log-probabilities: %.3e (the prompt pass runs fp16-operand "
              "GEMMs, the decode step int8 / fp32 GEMVs); perplexity %.1f" % (n - 1, worst, ppl)]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
