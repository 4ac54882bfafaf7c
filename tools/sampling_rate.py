"""Rate of sampled requests on the decode engine: the native sampler (csrc/woq_sample.hip, chained bursts) against the
torch sampler path (`iter_sampled` + `DeviceSampler`, one eager step + a dozen torch kernels per token) and the greedy
chain, in one process. Llama-2-7B geometry over synthetic int4 weights (`synth_llama_weights`), a 32-token prompt + 256
new tokens, prompt pass included (the harness of profiles/r04n_* / r04z_*). The paths alternate, every path is warmed
up once, then `--rounds` timed rounds each; host clock around work that ends in a synchronise (the last burst's token
read). Prints medians and min-max as tokens/s and writes them to `--out`.

    python tools/sampling_rate.py --out profiles/r07_native_sampler.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sampling_rate.py --rounds 1 --paths native_default

Paths `greedy_logprobs` and `native_default_logprobs` are the greedy chain and the default chat request with the
log-probability record on (csrc/woq_logprob.hip, 20 alternatives read back with every burst):

    python tools/sampling_rate.py --paths greedy,greedy_logprobs,native_default,native_default_logprobs

Path `native_default_controls` is the default chat request plus `frequency_penalty = 0.5, min_p = 0.05` (the sampler
controls: one pre-pass launch more per token):

    python tools/sampling_rate.py --paths native_default,native_default_controls

Path `native_default_guided` is the default chat request under a permissive regex guide (the guided pre-pass and the
state's advance: two launches more per token than `native_default`); `--guide-build` times the regex builder on the
host for the largest pattern of tests/test_guide_cpu.py at two vocabulary sizes (no GPU work):

    python tools/sampling_rate.py --paths native_default,native_default_guided
    python tools/sampling_rate.py --guide-build
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from intel_extension_for_transformers_amd.runtime.engine import (DeviceSampler, WoqDecoderEngine, generate_sampled,  # noqa: E402
                                                                 synth_llama_weights)

DEFAULT = dict(do_sample=True, temperature=0.1, top_k=40, top_p=0.75, repetition_penalty=1.1)  # neural_chat/config.py
PENALTY = dict(do_sample=False, repetition_penalty=1.1)
CONTROLS = dict(DEFAULT, frequency_penalty=0.5, min_p=0.05)
BUILD_REGEX = r'\{\"\w{1,4}\":(true|false|null)\}'  # the largest pattern of tests/test_guide_cpu.py


def synthetic_pieces(vocab, seed=1):
    """a vocabulary of `vocab` byte strings: the 256 single bytes, then random printable ASCII pieces of 2..8 bytes"""
    import numpy as np

    rng = np.random.default_rng(seed)
    pieces = [bytes([b]) for b in range(256)]
    pieces += [bytes(rng.integers(32, 127, rng.integers(2, 9)).tolist()) for _ in range(vocab - 256)]
    return pieces


def guide_build_times():
    from intel_extension_for_transformers_amd.runtime.guide import TokenGuide

    for vocab in (32000, 128256):
        pieces = synthetic_pieces(vocab)
        tic = time.perf_counter()
        g = TokenGuide.from_regex(BUILD_REGEX, pieces, [2])
        print("from_regex(%s) at vocab %d: %d states, %.2f s on the host" % (BUILD_REGEX, vocab, g.n_states,
                                                                           time.perf_counter() - tic))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--paths", default="native_default,torch_default,native_penalty,torch_penalty,greedy")
    ap.add_argument("--out", default=None)
    ap.add_argument("--guide-build", action="store_true", help="time the regex builder on the host and exit")
    a = ap.parse_args()
    if a.guide_build:
        guide_build_times()
        return
    geom = dict(hidden=4096, inter=11008, heads=32, kv_heads=32, head_dim=128, layers=a.layers, vocab=32000)
    eng = WoqDecoderEngine(max_ctx=512, **geom)
    synth_llama_weights(eng, **geom)
    prompt = torch.randint(3, geom["vocab"], (a.prompt,), generator=torch.Generator().manual_seed(1)).tolist()

    def native(kw):
        return lambda: eng.generate(prompt, a.new, sampler=dict(seed=1234, **kw))

    def torch_path(kw):
        return lambda: generate_sampled(eng, prompt, a.new, DeviceSampler(**kw))

    def guided():
        """the default request under a guide that permits every printable text (and EOS anywhere)"""
        from intel_extension_for_transformers_amd.runtime.guide import TokenGuide

        if "guide" not in cache:
            cache["guide"] = TokenGuide.from_regex(r"[ -~]*", synthetic_pieces(geom["vocab"]), [2])
        eng.set_sampler(seed=1234, **DEFAULT)
        eng.set_guide(cache["guide"])
        try:
            return sum(eng.iter_generate(prompt, a.new), [])
        finally:
            eng.clear_sampler()

    cache = {}
    paths = {"native_default_guided": guided, "native_default": native(DEFAULT), "torch_default": torch_path(DEFAULT), "native_penalty": native(PENALTY),
             "native_default_controls": native(CONTROLS),
             "torch_penalty": torch_path(PENALTY), "greedy": lambda: eng.generate(prompt, a.new),
             "greedy_logprobs": lambda: eng.generate(prompt, a.new, logprobs=20)[0],
             "native_default_logprobs": lambda: eng.generate(prompt, a.new, sampler=dict(seed=1234, **DEFAULT),
                                                             logprobs=20)[0]}
    names = [n for n in a.paths.split(",") if n]
    times = {n: [] for n in names}
    for r in range(a.rounds + 1):  # round 0 warms every path up (graph capture, torch's lazy kernels)
        for n in names:
            torch.cuda.synchronize()
            tic = time.perf_counter()
            out = paths[n]()  # ends on a host read of the last burst's tokens
            torch.cuda.synchronize()
            if r > 0:
                times[n].append(time.perf_counter() - tic)
            assert len(out) == a.new
    assert eng.status() == 0
    lines = ["# Llama-2-7B geometry (%d layers), int4 g128, %d-token prompt + %d new tokens, prompt pass included; "
             "tokens/s over %d alternating rounds after one warm-up round of every path" % (a.layers, a.prompt, a.new, a.rounds),
             "# path: median (min - max)"]
    for n in names:
        rate = sorted(a.new / t for t in times[n])
        lines.append("%-24s %8.1f (%.1f - %.1f)" % (n, statistics.median(rate), rate[0], rate[-1]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
