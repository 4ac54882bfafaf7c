"""Rolling KV cache, the parts that need no GPU: the rotation identity the shift rests on, the schedule
(`plan_stream`), `StreamingConfig`'s checks, the reference's own rounding, and the reference side of the GPU test's
bound — an fp32 emulation of the kernel's arithmetic on the GPU test's own inputs stays within 1 ulp of the rounded
float64 reference and differs from it in far fewer than 1 % of the elements, whichever way the compiler contracts."""
import os
import re

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib
from intel_extension_for_transformers_amd.runtime.streaming import (StreamingConfig, plan_steps, plan_stream,
                                                                    streaming_from_keywords)
from oracle import woq_oracle as orc
from tests import kv_shift_reference as R


def test_rotating_a_rotated_row_back_gives_the_row_of_the_lower_position():
    rng = np.random.default_rng(0)
    for D in (64, 128):
        x = rng.standard_normal((40, 3, D)).astype(np.float32)
        for n in (1, 8, 14, 30):
            pos = np.arange(30, 70, dtype=np.int32)
            there = orc.rope(x, pos, R.THETA)
            back = orc.rope(there, np.full(40, -n, np.int32), R.THETA)
            want = orc.rope(x, pos - n, R.THETA)
            assert np.abs(back - want).max() <= 2e-5 * np.abs(want).max()
            # and the kernel's form of it: the (d, d + D/2) pairing with row n of the engine's tables
            c, s = R.table_row(128, D, R.THETA, n)
            lo, hi = R.rotate_back(there[..., :D // 2].astype(np.float64), there[..., D // 2:].astype(np.float64), c, s)
            assert np.abs(np.concatenate([lo, hi], -1) - want).max() <= 2e-5 * np.abs(want).max()


def _bursts(plan):
    return [ev for ev in plan if ev[0] == "burst"]


def test_plan_without_streaming_equals_the_plain_bursts():
    for n, new, burst in [(5, 1, 16), (5, 2, 16), (7, 40, 16), (7, 33, 5), (1, 17, 1), (3, 0, 4)]:
        want, made = [], 1
        while made < new:
            k = min(burst, new - made)
            want.append(("burst", n + made - 1, k))
            made += k
        assert list(plan_stream(n, new, None, 0, 0, burst)) == want
        assert list(plan_stream(n, new, burst=burst)) == want


def test_plan_stream_invariants_over_a_sweep():
    checked = 0
    for ctx in (8, 32, 33):
        for keep in (0, 1, 4):
            for disc in (1, 2, (ctx - keep) // 2, ctx - keep):
                for n in (1, 5, ctx - 1):
                    for new in (1, 2, ctx - n, ctx - n + 1, 3 * ctx + 1, 100):
                        for burst in (1, 5, 16):
                            plan = list(plan_stream(n, new, ctx, keep, disc, burst))
                            assert sum(ev[2] for ev in _bursts(plan)) == max(new, 1) - 1
                            p, rows = n, n  # position the next step feeds == rows the cache holds
                            for i, ev in enumerate(plan):
                                if ev[0] == "shift":
                                    assert ev[1] == rows == ctx  # only a full cache is shifted ...
                                    assert i + 1 < len(plan) and plan[i + 1][0] == "burst"  # ... and only with tokens left
                                    p = rows = rows - disc
                                    continue
                                _, p0, k = ev
                                assert p0 == p and 1 <= k <= burst and p0 + k <= ctx  # no burst crosses ctx_size
                                p = rows = p0 + k
                            # clipping changes where bursts end, never which steps run
                            steps = [ev[1] for ev in plan_steps(plan) if ev[0] == "step"]
                            assert steps == [ev[1] for ev in plan_steps(plan_stream(n, new, ctx, keep, disc, 1))
                                             if ev[0] == "step"]
                            checked += 1
    assert checked > 1000
    # a request that fits never shifts and equals the plain plan
    assert list(plan_stream(5, 20, 32, 4, 14, 16)) == list(plan_stream(5, 20, None, 0, 0, 16))
    # the positions after a shift: ctx 32, discard 14 -> the next burst starts at 18
    plan = list(plan_stream(6, 100, 32, 4, 14, 16))
    at = [i for i, ev in enumerate(plan) if ev[0] == "shift"]
    # (99 steps: 26 fill the cache from position 6, then every 14 steps fill it again)
    assert len(at) == 6 and all(plan[i + 1][1] == 18 for i in at)
    with pytest.raises(ValueError):
        list(plan_stream(32, 4, 32, 4, 14, 16))  # the prompt fills the cache
    with pytest.raises(ValueError):
        list(plan_stream(3, 4, 32, 4, 0, 16))


def test_streaming_config_validation():
    assert StreamingConfig().resolve(2048, 10) == (2048, 4, 1022)  # the reference's "half"
    assert StreamingConfig(ctx_size=32, n_keep=4, n_discard=14).resolve(64, 31) == (32, 4, 14)
    assert StreamingConfig(32, 0, 32).resolve(32, 1) == (32, 0, 32)
    assert StreamingConfig(33, 4).resolve(64)[2] == 14
    for cfg, max_ctx, n in [(StreamingConfig(128), 64, 1),            # ctx_size beyond the engine
                            (StreamingConfig(32, 4, 0), 64, 1),       # n_discard < 1
                            (StreamingConfig(32, 4, -2), 64, 1),
                            (StreamingConfig(32, 20, 14), 64, 1),     # n_keep + n_discard > ctx_size
                            (StreamingConfig(32, -1, 4), 64, 1),
                            (StreamingConfig(5, 4), 64, 1),           # half of nothing
                            (StreamingConfig(32, 4, 14), 64, 32)]:    # prompt >= ctx_size
        with pytest.raises(ValueError, match="QBits:"):
            cfg.resolve(max_ctx, n)
    assert streaming_from_keywords() is None
    s = streaming_from_keywords(n_discard=7)
    assert (s.ctx_size, s.n_keep, s.n_discard) == (None, 4, 7)


def test_abi_names_the_rolling_cache_entry_points():
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "woq_hip.h")).read()
    declared = set(re.findall(r"WOQ_API[^;(]*?\b(woq_\w+)\s*\(", header))
    new = {"woq_engine_kv_shift", "woq_engine_discarded_ptr", "woq_engine_discarded_set"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert "#define WOQ_ABI_VERSION 4" in header
    assert "woq_probe_sample_stream" in _lib.EXPERIMENTAL_EXPORTS


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_rounding_is_round_to_nearest_even_on_the_cache_grid(kind):
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(20000), rng.standard_normal(2000) * 1e-3]).astype(np.float32)
    if kind == "e4m3":  # ties and the subnormal range on purpose
        x = np.concatenate([x, np.array([1.0625, 1.1875, 0.0009765625, 0.0029296875, -1.0625, 0.0, 17.0, 19.0], np.float32)])
    got = R.encode(x.astype(np.float64), kind)
    want = R.bits_of(torch.from_numpy(x).to(R.TORCH_DTYPE[kind]))  # fp32 -> cache type: one rounding in torch too
    assert np.array_equal(got, want)
    assert np.array_equal(R.encode(R.decode(got, kind), kind), got)  # decode is exact
    one = R.encode(np.array([1.0]), kind)
    assert R.ulp_distance(one, one + 1, kind)[0] == 1 and R.ulp_distance(one, one, kind)[0] == 0
    sign = 0x80 if kind == "e4m3" else 0x8000
    tiny = np.array([1], one.dtype)  # the smallest subnormal, and its negative
    assert R.ulp_distance(tiny | sign, tiny, kind)[0] == 2  # across zero, -0 == +0
    assert R.ulp_distance(np.array([sign], one.dtype), np.array([0], one.dtype), kind)[0] == 0


def _gap(got, want, kind):
    d = R.ulp_distance(got, want, kind)
    return int(d.max()), float((d != 0).mean())


def _emulation_gaps(k_bits, kind, max_ctx, D, case):
    """(worst ulp, differing fraction) of the kernel's arithmetic, and of the plain fp32 forms, against the reference"""
    n_keep, n_discard, n_cached = case
    c, s = R.table_row(max_ctx, D, R.THETA, n_discard)
    c32, s32 = c.astype(np.float32), s.astype(np.float32)
    want, _ = R.shift_reference(k_bits, k_bits, kind, c, s, n_keep, n_discard, n_cached)
    src = k_bits[..., n_keep + n_discard:n_cached, :, :]
    plain = [_gap(R.emulate_fp32(src, kind, c32, s32, fused), want, kind) for fused in (0, 1, 2)]
    return _gap(R.emulate_kernel(src, kind, c32, s32), want, kind), (max(w for w, _ in plain), max(f for _, f in plain))


@pytest.mark.parametrize("kind", R.KINDS)
def test_the_gpu_tests_bound_holds_for_an_emulation_of_the_kernels_arithmetic(kind):
    """The reference side of the GPU test's condition (K within 1 ulp, at most 1 % of elements differing), on the GPU
    test's own inputs at n_discard 1, 7, 8, 64 and 1022: the kernel's arithmetic (fp64 products and sum, rounded to fp32,
    then to the cache type) differs from the once-rounded float64 reference only by that double rounding.
    Also measured: the all-fp32 forms, each product and sum rounded on its own and the two contracted (fma) forms. For
    fp16 and e4m3 they stay within 1 ulp too (about 2e-4 / 5e-5 of the elements differ); for bf16, whose step shrinks with
    the value, a cancelling a * c + b * s lands 2 ulp off on the 2048-position rows — which is why the kernel does not
    sum in fp32."""
    kernel, plain = {}, {}
    for D in (64, 128):
        k_bits = R.bits_of(R.normal_cache(R.small_shape(D), kind, R.K_SEED))[0]
        for case in R.SMALL_CASES[:3]:
            kernel[(D,) + case], plain[(D,) + case] = _emulation_gaps(k_bits, kind, R.SMALL["max_ctx"], D, case)
    k_bits = R.bits_of(R.normal_cache(R.large_shape(), kind, R.K_SEED))[0, :1]  # one layer: 2 M elements per case
    for case in R.LARGE_CASES:
        key = ("large",) + case
        kernel[key], plain[key] = _emulation_gaps(k_bits, kind, R.LARGE["max_ctx"], R.LARGE["head_dim"], case)
    for name, seen in (("kernel", kernel), ("all-fp32", plain)):
        print(kind, name, {k: (w, "%.2e" % f) for k, (w, f) in seen.items()})
    assert all(w <= R.MAX_ULP for w, _ in kernel.values())
    assert all(f <= R.MAX_DIFFERING / 10 for _, f in kernel.values())  # an order of magnitude inside the GPU test's cap
    if kind != "bf16":
        assert all(w <= R.MAX_ULP and f <= R.MAX_DIFFERING / 10 for w, f in plain.values())
