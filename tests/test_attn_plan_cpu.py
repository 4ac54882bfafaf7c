"""The decode attention's plan (csrc/woq_attn_decode.hip plan_attn_decode) on the host, through
woq_probe_attn_decode_plan: which form a step's attention runs in (fused into the qkv launch, per query head, grouped
matrix-core slices), how its context slices merge, and the slice geometry. No device is touched. The kernel-test cases
are the list the GPU test runs (tests/test_gpu_attention_kernels.py), imported, not restated; the engine cases and the
boundaries are worked out here from the rules, not read back from the plan."""
import itertools
import os

import pytest

from intel_extension_for_transformers_amd import _lib as L
from tests.test_gpu_attention_kernels import DEC_CASES, FMT_CODE

pytestmark = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libwoq_hip.so not built (python __graft_entry__.py)")

FUSED, PER_HEAD, GROUPED = L.ATTN_FUSED, L.ATTN_PER_HEAD, L.ATTN_GROUPED
NONE, COMBINE, COUNTER, A2A = L.ATTN_MERGE_NONE, L.ATTN_MERGE_COMBINE, L.ATTN_MERGE_COUNTER, L.ATTN_MERGE_A2A


# ---- csrc/woq_attn_decode.h, restated once: LDS of one per-head attention workgroup ----------------------------------
def spw(span):
    return -(-span // 64) * 16 + 16


def lds_bytes(hd, span):
    return (9 * hd + 12 + 4 * spw(span)) * 4


def span_of(max_ctx, window, slices):
    reach = min(window, max_ctx) if window > 0 else max_ctx
    return ((-(-reach // slices) + 63) // 64) * 64 + 64 if slices > 1 else reach


def largest_span(hd, limit):
    """the largest span whose workgroup still fits `limit` bytes (the formula steps every 64 positions)"""
    s = 64
    while lds_bytes(hd, s + 64) <= limit:
        s += 64
    return s


# ---- the kernel-test cases --------------------------------------------------------------------------------------------
def _probe_plan(heads, kv, hd, fmt, pos, splits, window, grouped, chunk, merge):
    """the plan woq_probe_attn_decode follows for a DEC_CASES entry: no engine around it (fp32 step, no granules)"""
    return L.probe_attn_decode_plan(heads, kv, hd, FMT_CODE[fmt], pos + 40, window, splits, grouped, bool(merge), chunk,
                                    xq=False, granules=False, layers=0)


@pytest.mark.parametrize("case", DEC_CASES, ids=lambda c: "h%d_%d-d%d-%s-p%d-s%d-w%d-g%d-c%d" % c)
def test_kernel_test_cases_reach_the_form_they_name(case):
    heads, kv, hd, fmt, pos, splits, window, grouped, chunk = case
    for merge in (0, 1):
        p = _probe_plan(*case, merge)
        assert p["form"] == (GROUPED if grouped else PER_HEAD), (case, merge, p)
        assert p["merge"] == (NONE if splits == 1 else COUNTER if merge else COMBINE), (case, merge, p)
        assert p["slices"] == splits and p["chunk_fixed"] == (chunk if grouped else 0), (case, merge, p)
        assert (p["grid_x"], p["grid_y"]) == ((kv if grouped else heads), splits), (case, merge, p)
        assert p["launches"] == 2 + (p["merge"] == COMBINE)


def test_grouped_requests_the_grouped_kernel_does_not_cover_run_per_head():
    grouped = [c for c in DEC_CASES if c[7]]
    assert grouped
    for heads, kv, hd, fmt, pos, splits, window, _, chunk in grouped:
        for what, case in (("bf16 cache", (heads, kv, hd, "bf16", pos, splits, window, 1, chunk)),
                           ("one query head per kv head", (kv, kv, hd, fmt, pos, splits, window, 1, chunk)),
                           ("three query heads per kv head", (3 * kv, kv, hd, fmt, pos, splits, window, 1, chunk)),
                           ("head_dim 64", (heads, kv, 64, fmt, pos, splits, window, 1, chunk)),
                           ("one slice", (heads, kv, hd, fmt, pos, 1, window, 1, chunk))):
            for merge in (0, 1):
                p = _probe_plan(*case, merge)
                assert p["form"] == PER_HEAD and p["chunk_fixed"] == 0, (what, case, p)
                assert p["merge"] == (NONE if case[5] == 1 else COUNTER if merge else COMBINE), (what, case, p)
        # a chunk that is no multiple of 32 sub-tile positions: the adaptive geometry
        p = _probe_plan(heads, kv, hd, fmt, pos, splits, window, 1, 100, 0)
        assert p["form"] == GROUPED and p["chunk_fixed"] == 0, p


# ---- engine cases -----------------------------------------------------------------------------------------------------
# (name, heads, kv_heads, hidden = K of the qkv blob, window)
MODELS = [("Llama-2-7B", 32, 32, 4096, 0), ("Mistral-7B", 32, 8, 4096, 0), ("Mistral-7B window", 32, 8, 4096, 4096),
          ("70B rank shape", 64, 8, 4096, 0), ("Llama-2-70B", 64, 8, 8192, 0)]
SLOTS = 256  # resident workgroups of the grouped kernel the cases assume (one per CU)


def _expected(heads, kv, K, window, max_ctx, splits, grouped, fold, xq, layers, granules):
    """the rules of the plan for an int4 g128 blob, head_dim 128, an fp16 cache and every switch at its default"""
    slices = max(splits, 1)
    rep = heads // kv
    fused = (xq and granules and not grouped and layers <= 64 and K == 32 * 128 and slices <= 16
             and (slices == 1 or (not fold and heads * slices <= 512))
             and lds_bytes(128, span_of(max_ctx, window, slices)) <= 38 * 1024)
    if fused:
        return FUSED, (A2A if slices > 1 else NONE), 1
    form = GROUPED if grouped and slices > 1 and rep in (2, 4, 8) else PER_HEAD
    if slices == 1:
        merge = NONE
    elif fold:
        merge = COUNTER
    elif form == GROUPED and xq and granules and layers <= 64 and slices <= 32 and kv * slices <= SLOTS:
        merge = A2A
    else:
        merge = COMBINE
    return form, merge, 2 + (merge == COMBINE)


def test_engine_cases():
    n = {FUSED: 0, PER_HEAD: 0, GROUPED: 0, A2A: 0}
    for (name, heads, kv, K, window), max_ctx, splits, grouped, fold, xq, layers, granules in itertools.product(
            MODELS, (2304, 8448), (1, 2, 16, 17, 32, 33), (False, True), (False, True), (False, True), (64, 65),
            (False, True)):
        p = L.probe_attn_decode_plan(heads, kv, 128, L.F16, max_ctx, window, splits, grouped, fold, 0, xq=xq,
                                     granules=granules, layers=layers, slots=SLOTS, qkv_k=K, group=128)
        what = (name, max_ctx, splits, grouped, fold, xq, layers, granules, p)
        assert (p["form"], p["merge"], p["launches"]) == _expected(heads, kv, K, window, max_ctx, splits, grouped, fold,
                                                                    xq, layers, granules), what
        assert p["slices"] == splits, what
        if p["form"] == FUSED:  # the qkv GEMV's strips, then heads * slices attention workgroups
            assert p["grid_x"] == (heads + 2 * kv) * 128 // 16 + heads * splits and p["grid_y"] == 1, what
        if p["form"] != GROUPED:
            assert p["span"] == span_of(max_ctx, window, splits) and p["spw"] == spw(p["span"]), what
            assert p["lds"] == lds_bytes(128, p["span"]), what
        n[p["form"]] += 1
        n[A2A] += p["merge"] == A2A and p["form"] == GROUPED
    assert all(n.values()), n  # every form, and the grouped all-to-all merge, is reached


def test_blobs_the_fused_launch_does_not_take():
    base = dict(heads=32, kv_heads=32, head_dim=128, kv_dtype=L.F16, max_ctx=2304, qkv_k=4096, group=128)
    assert L.probe_attn_decode_plan(**base)["form"] == FUSED
    assert L.probe_attn_decode_plan(**dict(base, asym=True, group=32))["form"] == FUSED
    for what, change in (("no blob", dict(qkv_k=0)), ("act-order shuffle", dict(act_shuffle=True)),
                         ("nf4", dict(weight_type=L.W_NF4)), ("64 K tiles", dict(qkv_k=8192)),
                         ("padded K", dict(qkv_k=4000)), ("three tiles per group", dict(group=384)),
                         ("head_dim 64", dict(head_dim=64)), ("fuse_attn off", dict(fuse_attn=False)),
                         ("grouped asked for, one slice", dict(grouped=True)),
                         ("grouped asked for, no grouped kernel", dict(grouped=True, splits=4))):
        p = L.probe_attn_decode_plan(**dict(base, **change))
        assert p["form"] == PER_HEAD, (what, p)
    assert L.probe_attn_decode_plan(**dict(base, splits=4))["form"] == FUSED
    assert L.probe_attn_decode_plan(**dict(base, splits=4, fuse_sliced=False))["form"] == PER_HEAD


# ---- boundaries -------------------------------------------------------------------------------------------------------
def test_fused_lds_bound():
    """38 KiB: head_dim 128, one slice, no window -> max_ctx 8448 fuses, 8449 does not; sliced and windowed neighbours
    from the same formula"""
    top = largest_span(128, 38 * 1024)
    assert top == 8448 and lds_bytes(128, top) <= 38 * 1024 < lds_bytes(128, top + 1)
    args = dict(heads=32, kv_heads=32, head_dim=128, kv_dtype=L.F16, qkv_k=4096)

    def form(**kw):
        return L.probe_attn_decode_plan(**dict(args, **kw))["form"]

    assert form(max_ctx=top) == FUSED and form(max_ctx=top + 1) == PER_HEAD
    # a window caps what a query can see
    assert form(max_ctx=100000, window=top) == FUSED and form(max_ctx=100000, window=top + 1) == PER_HEAD
    # slices: each holds its share rounded up to 64, plus 64
    for s in (2, 5, 16):
        reach = (top - 64) * s
        assert span_of(reach, 0, s) == top and span_of(reach + 1, 0, s) == top + 64
        assert form(max_ctx=reach, splits=s) == FUSED and form(max_ctx=reach + 1, splits=s) == PER_HEAD
        assert form(max_ctx=10 ** 6, window=reach, splits=s) == FUSED
        assert form(max_ctx=10 ** 6, window=reach + 1, splits=s) == PER_HEAD


def test_fused_slices_must_be_resident_together():
    args = dict(kv_dtype=L.F16, head_dim=128, max_ctx=2304, qkv_k=4096)
    for heads, kv, s, want in ((32, 8, 16, FUSED), (64, 8, 8, FUSED), (128, 8, 4, FUSED), (128, 8, 5, PER_HEAD),
                               (171, 171, 3, PER_HEAD), (256, 32, 2, FUSED), (257, 257, 2, PER_HEAD)):
        assert (heads * s <= 512) == (want == FUSED)
        assert L.probe_attn_decode_plan(heads=heads, kv_heads=kv, splits=s, **args)["form"] == want, (heads, kv, s)
    assert L.probe_attn_decode_plan(heads=32, kv_heads=8, splits=17, **args)["form"] == PER_HEAD  # at most 16 slices


def test_grouped_all_to_all_needs_the_whole_grid_resident():
    args = dict(heads=32, kv_heads=8, head_dim=128, kv_dtype=L.FP8_E4M3, max_ctx=16384, grouped=True, qkv_k=4096)
    for splits in (2, 16, 32):
        slots = 8 * splits
        assert L.probe_attn_decode_plan(splits=splits, slots=slots, **args)["merge"] == A2A
        assert L.probe_attn_decode_plan(splits=splits, slots=slots - 1, **args)["merge"] == COMBINE
        assert L.probe_attn_decode_plan(splits=splits, slots=slots, fold=True, **args)["merge"] == COUNTER
        assert L.probe_attn_decode_plan(splits=splits, slots=slots, grouped_a2a=False, **args)["merge"] == COMBINE
        assert L.probe_attn_decode_plan(splits=splits, slots=slots, xq=False, **args)["merge"] == COMBINE
    assert L.probe_attn_decode_plan(splits=33, slots=10 ** 6, **args)["merge"] == COMBINE


def test_refusals_carry_the_launchers_text():
    top = largest_span(128, 160 * 1024)
    assert top == 39680
    args = dict(heads=8, kv_heads=2, head_dim=128, kv_dtype=L.F16)
    p = L.probe_attn_decode_plan(max_ctx=top, **args)
    assert p["form"] == PER_HEAD and p["lds"] == lds_bytes(128, top) <= 160 * 1024
    with pytest.raises(RuntimeError, match=r"^QBits: max_ctx too large for the decode attention"):
        L.probe_attn_decode_plan(max_ctx=top + 1, **args)
    assert L.probe_attn_decode_plan(max_ctx=top + 1, splits=2, **args)["lds"] <= 160 * 1024  # slices bring it back
    # two slices: each holds half the context rounded up to 64, plus 64 -> 79232 positions fit, 79233 do not (what the
    # engine's tuner asks about at two slices before it settles on more of them)
    two = 2 * (top - 64)
    assert two == 79232 and span_of(two, 0, 2) == top and span_of(two + 1, 0, 2) == top + 64
    p = L.probe_attn_decode_plan(max_ctx=two, splits=2, **args)
    assert (p["form"], p["merge"], p["span"], p["refused"]) == (PER_HEAD, COMBINE, top, 0)
    with pytest.raises(RuntimeError, match=r"^QBits: max_ctx too large for the decode attention"):
        L.probe_attn_decode_plan(max_ctx=two + 1, splits=2, **args)
    assert L.probe_attn_decode_plan(max_ctx=two + 1, splits=3, **args)["refused"] == 0
    # the grouped form does not depend on the context's length: no refusal where it applies
    assert L.probe_attn_decode_plan(max_ctx=131072, splits=2, grouped=True, **dict(args, heads=8, kv_heads=2))["form"] == GROUPED
    assert L.probe_attn_decode_plan(max_ctx=top + 1, window=top, **args)["span"] == top      # and so does a window
    with pytest.raises(RuntimeError, match=r"^QBits: attention head_dim must be 64 or 128"):
        L.probe_attn_decode_plan(**dict(args, head_dim=96, max_ctx=512))
    assert L.probe_attn_decode_plan(max_ctx=512, splits=64, **args)["slices"] == 64
    with pytest.raises(RuntimeError, match=r"^QBits: at most 64 context slices"):
        L.probe_attn_decode_plan(max_ctx=512, splits=65, **args)


# ---- invariants over a sweep ------------------------------------------------------------------------------------------
def test_invariants_over_a_sweep():
    shapes = [(32, 32), (32, 8), (64, 8), (8, 4), (12, 4), (24, 8), (16, 1), (40, 40)]
    opts = list(itertools.product((False, True), repeat=8))  # grouped fold fuse_attn fuse_sliced a2a xq granules deep
    n = errors = 0
    seen = set()
    for i, ((heads, kv), hd, dt, max_ctx, window, splits) in enumerate(itertools.product(
            shapes, (64, 128), (L.F16, L.BF16, L.FP8_E4M3), (512, 8448, 8449, 40000), (0, 4096), (1, 2, 16, 17, 32, 33, 64))):
        for j in range(8):  # eight of the 256 option sets per shape point, all of them over the sweep
            grouped, fold, fuse_attn, fuse_sliced, a2a, xq, granules, deep = opts[(i * 8 + j * 37) % 256]
            kw = dict(heads=heads, kv_heads=kv, head_dim=hd, kv_dtype=dt, max_ctx=max_ctx, window=window, splits=splits,
                      grouped=grouped, fold=fold, chunk_fixed=(0, 64, 100, 256)[(i + j) % 4], fuse_attn=fuse_attn,
                      fuse_sliced=fuse_sliced, grouped_a2a=a2a, xq=xq, granules=granules, layers=80 if deep else 32,
                      slots=(0, 64, 256, 512)[(i // 3 + j) % 4], qkv_k=4096 if (i + j) % 5 else 0)
            n += 1
            try:
                p = L.probe_attn_decode_plan(**kw)
            except RuntimeError as e:  # the per-head workgroup does not fit: nothing else fails in this sweep
                assert "max_ctx too large" in str(e) and lds_bytes(hd, span_of(max_ctx, window, splits)) > 160 * 1024, kw
                errors += 1
                continue
            what = (kw, p)
            seen.add((p["form"], p["merge"]))
            assert (p["merge"] == NONE) == (p["slices"] <= 1), what
            assert not (p["merge"] == A2A and fold), what
            if p["merge"] == A2A:
                assert p["slices"] <= (32 if p["form"] == GROUPED else 16) and p["form"] != PER_HEAD, what
            if p["form"] == GROUPED:
                assert hd == 128 and heads // kv in (2, 4, 8) and dt in (L.F16, L.FP8_E4M3) and grouped, what
                assert p["chunk_fixed"] % 32 == 0, what
            if p["form"] == FUSED:
                assert not grouped and xq and granules and not deep and fuse_attn, what
            assert p["launches"] == (1 if p["form"] == FUSED else 2 + (p["merge"] == COMBINE)), what
            assert p["lds"] <= 160 * 1024, what
    assert n >= 4000 and errors > 0
    assert seen == {(FUSED, NONE), (FUSED, A2A), (PER_HEAD, NONE), (PER_HEAD, COMBINE), (PER_HEAD, COUNTER),
                    (GROUPED, COMBINE), (GROUPED, COUNTER), (GROUPED, A2A)}, seen
