"""`woq_engine_kv_shift` (csrc/woq_kv_shift.hip) alone, on engines without weights whose cache is filled through
`kv_cache()`, against tests/kv_shift_reference.py (float64, one rounding to the cache type).

Bounds: V rows are copied bit for bit. K rows lie within 1 ulp of the reference and at most 1 % of the elements differ at
all — the kernel rounds its fp64 sum to fp32 before the cache type, the reference rounds once; tests/test_kv_shift_cpu.py
shows an emulation of that arithmetic on these same inputs differing in under 2e-4 of the elements, never by more than
1 ulp. Sink rows, rows at or beyond n_cached and the other sequence stay bit-unchanged; rows
[n_cached - n_discard, n_cached) are unspecified and not looked at. The 2048-position engine has 8 kv heads so that many
workgroups are in flight over overlapping source and destination ranges."""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import kv_shift_reference as R

pytestmark = pytest.mark.gpu


def _bare_engine(kind, kv_heads, head_dim, max_ctx, max_batch, layers=2, **kw):
    """an engine with a cache, rotation tables and nothing else; its K / V filled with this file's standard-normal rows"""
    from intel_extension_for_transformers_amd.runtime import WoqDecoderEngine

    hidden = kv_heads * head_dim
    eng = WoqDecoderEngine(hidden, 16, kv_heads, kv_heads, head_dim, layers, 32, max_ctx=max_ctx, rope_theta=R.THETA,
                           kv_dtype=R.TORCH_DTYPE[kind], max_batch=max_batch, **kw)
    eng.set_head(torch.zeros(32, hidden, dtype=torch.float16), torch.ones(hidden), torch.zeros(32, hidden, dtype=torch.float16))
    shape = (max_batch, layers, max_ctx, kv_heads, head_dim)
    k0, v0 = R.normal_cache(shape, kind, R.K_SEED), R.normal_cache(shape, kind, R.V_SEED)
    _store(eng, k0, v0)
    return eng, R.bits_of(k0), R.bits_of(v0)


def _raw(t):
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t.view(torch.int16)


def _store(eng, k, v):
    _raw(eng.kv_cache("k")).copy_(_raw(k).to(eng.device))
    _raw(eng.kv_cache("v")).copy_(_raw(v).to(eng.device))


def _load(eng):
    return R.bits_of(eng.kv_cache("k")), R.bits_of(eng.kv_cache("v"))


def _check_shift(eng, kind, k0, v0, case, seq, max_ctx, head_dim):
    """one shift of sequence `seq` from the state (k0, v0); every assertion of the issue's list on the cache"""
    n_keep, n_discard, n_cached = case
    k1, v1 = _load(eng)
    moved = slice(n_keep, n_cached - n_discard)
    c, s = R.table_row(max_ctx, head_dim, R.THETA, min(n_discard, max_ctx - 1))  # (row n_discard is read only when rows move)
    want_k, want_v = R.shift_reference(k0[seq], v0[seq], kind, c, s, n_keep, n_discard, n_cached)
    assert np.array_equal(v1[seq][:, moved], want_v), "V rows are a bit copy"
    d = R.ulp_distance(k1[seq][:, moved], want_k, kind)
    worst, frac = (int(d.max()), float((d != 0).mean())) if d.size else (0, 0.0)
    print(kind, head_dim, case, "seq", seq, "worst ulp", worst, "differing", "%.2e" % frac)
    assert worst <= R.MAX_ULP and frac <= R.MAX_DIFFERING, (worst, frac)
    for got, was in ((k1, k0), (v1, v0)):
        assert np.array_equal(got[seq][:, :n_keep], was[seq][:, :n_keep]), "sink rows"
        assert np.array_equal(got[seq][:, n_cached:], was[seq][:, n_cached:]), "rows at or beyond n_cached"
        for other in range(got.shape[0]):
            if other != seq:
                assert np.array_equal(got[other], was[other]), "the other sequence"


@pytest.mark.parametrize("head_dim", [64, 128])
@pytest.mark.parametrize("kind", R.KINDS)
def test_small_shifts_against_the_float64_reference(kind, head_dim):
    max_ctx = R.SMALL["max_ctx"]
    eng, k0, v0 = _bare_engine(kind, R.SMALL_HEADS[head_dim], head_dim, max_ctx, R.SMALL["max_batch"], R.SMALL["layers"])
    k_t, v_t = R.from_bits(k0, kind), R.from_bits(v0, kind)
    for case in R.SMALL_CASES:
        _store(eng, k_t, v_t)
        eng.pos.fill_(case[2])
        eng.set_discarded(5)
        eng.kv_shift(*case)  # sequence 0, the position and the dropped count follow
        assert int(eng.pos.item()) == case[2] - case[1] and eng.discarded() == 5 + case[1]
        assert eng.status() == 0
        _check_shift(eng, kind, k0, v0, case, 0, max_ctx, head_dim)
    # sequence 1: sequence 0 compared bitwise, and the two device words stay where they are
    _store(eng, k_t, v_t)
    eng.pos.fill_(40)
    eng.set_discarded(0)
    eng.kv_shift(4, 8, 64, seq=1, move_pos=False)
    assert int(eng.pos.item()) == 40 and eng.discarded() == 0
    _check_shift(eng, kind, k0, v0, (4, 8, 64), 1, max_ctx, head_dim)
    # without move_pos on sequence 0 the words do not move either
    eng.kv_shift(4, 8, 64, seq=0, move_pos=False)
    assert int(eng.pos.item()) == 40 and eng.discarded() == 0


@pytest.mark.parametrize("kind", R.KINDS)
def test_many_workgroups_over_overlapping_ranges(kind):
    g = R.LARGE
    eng, k0, v0 = _bare_engine(kind, g["kv_heads"], g["head_dim"], g["max_ctx"], g["max_batch"], g["layers"])
    k_t, v_t = R.from_bits(k0, kind), R.from_bits(v0, kind)
    for i, case in enumerate(R.LARGE_CASES):
        if i:
            _store(eng, k_t, v_t)
        eng.pos.fill_(case[2])
        eng.kv_shift(*case)
        assert int(eng.pos.item()) == case[2] - case[1]
        _check_shift(eng, kind, k0, v0, case, 0, g["max_ctx"], g["head_dim"])
    eng.set_discarded(0)


def test_a_shift_is_capturable_and_stream_ordered():
    """nothing allocates or synchronises: the call records into a hipGraph, and the replay does what the eager call does"""
    eng, k0, v0 = _bare_engine("fp16", 2, 64, 64, 1)
    eng.kv_shift(4, 8, 64)
    eager = _load(eng)
    _store(eng, R.from_bits(k0, "fp16"), R.from_bits(v0, "fp16"))
    eng.pos.fill_(64)
    eng.set_discarded(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.kv_shift(4, 8, 64)
    graph.replay()
    torch.cuda.synchronize()
    got = _load(eng)
    assert np.array_equal(got[0], eager[0]) and np.array_equal(got[1], eager[1])
    assert int(eng.pos.item()) == 56 and eng.discarded() == 8


REFUSED = [  # (seq, n_keep, n_discard, n_cached, move_pos)
    (2, 4, 8, 64, False), (-1, 4, 8, 64, False),  # sequence outside [0, max_batch)
    (0, -1, 8, 64, True), (0, 4, 0, 64, True), (0, 4, -3, 64, True),  # n_keep < 0, n_discard < 1
    (0, 4, 61, 64, True), (0, 40, 30, 64, True),  # n_keep + n_discard > n_cached
    (0, 4, 8, 65, True),  # n_cached > max_ctx
    (1, 4, 8, 64, True),  # move_pos on another sequence
]


def test_refused_arguments_launch_nothing():
    eng, k0, v0 = _bare_engine("fp16", 2, 64, 64, 2)
    eng.pos.fill_(64)
    eng.set_discarded(3)
    for seq, n_keep, n_discard, n_cached, move_pos in REFUSED:
        with pytest.raises(RuntimeError, match="QBits:"):
            eng.kv_shift(n_keep, n_discard, n_cached, seq=seq, move_pos=move_pos)
    k1, v1 = _load(eng)
    assert np.array_equal(k1, k0) and np.array_equal(v1, v0)
    assert int(eng.pos.item()) == 64 and eng.discarded() == 3
    assert eng.status() == 0


@pytest.mark.parametrize("kw", [dict(tp_rank=0, tp_size=2), dict(sliding_window=16)])
def test_tensor_parallel_and_sliding_window_engines_are_refused(kw):
    eng, k0, v0 = _bare_engine("fp16", 2, 64, 64, 1, **kw)
    with pytest.raises(RuntimeError, match="QBits:.*(tensor-parallel|sliding window)"):
        eng.kv_shift(4, 8, 64)
    k1, v1 = _load(eng)
    assert np.array_equal(k1, k0) and np.array_equal(v1, v0)


def test_the_discarded_word_is_the_engines_and_starts_at_zero():
    eng, _, _ = _bare_engine("fp16", 2, 64, 64, 1)
    assert L.lib().woq_engine_discarded_ptr(eng._h) and eng.discarded() == 0
    eng.set_discarded(7)
    assert eng.discarded() == 7
    eng.set_discarded(0)
