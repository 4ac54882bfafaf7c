"""The engine's attention kernels on their own, element by element against a float64 reference (tests/attn_reference.py),
through the test entry points of include/woq_hip_experimental.h: `rope_append_kernel` and `attn_prefill_kernel`
(csrc/woq_prefill.hip), and the decode launches (csrc/woq_attn_decode.hip) — `attn_decode_kernel` with one workgroup
per head or context slices, `attn_combine_kernel`, the last-arriver slice merge and the grouped-query
`attn_decode_mfma_kernel`.

Inputs (every family at every shape where it applies): random; needles (query p of head h is beta times the stored K
row of one target — p + 1, the first future position; p, the diagonal; p + 1 - window, the oldest visible one;
p - window, the newest one below the window — asserted on the reference alone to carry >= 0.8 of the softmax weight
when visible, beta raised per case until it does); K ramped up along the position (the running maximum moves in every
tile: the rescale path) and down (the maximum settles in tile 0: the skipped rescale); a long tail (one dominant
position in ~40, the rest 10-16 below it in log2: most probabilities in fp16's subnormal range); flat (q = 0: the mean
of the visible V rows). Every buffer a call must not write, every cache row it must not read and the output buffer are
filled with large finite garbage (+-60000 in fp16 / bf16, +-448 in e4m3); after each call every byte outside what the
call owns is compared with its old value, and each call runs twice with bit-identical results.

Bounds (derivation in the PR that added this file, repeated here):
* fp16-operand attention (`attn_prefill_kernel`, `attn_decode_mfma_kernel`: Q, K, V and P enter the MFMA as fp16, fp32
  accumulation, l summed from the unrounded p): |o - ref| <= 2^-10 max_visible|v| + 2^-11 |ref| (+ 1e-6 for fp32
  outputs). P's rounding costs 2^-11 relative plus 2^-25 absolute per subnormal term; l >= 1, so <= 2^-11 + T 2^-25 <=
  2^-10 of max|v| up to T = 8192; the fp16 store adds half an ulp (2^-11 |ref|); the fp32 scores of fp16-exact
  products are accurate far beyond this.
* fp32 decode kernel and combine: DESIGN §4's per-op criterion 1e-4 max|ref| + 1e-6.
* RoPE / append: the float64 rotation rounded to the storage dtype (fp16 saturating at +-65504, e4m3 at +-448), one
  ulp of storage allowed only where the fp32 rotation's own error reaches a rounding tie.

Measured worst err / bound on an MI355X over this file's cases (printed by every test under -s; the bounds are not
tightened to these):
  attn_prefill_kernel      random 0.312, needles 0.298, ramp up 0.307, ramp down 0.300, long tail 0.319, flat 0.279
  attn_decode_mfma_kernel  random 0.074, needles 0.066, ramp up 0.102, ramp down 0.080, long tail 0.060, flat 0.000
  attn_decode_kernel       random 0.002, needles 0.003, ramp up 0.003, ramp down 0.002, long tail 0.002, flat 0.000
  + context slices         random 0.003, needles 0.006, ramp up 0.005, ramp down 0.005, long tail 0.002, flat 0.001
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import attn_reference as R

FMT_CODE = {"fp16": L.F16, "bf16": L.BF16, "fp8": L.FP8_E4M3}
POISON = {"fp16": 60000.0, "bf16": 59904.0, "fp8": 448.0}  # large finite garbage, exact in the format
FAMILIES = ("random", "needles", "ramp_up", "ramp_down", "long_tail", "flat")
WORST = {}


def _e4m3_table():
    v = np.empty(256)
    for c in range(256):
        s, e, m = (-1.0 if c & 0x80 else 1.0), (c >> 3) & 15, c & 7
        v[c] = np.nan if (e == 15 and m == 7) else s * (m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    return v


E4M3 = _e4m3_table()


def encode(x, fmt):
    """values exact in `fmt` -> raw storage (uint16 / uint8)"""
    x = np.asarray(x, dtype=np.float64)
    if fmt == "fp16":
        return x.astype(np.float16).view(np.uint16)
    if fmt == "bf16":
        return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    mag = np.searchsorted(E4M3[:127], np.abs(x))
    assert np.array_equal(E4M3[np.minimum(mag, 126)], np.abs(x)), "value not exact in e4m3"
    return (mag | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def decode(raw, fmt):
    if fmt == "fp16":
        return raw.view(np.float16).astype(np.float64)
    if fmt == "bf16":
        return (raw.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return E4M3[raw]


def to_dev(raw):
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16 if raw.dtype == np.uint16 else raw.dtype)).cuda()


def from_dev(t, like):
    return t.cpu().numpy().view(like)


def poison(shape, fmt, rng):
    return encode(POISON[fmt] * rng.choice([-1.0, 1.0], size=shape), fmt)


def rope_tables(n_pos, HD, theta=10000.0):
    inv = 1.0 / theta ** (np.arange(0, HD, 2, dtype=np.float64) / HD)
    ang = np.arange(n_pos, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _f16(x):
    return R.round_to(x, "fp16")


def _record(kernel, family, ratio):
    WORST[(kernel, family)] = max(WORST.get((kernel, family), 0.0), float(ratio))


def _report(tag):
    print("\n%s worst err/bound: %s" % (tag, ", ".join("%s/%s %.3f" % (k[0], k[1], v) for k, v in sorted(WORST.items()))))


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _cache_rows(family, rng, n_seq, N, kv, HD, fmt):
    """stored K, V [n_seq, N, kv, HD] (fp16 draws rounded to the cache dtype) and the long tail's query direction"""
    K = _f16(rng.standard_normal((n_seq, N, kv, HD)))
    V = _f16(rng.standard_normal((n_seq, N, kv, HD)))
    u = None
    if family == "ramp_up":
        K = _f16(K * np.linspace(0.25, 3.0, N)[None, :, None, None])
    elif family == "ramp_down":
        K = _f16(K * np.linspace(3.0, 0.25, N)[None, :, None, None])
    elif family == "long_tail":
        u = _f16(rng.standard_normal((n_seq, kv, HD)))
        lvl = np.where(rng.random((n_seq, N, kv)) < 1 / 40, 6.0, 6.0 - rng.uniform(10, 16, (n_seq, N, kv)))
        a = lvl * np.sqrt(HD) / (np.log2(np.e) * (u * u).sum(-1))[:, None, :]
        K = _f16(a[..., None] * u[:, None, :, :])
    return R.round_to(K, fmt), R.round_to(V, fmt), u


def _needle_targets(qpos, heads, window, npass):
    """[R, heads] target position and whether it is visible, by type (row + head + npass * heads) % n_types"""
    offs = [1, 0, 1 - window, -window] if window > 0 else [1, 0]
    typ = (np.arange(len(qpos))[:, None] + np.arange(heads)[None, :] + npass * heads) % len(offs)
    tgt = qpos[:, None] + np.array(offs)[typ]
    return tgt, (typ == 1) | (typ == 2)


def _queries(family, rng, K, u, qpos, n_valid, heads, window, beta, npass):
    """q [n_seq, R, heads, HD] (fp16 values) for query positions qpos over the stored rows K; needles: (target, visible,
    placed) [R, heads] each"""
    n_seq, _, kv, HD = K.shape
    rep = heads // kv
    q = _f16(rng.standard_normal((n_seq, len(qpos), heads, HD)))
    needle = None
    if family == "long_tail":
        q = np.broadcast_to(np.repeat(u, rep, axis=1)[:, None], q.shape).copy()
    elif family == "flat":
        q[:] = 0.0
    elif family == "needles":
        tgt, vis = _needle_targets(qpos, heads, window, npass)
        placed = (tgt >= 0) & (tgt < n_valid)
        r_i, h_i = np.nonzero(placed)
        for s in range(n_seq):
            q[s, r_i, h_i] = _f16(beta * K[s, tgt[r_i, h_i], h_i // rep])
        needle = (tgt, vis, placed)
    return q, needle


def _needle_passes(heads, window):
    return -(-(4 if window > 0 else 2) // heads)


# ---- the prompt pass ------------------------------------------------------------------------------------------------
def _prefill_call(Kst, Vst, q, T, start, heads, kv, HD, fmt, window, rng):
    """attn_prefill_kernel over a cache whose rows [0, start + T) are Kst / Vst and all others poison: the fp16 output
    [n_seq, T, heads, HD] as float64, after checking the untouched buffers and a bit-identical second call"""
    n_seq = q.shape[0]
    n_valid = start + T
    stride = (n_valid + 5) * kv * HD  # elements between sequences: more than needed
    caches = []
    for X in (Kst, Vst):
        raw = poison((n_seq * stride + 3 * kv * HD,), fmt, rng)
        for s in range(n_seq):
            raw[s * stride:s * stride + n_valid * kv * HD] = encode(X[s, :n_valid], fmt).reshape(-1)
        caches.append(raw)
    nsl = heads + 2 * kv
    qkv = poison((n_seq * T, nsl * HD), "fp16", rng)
    qkv.reshape(n_seq * T, nsl, HD)[:, :heads] = encode(q, "fp16").reshape(n_seq * T, heads, HD)
    out0 = poison(((n_seq * T + 2) * heads * HD,), "fp16", rng)
    dk, dv, dq = to_dev(caches[0]), to_dev(caches[1]), to_dev(qkv)
    got = []
    for _ in range(2):
        dout = to_dev(out0)
        L.probe_attn_prefill(dq, n_seq, T, start, heads, kv, HD, dk, dv, FMT_CODE[fmt], stride, dout, window)
        torch.cuda.synchronize()
        got.append(from_dev(dout, np.uint16))
    assert np.array_equal(got[0], got[1]), "second call differs"
    assert np.array_equal(from_dev(dk, caches[0].dtype), caches[0]), "K cache written"
    assert np.array_equal(from_dev(dv, caches[1].dtype), caches[1]), "V cache written"
    assert np.array_equal(from_dev(dq, np.uint16), qkv), "qkv written"
    guard = n_seq * T * heads * HD
    assert np.array_equal(got[0][guard:], out0[guard:]), "stores past the output"
    return decode(got[0][:guard], "fp16").reshape(n_seq, T, heads, HD)


def _rows_to_check(T, heads, rng):
    """all rows, or for long chunks the issue's classes: every row of heads 0 and heads - 1; for every head every row
    within 2 of a 64- or 128-row boundary (both ends of the chunk included) and 256 random rows"""
    if T < 2048:
        return {h: np.arange(T) for h in range(heads)}
    near = np.unique(np.clip((np.arange(0, T + 64, 64)[:, None] + np.arange(-2, 3)[None, :]).ravel(), 0, T - 1))
    sel = {}
    for h in range(heads):
        if h in (0, heads - 1):
            sel[h] = np.arange(T)
        else:
            sel[h] = np.unique(np.concatenate([near, rng.choice(T, 256, replace=False), [0, T - 1]]))
        # coverage is a condition: no boundary row and no end of the chunk is left out
        assert set(near) <= set(sel[h]) and {0, T - 1} <= set(sel[h])
    return sel




def _reference(Kst, Vst, q, qpos, n_valid, heads, window, rows, needle):
    """{(sequence, head): (ref, max_visible|v|)} over the checked rows, and the smallest weight of a visible needle"""
    n_seq, _, kv, _ = Kst.shape
    rep = heads // kv
    refs, low = {}, 1.0
    for s in range(n_seq):
        for h in range(heads):
            r = rows[h]
            tg = None if needle is None else needle[0][r, h]
            ref, vmax, wt = R.attend(q[s, r, h], Kst[s, :n_valid, h // rep], Vst[s, :n_valid, h // rep], qpos[r],
                                     window, targets=tg)
            refs[(s, h)] = (ref, vmax)
            if needle is not None:
                m = needle[1][r, h] & needle[2][r, h]
                if m.any():
                    low = min(low, float(wt[m].min()))
    return refs, low


def _check_fp16_operand(got, ref, vmax, extra, name):
    """|o - ref| <= 2^-10 max_visible|v| + 2^-11 |ref| (+ extra); names the first element out of bound"""
    bound = 2.0 ** -10 * vmax[:, None] + 2.0 ** -11 * np.abs(ref) + extra
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i, d = np.argwhere(bad)[0]
        pytest.fail("%s, d %d: got %r, reference %r, bound %.3g (%d elements out of bound)"
                    % (name(i), d, got[i, d], ref[i, d], bound[i, d], int(bad.sum())))
    return float((err / bound).max())


def _prefill_family(family, rng, Kst, Vst, u, T, start, heads, kv, HD, fmt, window, rows, what):
    """one family at one chunk: every needle pass, beta raised until the visible needles hold >= 0.8 of the weight"""
    qpos = start + np.arange(T)
    n_valid = start + T
    for npass in range(_needle_passes(heads, window) if family == "needles" else 1):
        beta = 1.5 if HD == 128 else 2.0
        while True:
            q, needle = _queries(family, rng, Kst, u, qpos, n_valid, heads, window, beta, npass)
            refs, low = _reference(Kst, Vst, q, qpos, n_valid, heads, window, rows, needle)
            if low >= 0.8 or beta > 20:
                break
            beta *= 1.5
        assert low >= 0.8, "%s: a visible needle holds only %.3f of the weight at beta %.1f" % (what, low, beta)
        got = _prefill_call(Kst, Vst, q, T, start, heads, kv, HD, fmt, window, rng)
        worst = 0.0
        for (s, h), (ref, vmax) in refs.items():
            r = rows[h]
            worst = max(worst, _check_fp16_operand(
                got[s, r, h], ref, vmax, 0.0,
                lambda i: "%s, %s: sequence %d, head %d, query row %d (position %d)" % (what, family, s, h, r[i],
                                                                                        qpos[r[i]])))
        _record("attn_prefill", family, worst)


def _prefill_case(n_seq, T, start, heads, kv, HD, fmt, window, seed=0):
    rng = np.random.default_rng(seed)
    what = "attn_prefill(n_seq %d, T %d, start %d, heads %d/%d, hd %d, %s, window %d)" % (n_seq, T, start, heads, kv,
                                                                                         HD, fmt, window)
    for family in FAMILIES:
        Kst, Vst, u = _cache_rows(family, rng, n_seq, start + T, kv, HD, fmt)
        _prefill_family(family, rng, Kst, Vst, u, T, start, heads, kv, HD, fmt, window, _rows_to_check(T, heads, rng),
                        what)


# The prompt-pass cases: a deliberate cross-product subset. Every T meets the plain causal mask (window 0) and a window
# edge; every start, head geometry, head_dim, cache dtype and sequence count meets both; every window below 4096 sits
# inside the span (start + T > window). 4096 appears once with start + T below it and once above it (the chunked long
# case). (32, 32) / (32, 8) / (8, 1) take the 1-D XCD work order, the others the 3-D grid.
PF_T = [1, 2, 31, 32, 33, 127, 128, 129, 200, 2049]
PF_START = [0, 1, 63, 64, 65, 1000]
PF_WINDOW = [1, 31, 32, 33, 64, 65]
PF_GEOM = [(32, 32), (32, 8), (8, 1), (12, 4), (4, 4), (1, 1)]
PF_HD = [64, 128]
PF_FMT = ["fp16", "bf16", "fp8"]
PF_NSEQ = [1, 3]


def _prefill_cases():
    cases = []
    for i, T in enumerate(PF_T):
        big = T > 1024  # the long chunks: the geometries with fewer heads (the reference's cost)
        g0 = PF_GEOM[i % 6] if not big else (12, 4)
        cases.append((PF_NSEQ[(i // 2) % 2], T, PF_START[i % 6], *g0, PF_HD[i % 2], PF_FMT[i % 3], 0))
        w = PF_WINDOW[i % 6]
        start = PF_START[(i + 2) % 6]
        if start + T <= w:
            start = next(s for s in PF_START if s + T > w)
        g1 = PF_GEOM[(i + 3) % 6] if not big else (8, 1)
        cases.append((PF_NSEQ[((i + 1) // 2) % 2], T, start, *g1, PF_HD[(i + 1) % 2], PF_FMT[(i + 1) % 3], w))
    cases.append((1, 200, 1000, 12, 4, 128, "bf16", 4096))  # window wider than everything cached
    cases.append((3, 129, 0, 32, 8, 64, "bf16", 65))  # head_dim 64 on the 1-D work order, with a window
    cases.append((1, 129, 64, 8, 1, 64, "fp8", 0))
    return cases


PF_CASES = _prefill_cases()


def test_prefill_case_list_covers_every_axis_at_every_mask_edge():
    """The case list is the coverage: every value of every axis meets the plain causal mask and a window edge inside
    the span, and every window value sits inside the span at least once (CPU only: checks the list)."""
    axes = {"n_seq": (0, PF_NSEQ), "T": (1, PF_T), "start": (2, PF_START), "geom": (None, PF_GEOM),
            "hd": (5, PF_HD), "fmt": (6, PF_FMT)}
    for name, (k, values) in axes.items():
        for v in values:
            sel = [c for c in PF_CASES if (c[3], c[4]) == v] if k is None else [c for c in PF_CASES if c[k] == v]
            assert any(c[7] == 0 for c in sel), (name, v, "never without a window")
            assert any(0 < c[7] < c[2] + c[1] for c in sel), (name, v, "never at a window edge")
    for w in PF_WINDOW:
        assert any(c[7] == w and c[2] + c[1] > w for c in PF_CASES), w
    assert any(c[7] == 4096 and c[2] + c[1] <= 4096 for c in PF_CASES)
    assert any(c[5] == 64 and c[3] % 8 == 0 and c[7] > 0 for c in PF_CASES)  # hd 64 on the 1-D XCD order


@pytest.mark.gpu
@pytest.mark.parametrize("case", PF_CASES, ids=lambda c: "n%d-T%d-s%d-h%d_%d-d%d-%s-w%d" % c)
def test_attn_prefill_matches_float64_reference(case):
    _prefill_case(*case)
    _report("attn_prefill")


@pytest.mark.gpu
def test_attn_prefill_long_4x2048_32_heads():
    """4 sequences x 2048 positions at 32 heads, head_dim 128, fp16 cache: every row of heads 0 and 31, for every head
    the rows around every 64-row boundary and 256 random rows"""
    _prefill_case(4, 2048, 0, 32, 32, 128, "fp16", 0, seed=1)
    _report("attn_prefill")


@pytest.mark.gpu
def test_attn_prefill_long_8192_in_chunks_window_4096():
    """8192 positions in four chunks of 2048 with window 4096 (Mistral's geometry, 32 / 8 heads, fp8 cache): each chunk
    over the rows earlier chunks left, the rows at and beyond its end poisoned"""
    rng = np.random.default_rng(2)
    heads, kv, HD, fmt, window = 32, 8, 128, "fp8", 4096
    for family in FAMILIES:
        Kst, Vst, u = _cache_rows(family, rng, 1, 8192, kv, HD, fmt)
        for start in range(0, 8192, 2048):
            what = "attn_prefill(8192 in chunks, start %d, window %d)" % (start, window)
            _prefill_family(family, rng, Kst, Vst, u, 2048, start, heads, kv, HD, fmt, window,
                            _rows_to_check(2048, heads, rng), what)
    _report("attn_prefill")


# ---- RoPE + KV append -----------------------------------------------------------------------------------------------
def _check_stored(got, lo, hi, name):
    bad = ~((got >= lo) & (got <= hi))
    if bad.any():
        idx = tuple(np.argwhere(bad)[0])
        pytest.fail("%s at %s: got %r, expected %r (or %r at a rounding tie)" % (name, idx, got[idx], lo[idx], hi[idx]))
    return int((lo != hi).sum())


def _rope_case(n_seq, T, start, heads, kv, HD, fmt, seed=0):
    rng = np.random.default_rng(seed)
    nsl = heads + 2 * kv
    x = _f16(4.0 * rng.standard_normal((n_seq, T, nsl, HD)))
    big = rng.random(x.shape) < 0.03  # saturating inputs: rotations beyond fp16's and e4m3's largest values
    x[big] = _f16(rng.choice([-1.0, 1.0], int(big.sum())) * rng.uniform(30000.0, 65504.0, int(big.sum())))
    qkv0 = encode(x, "fp16").reshape(n_seq * T, nsl * HD)
    cos, sin = rope_tables(start + T + 3, HD)
    stride = (start + T + 7) * kv * HD
    k0 = poison((n_seq * stride + kv * HD,), fmt, rng)
    v0 = poison((n_seq * stride + kv * HD,), fmt, rng)
    like = k0.dtype
    dcos, dsin = torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda()
    res = []
    for _ in range(2):  # twice from the same state: bit-identical
        dq, dk, dv = to_dev(qkv0), to_dev(k0), to_dev(v0)
        L.probe_rope_append(dq, n_seq, T, start, heads, kv, HD, dcos, dsin, dk, dv, FMT_CODE[fmt], stride)
        torch.cuda.synchronize()
        res.append((from_dev(dq, np.uint16), from_dev(dk, like), from_dev(dv, like)))
    for a, b in zip(*res):
        assert np.array_equal(a, b), "second call differs"
    gq, gk, gv = res[0]
    what = "rope_append(n_seq %d, T %d, start %d, heads %d/%d, hd %d, %s)" % (n_seq, T, start, heads, kv, HD, fmt)
    pos = start + np.arange(T)
    c, s = cos[pos][None, :, None, :], sin[pos][None, :, None, :]
    # q rotated in place (fp16, saturating); the k / v slots of qkv untouched
    gq3 = gq.reshape(n_seq, T, nsl, HD)
    ties = _check_stored(decode(gq3[:, :, :heads], "fp16"),
                         *R.stored_bounds(R.rotate(x[:, :, :heads], c, s), R.rotate_error(x[:, :, :heads], c, s), "fp16"),
                         what + " q")
    assert np.array_equal(gq3[:, :, heads:], qkv0.reshape(n_seq, T, nsl, HD)[:, :, heads:]), what + ": k / v slots written"
    # the cache: rows [start, start + T) of every sequence appended, every other byte untouched
    kx, vx = x[:, :, heads:heads + kv], x[:, :, heads + kv:]
    lo_k, hi_k = R.stored_bounds(R.rotate(kx, c, s), R.rotate_error(kx, c, s), fmt)
    want_v = R.round_to(vx, fmt)
    for raw0, got, name in ((k0, gk, "k"), (v0, gv, "v")):
        owned = np.zeros(raw0.shape, bool)
        for sq in range(n_seq):
            a = sq * stride + start * kv * HD
            owned[a:a + T * kv * HD] = True
            rows = decode(got[a:a + T * kv * HD], fmt).reshape(T, kv, HD)
            if name == "k":
                ties += _check_stored(rows, lo_k[sq], hi_k[sq], "%s %s cache, sequence %d" % (what, name, sq))
            else:
                _check_stored(rows, want_v[sq], want_v[sq], "%s %s cache, sequence %d" % (what, name, sq))
        assert np.array_equal(got[~owned], raw0[~owned]), "%s: %s cache written outside the appended rows" % (what, name)
    print("\n%s: ok (%d elements within the fp32 rotation's error of a rounding tie)" % (what, ties))


ROPE_CASES = [(PF_NSEQ[(i + j) % 2], [1, 7, 64, 129][(i + 2 * j) % 4], start, *[(8, 2), (4, 4), (12, 4), (1, 1)][(i + j) % 4],
               PF_HD[(i + j // 2) % 2], fmt)
              for i, start in enumerate(PF_START) for j, fmt in enumerate(PF_FMT)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROPE_CASES, ids=lambda c: "n%d-T%d-s%d-h%d_%d-d%d-%s" % c)
def test_rope_append_matches_float64_rotation(case):
    _rope_case(*case)


# ---- decode ---------------------------------------------------------------------------------------------------------
def _decode_case(heads, kv, HD, fmt, pos, splits, window, grouped=0, chunk=0, seed=0):
    rng = np.random.default_rng(seed)
    rep = heads // kv
    max_ctx = pos + 40  # rows beyond the position: poison the kernels may load and must mask
    cos, sin = rope_tables(max_ctx, HD)
    c, s = cos[pos], sin[pos]
    dcos, dsin = torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda()
    dpos = torch.tensor([pos], dtype=torch.int32).cuda()
    mfma = bool(grouped) and HD == 128 and 1 < splits <= 64 and rep in (2, 4, 8) and fmt in ("fp16", "fp8")
    kernel = "attn_decode_mfma" if mfma else ("attn_decode+slices" if splits > 1 else "attn_decode")
    w_lo = max(0, pos + 1 - window) if window > 0 else 0
    what = "%s(heads %d/%d, hd %d, %s, pos %d, splits %d, window %d, chunk %d)" % (kernel, heads, kv, HD, fmt, pos,
                                                                                  splits, window, chunk)
    merges = (0, 1) if splits > 1 else (0,)
    kpoison, vpoison = poison((max_ctx, kv, HD), fmt, rng), poison((max_ctx, kv, HD), fmt, rng)
    for family in FAMILIES:
        Kst, Vst, u = _cache_rows(family, rng, 1, pos + 1, kv, HD, fmt)  # row `pos` = the new token's rotated k, v
        Kst, Vst = Kst[0], Vst[0]
        kinds = [0, 1, 2] if window > 0 and w_lo >= 1 else [0, 1]  # diagonal, oldest visible, newest below the window
        for npass in range(-(-len(kinds) // heads) if family == "needles" else 1):
            beta = 1.5 if HD == 128 else 2.0
            while True:
                qrot = _f16(rng.standard_normal((heads, HD)))
                tgt = vis = None
                if family == "long_tail":
                    qrot = np.repeat(u[0], rep, axis=0)
                elif family == "flat":
                    qrot[:] = 0.0
                elif family == "needles":
                    kind = np.array([kinds[(h + npass * heads) % len(kinds)] for h in range(heads)])
                    tgt = np.where(kind == 0, pos, np.where(kind == 1, w_lo, w_lo - 1))
                    vis = kind != 2
                    qrot = beta * Kst[tgt, np.arange(heads) // rep]
                qkv = np.concatenate([R.unrotate(qrot, c, s).ravel(), R.unrotate(Kst[pos], c, s).ravel(),
                                      Vst[pos].ravel()]).astype(np.float32)
                if tgt is None:
                    break
                qr = R.rotate(qkv[:heads * HD].reshape(heads, HD).astype(np.float64), c, s)
                low = min(R.attend(qr[h][None], Kst[:, h // rep], Vst[:, h // rep], [pos], window,
                                   targets=[tgt[h]])[2][0] for h in range(heads) if vis[h])
                if low >= 0.8 or beta > 20:
                    break
                beta *= 1.5
            if tgt is not None:
                assert low >= 0.8, "%s: a visible needle holds only %.3f of the weight at beta %.1f" % (what, low, beta)
            kraw0, vraw0 = kpoison.copy(), vpoison.copy()
            kraw0[:pos], vraw0[:pos] = encode(Kst[:pos], fmt), encode(Vst[:pos], fmt)
            out0 = np.float32(POISON["fp16"]) * rng.choice([-1.0, 1.0], heads * HD + 64).astype(np.float32)
            dqkv = torch.from_numpy(qkv).cuda()
            outs = []
            for merge in merges:
                for _ in range(2):
                    dk, dv, dout = to_dev(kraw0), to_dev(vraw0), torch.from_numpy(out0).cuda()
                    L.probe_attn_decode(dqkv, dk, dv, FMT_CODE[fmt], dpos, dcos, dsin, heads, kv, HD, max_ctx, window,
                                        splits, grouped, merge, chunk, dout)
                    torch.cuda.synchronize()
                    outs.append((dout.cpu().numpy(), from_dev(dk, kraw0.dtype), from_dev(dv, vraw0.dtype)))
            for o in outs[1:]:  # repeated calls and the two merges: same sums in the same order
                for a, b in zip(outs[0], o):
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what + ": calls / merges not bit-identical"
            got, gk, gv = outs[0]
            assert np.array_equal(dqkv.cpu().numpy(), qkv), what + ": qkv written"
            assert np.array_equal(got[heads * HD:], out0[heads * HD:]), what + ": stores past the output"
            # the appended row: float64 rotation rounded to the cache dtype; no other cache byte changed
            kx = qkv[heads * HD:(heads + kv) * HD].reshape(kv, HD).astype(np.float64)
            _check_stored(decode(gk[pos], fmt), *R.stored_bounds(R.rotate(kx, c, s), R.rotate_error(kx, c, s), fmt),
                          what + " appended k")
            want_v = R.round_to(qkv[(heads + kv) * HD:].reshape(kv, HD).astype(np.float64), fmt)
            _check_stored(decode(gv[pos], fmt), want_v, want_v, what + " appended v")
            for g, r0, name in ((gk, kraw0, "k"), (gv, vraw0, "v")):
                rest = np.ones(max_ctx, bool)
                rest[pos] = False
                assert np.array_equal(g[rest], r0[rest]), "%s: %s cache written beside row %d" % (what, name, pos)
            # attention over the cache as stored
            K, V = decode(gk[:pos + 1], fmt), decode(gv[:pos + 1], fmt)
            qr = R.rotate(qkv[:heads * HD].reshape(heads, HD).astype(np.float64), c, s)
            refs = [R.attend(qr[h][None], K[:, h // rep], V[:, h // rep], [pos], window) for h in range(heads)]
            ref = np.concatenate([r[0] for r in refs])
            got = got[:heads * HD].astype(np.float64).reshape(heads, HD)
            if mfma:
                worst = _check_fp16_operand(got, ref, np.array([r[1][0] for r in refs]), 1e-6,
                                            lambda h: "%s, %s: head %d (position %d)" % (what, family, h, pos))
            else:
                bound = 1e-4 * np.abs(ref).max() + 1e-6
                err = np.abs(got - ref)
                if not (err <= bound).all():
                    h, d = np.argwhere(~(err <= bound))[0]
                    pytest.fail("%s, %s: head %d (position %d), d %d: got %r, reference %r, bound %.3g"
                                % (what, family, h, pos, d, got[h, d], ref[h, d], bound))
                worst = float(err.max() / bound)
            _record(kernel, family, worst)


DEC_POS = [0, 1, 15, 16, 17, 63, 64, 65, 191, 192, 193, 1000, 4095, 8191]
DEC_SPLITS = [1, 2, 3, 5, 16, 33, 64]
DEC_WINDOW = [0, 1, 17, 64, 4096]
DEC_FMT = ["fp16", "bf16", "fp8"]


def _decode_cases():
    """per-head kernel: every position twice, splits / window / head_dim / dtype on co-prime cycles (slices beyond the
    positions included); grouped form: every (rep, dtype, chunk) combination, windows forcing the adaptive geometry"""
    cases = []
    for i, pos in enumerate(DEC_POS):
        for k, hd in ((0, [64, 128][i % 2]), (1, [128, 64][i % 2])):
            geom = (8, 2) if hd == 128 else (12, 4)
            cases.append((*geom, hd, DEC_FMT[(i + k) % 3], pos, DEC_SPLITS[(i + 3 * k) % 7], DEC_WINDOW[(i + 2 * k) % 5],
                          0, 0))
    i = 0
    for rep, geom in ((2, (8, 4)), (4, (32, 8)), (8, (16, 2))):
        for fmt in ("fp16", "fp8"):
            for chunk in (0, 64, 96):
                cases.append((*geom, 128, fmt, DEC_POS[(5 * i + 3) % 14], [2, 3, 5, 16, 33, 64][i % 6],
                              [0, 0, 17, 4096][i % 4], 1, chunk))
                i += 1
    return cases


DEC_CASES = _decode_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEC_CASES, ids=lambda c: "h%d_%d-d%d-%s-p%d-s%d-w%d-g%d-c%d" % c)
def test_attn_decode_matches_float64_reference(case):
    _decode_case(*case)
    _report("attn_decode")


@pytest.mark.gpu
def test_attn_decode_lds_limit_raises_and_launches_nothing():
    """max_ctx beyond the 160 KiB LDS of one workgroup per head (splits = 1): a QBits error, nothing written"""
    heads, kv, HD, max_ctx = 8, 2, 128, 65536
    rng = np.random.default_rng(5)
    qkv = torch.from_numpy(rng.standard_normal((heads + 2 * kv) * HD).astype(np.float32)).cuda()
    k0 = poison((max_ctx, kv, HD), "fp16", rng)
    dk, dv = to_dev(k0), to_dev(k0)
    cos, sin = rope_tables(max_ctx, HD)
    out0 = np.full(heads * HD, 12345.0, np.float32)
    dout = torch.from_numpy(out0).cuda()
    with pytest.raises(RuntimeError, match=r"^QBits:"):
        L.probe_attn_decode(qkv, dk, dv, L.F16, torch.tensor([100], dtype=torch.int32).cuda(),
                            torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda(), heads, kv, HD, max_ctx, 0, 1, 0,
                            0, 0, dout)
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), out0)
    assert np.array_equal(from_dev(dk, np.uint16), k0) and np.array_equal(from_dev(dv, np.uint16), k0)
