"""H2O eviction's four kernels (csrc/woq_h2o.hip) on caller buffers, against plain numpy float64 on the same inputs.

Score tolerances are measured, not chosen: 4 x the largest deviation of a numpy float32 evaluation of the same formula
from the float64 one (the construction of tests/test_gpu_logprob_kernel.py). The decode kernel feeds q to the matrix cores
as fp16 hi + lo, so the reference does not round q; the prompt kernel reads the fp16 q rows the test itself supplies."""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from intel_extension_for_transformers_amd.runtime.engine import build_rope_tables
from tests import kv_shift_reference as R

pytestmark = pytest.mark.gpu
CODE = {"fp16": L.F16, "bf16": L.BF16, "e4m3": L.FP8_E4M3}
GEOMS = [(8, 2), (4, 4)]  # (heads, kv_heads): G = 4 and G = 1
MAX_CTX = 512             # two slices of the decode kernel's 256 rows


def _cache(rng, rows, kv_heads, D, kind, scale=0.5):
    """[MAX_CTX, kv_heads, D] in the cache type with `rows` random rows -> (device tensor, float64 values)"""
    x = np.zeros((MAX_CTX, kv_heads, D), np.float32)
    x[:rows] = rng.standard_normal((rows, kv_heads, D)) * scale
    t = torch.from_numpy(x).to(R.TORCH_DTYPE[kind])
    return t.cuda(), R.decode(R.bits_of(t), kind)


def _softmax(s, dt):
    e = np.exp((s - s.max(-1, keepdims=True)).astype(dt))
    return e / e.sum(-1, keepdims=True, dtype=dt)


@pytest.mark.parametrize("rows", [1, 17, 300])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_decode_score_adds_the_groups_probabilities(kind, geom, D, rows):
    heads, kv_heads = geom
    G, half, pos = heads // kv_heads, D // 2, rows - 1
    rng = np.random.default_rng(rows * 7 + D)
    kc, k64 = _cache(rng, rows, kv_heads, D, kind)
    qkv = rng.standard_normal((heads + 2 * kv_heads) * D).astype(np.float32)
    cos, sin = build_rope_tables(MAX_CTX, D, R.THETA, "cpu")
    # a non-zero pattern (the launch must add, not store) off the binary grid, so that the sum rounds in fp32 even where
    # the probabilities are exact (one row: every probability is 1)
    start = (0.1 * (1 + np.arange(kv_heads * MAX_CTX) % 7)).astype(np.float32).reshape(kv_heads, MAX_CTX)
    score = torch.from_numpy(start.copy()).cuda()
    scratch = torch.zeros(L.h2o_decode_scratch_bytes(kv_heads, MAX_CTX), dtype=torch.uint8, device="cuda")
    # the ragged case also runs the per-head q-norm (Qwen3): x * rsqrt(mean(x^2) + eps) * w in front of the rotation
    qw, eps = ((1 + 0.1 * rng.standard_normal(D)).astype(np.float32), 1e-5) if rows == 17 else (None, 0.0)
    L.h2o_score_decode(torch.from_numpy(qkv).cuda(), kc, CODE[kind], heads, kv_heads, D, torch.tensor([pos], dtype=torch.int32).cuda(),
                       cos.cuda(), sin.cuda(), score, scratch, q_norm=None if qw is None else torch.from_numpy(qw).cuda(), eps=eps)
    got = score.cpu().numpy()
    assert not scratch[:kv_heads * 4].any()  # the arrival counters are zero again

    def formula(dt):
        c, s = cos[pos].numpy().astype(dt), sin[pos].numpy().astype(dt)
        q = qkv[:heads * D].astype(dt).reshape(kv_heads, G, D)
        if qw is not None:
            q = q / np.sqrt((q * q).mean(-1, keepdims=True, dtype=dt) + dt(eps)) * qw.astype(dt)
        qr = np.concatenate([q[..., :half] * c - q[..., half:] * s, q[..., half:] * c + q[..., :half] * s], -1)
        logits = np.einsum("kgd,pkd->kgp", qr, k64[:rows].astype(dt)) * dt(1.0 / np.sqrt(D))
        p = _softmax(logits, dt)
        return start[:, :rows].astype(dt) + p.sum(1, dtype=dt), p

    want, p64 = formula(np.float64)
    tol = 4 * float(np.abs(formula(np.float32)[0].astype(np.float64) - want).max())
    worst = float(np.abs(got[:, :rows] - want).max())
    print(kind, geom, D, rows, "tolerance %.3e worst %.3e smallest probability %.3e" % (tol, worst, p64.min()))
    assert 0 < tol < G * p64.min()  # a dropped row or head would exceed it
    assert worst <= tol
    assert np.array_equal(got[:, rows:], start[:, rows:])  # rows past the position are untouched


@pytest.mark.parametrize("start,T", [(0, 1), (0, 33), (0, 130), (48, 70)])
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_prompt_score_is_the_column_sum_of_the_causal_attention(kind, geom, start, T):
    heads, kv_heads = geom
    G, D, n = heads // kv_heads, 128, start + T
    rng = np.random.default_rng(T)
    kc, k64 = _cache(rng, n, kv_heads, D, kind)
    qkv = torch.from_numpy(rng.standard_normal((T, (heads + 2 * kv_heads) * D)).astype(np.float32)).half()
    score = torch.zeros(kv_heads, MAX_CTX, device="cuda")
    lse = torch.empty(heads, T, device="cuda")
    L.h2o_score_prompt(qkv.cuda(), start, heads, kv_heads, D, kc, CODE[kind], lse, score)
    got = score.cpu().numpy()
    seen = np.arange(n)[None, :] <= start + np.arange(T)[:, None]  # [query, row]

    def formula(dt):
        q = qkv.numpy().astype(dt)[:, :heads * D].reshape(T, kv_heads, G, D)
        logits = np.einsum("tkgd,pkd->kgtp", q, k64[:n].astype(dt)) * dt(1.0 / np.sqrt(D))
        return np.where(seen, _softmax(np.where(seen, logits, -np.inf), dt), dt(0))

    p64 = formula(np.float64)
    want = p64.sum((1, 2))
    tol = 4 * float(np.abs(formula(np.float32).astype(np.float64) - p64).max()) * G * seen.sum(0)  # per row: the terms summed
    err = np.abs(got[:, :n] - want)
    print(kind, geom, start, T, "tolerance %.3e .. %.3e worst %.3e" % (tol.min(), tol.max(), err.max()))
    # (one query over one row: the probability is exactly 1 in any precision, the tolerance is 0 and the kernel must be exact)
    assert (tol.min() > 0 or n == 1) and tol.max() < G * p64[p64 > 0].min()
    assert (err <= tol).all()
    assert not got[:, n:].any()                             # rows no query saw received exactly nothing
    assert (got[:, :n] <= G * seen.sum(0) + tol).all()      # ... and no row more than its queries could give
    if (start, T) == (0, 33):
        assert (got[:, 32] <= G).all()


def _scores(which, layers, kv_heads, n):
    rng = np.random.default_rng(5)
    if which == "distinct":  # a factor apart, another order per (layer, kv head)
        return np.stack([[1.07 ** rng.permutation(n) for _ in range(kv_heads)] for _ in range(layers)]).astype(np.float32)
    return rng.integers(0, 4, (layers, kv_heads, n)).astype(np.float32)  # ties inside the range and across its edges


@pytest.mark.parametrize("which", ["distinct", "ties"])
@pytest.mark.parametrize("n_cached,D", [(24, 128), (257, 64)])
@pytest.mark.parametrize("kind", R.KINDS)
def test_select_and_compact_follow_the_stable_argsort(kind, n_cached, D, which):
    layers, kv_heads, max_ctx = 2, 2, 320
    shape = (layers, max_ctx, kv_heads, D)
    k0, v0 = R.normal_cache(shape, kind, R.K_SEED), R.normal_cache(shape, kind, R.V_SEED)
    kb, vb = R.bits_of(k0), R.bits_of(v0)
    s0 = np.zeros((layers, kv_heads, max_ctx), np.float32)
    s0[..., :n_cached] = _scores(which, layers, kv_heads, n_cached)
    cos, sin = build_rope_tables(max_ctx, D, R.THETA, "cpu")
    c64, s64 = cos.numpy().astype(np.float64), sin.numpy().astype(np.float64)
    for n_keep in (0, 4):
        for n_discard in (1, 7):
            for recent in (0, 5):
                kc, vc, sc = k0.clone().cuda(), v0.clone().cuda(), torch.from_numpy(s0).cuda()
                dst = torch.full((layers, kv_heads, max_ctx), -7, dtype=torch.int32, device="cuda")
                L.h2o_select(sc, dst, n_keep, n_discard, recent, n_cached)
                L.h2o_compact(kc, vc, sc, dst, CODE[kind], D, cos.cuda(), sin.cuda(), n_keep, n_discard, n_cached)
                got_dst, k1, v1, s1 = dst.cpu().numpy(), R.bits_of(kc), R.bits_of(vc), sc.cpu().numpy()
                worst, differing = 0, 0.0
                for l in range(layers):
                    for h in range(kv_heads):
                        lo, hi = n_keep, n_cached - recent
                        keep = np.ones(n_cached, bool)
                        keep[lo + np.argsort(s0[l, h, lo:hi], kind="stable")[:n_discard]] = False
                        want = np.where(keep, np.cumsum(keep) - 1, -1)
                        assert np.array_equal(got_dst[l, h, :n_cached], want), (n_keep, n_discard, recent, l, h)
                        src = np.flatnonzero(keep)
                        to = np.arange(src.size)
                        assert np.array_equal(v1[l, to, h], vb[l, src, h]) and np.array_equal(s1[l, h, to], s0[l, h, src])
                        a, b = R.decode(kb[l, src, h, :D // 2], kind), R.decode(kb[l, src, h, D // 2:], kind)
                        ra, rb = R.rotate_back(a, b, c64[src - to], s64[src - to])
                        d = R.ulp_distance(k1[l, to, h], R.encode(np.concatenate([ra, rb], -1), kind), kind)
                        worst, differing = max(worst, int(d.max())), max(differing, float((d != 0).mean()))
                        assert np.array_equal(k1[l, to[src == to], h], kb[l, src[src == to], h])  # unmoved rows keep their bytes
                print(kind, n_cached, which, (n_keep, n_discard, recent), "K worst ulp", worst, "differing %.2e" % differing)
                assert worst <= R.MAX_ULP and differing <= R.MAX_DIFFERING
