"""tests/lora_reference.py against plain torch float64: the two-stage maths s (x A^T) B^T, the column layouts of the fused
projections (q | k | v concatenated; gate / up interleaved exactly as runtime.fuse_gate_up interleaves), the XQ decode of
the input, and the tolerance function. No GPU."""
import numpy as np
import torch

from tests import lora_reference as R
from tests import xq_reference as X


def _part(rng, r, K, n, s):
    return (rng.standard_normal((r, K)).astype(np.float32), rng.standard_normal((n, r)).astype(np.float32), s)


def _torch_term(x, part):
    A, B = (torch.from_numpy(np.asarray(t)).double() for t in part[:2])
    s = float(np.float32(part[2]))
    return (s * ((torch.from_numpy(np.asarray(x)).double() @ A.t()) @ B.t())).numpy()


def test_delta_is_the_two_stage_product_per_part_concatenated():
    rng = np.random.default_rng(0)
    K = 128
    x = rng.standard_normal(K).astype(np.float32)
    q, v = _part(rng, 4, K, 128, 2.0), _part(rng, 1, K, 64, 0.25)
    bias = rng.standard_normal(128 + 64 + 64).astype(np.float32)
    d, tol = R.delta(x, [q, (None, 64, 0.0), v], base_bias=bias, inv=0.5)
    want = np.concatenate([0.5 * _torch_term(x, q), np.zeros(64), 0.5 * _torch_term(x, v)]) + bias.astype(np.float64)
    assert np.allclose(d, want, rtol=1e-13, atol=1e-13)
    assert tol.shape == d.shape and (tol > 0).all()
    # an absent part: the static bias and the one rounding of its addition, nothing else
    assert np.array_equal(d[128:192], bias[128:192].astype(np.float64))
    assert np.allclose(tol[128:192], R.U * np.abs(bias[128:192]))
    # no bias, no adapter: zeros with no tolerance
    d0, t0 = R.delta(x, [(None, 32, 0.0)])
    assert not d0.any() and not t0.any()


def test_interleaved_delta_equals_fuse_gate_up_of_the_separate_deltas():
    from intel_extension_for_transformers_amd.runtime.engine import fuse_gate_up

    rng = np.random.default_rng(1)
    K, inter = 128, 256
    x = rng.standard_normal(K).astype(np.float32)
    g, u = _part(rng, 4, K, inter, 2.0), _part(rng, 64, K, inter, 1.0 / 64)
    d, tol = R.delta(x, [g, u], interleave=True)
    dg, du = _torch_term(x, g), _torch_term(x, u)
    want = fuse_gate_up(torch.from_numpy(dg)[None], torch.from_numpy(du)[None])[0].numpy()
    assert d.shape == (2 * inter,) and np.allclose(d, want, rtol=1e-13, atol=1e-13)
    # the layout itself: tile 2 t is gate tile t, tile 2 t + 1 is up tile t
    assert np.allclose(d[:16], dg[:16]) and np.allclose(d[16:32], du[:16]) and np.allclose(d[32:48], dg[16:32])
    tg, tu = R.delta(x, [g])[1], R.delta(x, [u])[1]
    assert np.array_equal(tol, R.fuse_cols(tg, tu))
    a, b = rng.standard_normal((3, inter)), rng.standard_normal((3, inter))
    assert np.array_equal(R.fuse_cols(a, b), fuse_gate_up(torch.from_numpy(a), torch.from_numpy(b)).numpy())


def test_rows_are_the_delta_of_every_row():
    rng = np.random.default_rng(2)
    M, K = 5, 128
    Xr = rng.standard_normal((M, K)).astype(np.float32)
    nw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    parts = [_part(rng, 4, K, 32, 2.0), (None, 16, 0.0), _part(rng, 3, K, 16, 0.5)]
    D, tol = R.expand(Xr, parts, norm_w=nw, eps=1e-5)
    T, _ = R.shrink(Xr, [parts[0][0], parts[2][0]], norm_w=nw, eps=1e-5)
    assert T.shape == (M, 7) and D.shape == (M, 64)
    for m in range(M):
        inv = X.rms_inv(Xr[m], 1e-5)
        d, t = R.delta(Xr[m].astype(np.float64) * nw.astype(np.float64), parts, inv=inv)
        assert np.allclose(D[m], d, rtol=1e-12, atol=1e-14) and np.allclose(tol[m], t, rtol=1e-12)
        want_t = inv * (torch.from_numpy(Xr[m].astype(np.float64) * nw.astype(np.float64)) @
                        torch.from_numpy(np.concatenate([parts[0][0], parts[2][0]])).double().t()).numpy()
        assert np.allclose(T[m], want_t, rtol=1e-12, atol=1e-14)
    # fp16 rows without a norm are taken exactly
    X16 = Xr.astype(np.float16)
    D16, _ = R.expand(X16, [parts[0]])
    assert np.allclose(D16, np.stack([_torch_term(X16[m].astype(np.float64), parts[0]) for m in range(M)]), rtol=1e-12)


def test_xq_input_is_the_decoded_vector_and_the_factor_of_the_partial_sums():
    rng = np.random.default_rng(3)
    K = 256
    x = rng.standard_normal(K).astype(np.float32)
    x[7] *= 30
    nw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    y = (x * nw).astype(np.float32)
    dec, inv = R.xq_input(y, ssq_of=x, eps=1e-5)
    limbs, u, _ = X.encode(y)
    assert np.array_equal(dec, X.decode(limbs, u))
    v, e = X.fixed_point(y)
    assert np.array_equal(dec, (v * np.ldexp(1.0, e - 21)[:, None]).reshape(-1))  # v 2^(e - 21), block by block
    assert np.abs(dec - y.astype(np.float64)).max() <= np.abs(y).max() * 2.0 ** -21
    assert np.isclose(inv, X.rms_inv(x, 1e-5), rtol=1e-14)
    assert R.xq_input(y)[1] == 1.0


def test_tolerance_bounds_an_fp32_evaluation_in_any_order():
    """the derived bound holds for a plain fp32 evaluation, chained in order and pairwise, with a wide margin to spare on
    random data — and it scales with the terms' magnitudes, not with the result's"""
    rng = np.random.default_rng(4)
    K = 512
    x = rng.standard_normal(K).astype(np.float32)
    p = _part(rng, 8, K, 48, 0.125)
    d, tol = R.delta(x, [p], inv=0.75)
    A, B = p[0], p[1]
    t = np.zeros(8, np.float32)
    for k in range(K):
        t = (t + A[:, k] * x[k]).astype(np.float32)
    t = (t * np.float32(0.75)).astype(np.float32)
    got = np.zeros(48, np.float32)
    for j in range(8):
        got = (got + B[:, j] * t[j]).astype(np.float32)
    got = (np.float32(0.125) * got).astype(np.float32)
    assert (np.abs(got.astype(np.float64) - d) <= tol).all()
    pair = (np.float32(0.125) * (B @ ((A @ x) * np.float32(0.75)))).astype(np.float32)
    assert (np.abs(pair.astype(np.float64) - d) <= tol).all()
    d2, tol2 = R.delta(2 * x, [p], inv=0.75)
    assert np.allclose(tol2, 2 * tol)


def test_half_ulp16_and_silu_pairs():
    assert R.half_ulp16(1.0) == 2.0 ** -11 and R.half_ulp16(1.999) == 2.0 ** -11 and R.half_ulp16(2.0) == 2.0 ** -10
    assert R.half_ulp16(0.0) == 2.0 ** -25 and R.half_ulp16(-3e-5) == 2.0 ** -25
    for v in (0.1, 1.5, 300.0, 6e-5):
        assert abs(float(np.float16(v)) - v) <= R.half_ulp16(v)
    rng = np.random.default_rng(5)
    g, u = rng.standard_normal((2, 32)), rng.standard_normal((2, 32))
    gu = R.fuse_cols(g, u)
    out, tol = R.silu_pairs(gu, np.full_like(gu, 1e-6))
    assert np.allclose(out, (torch.nn.functional.silu(torch.from_numpy(g)) * torch.from_numpy(u)).numpy(), rtol=1e-13)
    # moving gate and up by their tolerances stays inside the propagated one
    moved, _ = R.silu_pairs(gu + 1e-6 * np.sign(rng.standard_normal(gu.shape)), np.zeros_like(gu))
    assert (np.abs(moved - out) <= tol).all()
