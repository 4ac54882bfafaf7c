"""No-GPU checks of tests/xq_reference.py, the model of the XQ activation format (csrc/woq_xq.h) the GPU tests compare
the kernels with bit for bit: the digits are balanced and recombine to v, |v| <= 2^21, sx is the block's sum of v, the
decoded value lies within half a unit, 2^(e_b - 22), of the input, and an all-zero block encodes to zeros.

Inputs: N(0, 1) blocks, blocks whose maximum is exactly a power of two and just below one, a block mixing 1e-6 and 1e3,
magnitudes 1e-35 and 1e30 (where the exponent clamp applies) and an all-zero block; seed 0."""
import numpy as np

from tests import xq_reference as X


def special_inputs():
    """fp32 [16 nb]: the blocks of the module docstring (also the GPU conversion test's special input)"""
    rng = np.random.default_rng(0)
    blocks = [rng.standard_normal((8, 16)).astype(np.float32)]
    for p in (-3, 0, 5):  # maximum exactly a power of two: the bottom of its binade, v = +-2^20
        b = (rng.uniform(-1, 1, (2, 16)) * 2.0 ** p).astype(np.float32)
        b[0, 3], b[1, 7] = 2.0 ** p, -2.0 ** p
        blocks.append(b)
    for p in (-3, 0, 5):  # just below a power of two: the top of the binade, v rounds up to +-2^21
        b = (rng.uniform(-1, 1, (2, 16)) * 2.0 ** p).astype(np.float32)
        b[0, 11] = np.nextafter(np.float32(2.0 ** p), np.float32(0))
        b[1, 0] = -np.nextafter(np.float32(2.0 ** p), np.float32(0))
        blocks.append(b)
    mixed = np.full((1, 16), 1e-6, np.float32)
    mixed[0, 5], mixed[0, 9] = 1e3, -1e-6
    blocks.append(mixed)
    blocks.append((rng.standard_normal((1, 16)) * 1e-35).astype(np.float32))  # 2^-117: clamped to e = -100
    big = (rng.uniform(-1, 1, (1, 16)) * 1e30).astype(np.float32)             # 1e30 in [2^99, 2^100): e = 100
    big[0, 2] = 1e30
    blocks.append(big)
    blocks.append(np.zeros((1, 16), np.float32))
    half = np.zeros((1, 16), np.float32)  # ties: v + 0.5 exactly, rounded to even
    half[0, 0], half[0, 1], half[0, 2], half[0, 3] = 1.0, 2.5 * 2.0 ** -20, 3.5 * 2.0 ** -20, -0.5 * 2.0 ** -20
    blocks.append(half)
    return np.concatenate(blocks).reshape(-1)


def test_encode_properties():
    y = special_inputs()
    limbs, u, sx = X.encode(y)
    nb = y.size // 16
    assert limbs.shape == (nb, 3, 16) and limbs.dtype == np.int8 and u.shape == (nb,) and sx.shape == (nb,)
    v, e = X.fixed_point(y)
    lm = limbs.astype(np.int64)
    assert (lm[:, 0] + 256 * lm[:, 1] + 65536 * lm[:, 2] == v).all()
    assert lm[:, :2].min() >= -128 and lm[:, :2].max() <= 127  # (int8 holds them: the sum above is the statement)
    assert np.abs(lm[:, 2]).max() <= 32
    assert np.abs(v).max() == 2 ** 21  # reached by the blocks just below a power of two, never exceeded
    tot = v.sum(axis=1)
    assert (np.abs(sx.astype(np.float64) - tot) <= np.abs(tot) * 2.0 ** -24).all()  # the fp32 nearest to the sum
    assert (u == np.ldexp(1.0, e - 25).astype(np.float32)).all() and (u > 0).all()
    err = np.abs(X.decode(limbs, u).reshape(nb, 16) - y.astype(np.float64).reshape(nb, 16))
    assert (err <= np.ldexp(1.0, e - 22)[:, None]).all()
    # ... which is at most max|y_block| * 2^-21 wherever the exponent is not clamped
    amax = np.abs(y.astype(np.float64)).reshape(nb, 16).max(axis=1)
    free = (amax > 0) & (e > -100) & (e < 100)
    assert free.sum() >= nb - 3 and (err[free].max(axis=1) <= amax[free] * 2.0 ** -21).all()


def test_exponent_edges_and_ties():
    y = special_inputs().reshape(-1, 16)
    e = X.block_exponents(y.reshape(-1))
    assert e[8] == -2 and e[10] == 1 and e[12] == 6       # max exactly 2^p: e = p + 1
    assert e[14] == -3 and e[16] == 0 and e[18] == 5      # just below 2^p: e = p
    assert e[20] == 10                                    # 1e3 in [2^9, 2^10)
    assert e[21] == -100 and e[22] == 100 and e[23] == 0  # clamped, top of the range, all zero
    v, _ = X.fixed_point(y.reshape(-1))
    assert v[20][5] == 1000 * 2 ** 11 and not np.delete(v[20], 5).any()  # 1e-6 * 2^11 rounds to 0 beside 1e3
    assert (v[24][:4] == [2 ** 20, 2, 4, 0]).all()  # e = 1: 2.5 -> 2, 3.5 -> 4, -0.5 -> 0


def test_zero_block_encodes_to_zeros():
    limbs, u, sx = X.encode(np.zeros(32, np.float32))
    assert not limbs.any() and not sx.any() and (u == np.float32(2.0 ** -25)).all()
    assert not X.decode(limbs, u).any()


def test_geometry_restates_the_launch_rule():
    """the forms the GEMV sweep names (tests/test_gpu_xq_gemv_kernel.py)"""
    g = X.geometry
    assert g(128) == [(0, 1, 1, 4, [1])]
    assert g(640) == [(0, 5, 2, 4, [3, 2])]
    assert g(2048)[0][2:4] == (4, 4) and g(2176) == [(0, 17, 3, 8, [6, 6, 5])]
    assert g(4096) == [(0, 32, 4, 8, [8] * 4)]
    assert g(11008) == [(0, 86, 11, 8, [8] * 9 + [7] * 2)]
    assert g(16384)[0][2] == 16 and len(g(16384)) == 1
    assert [(b, c) for b, c, *_ in g(16512)] == [(0, 65), (65, 64)]
    assert [(b, c, nw) for b, c, nw, *_ in g(28672)] == [(0, 112, 14), (112, 112, 14)]
    assert g(8192, epi=1)[0][2:4] == (16, 4) and g(8320, epi=1) == []       # gate/up: 4 tiles per wave, never chained
    assert g(4224, epi=1, ndig=3)[0][2:4] == (5, 8) and g(4096, epi=1, ndig=3)[0][2:4] == (8, 4)  # the wide form
