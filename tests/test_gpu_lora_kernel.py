"""The LoRA adapter kernels alone (csrc/woq_lora.hip) through `woq_probe_lora_delta` / `_shrink` / `_expand`, against
tests/lora_reference.py (float64) on the input each kernel really reads.

Delta (the decode step's launch): the XQ vector is made on the device (`woq_probe_xq_from_f32`), read back and decoded
by tests/xq_reference.py, and the RMSNorm factor is taken from the device's own K / 16 partial sums; the fp32 form reads
x and the norm weight as they are. Every case: the output is NaN-poisoned first and every column must be written, a
second run gives the same bytes, and with every rank 0 the launch returns the static bias bit for bit (zeros without one).

Rows (the prompt pass's two launches): shrink over fp32 rows with a norm weight and over fp16 rows without, then the
expand in its three store modes over the shrink's own output, M x K x R_tot as the parameters say. The gate/up mode has
two parts by construction, so at R_tot = 192 it runs ranks (64, 64) over a 128-row shrink. Buffers are padded in rows
and columns; the padding keeps its poison.

Tolerance: tests/lora_reference.py derives it per element, (K + r + 2) 2^-24 sum_j |s B| sum_k |inv A x| plus one rounding
for an addition onto a stored value and half an fp16 ulp for an fp16 store. Nothing is measured into it: every test
prints the worst observed / allowed ratio, and a ratio above 1 is a finding about the kernel.

Worst observed / allowed on an MI355X: delta over XQ 0.005, over fp32 0.31 (the static bias's one rounding is most of that
bound), shrink 0.014, expand onto fp32 0.15, onto fp16 0.99 and gate/up 0.99 (both: the fp16 store's own half ulp).
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import lora_reference as R
from tests import xq_reference as X

pytestmark = pytest.mark.gpu

EPS = 1e-5
POISON16 = np.float16(-123.0)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _parts(rng, K, ranks, cols, scale=0.05):
    """[(A, B, s) | (None, n, 0.0)]: A ~ N(0, 1) / sqrt(K) as Kaiming leaves it, B ~ scale N(0, 1), s = 16 / r"""
    out = []
    for r, n in zip(ranks, cols):
        if r == 0:
            out.append((None, n, 0.0))
            continue
        out.append(((rng.standard_normal((r, K)) / np.sqrt(K)).astype(np.float32),
                    (scale * rng.standard_normal((n, r))).astype(np.float32), 16.0 / r))
    return out


def _dev_parts(parts):
    return [p if p[0] is None else (_dev(p[0]), _dev(p[1]), p[2]) for p in parts]


def _zero_rank(parts):
    return [(None, R.part_cols(p), 0.0) for p in parts]


def _worst(got, want, tol, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.isfinite(np.asarray(got, np.float64)).all(), "%s: a column was not written (or is not finite)" % what
    ratio = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print("%s: worst observed / allowed = %.4f (max error %.3e)" % (what, ratio, float(err.max())))
    assert ratio <= 1.0, what
    return ratio


def _input(K, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(K).astype(np.float32)
    x[K // 3] *= 30
    return x, (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)


def _xq_on_device(x, norm_w):
    """-> ((limbs, u, sx) device, ssq device, decoded float64 [K], inv from the device's partial sums)"""
    K = len(x)
    limbs = torch.zeros(L.xq_limb_bytes(K), dtype=torch.uint8, device="cuda")
    u, sx, ssq = (torch.zeros(K // 16, dtype=torch.float32, device="cuda") for _ in range(3))
    L.probe_xq_from_f32(_dev(x), _dev(norm_w), limbs, u, sx, ssq)
    torch.cuda.synchronize()
    lm = limbs.cpu().numpy()[:K // 16 * 48].view(np.int8).reshape(K // 16, 3, 16)
    dec = X.decode(lm, u.cpu().numpy())
    # the format's own model agrees with the device about what the vector holds
    y = x if norm_w is None else (x * norm_w).astype(np.float32)
    assert np.array_equal(dec, R.xq_input(y)[0])
    inv = 1.0 / np.sqrt(ssq.cpu().numpy().astype(np.float64).sum() / K + EPS)
    return (limbs, u, sx), ssq, dec, inv


def _run_delta(parts, N, base, **kw):
    out = torch.full((N + 8,), float("nan"), dtype=torch.float32, device="cuda")
    out[N:] = 777.0
    L.probe_lora_delta(_dev_parts(parts), out[:N], base_bias=_dev(base), **kw)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[N:] == 777.0).all(), "the launch wrote past its N columns"
    return got[:N]


def _check_delta(what, parts, N, base, x_read, inv, interleave, **kw):
    got = _run_delta(parts, N, base, interleave=interleave, **kw)
    again = _run_delta(parts, N, base, interleave=interleave, **kw)
    assert got.tobytes() == again.tobytes(), "%s: two runs differ" % what
    want, tol = R.delta(x_read, parts, base_bias=base, inv=inv, interleave=interleave)
    _worst(got, want, tol, what)
    none = _run_delta(_zero_rank(parts), N, base, interleave=interleave, **kw)
    assert none.tobytes() == (np.zeros(N, np.float32) if base is None else base).tobytes(), "%s: rank 0 is not the bias" % what
    # the columns of an absent part are the static bias bit for bit with the other parts installed, too
    ref0 = R.delta(x_read, parts, base_bias=None, inv=inv, interleave=interleave)[1] == 0
    assert got[ref0].tobytes() == (np.zeros(N, np.float32) if base is None else base)[ref0].tobytes()


XQ_CASES = {
    # name: (K, ranks, cols, interleave, norm, bias)
    "qkv-128-absent-middle": (128, (4, 0, 4), (128, 128, 128), False, True, False),
    "qkv-4096-ranks-16-1-64-bias": (4096, (16, 1, 64), (4096, 1024, 1024), False, True, True),
    "gate-up-128-r4-r4": (128, (4, 4), (256, 256), True, True, False),
    "gate-up-128-r1-r64": (128, (1, 64), (256, 256), True, True, False),
    "down-11008-r64-no-norm": (11008, (64,), (4096,), False, False, False),
}


@pytest.mark.parametrize("name", list(XQ_CASES))
def test_delta_over_an_xq_vector(name):
    K, ranks, cols, interleave, norm, bias = XQ_CASES[name]
    rng = np.random.default_rng(7)
    parts = _parts(rng, K, ranks, cols)
    N = sum(cols)
    base = rng.standard_normal(N).astype(np.float32) if bias else None
    x, nw = _input(K, 8)
    xq, ssq, dec, inv = _xq_on_device(x, nw if norm else None)
    _check_delta(name, parts, N, base, dec, inv if norm else 1.0, interleave, xq=xq, ssq=ssq if norm else None, eps=EPS)


@pytest.mark.parametrize("K,norm", [(128, True), (128, False), (4096, True), (4096, False)])
def test_delta_over_an_fp32_vector(K, norm):
    rng = np.random.default_rng(9)
    ranks, cols = ((4, 0, 4), (64, 32, 32)) if K == 128 else ((16, 1, 64), (4096, 1024, 1024))
    parts = _parts(rng, K, ranks, cols)
    N = sum(cols)
    base = rng.standard_normal(N).astype(np.float32)
    x, nw = _input(K, 10)
    # what the projection's input is: x times the norm weight, exactly (the kernel's fp32 product of the two is part of
    # its arithmetic, not of its input)
    x_read = x.astype(np.float64) * nw.astype(np.float64) if norm else x.astype(np.float64)
    inv = X.rms_inv(x, EPS) if norm else 1.0
    _check_delta("fp32-K%d-%s" % (K, "norm" if norm else "plain"), parts, N, base, x_read, inv, False,
                 x=_dev(x), norm_w=_dev(nw) if norm else None, eps=EPS)


def test_delta_refuses_what_it_cannot_hold():
    rng = np.random.default_rng(11)
    parts = _dev_parts(_parts(rng, 128, (4,), (64,)))
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    x = torch.zeros(120, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="QBits"):  # K no multiple of 16
        L.probe_lora_delta(parts, out, x=x)
    with pytest.raises(RuntimeError, match="QBits"):  # the parts' columns do not add up to N
        L.probe_lora_delta(parts, out[:48], x=torch.zeros(128, dtype=torch.float32, device="cuda"))


# ---- rows ------------------------------------------------------------------------------------------------------------
RANKS3 = {1: (1, 0, 0), 12: (4, 0, 8), 192: (64, 64, 64)}
RANKS2 = {1: (1, 0), 12: (4, 8), 192: (64, 64)}
COLS3, INTER = (32, 16, 48), 80


def _padded(rows, ld, fill, dtype):
    return torch.full((rows, ld), fill, dtype=dtype, device="cuda")


def _shrink(Xd, M, K, a_parts, r_tot, ldx, norm_w):
    """the shrink into a padded, poisoned T -> (T device [M + 3, ldt], host copy)"""
    T = _padded(M + 3, r_tot + 5, float("nan"), torch.float32)
    L.probe_lora_shrink(Xd, M, K, [_dev(a) for a in a_parts], T, ldx=ldx, norm_w=_dev(norm_w), eps=EPS)
    torch.cuda.synchronize()
    t = T.cpu().numpy()
    assert np.isnan(t[M:]).all() and np.isnan(t[:, r_tot:]).all(), "the shrink wrote outside its M x R_tot block"
    return T, t


@pytest.mark.parametrize("r_tot", [1, 12, 192])
@pytest.mark.parametrize("K", [128, 4096])
@pytest.mark.parametrize("M", [1, 17, 130])
def test_rows_shrink_and_the_three_expand_modes(M, K, r_tot):
    rng = np.random.default_rng(100 * M + r_tot + K)
    nw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    X32 = rng.standard_normal((M, K)).astype(np.float32)
    X32[0, K // 3] *= 30
    X16 = rng.standard_normal((M, K)).astype(np.float16)
    ldx = K + 16
    Xd32 = _padded(M, ldx, 5.0, torch.float32)
    Xd32[:, :K] = _dev(X32)
    Xd16 = _padded(M, ldx, 5.0, torch.float16)
    Xd16[:, :K] = _dev(X16)
    tag = "M%d-K%d-R%d" % (M, K, r_tot)
    worst = 0.0

    # shrink, both input forms, three stacked parts
    parts3 = _parts(rng, K, RANKS3[r_tot], COLS3)
    a3 = [p[0] for p in parts3 if p[0] is not None]
    # (an absent part has no A: the stacked rows skip it, as the descriptor's rank 0 does)
    T_norm, t_norm = _shrink(Xd32, M, K, a3, r_tot, ldx, nw)
    T_f16, t_f16 = _shrink(Xd16, M, K, a3, r_tot, ldx, None)
    assert _shrink(Xd32, M, K, a3, r_tot, ldx, nw)[1].tobytes() == t_norm.tobytes(), "two shrink runs differ"
    want, tol = R.shrink(X32, a3, norm_w=nw, eps=EPS)
    worst = max(worst, _worst(t_norm[:M, :r_tot], want, tol, tag + " shrink fp32 + norm"))
    want, tol = R.shrink(X16, a3)
    worst = max(worst, _worst(t_f16[:M, :r_tot], want, tol, tag + " shrink fp16"))

    # the expand reads a descriptor whose absent parts have rank 0; the probe's T columns are the stacked live ranks
    N = sum(COLS3)
    ldo = N + 8
    # (i) onto fp32 rows: o_proj / down_proj style, over the fp16 rows' T
    base32 = rng.standard_normal((M + 3, ldo)).astype(np.float32)
    out = _dev(base32)
    L.probe_lora_expand(L.LORA_EXPAND_ADD_F32, T_f16, M, N, _expand_parts(parts3), out, ldo)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[M:].tobytes() == base32[M:].tobytes() and got[:, N:].tobytes() == base32[:, N:].tobytes()
    D, tolD = R.expand(X16, parts3)
    want = base32[:M, :N].astype(np.float64) + D
    worst = max(worst, _worst(got[:M, :N], want, tolD + R.U * np.abs(want), tag + " expand onto fp32"))
    out2 = _dev(base32)
    L.probe_lora_expand(L.LORA_EXPAND_ADD_F32, T_f16, M, N, _expand_parts(parts3), out2, ldo)
    torch.cuda.synchronize()
    assert out2.cpu().numpy().tobytes() == got.tobytes(), "two expand runs differ"

    # (ii) onto fp16 rows: qkv style, over the normalised rows' T
    base16 = rng.standard_normal((M + 3, ldo)).astype(np.float16)
    out = _dev(base16)
    L.probe_lora_expand(L.LORA_EXPAND_ADD_F16, T_norm, M, N, _expand_parts(parts3), out, ldo)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[M:].tobytes() == base16[M:].tobytes() and got[:, N:].tobytes() == base16[:, N:].tobytes()
    D, tolD = R.expand(X32, parts3, norm_w=nw, eps=EPS)
    want = base16[:M, :N].astype(np.float64) + D
    tol = tolD + R.U * np.abs(want)
    live = np.concatenate([np.full(n, r > 0) for r, n in zip(RANKS3[r_tot], COLS3)])
    worst = max(worst, _worst(got[:M, :N], want, tol + R.half_ulp16(np.abs(want) + tol), tag + " expand onto fp16"))
    assert got[:M, :N][:, ~live].tobytes() == base16[:M, :N][:, ~live].tobytes(), "an absent part's columns were touched"

    # (iii) gate / up: two interleaved parts over their own shrink, SiLU(gate + D) * (up + D) from fp16 gate/up rows
    ranks2 = RANKS2[r_tot]
    parts2 = _parts(rng, K, ranks2, (INTER, INTER), scale=0.2)
    a2 = [p[0] for p in parts2 if p[0] is not None]
    T2, _ = _shrink(Xd32, M, K, a2, sum(ranks2), ldx, nw)
    ld_gu = 2 * INTER + 16
    gu = np.full((M + 3, ld_gu), POISON16, np.float16)
    gu[:M, :2 * INTER] = rng.standard_normal((M, 2 * INTER)).astype(np.float16)
    act = _padded(M + 3, INTER + 8, float("nan"), torch.float16)
    L.probe_lora_expand(L.LORA_EXPAND_SILU, T2, M, 2 * INTER, _expand_parts(parts2), act, INTER + 8, gu=_dev(gu), ld_gu=ld_gu)
    torch.cuda.synchronize()
    got = act.cpu().numpy()
    assert np.isnan(got[M:]).all() and np.isnan(got[:, INTER:]).all(), "the gate/up expand wrote outside its block"
    D, tolD = R.expand(X32, parts2, norm_w=nw, eps=EPS, interleave=True)
    pre = gu[:M, :2 * INTER].astype(np.float64) + D
    want, tol = R.silu_pairs(pre, tolD + R.U * np.abs(pre))
    worst = max(worst, _worst(got[:M, :INTER], want, tol + R.half_ulp16(np.abs(want) + tol), tag + " expand gate/up"))
    print("%s: worst ratio over the case = %.4f" % (tag, worst))


def _expand_parts(parts):
    return [(None, R.part_cols(p), 0.0) if p[0] is None else (None, _dev(p[1]), p[2]) for p in parts]
