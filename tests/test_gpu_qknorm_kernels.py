"""The attention kernels with a per-head q / k RMSNorm in front of RoPE (Qwen3; woq_engine_set_layer_extras), alone,
through woq_probe_attn_decode_qknorm and woq_probe_rope_append_qknorm, against the float64 reference of
tests/qknorm_reference.py.

Bounds:
* decode attention output: 1e-4 * max|ref| + 1e-6 — the bound tests/test_gpu_attention_kernels.py (_decode_case) holds
  the per-query-head form to, for every cache type, against the cache as stored;
* the appended K row: the reference's normalised, rotated k rounded to the cache type, within one unit of the cache
  type's last place (the kernel's fp32 norm + rotation may land on the other side of a rounding tie);
* rope_append: q rows within one fp16 ulp of the row's largest reference magnitude, K rows within one unit of the cache
  type's last place, v rows and everything outside the appended rows bit-exact.
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import attn_reference as R
from tests import qknorm_reference as Q

FMT_CODE = {"fp16": L.F16, "fp8": L.FP8_E4M3}
EPS = 1e-6
_TABLES = {}


def _tables(n_pos, HD):
    """fp32 cos / sin tables [n_pos, HD / 2] (computed once per head_dim, shared, never written)"""
    if HD not in _TABLES:
        inv = 1.0 / 10000.0 ** (np.arange(0, HD, 2, dtype=np.float64) / HD)
        ang = np.arange(256, dtype=np.float64)[:, None] * inv[None, :]
        cos, sin = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
        cos.setflags(write=False), sin.setflags(write=False)
        _TABLES[HD] = (cos, sin, torch.from_numpy(cos.copy()).cuda(), torch.from_numpy(sin.copy()).cuda())
    assert n_pos <= 256
    return _TABLES[HD]


def _dev(raw):
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.int16 if raw.dtype == np.uint16 else raw.dtype)).cuda()


def _weights(rng, HD):
    return rng.uniform(0.5, 1.5, HD).astype(np.float32), rng.uniform(0.5, 1.5, HD).astype(np.float32)


DEC_CASES = [(heads, kv, HD, fmt, pos, splits)
             for HD in (64, 128) for heads, kv in ((4, 4), (4, 2)) for fmt in ("fp16", "fp8")
             for pos in (0, 1, 63, 64, 130) for splits in (1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEC_CASES, ids=lambda c: "h%d_%d-d%d-%s-p%d-s%d" % c)
def test_attn_decode_qknorm_matches_float64_reference(case):
    heads, kv, HD, fmt, pos, splits = case
    rng = np.random.default_rng(1000 * pos + 10 * HD + heads + kv + splits)
    max_ctx = pos + 40
    cos, sin, dcos, dsin = _tables(max_ctx, HD)
    q_w, k_w = _weights(rng, HD)
    # cached rows exact in the cache type; rows at and beyond the position: finite garbage the kernel must not use
    Kst = R.round_to(rng.standard_normal((max_ctx, kv, HD)), fmt)
    Vst = R.round_to(rng.standard_normal((max_ctx, kv, HD)), fmt)
    Kst[pos:], Vst[pos:] = 448.0, -448.0
    qkv = (3.0 * rng.standard_normal((heads + 2 * kv) * HD)).astype(np.float32)
    kraw0, vraw0 = Q.encode(Kst, fmt), Q.encode(Vst, fmt)
    dpos = torch.tensor([pos], dtype=torch.int32).cuda()
    dqw, dkw = torch.from_numpy(q_w).cuda(), torch.from_numpy(k_w).cuda()
    outs = []
    for merge in ((0, 1) if splits > 1 else (0,)):
        dk, dv = _dev(kraw0), _dev(vraw0)
        dout = torch.full((heads * HD + 64,), 60000.0, dtype=torch.float32).cuda()
        L.probe_attn_decode_qknorm(torch.from_numpy(qkv).cuda(), dk, dv, FMT_CODE[fmt], dpos, dcos, dsin, heads, kv, HD,
                                   max_ctx, 0, splits, merge, dqw, dkw, EPS, dout)
        torch.cuda.synchronize()
        outs.append((dout.cpu().numpy(), dk.cpu().numpy().view(kraw0.dtype), dv.cpu().numpy().view(vraw0.dtype)))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the two merges are not bit-identical"
    got, gk, gv = outs[0]
    assert np.all(got[heads * HD:] == 60000.0), "stores past the output"
    rest = np.ones(max_ctx, bool)
    rest[pos] = False
    assert np.array_equal(gk[rest], kraw0[rest]) and np.array_equal(gv[rest], vraw0[rest]), "cache written beside the row"
    K, V = Q.decode(gk[:pos + 1], fmt), Q.decode(gv[:pos + 1], fmt)
    ref, kr = Q.decode_attention(qkv, K, V, pos, heads, kv, HD, q_w, k_w, EPS, cos, sin)
    # the appended rows
    want_k = R.round_to(kr, fmt)
    k_err = np.abs(K[pos] - want_k)
    assert (k_err <= Q.ulp(want_k, fmt)).all(), "appended k: worst %g units" % (k_err / Q.ulp(want_k, fmt)).max()
    want_v = R.round_to(qkv[(heads + kv) * HD:].reshape(kv, HD).astype(np.float64), fmt)
    assert np.array_equal(V[pos], want_v), "appended v"
    # the attention output, over the cache as stored
    got = got[:heads * HD].astype(np.float64).reshape(heads, HD)
    bound = 1e-4 * np.abs(ref).max() + 1e-6
    err = np.abs(got - ref).max()
    print("\nattn_decode_qknorm %s: err %.3g, bound %.3g" % (case, err, bound))
    assert err <= bound, "err %.3g > bound %.3g" % (err, bound)


# heads 3 / kv 1: 5 head slots a row, so T rows make 20 T (head_dim 64) or 40 T (128) threads — never a whole number of
# 64-lane waves at T = 1, 5, 33 (the last wave is partial), and 33 rows span several 256-thread workgroups
ROPE_CASES = [(T, start, HD, fmt) for T in (1, 5, 33) for start in (0, 7) for HD in (64, 128) for fmt in ("fp16", "fp8")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROPE_CASES, ids=lambda c: "T%d-s%d-d%d-%s" % c)
def test_rope_append_qknorm_matches_float64_reference(case):
    T, start, HD, fmt = case
    heads, kv, n_seq = 3, 1, 1
    nsl = heads + 2 * kv
    assert (T * nsl * (HD // 16)) % 64 != 0
    rng = np.random.default_rng(100 * T + start + HD)
    cos, sin, dcos, dsin = _tables(start + T, HD)
    q_w, k_w = _weights(rng, HD)
    x = R.round_to(4.0 * rng.standard_normal((T, nsl, HD)), "fp16")
    qkv0 = Q.encode(x, "fp16").reshape(T, nsl * HD)
    stride = (start + T + 3) * kv * HD
    k0 = Q.encode(np.full(stride, 448.0), fmt)
    v0 = Q.encode(np.full(stride, -448.0), fmt)
    dq, dk, dv = _dev(qkv0), _dev(k0), _dev(v0)
    L.probe_rope_append_qknorm(dq, n_seq, T, start, heads, kv, HD, dcos, dsin, dk, dv, FMT_CODE[fmt], stride,
                               torch.from_numpy(q_w).cuda(), torch.from_numpy(k_w).cuda(), EPS)
    torch.cuda.synchronize()
    gq = dq.cpu().numpy().view(np.uint16).reshape(T, nsl, HD)
    gk, gv = dk.cpu().numpy().view(k0.dtype), dv.cpu().numpy().view(v0.dtype)
    c, s = cos[start:start + T][:, None, :], sin[start:start + T][:, None, :]
    # q rows, rotated in place; the k / v slots of qkv untouched
    ref_q = Q.normed_rotated(x[:, :heads], q_w, EPS, c, s)
    q_err = np.abs(Q.decode(gq[:, :heads], "fp16") - ref_q)
    q_bound = Q.ulp(np.abs(ref_q).max(axis=-1, keepdims=True), "fp16")
    assert (q_err <= q_bound).all(), "q: worst %g of the bound" % (q_err / q_bound).max()
    assert np.array_equal(gq[:, heads:], qkv0.reshape(T, nsl, HD)[:, heads:]), "k / v slots of qkv written"
    # K rows [start, start + T): normalised, rotated, rounded once; V rows: the fp16 values rounded to the cache type
    a = start * kv * HD
    want_k = R.round_to(Q.normed_rotated(x[:, heads:heads + kv], k_w, EPS, c, s), fmt)
    k_err = np.abs(Q.decode(gk[a:a + T * kv * HD], fmt).reshape(T, kv, HD) - want_k)
    assert (k_err <= Q.ulp(want_k, fmt)).all(), "k: worst %g units" % (k_err / Q.ulp(want_k, fmt)).max()
    want_v = R.round_to(x[:, heads + kv:], fmt)
    assert np.array_equal(Q.decode(gv[a:a + T * kv * HD], fmt).reshape(T, kv, HD), want_v), "v rows"
    owned = np.zeros(stride, bool)
    owned[a:a + T * kv * HD] = True
    assert np.array_equal(gk[~owned], k0[~owned]) and np.array_equal(gv[~owned], v0[~owned]), "cache written outside the rows"
    print("\nrope_append_qknorm %s: q worst %.3f of the bound, k worst %.3f units"
          % (case, (q_err / q_bound).max(), (k_err / Q.ulp(want_k, fmt)).max()))


@pytest.mark.gpu
def test_qknorm_probes_refuse_half_a_norm_by_name():
    z = torch.zeros(64, dtype=torch.float32).cuda()
    rc = L.lib().woq_probe_attn_decode_qknorm(None, None, None, L.F16, None, None, None, 4, 4, 64, 8, 0, 1, 0,
                                              z.data_ptr(), None, EPS, None, None)
    assert rc != 0 and b"q_norm and k_norm" in L.lib().woq_last_error()
