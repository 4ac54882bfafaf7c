"""tests/engine_stage_shadow.py without a GPU: the plain arithmetic it holds (trace comparison, changed cache rows, the
float64 decode attention, the restatement's view of a blob) and what its stage ratios would catch — each ratio is at most
1 on a correctly computed output and above 1 on the same output with a wiring slip of relative size 1e-4 (the size that
passes the whole-model oracle bounds).
"""
import numpy as np
import pytest

from oracle import woq_oracle as orc
from tests import attn_reference as R
from tests import engine_stage_shadow as S
from tests import xq_reference as X

F32 = np.float32


def test_first_difference_compares_bytes_stage_by_stage():
    a = [("L0.attn", dict(hidden=np.arange(4, dtype=F32), k=np.zeros(3, np.int16))), ("head", dict(token=np.array([7], np.int32)))]
    b = [(n, {k: v.copy() for k, v in f.items()}) for n, f in a]
    assert S.first_difference(a, b) is None
    b[1][1]["token"][0] = 8
    assert S.first_difference(a, b) == ("head", "token")
    b[0][1]["k"][2] = 1
    assert S.first_difference(a, b) == ("L0.attn", "k")  # the first stage that differs, not the last
    c = [(n, {k: v.copy() for k, v in f.items()}) for n, f in a]
    c[0][1]["hidden"][0] = F32(-0.0)  # equal as numbers, not as bytes
    assert S.first_difference(a, c) == ("L0.attn", "hidden")
    assert S.first_difference(a, a[:1])[0] == "<shape>"
    assert S.first_difference(a, [("L0.attn", dict(hidden=a[0][1]["hidden"])), a[1]])[0] == "<shape>"
    assert S.first_difference(a, [("L0.attn", dict(hidden=a[0][1]["hidden"].astype(np.float64), k=a[0][1]["k"])), a[1]]) \
        == ("L0.attn", "hidden")


def test_changed_rows_names_every_touched_row():
    before = np.zeros((2, 3, 5, 2, 4), np.int16)  # [sequence, layer, position, kv head, d]
    after = before.copy()
    assert S.changed_rows(before, after) == []
    after[1, 2, 4, 1, 3] = 1
    after[0, 0, 0, 0, 0] = -1
    assert S.changed_rows(before, after) == [(0, 0, 0), (1, 2, 4)]


def _brute_attention(q, K, V, pos, window):
    lo = max(0, pos + 1 - window) if window > 0 else 0
    s = np.array([float(q @ K[t]) / np.sqrt(len(q)) for t in range(lo, pos + 1)])
    p = np.exp(s - s.max())
    return (p[:, None] * V[lo:pos + 1]).sum(0) / p.sum()


@pytest.mark.parametrize("window,norm", [(0, False), (3, False), (0, True), (4, True)])
def test_decode_attention_f64_against_a_loop(window, norm):
    rng = np.random.default_rng(3)
    heads, kv, HD, pos = 4, 2, 8, 6
    inv = 1.0 / 10000.0 ** (np.arange(0, HD, 2) / HD)
    ang = np.arange(pos + 3)[:, None] * inv[None, :]
    cos, sin = np.cos(ang), np.sin(ang)
    qkv = rng.standard_normal((heads + 2 * kv) * HD).astype(F32)
    K, V = rng.standard_normal((pos + 1, kv, HD)), rng.standard_normal((pos + 1, kv, HD))
    q_w, k_w = (1 + 0.3 * rng.standard_normal(HD), 1 + 0.3 * rng.standard_normal(HD)) if norm else (None, None)
    out, kr, kerr, v = S.decode_attention_f64(qkv, K, V, pos, heads, kv, HD, cos, sin, window, q_w, k_w, 1e-6)
    x = qkv.astype(np.float64).reshape(heads + 2 * kv, HD)
    for h in range(heads):
        q = x[h]
        if norm:
            q = q / np.sqrt((q * q).mean() + 1e-6) * q_w
        a, b = q[:HD // 2], q[HD // 2:]
        qr = np.concatenate([a * cos[pos] - b * sin[pos], b * cos[pos] + a * sin[pos]])
        want = _brute_attention(qr, K[:, h // 2], V[:, h // 2], pos, window)
        assert np.abs(out[h] - want).max() <= 1e-12
    k0 = x[heads]
    if norm:
        k0 = k0 / np.sqrt((k0 * k0).mean() + 1e-6) * k_w
    a, b = k0[:HD // 2], k0[HD // 2:]
    assert np.abs(kr[0] - np.concatenate([a * cos[pos] - b * sin[pos], b * cos[pos] + a * sin[pos]])).max() <= 1e-12
    assert np.array_equal(v, x[heads + kv:]) and (kerr >= 0).all() and kerr.max() <= 4 * 2.0 ** -24 * np.abs(k0).max() * 2


def _info(group, asym, sname, wname="int4_clip"):
    st = S.STYPE[sname]
    pack = (lambda q, s, z, gi: orc.repack(q, s, z, None if gi is None else orc.convert_idx(gi, q.shape[0], group), group,
                                           scale_type=st)) if wname == "int4_clip" else \
        (lambda q, s, z, gi: orc.repack_table(q, s, S.TABLES[wname], group, scale_type=st))
    return dict(cpu_pack=pack, group=group, asym=asym, scale_dtype=sname, weight_dtype=wname, compute_dtype="fp32")


@pytest.mark.parametrize("group,asym,sname", [(32, True, "fp32"), (128, False, "fp16"), (-1, False, "bf16")])
def test_weight_view_dequantises_to_the_oracles_matrix(group, asym, sname):
    rng = np.random.default_rng(1)
    w = (0.05 * rng.standard_normal((256, 48))).astype(F32)
    q, s, z = orc.rtn_quantize(w, False, group, asym)
    wv = S.weight_view((q, s, z, None), _info(group, asym, sname))
    assert wv["W64"].shape == (256, 48) and wv["K"] == 256 and wv["N"] == 48 and wv["shuffle"] is None
    assert wv["smode"] == (1 if group == 32 else 0) and (wv["zp_kn"] is not None) == asym
    assert np.array_equal(wv["W64"], orc.dequantize_blob(wv["blob"]).astype(np.float64))
    # (the view's own check — codes, stored scales and zero points give W64 — ran inside weight_view)
    gi = rng.permutation(np.arange(256, dtype=np.int32) // 64).astype(np.int32)
    wa = S.weight_view((q[:, :16], orc.rtn_quantize(w[:, :16], False, 64, False)[1], None, gi), _info(64, False, "fp16"))
    assert wa["shuffle"] is not None and sorted(wa["shuffle"].tolist()) == list(range(256))


def test_weight_view_of_a_table_type():
    rng = np.random.default_rng(2)
    q, s = orc.rtn_quantize_table((0.05 * rng.standard_normal((256, 32))).astype(F32), False, 128, orc.W_NF4)
    wv = S.weight_view((q, s, None, None), _info(128, False, "fp16", "nf4"))
    assert wv["ndig"] == 3 and wv["table"] is not None and wv["zp_kn"] is None


def _xq_case(epi):
    rng = np.random.default_rng(4)
    K, cols = 256, 64
    q, s, z = orc.rtn_quantize((0.05 * rng.standard_normal((K, cols))).astype(F32), False, 32, True)
    wv = S.weight_view((q, s, z, None), _info(32, True, "fp32"))
    x = rng.standard_normal(K).astype(F32)
    g = (1 + 0.1 * rng.standard_normal(K)).astype(F32)
    res = None if epi == 1 else rng.standard_normal(cols).astype(F32)
    launches = X.geometry(K, epi, wv["smode"], 0)

    def kernel(gw):  # what the kernel returns when the norm weight `gw` rides in: the fp32 restatement
        return X.gemv_f32((x * gw).astype(F32), wv["codes"], wv["scales_kn"], wv["zp_kn"], launches, wv["smode"],
                          X.inv_f32(x, 1e-5), None, res, epi, None)

    return wv, x, g, res, kernel


@pytest.mark.parametrize("epi", [0, 1])
def test_xq_gemv_ratio_holds_the_kernel_and_catches_a_slip_of_1e_4(epi):
    wv, x, g, res, kernel = _xq_case(epi)
    assert S.xq_gemv_ratio(wv, x, kernel(g), g, 1e-5, None, res, epi) <= 0.25 + 1e-9  # A is this restatement's own error
    slipped = kernel((g * F32(1 + 1e-4)).astype(F32))  # the norm weight off by 1e-4 relative
    assert S.xq_gemv_ratio(wv, x, slipped, g, 1e-5, None, res, epi) > 1
    other = np.roll(g, 1)  # another layer's norm weight
    assert S.xq_gemv_ratio(wv, x, kernel(other), g, 1e-5, None, res, epi) > 1


def test_decode_attention_ratio_holds_float64_and_catches_a_slip():
    rng = np.random.default_rng(5)
    heads, kv, HD, pos = 4, 2, 64, 9
    inv = 1.0 / 10000.0 ** (np.arange(0, HD, 2) / HD)
    ang = np.arange(pos + 1)[:, None] * inv[None, :]
    cos, sin = np.cos(ang).astype(F32).astype(np.float64), np.sin(ang).astype(F32).astype(np.float64)
    qkv = rng.standard_normal((heads + 2 * kv) * HD).astype(F32)
    K, V = R.round_to(rng.standard_normal((pos + 1, kv, HD)), "fp16"), R.round_to(rng.standard_normal((pos + 1, kv, HD)), "fp16")
    x = qkv.astype(np.float64).reshape(heads + 2 * kv, HD)
    K[pos] = R.round_to(R.rotate(x[heads:heads + kv], cos[pos], sin[pos]), "fp16")
    V[pos] = R.round_to(x[heads + kv:], "fp16")
    out = S.decode_attention_f64(qkv, K, V, pos, heads, kv, HD, cos, sin)[0].astype(F32)
    ratio, rows = S.decode_attention_ratio(qkv, K, V, out, pos, heads, kv, HD, cos, sin, "fp16")
    assert ratio <= 1e-2 and rows
    assert S.decode_attention_ratio(qkv, K, V, out * F32(1 + 1e-3), pos, heads, kv, HD, cos, sin, "fp16")[0] > 1
    K2 = K.copy()
    K2[pos, 0, 0] += 2 * 2.0 ** -10 * max(1.0, abs(K2[pos, 0, 0]))  # two units of storage off: no rounding tie explains it
    assert not S.decode_attention_ratio(qkv, K2, V, out, pos, heads, kv, HD, cos, sin, "fp16")[1]
    assert not S.decode_attention_ratio(qkv, K, V, out, pos, heads, kv, HD, cos, sin, "fp16", window=0,
                                        q_w=np.full(HD, 1.5), k_w=np.full(HD, 1.5), eps=1e-6)[1]  # rows of another norm
    # with a q / k norm: the rounded float64 row is accepted, one unit of storage beside it too, two units are not
    from tests import qknorm_reference as QN

    q_w, k_w = 1 + 0.3 * rng.standard_normal(HD), 1 + 0.3 * rng.standard_normal(HD)
    K3 = K.copy()
    K3[pos] = R.round_to(QN.normed_rotated(x[heads:heads + kv], k_w, 1e-6, cos[pos], sin[pos]), "fp16")
    args = (pos, heads, kv, HD, cos, sin, "fp16", 0, q_w, k_w, 1e-6)
    assert S.decode_attention_ratio(qkv, K3, V, out, *args)[1]
    for units, ok in ((1, True), (2, False)):
        K4 = K3.copy()
        K4[pos, 1, 3] += units * QN.ulp(K3[pos, 1, 3], "fp16")
        assert S.decode_attention_ratio(qkv, K4, V, out, *args)[1] == ok


def test_gemm_and_lm_head_ratios():
    import torch

    rng = np.random.default_rng(6)
    q, s, z = orc.rtn_quantize((0.05 * rng.standard_normal((256, 32))).astype(F32), False, 128, False)
    wv = S.weight_view((q, s, z, None), _info(128, False, "fp16"))
    x = rng.standard_normal((5, 256)).astype(F32)
    g = (1 + 0.1 * rng.standard_normal(256)).astype(F32)
    inv = 1.0 / np.sqrt((x.astype(np.float64) ** 2).mean(1, keepdims=True) + 1e-5)
    exact = ((x.astype(np.float64) * g) @ wv["W64"]) * inv
    assert S.gemm_ratio(wv, x, exact.astype(np.float16), g, 1e-5, out_kind="fp16") <= 1
    assert S.gemm_ratio(wv, x, (exact * 1.02).astype(np.float16), g, 1e-5, out_kind="fp16") > 1
    W = torch.from_numpy((0.1 * rng.standard_normal((48, 256))).astype(np.float16))
    ref = X.lm_head_f64(x[0], g, 1e-5, W)
    assert S.lm_head_ratio(x[0], g, 1e-5, W, X.lm_head_f32(x[0], g, 1e-5, W)) <= 0.25 + 1e-9
    assert S.lm_head_ratio(x[0], g, 1e-5, W, (ref * (1 + 1e-4)).astype(F32)) > 1


def test_stored_ok():
    lo, hi = np.array([1.0, 2.0]), np.array([1.0, 2.5])
    assert S.stored_ok(np.array([1.0, 2.5]), lo, hi) and S.stored_ok(np.array([1.0, 2.0]), lo, hi)
    assert not S.stored_ok(np.array([1.5, 2.0]), lo, hi)
