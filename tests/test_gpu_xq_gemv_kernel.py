"""The XQ decode GEMV alone (csrc/woq_gemv_xqs.h, launched from csrc/woq_gemv_xq.hip) and the fp32 -> XQ conversion,
through `woq_probe_gemv_xq` / `woq_probe_xq_from_f32`, against tests/xq_reference.py (float64).

Inputs, seed 0: weights RTN-quantised by the oracle from 0.05 * N(0, 1), x ~ N(0, 1) with one element times 30, norm
weights 1 + 0.1 N(0, 1). N is 16 .. 64: K alone selects the launch geometry, and every case asserts first that its K
still selects the form it names (`xq_reference.geometry` restates `xq_geometry` / `xq_k_plan`). The device blob must
equal the oracle's repack byte for byte before anything is multiplied; W_deq is the oracle's dequantise of that repack.

Per case (tolerance terms A, B from the reference alone, printed): |out - R0| <= 4 (A + B), |out - R1| <= 4 A; an XQ output
equals `encode(fl32(out * next_norm_w))` of the kernel's own `out` bit for bit, its sums of squares lie within
8 * 2^-24 relative of the float64 block sums of out^2; without `out`, decode(xo) lies within 4 (A + B) + 2^(e_b - 22) of
R0 * next_norm_w. Memory behind every output keeps its sentinel.
"""
import functools

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from oracle import woq_oracle as orc
from tests import xq_reference as X
from tests.test_xq_reference_cpu import special_inputs

pytestmark = pytest.mark.gpu

EPS = 1e-5
STYPE = {"fp32": orc.F32, "fp16": orc.F16, "bf16": orc.BF16}
G128, G32A = (128, False, "fp16"), (32, True, "fp32")  # the second selects SMODE 1, ASYM and S32
TABLES = {"nf4": orc.W_NF4, "fp4_e2m1": orc.W_FP4_E2M1, "fp4_e2m1_bnb": orc.W_FP4_E2M1_BNB}
SENT = 777.0


def _form_id(form):
    return "g%d-%s-%s" % (form[0], "asym" if form[1] else "sym", form[2])


def _stored(s, sname):
    """fp32 scales rounded to their stored type"""
    if sname == "fp16":
        return s.astype(np.float16).astype(np.float32)
    return orc.bf16_round(s) if sname == "bf16" else s


@functools.lru_cache(maxsize=None)
def _weight(K, N, form, wname="int4_clip", cname="fp32", epi=0):
    """-> dict(blob uint8, W64 [K, Ncols], codes, scales_kn, zp_kn, smode, ndig, table); epi 1: N = inter, the blob
    holds gate and up interleaved by runtime.fuse_gate_up (2 N columns)"""
    from intel_extension_for_transformers_amd.runtime import fuse_gate_up

    group, asym, sname = form
    rng = np.random.default_rng(0)
    parts = []
    for _ in range(2 if epi == 1 else 1):
        w = (0.05 * rng.standard_normal((N, K))).astype(np.float32)
        if wname == "int4_clip":
            parts.append(orc.rtn_quantize(w, True, group, asym))
        else:
            parts.append(orc.rtn_quantize_table(w, True, group, TABLES[wname]) + (None,))
    if epi == 1:
        fuse = lambda a, b: fuse_gate_up(torch.from_numpy(a), torch.from_numpy(b)).numpy()  # noqa: E731
        q, s = fuse(parts[0][0], parts[1][0]), fuse(parts[0][1], parts[1][1])
        z = fuse(parts[0][2], parts[1][2]) if asym else None
    else:
        q, s, z = parts[0]
    ct = L.COMPUTE_TYPES[cname]
    if wname == "int4_clip":
        blob = orc.repack(q, s, z, None, group, scale_type=STYPE[sname], compute_type=ct)
        table, ndig = None, 0
    else:
        blob = orc.repack_table(q, s, TABLES[wname], group, scale_type=STYPE[sname], compute_type=ct)
        ndig = 1 if wname == "fp4_e2m1" else (3 if (wname == "nf4" and cname == "fp32") else 2)
        table = X.table_planes(TABLES[wname], ndig)
    h = orc.header(blob)
    g = K if group in (-1, 0) or group > K else group
    rep = lambda a: np.repeat(a, g, axis=0)[:K]  # noqa: E731
    scales_kn = rep(_stored(s, sname))
    zp_kn = rep(z).astype(np.int64) if z is not None else None
    W = orc.dequantize_blob(blob)
    # the restatement's view of the blob (codes, stored scales, zero points) dequantises to the oracle's matrix
    if table is None:
        mine = ((q.astype(np.int64) - (0 if zp_kn is None else zp_kn)) * scales_kn.astype(np.float64)).astype(np.float32)
    else:
        mine = (orc.LUTS[TABLES[wname]][q] * scales_kn).astype(np.float32)
    assert np.array_equal(mine, W)
    return dict(blob=blob, W64=W.astype(np.float64), codes=q.astype(np.int64), scales_kn=scales_kn, zp_kn=zp_kn,
                smode=h["scale_mode"], ndig=ndig, table=table, q=q, s=s, z=z, wname=wname, sname=sname, cname=cname,
                group=group, asym=asym, K=K, epi=epi)


_DEV_BLOBS = {}


def _dev_blob(wt):
    """the device repack of the same (q, scale, zp): equal to the oracle's blob byte for byte"""
    from intel_extension_for_transformers_amd import qbits

    key = id(wt["blob"])
    if key not in _DEV_BLOBS:
        e8, e32 = torch.empty(0, dtype=torch.int8), torch.empty(0, dtype=torch.int32)
        blob = qbits.repack_quantized_weight(torch.from_numpy(wt["q"]).cuda(), torch.from_numpy(wt["s"]).cuda(),
                                             e8 if wt["z"] is None else torch.from_numpy(wt["z"]).cuda(), e32, wt["wname"],
                                             wt["sname"], wt["cname"], wt["asym"], wt["group"])
        assert np.array_equal(blob.cpu().numpy().view(np.uint8), wt["blob"]), "device repack != oracle repack"
        _DEV_BLOBS[key] = blob
    return _DEV_BLOBS[key]


@functools.lru_cache(maxsize=None)
def _vectors(K, n):
    """x [K] with one element times 30, the input norm weight [K]; bias, residual, next norm weight [n]"""
    rng = np.random.Generator(np.random.PCG64(0).jumped())  # seed 0, a stream apart from the weights' (else x = 20 w[0])
    x = rng.standard_normal(K).astype(np.float32)
    x[K // 3] *= 30
    nw = lambda m: (1 + 0.1 * rng.standard_normal(m)).astype(np.float32)  # noqa: E731
    return x, nw(K), rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32), nw(n)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _xo_buffers(n):
    nb = n // 16
    return (torch.full((L.xq_limb_bytes(n),), 0x5A, dtype=torch.uint8, device="cuda"),
            torch.full((nb + 4,), SENT, device="cuda"), torch.full((nb + 4,), SENT, device="cuda"))


def _check_xo(xo, n, y32, what):
    """the XQ vector equals encode(y32) bit for bit; nothing behind it was written"""
    nb = n // 16
    limbs, u, sx = (t.cpu().numpy() for t in xo)
    want = X.encode(y32)
    assert np.array_equal(limbs[:nb * 48].view(np.int8).reshape(nb, 3, 16), want[0]), what
    assert np.array_equal(u[:nb], want[1]) and np.array_equal(sx[:nb], want[2]), what
    assert (limbs[nb * 48:] == 0x5A).all() and (u[nb:] == SENT).all() and (sx[nb:] == SENT).all(), what


def _check_ssq(got, x32, what):
    """blocks whose sum of squares fp32 cannot hold as a normal number (1e30^2, 1e-35^2) have no specified value"""
    want = X.block_ssq(x32)
    held = (want == 0) | ((want > 2.0 ** -100) & (want < 2.0 ** 100))
    assert (np.abs(got.astype(np.float64) - want)[held] <= X.SSQ_REL * want[held]).all(), what


RECORD = []  # (case, A, B, tolerance, worst error): printed per case; a job script may collect it


def _run(wt, geom, in_norm=False, bias=False, residual=False, xo=False, next_norm=False, ssq=False, out=True, N=None,
         what=""):
    K, epi = wt["K"], wt["epi"]
    cols = wt["W64"].shape[1]
    n_out = cols // 2 if epi == 1 else cols
    N = n_out if N is None else N  # ragged N: the blob's own N
    launches = X.geometry(K, epi, wt["smode"], wt["ndig"])
    got_geom = [(c, nw, tpw) for _, c, nw, tpw, _ in launches]
    assert got_geom == geom, (what, got_geom)
    x, g_in, b_, r_, g_next = _vectors(K, 64)
    g = g_in if in_norm else None
    bvec = b_[:cols] if bias else None
    rvec = r_[:n_out] if residual else None
    gn = g_next[:n_out] if next_norm else None
    restate = lambda y32, inv32: X.gemv_f32(y32, wt["codes"], wt["scales_kn"], wt["zp_kn"], launches, wt["smode"],  # noqa: E731
                                            inv32, bvec, rvec, epi, wt["table"])
    r0, r1, a, b = X.tolerance_terms(x, g, EPS, wt["W64"], restate, bvec, rvec, epi)
    tol = 4 * (a + b)
    assert 0 < tol < 1e-2 * max(1.0, float(np.abs(r0).max())), (what, a, b)
    blob = _dev_blob(wt)
    npad = (n_out + 15) // 16 * 16
    d_out = torch.full((npad + 16,), SENT, device="cuda") if out else None
    d_xo = _xo_buffers(n_out) if xo else None
    d_ssq = torch.full((n_out // 16 + 4,), SENT, device="cuda") if ssq else None
    L.probe_gemv_xq(_dev(x), blob, epi, _dev(g), EPS, _dev(bvec), _dev(rvec), _dev(gn), d_out, d_xo, d_ssq)
    torch.cuda.synchronize()
    worst = 0.0
    if out:
        o = d_out.cpu().numpy()
        assert (o[N:] == SENT).all(), what + ": written past N"
        o = o[:N]
        worst = float(np.abs(o - r0[:N]).max())
        worst1 = float(np.abs(o - r1[:N]).max())
        print("%s: A = %.3e, B = %.3e, tolerance = %.3e, max |out - R0| = %.3e (ratio %.3f), max |out - R1| = %.3e "
              "(of 4 A: %.3f)" % (what, a, b, tol, worst, worst / tol, worst1, worst1 / (4 * a)))
        RECORD.append((what, a, b, tol, worst))
        assert worst <= tol and worst1 <= 4 * a, what
        if xo:
            y32 = o if gn is None else (o * gn).astype(np.float32)
            _check_xo(d_xo, n_out, y32, what)
        if ssq:
            s = d_ssq.cpu().numpy()
            assert (s[n_out // 16:] == SENT).all(), what
            _check_ssq(s[:n_out // 16], o, what)
    else:
        nb = n_out // 16
        limbs, u, _ = (t.cpu().numpy() for t in d_xo)
        dec = X.decode(limbs[:nb * 48].view(np.int8).reshape(nb, 3, 16), u[:nb])
        want = r0 if gn is None else r0 * gn.astype(np.float64)
        half_unit = np.repeat(u[:nb].astype(np.float64) * 8.0, 16)  # 2^(e_b - 22) = u * 2^3
        err = np.abs(dec - want)
        worst = float(err.max())
        print("%s: A = %.3e, B = %.3e, tolerance = %.3e, max |decode(xo) - R0| = %.3e" % (what, a, b, tol, worst))
        RECORD.append((what, a, b, tol, worst))
        assert (err <= tol + half_unit).all(), what
        assert (limbs[nb * 48:] == 0x5A).all(), what
    return d_out


# ---- conversion ------------------------------------------------------------------------------------------------------
def _convert(x, g, extra=""):
    K = x.size
    xo = _xo_buffers(K)
    ssq = torch.full((K // 16 + 4,), SENT, device="cuda")
    L.probe_xq_from_f32(_dev(x), _dev(g), *xo, ssq)
    torch.cuda.synchronize()
    what = "xq_from_f32 K %d%s%s" % (K, " norm" if g is not None else "", extra)
    _check_xo(xo, K, x if g is None else (x * g).astype(np.float32), what)
    s = ssq.cpu().numpy()
    assert (s[K // 16:] == SENT).all(), what
    _check_ssq(s[:K // 16], x, what)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("K", [128, 640, 4096])
def test_conversion_matches_encode_bit_for_bit(K, norm):
    x, g, *_ = _vectors(K, 64)
    _convert(x, g if norm else None)


@pytest.mark.parametrize("norm", [False, True])
def test_conversion_of_the_format_edges(norm):
    """powers of two, just below them, 1e-6 beside 1e3, the exponent clamp at both ends, a zero block, ties"""
    y = special_inputs()
    g = (1 + 0.1 * np.random.default_rng(0).standard_normal(y.size)).astype(np.float32)
    g[-64:] = 1  # the clamped-range, zero and tie blocks keep their values (1e30 * 1.2 would leave the specified range)
    _convert(y, g if norm else None, " (format edges)")
    # without ssq_out nothing is written there
    xo = _xo_buffers(y.size)
    L.probe_xq_from_f32(_dev(y), None, *xo, None)
    torch.cuda.synchronize()
    _check_xo(xo, y.size, y, "xq_from_f32 without ssq_out")


# ---- geometry sweep --------------------------------------------------------------------------------------------------
SWEEP = {  # K: [(tiles, waves, tiles per wave) of each chained launch]
    128: [(1, 1, 4)], 640: [(5, 2, 4)], 2048: [(16, 4, 4)], 2176: [(17, 3, 8)], 4096: [(32, 4, 8)],
    11008: [(86, 11, 8)], 16384: [(128, 16, 8)], 16512: [(65, 9, 8), (64, 8, 8)], 28672: [(112, 14, 8), (112, 14, 8)],
}


@pytest.mark.parametrize("form", [G128, G32A], ids=_form_id)
@pytest.mark.parametrize("K", sorted(SWEEP))
def test_geometry_sweep(K, form):
    _run(_weight(K, 32, form), SWEEP[K], what="sweep K %d %s" % (K, _form_id(form)))


def test_sweep_slices_are_the_named_ones():
    """uneven wave slices and windows shorter / longer than a slice, as the sweep's table names them"""
    per_wave = lambda K: [w for *_, w in X.geometry(K)]  # noqa: E731
    assert per_wave(128) == [[1]] and per_wave(640) == [[3, 2]] and per_wave(2176) == [[6, 6, 5]]
    assert per_wave(4096) == [[8] * 4] and per_wave(11008) == [[8] * 9 + [7] * 2]
    assert per_wave(16512) == [[8] * 2 + [7] * 7, [8] * 8]


# ---- quantisation forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [(-1, False, "bf16"), (64, True, "bf16"), (256, False, "fp16"), (512, False, "fp32"),
                                  (128, True, "fp16")], ids=_form_id)
@pytest.mark.parametrize("K", [1024, 4096])
def test_quantisation_forms(K, form):
    """one group, per-64 groups with zero points, tpg_shift 1 and 2, and per-128 groups with zero points (the zero-point
    term of the per-group form, which neither sweep form reaches)"""
    wt = _weight(K, 32, form)
    assert wt["smode"] == (1 if form[0] == 64 else 0)
    _run(wt, [(K // 128, 2 if K == 1024 else 4, 4 if K == 1024 else 8)], what="forms K %d %s" % (K, _form_id(form)))


# ---- table types -----------------------------------------------------------------------------------------------------
TABLE_CASES = [("nf4", "fp32", 3), ("nf4", "bf16", 2), ("fp4_e2m1", "fp32", 1), ("fp4_e2m1_bnb", "fp32", 2)]


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("group", [128, 32])
@pytest.mark.parametrize("K", [640, 4096])
@pytest.mark.parametrize("wname,cname,ndig", TABLE_CASES)
def test_table_types(wname, cname, ndig, K, group, epi):
    wt = _weight(K, 32, (group, False, "fp16"), wname, cname, epi)
    assert wt["ndig"] == ndig
    tiles = K // 128
    geom = [(tiles, (tiles + 3) // 4, 4)] if (epi == 1 or tiles <= 16) else [(tiles, tiles // 8, 8)]
    _run(wt, geom, what="table %s/%s K %d g%d epi %d" % (wname, cname, K, group, epi))


def test_table_wide_form():
    """nf4 at compute fp32, gate/up, 33 tiles: the 512-thread launch with 8 tiles per wave"""
    _run(_weight(4224, 32, (128, False, "fp16"), "nf4", "fp32", 1), [(33, 5, 8)], what="table nf4/fp32 K 4224 wide")


# ---- gate/up ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [G128, G32A], ids=_form_id)
@pytest.mark.parametrize("K,waves", [(128, 1), (640, 2), (4096, 8), (8192, 16)])
def test_gate_up(K, waves, form):
    """inter 32; with an fp32 out, with the XQ output alone (the engine's call), and with the input norm and a bias"""
    wt = _weight(K, 32, form, epi=1)
    geom, what = [(K // 128, waves, 4)], "gate/up K %d %s" % (K, _form_id(form))
    _run(wt, geom, what=what + " out")
    _run(wt, geom, out=False, xo=True, ssq=False, what=what + " xo only")
    _run(wt, geom, in_norm=True, bias=True, xo=True, what=what + " norm + bias")


def test_gate_up_beyond_one_launch_is_refused():
    wt = _weight(8320, 32, G128, epi=1)
    out = torch.full((48,), SENT, device="cuda")
    with pytest.raises(RuntimeError, match="QBits: shape not covered by the XQ GEMV"):
        L.probe_gemv_xq(_dev(_vectors(8320, 64)[0]), _dev_blob(wt), 1, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()


# ---- epilogues -------------------------------------------------------------------------------------------------------
EPILOGUES = {
    "norm": dict(in_norm=True), "bias": dict(bias=True), "residual": dict(residual=True),
    "o/down form": dict(residual=True, next_norm=True, xo=True, ssq=True),
    "all": dict(in_norm=True, bias=True, residual=True, next_norm=True, xo=True, ssq=True),
}


@pytest.mark.parametrize("name", list(EPILOGUES))
@pytest.mark.parametrize("form", [G128, G32A], ids=_form_id)
@pytest.mark.parametrize("K", [640, 4096, 16512])
def test_epilogues(K, form, name):
    wt = _weight(K, 32, form)
    kw = dict(EPILOGUES[name])
    what = "epilogue %s K %d %s" % (name, K, _form_id(form))
    if K == 16512 and kw.get("in_norm"):
        # a K range split over chained launches takes no norm: refused with the library's error, nothing written
        out, xo = torch.full((48,), SENT, device="cuda"), _xo_buffers(32)
        x, g, b_, r_, gn = _vectors(K, 64)
        with pytest.raises(RuntimeError, match="QBits: (RMSNorm partials beyond K = 16384|a K range split over chained launches)"):
            L.probe_gemv_xq(_dev(x), _dev_blob(wt), 0, _dev(g), EPS, _dev(b_[:32]), _dev(r_[:32]), _dev(gn[:32]), out, xo)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == SENT).all() and (xo[0].cpu().numpy() == 0x5A).all()
        assert (xo[1].cpu().numpy() == SENT).all() and (xo[2].cpu().numpy() == SENT).all()
        if name == "norm":
            return
        kw["in_norm"] = False  # everything else together: the residual once, the XQ output from the last chunk only
    _run(wt, SWEEP[K], what=what, **kw)


# ---- ragged N --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [G128, G32A], ids=_form_id)
@pytest.mark.parametrize("N", [40, 17])
def test_ragged_n(N, form):
    """N no multiple of the 16-column tile: elements [N, Npad) of `out` stay untouched"""
    wt = _weight(640, N, form)
    assert orc.header(wt["blob"])["Npad"] == (N + 15) // 16 * 16
    _run(wt, SWEEP[640], bias=True, N=N, what="ragged N %d %s" % (N, _form_id(form)))
