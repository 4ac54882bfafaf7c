"""No-GPU checks of tests/quant_reference.py (the float64 definition of the RTN quantisers) and of the CPU oracle's
quantisers against it, on the input families and shapes the GPU test (tests/test_gpu_quantize_kernel.py) uses.

Reference alone: the rule's own dequantisation error is at most half a step for the integer types, the chosen table /
fp8 entry is the nearest one, the planted tie cells have scale exactly 1, and with 16-bit scale storage every scale
of the families is a normal fp16 — the conditions under which the bounds of `quant_reference.bounds` can be met.

Oracle against the reference: `orc.rtn_quantize` (C), `orc.rtn_quantize_bits`, `orc.rtn_quantize_table` and
`orc.rtn_quantize_fp8`, through the oracle's repack and dequantise, are held to the same bounds as the device. With
the asym scale taken over (max - min) instead of the range widened to hold zero, the one-sided and constant families
fail here: int4 asym reads U[1, 1.1] back as about 0.1 (150 steps off), int8 asym 2550 steps off.
"""
import numpy as np
import pytest

from oracle import woq_oracle as orc
from tests import quant_reference as Q

STYPE = {"fp32": orc.F32, "fp16": orc.F16, "bf16": orc.BF16}
TABLE_IDS = {"nf4": orc.W_NF4, "fp4_e2m1": orc.W_FP4_E2M1, "fp4_e2m1_bnb": orc.W_FP4_E2M1_BNB}
FP8_IDS = {"fp8_e4m3": orc.W_FP8_E4M3, "fp8_e5m2": orc.W_FP8_E5M2}

# (weight type, scale type, asym): every type with fp32 scales, fp8 with fp8_e8m0 too; 16-bit storage on three of them
TYPES = [(w, "fp32", a) for w in ("int4_clip", "int8", "int3_clip", "int2_clip") for a in (False, True)]
TYPES += [(w, "fp32", False) for w in ("nf4", "fp4_e2m1", "fp4_e2m1_bnb")]
TYPES += [(w, s, False) for w in ("fp8_e4m3", "fp8_e5m2") for s in ("fp32", "fp8_e8m0")]
TYPES += [(w, s, a) for s in ("fp16", "bf16") for w, a in (("int4_clip", False), ("int4_clip", True), ("int8", False),
                                                          ("int8", True), ("fp8_e4m3", False))]


def type_id(t):
    return "%s-%s-%s" % (t[0], t[1], "asym" if t[2] else "sym")


def stored(s, sname):
    """fp32 scales as their storage type keeps them"""
    s = np.asarray(s, np.float32)
    if sname == "fp16":
        return s.astype(np.float16).astype(np.float32)
    return orc.bf16_round(s) if sname == "bf16" else s


def oracle_quantize(w, transpose, group, wname, sname, asym):
    """the oracle's quantiser for this type on w ([N, K] when transpose) -> (blob, scales fp32 [G, N], zp or None)"""
    st = STYPE.get(sname, orc.F32)
    if wname == "int4_clip":
        q, s, z = orc.rtn_quantize(w, transpose, group, asym)
        return orc.repack(q, s, z, None, group, scale_type=st), s, z
    if wname == "int8":
        q, s, z = orc.rtn_quantize_int8(w, transpose, group, asym)
        return orc.repack_int8(q, s, z, None, group, scale_type=st), s, z
    if wname in orc.NARROW_BITS:
        bits = orc.NARROW_BITS[wname]
        q, s, z = orc.rtn_quantize_bits(w, transpose, group, asym, bits)
        return orc.repack_narrow(q, s, z, None, group, scale_type=st, bits=bits), s, z
    if wname in TABLE_IDS:
        q, s = orc.rtn_quantize_table(w, transpose, group, TABLE_IDS[wname])
        return orc.repack_table(q, s, TABLE_IDS[wname], group, scale_type=st), s, None
    e8 = sname == "fp8_e8m0"
    q, s = orc.rtn_quantize_fp8(w, transpose, group, FP8_IDS[wname], e8, scale_type=st)
    return orc.repack_fp8(q, s, FP8_IDS[wname], None, group, scale_type=st, e8m0=e8), s, None


def case_input(K, N, group, wname, sname, asym):
    return Q.families(K, N, group, wname, asym, scale16=sname in ("fp16", "bf16"))


@pytest.mark.parametrize("typ", TYPES, ids=type_id)
def test_reference_alone(typ):
    wname, sname, asym = typ
    for K, N, group in Q.SHAPES:
        w, fam, e = case_input(K, N, group, wname, sname, asym)
        g, G = Q.group_of(K, group)
        assert set(fam.ravel()) == set(range(len(Q.FAMILIES)))  # every family appears in every matrix
        ref = Q.quantize(w, group, wname, asym, sname == "fp8_e8m0")
        sk = np.repeat(ref["s"], g, axis=0)[:K]
        w64 = w.astype(np.float64)
        if wname in Q.INT_BITS:
            # 2^-40: the float64 quotient and product of the reference's own arithmetic
            assert (np.abs(ref["deq"] - w64) <= 0.5 * sk * (1 + 2.0 ** -40)).all()
        else:
            tab, tmax = Q.grid(wname)
            fin = tab[~np.isnan(tab)]
            d = np.abs((w64 / sk)[..., None] - fin)
            assert np.array_equal(np.abs(w64 / sk - tab[ref["code"]]), d.min(-1))
            assert (np.abs(w64 / sk) <= tmax * (1 + 2.0 ** -50)).all()  # nothing leaves the grid's range
        ties = np.array([Q.FAMILIES[f] == "ties" for f in fam.ravel()]).reshape(fam.shape)
        if wname in Q.INT_BITS or wname in ("fp4_e2m1", "fp8_e4m3", "fp8_e5m2"):
            assert (ref["s"][ties] == 1.0).all()
            v = (w64 / sk)[np.repeat(ties, g, axis=0)[:K]]
            if wname in Q.INT_BITS:
                assert (np.abs(v - np.rint(v)) == 0.5).mean() > 0.9  # the planted range ends are the rest
        if sname in ("fp16", "bf16"):  # every stored scale a normal fp16, below its largest: 2^-14 <= s <= 65504
            assert ref["s"].min() >= 2.0 ** -14 and ref["s"].max() <= 65504.0
        if sname == "fp8_e8m0":
            assert (np.frexp(ref["s"])[0] == 0.5).all() and (ref["s"] >= ref["r"]).all()
            assert (ref["s"][ref["r"] > 0] < 2 * ref["r"][ref["r"] > 0]).all()


@pytest.mark.parametrize("transpose", [False, True], ids=["kn", "nk"])
@pytest.mark.parametrize("typ", TYPES, ids=type_id)
def test_oracle_against_reference(typ, transpose):
    wname, sname, asym = typ
    worst = {}
    for K, N, group in Q.SHAPES:
        w, fam, e = case_input(K, N, group, wname, sname, asym)
        wt = np.ascontiguousarray(w.T) if transpose else w
        blob, s, z = oracle_quantize(wt, transpose, group, wname, sname, asym)
        W = orc.dequantize_blob(blob)
        assert np.array_equal(orc.dequantize_blob(blob, transpose=True), W.T)
        off = 2 ** (Q.INT_BITS[wname] - 1) if asym else 0
        rep = Q.check(w, group, wname, sname, asym, stored(s, sname), None if z is None else z.astype(np.int64) + off,
                      W, fam)
        for k, v in rep.items():
            worst[k] = max(worst.get(k, 0), v)
    print("\n%s %s: largest err / bound %s" % (type_id(typ), "nk" if transpose else "kn", worst))


def test_c_and_numpy_oracle_agree_on_the_families():
    """the two 4-bit restatements, bit for bit, on every family (the existing check uses N(0, 0.05) only)"""
    for asym in (False, True):
        for K, N, group in Q.SHAPES:
            w, fam, e = Q.families(K, N, group, "int4_clip", asym)
            a, b = orc.rtn_quantize(w, False, group, asym), orc.rtn_quantize_bits(w, False, group, asym, 4)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert (not asym) or np.array_equal(a[2], b[2])
