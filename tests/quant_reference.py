"""The round-to-nearest (RTN) weight quantisers, stated in float64: what `qbits.quantize_to_packed_weight`
(csrc/woq_pack.hip rtn_kernel / rtn_lut_kernel / rtn_fp8_kernel) has to compute. Pure numpy, independent of oracle/:
the tables are copied from include/woq_blob.h, the fp8 grids are built from the OCP definition.

One group of values v (a run of `group` consecutive k of one output column; the last group may be shorter):

  integer types, bits in {2, 3, 4, 8}: qmax = 2^(bits-1) - 1, levels = 2^bits - 1, off = 2^(bits-1)
    sym   s = max|v| / qmax;                          code = clip(rne(v / s), -off, qmax);      W' = code * s
    asym  lo = min(min v, 0), hi = max(max v, 0): s = (hi - lo) / levels, z = clip(rne(-lo / s), 0, levels);
          code = clip(rne(v / s) + z, 0, levels);                                                W' = (code - z) * s
    an all-zero group has s = 1; rne = round half to even
  table types (nf4, fp4_e2m1, fp4_e2m1_bnb): s = max|v| / table_max (all zero: 1), code = the entry nearest to v / s,
    lowest code on a tie;                                                                        W' = table[code] * s
  fp8 (e4m3fn, e5m2): s = max|v| / fp8_max (all zero: 1), with e8m0 scales the smallest power of two at or above
    that; code = the finite code nearest to v / s, lowest code on a tie;                         W' = value(code) * s

`families` builds the test inputs, `bounds` / `check` hold an implementation's (scales, zero points, dequantised
weight) to this definition; nothing in them is taken from an implementation's output.
"""
import numpy as np

INT_BITS = {"int4_clip": 4, "int8": 8, "int3_clip": 3, "int2_clip": 2}

# include/woq_blob.h WOQ_LUT_NF4 / WOQ_LUT_FP4_E2M1 / WOQ_LUT_FP4_BNB (fp32 constants there: rounded to fp32 here too)
_NF4 = [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
        -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
        0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0]
_E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
_f = np.float32
_BNB = [_f(0), _f(0.0625) / _f(12), _f(8) / _f(12), _f(1), _f(4) / _f(12), _f(0.5), _f(2) / _f(12), _f(0.25),
        -_f(0), -_f(0.0625) / _f(12), -_f(8) / _f(12), -_f(1), -_f(4) / _f(12), -_f(0.5), -_f(2) / _f(12), -_f(0.25)]
TABLES = {"nf4": np.array(_NF4, np.float32).astype(np.float64), "fp4_e2m1": np.array(_E2M1, np.float64),
          "fp4_e2m1_bnb": np.array(_BNB, np.float32).astype(np.float64)}
TABLE_MAX = {"nf4": 1.0, "fp4_e2m1": 6.0, "fp4_e2m1_bnb": 1.0}


def _fp8_grid(wname):
    """value of every code byte; NaN / inf codes as NaN (never produced). OCP 8-bit floating point: e4m3fn has no
    infinities and S.1111.111 = NaN, bias 7; e5m2 is IEEE-like, exponent 31 = inf / NaN, bias 15."""
    t = np.full(256, np.nan)
    for c in range(256):
        if wname == "fp8_e4m3":
            e, m = (c >> 3) & 15, c & 7
            if e == 15 and m == 7:
                continue
            v = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        else:
            e, m = (c >> 2) & 31, c & 3
            if e == 31:
                continue
            v = m * 2.0 ** -16 if e == 0 else (1 + m / 4) * 2.0 ** (e - 15)
        t[c] = -v if c & 0x80 else v
    return t


FP8 = {"fp8_e4m3": _fp8_grid("fp8_e4m3"), "fp8_e5m2": _fp8_grid("fp8_e5m2")}
FP8_MAX = {"fp8_e4m3": 448.0, "fp8_e5m2": 57344.0}

# relative rounding error of the stored scale; fp8_e8m0 scales are powers of two, exact in their bf16 storage
U = {"fp32": 0.0, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8, "fp8_e8m0": 0.0}
FP32_SLOP = 2.0 ** -22  # two fp32 roundings (the range's subtraction and the division), 2^-24 each, with room


def kind(wname):
    return "int" if wname in INT_BITS else ("table" if wname in TABLES else "fp8")


def grid(wname):
    """the values a table / fp8 code can take (NaN where the code is never produced) and the largest magnitude"""
    return (TABLES[wname], TABLE_MAX[wname]) if wname in TABLES else (FP8[wname], FP8_MAX[wname])


def group_of(K, group):
    g = K if group <= 0 or group > K else group
    return g, (K + g - 1) // g


def _nearest(x, tab):
    """lowest code among the entries nearest to x"""
    d = np.abs(x[..., None] - tab)
    d[..., np.isnan(tab)] = np.inf
    return d.argmin(-1)  # argmin returns the first minimum


def quantize(w, group, wname, asym=False, e8m0=False):
    """w [K, N] (fp32 values, taken as float64) -> dict: s [G, N]; z [G, N] (asym integers) or None; code [K, N];
    deq [K, N] = W' in float64; zt [G, N] = -lo / s before rounding (asym); r [G, N] = max|v| / fp8_max (fp8)"""
    w = np.asarray(w, np.float64)
    K, N = w.shape
    g, G = group_of(K, group)
    out = dict(s=np.empty((G, N)), z=None, code=np.empty((K, N), np.int64), deq=np.empty((K, N)), zt=None, r=None)
    k = kind(wname)
    if k == "int":
        bits = INT_BITS[wname]
        qmax, levels, off = 2 ** (bits - 1) - 1, 2 ** bits - 1, 2 ** (bits - 1)
        if asym:
            out["z"], out["zt"] = np.empty((G, N), np.int64), np.empty((G, N))
    elif k == "fp8":
        out["r"] = np.empty((G, N))
    for gi in range(G):
        rows = slice(gi * g, min(K, (gi + 1) * g))
        v = w[rows]
        amax = np.abs(v).max(0)
        if k == "int" and asym:
            lo, hi = np.minimum(v.min(0), 0.0), np.maximum(v.max(0), 0.0)
            s = (hi - lo) / levels
            s[s == 0] = 1.0
            zt = -lo / s
            z = np.clip(np.rint(zt), 0, levels).astype(np.int64)
            code = np.clip(np.rint(v / s).astype(np.int64) + z, 0, levels)
            out["z"][gi], out["zt"][gi], out["deq"][rows] = z, zt, (code - z) * s
        elif k == "int":
            s = amax / qmax
            s[s == 0] = 1.0
            code = np.clip(np.rint(v / s).astype(np.int64), -off, qmax)
            out["deq"][rows] = code * s
        else:
            tab, tmax = grid(wname)
            s = amax / tmax
            if k == "fp8":
                out["r"][gi] = s
                if e8m0:
                    f, e = np.frexp(s)  # s = f 2^e, f in [0.5, 1): 2^(e-1) if s is that power of two, else 2^e
                    s = np.where(s == 0, 0.0, np.ldexp(1.0, np.where(f == 0.5, e - 1, e)))
            s[s == 0] = 1.0
            code = _nearest(v / s, tab)
            out["deq"][rows] = tab[code] * s
        out["s"][gi], out["code"][rows] = s, code
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------
FAMILIES = ["gauss", "pos", "neg", "touch0", "const0.3", "const-2.5", "zero", "onehot", "pmzero", "ties",
            "mag", "mag", "mag", "mag", "mag", "mag"]  # one slot per (group, column) cell, cycled in cell order
SHAPES = [(128, 24, 32), (160, 24, 64), (96, 17, 128), (512, 20, -1)]  # K, N, group: tail group of 32 rows; ragged N
# with group > K (per channel); one group of 512 rows


def tie_values(wname, asym, m, cell):
    """m values that sit exactly on rounding ties once divided by the scale the planted range gives (exactly 1):
    integer types k + 0.5 over the whole code range, sym planted +-qmax, asym planted lo = -5 (-1 where the type has
    fewer than 6 levels) and hi = levels + lo; fp4_e2m1 and fp8 the midpoints between neighbouring entries under a
    planted +-max. nf4 / fp4_e2m1_bnb midpoints are not fp32 numbers: theirs are the fp32 nearest to each midpoint
    under a planted +-1, near ties that fall under the slop rule."""
    sign = -1.0 if cell & 1 else 1.0
    if wname in INT_BITS:
        bits = INT_BITS[wname]
        qmax, levels = 2 ** (bits - 1) - 1, 2 ** bits - 1
        if asym:
            lo = -5 if levels > 5 else -1
            vals = np.arange(lo, lo + levels) + 0.5
            plant = [float(lo), float(lo + levels)]
        else:
            vals = np.arange(-qmax, qmax) + 0.5
            plant = [sign * qmax]
    else:
        tab, tmax = grid(wname)
        pos = np.unique(np.abs(tab[~np.isnan(tab)]))
        mid = (pos[:-1] + pos[1:]) / 2
        vals = np.concatenate([mid, -mid])
        plant = [sign * tmax]
    v = np.resize(np.roll(vals, -3 * cell), m)
    v[:len(plant)] = plant
    return v.astype(np.float32)


def families(K, N, group, wname, asym=False, scale16=False, seed=0):
    """-> (w fp32 [K, N], fam [G, N] indices into FAMILIES, e [G, N] the exponent of a magnitude cell else 0).
    Cell (g, n) = rows of group g in column n holds FAMILIES[(g N + n) % 16]:
      gauss 0.05 N(0,1) | pos U[1, 1.1] | neg -U[0.2, 0.9] | touch0 U[0, 1) with one exact 0 | const0.3 | const-2.5 |
      zero | onehot: zeros and one +-0.7 | pmzero: +0 and -0 alternating | ties: tie_values |
      mag: N(0,1) 2^e with one planted +-3 2^e, e stepping through -20 .. 20 (4 .. 8 with 16-bit scale storage, which
      keeps every stored scale a normal fp16) over the matrix's magnitude cells."""
    rng = np.random.default_rng(seed)
    g, G = group_of(K, group)
    w = np.zeros((K, N), np.float32)
    fam = (np.arange(G * N).reshape(G, N)) % len(FAMILIES)
    e = np.zeros((G, N), np.int64)
    nmag = sum(FAMILIES[f] == "mag" for f in fam.ravel())
    emin, emax = (4, 8) if scale16 else (-20, 20)
    imag = 0
    for gi in range(G):
        k0, k1 = gi * g, min(K, (gi + 1) * g)
        m = k1 - k0
        for n in range(N):
            cell, name = gi * N + n, FAMILIES[fam[gi, n]]
            if name == "gauss":
                v = 0.05 * rng.standard_normal(m)
            elif name == "pos":
                v = rng.uniform(1.0, 1.1, m)
            elif name == "neg":
                v = -rng.uniform(0.2, 0.9, m)
            elif name == "touch0":
                v = rng.random(m)
                v[rng.integers(m)] = 0.0
            elif name == "const0.3":
                v = np.full(m, 0.3)
            elif name == "const-2.5":
                v = np.full(m, -2.5)
            elif name == "zero":
                v = np.zeros(m)
            elif name == "onehot":
                v = np.zeros(m)
                v[rng.integers(m)] = -0.7 if cell & 1 else 0.7
            elif name == "pmzero":
                v = np.where(np.arange(m) & 1, -0.0, 0.0)
            elif name == "ties":
                v = tie_values(wname, asym, m, cell)
            else:
                e[gi, n] = emin + round(imag * (emax - emin) / max(1, nmag - 1))
                imag += 1
                v = rng.standard_normal(m) * 2.0 ** e[gi, n]
                v[rng.integers(m)] = (3.0 if rng.random() < 0.5 else -3.0) * 2.0 ** e[gi, n]
            w[k0:k1, n] = v
    return w, fam, e


# ---- bounds ---------------------------------------------------------------------------------------------------------
def bounds(wname, sname):
    """tolerances, each as a multiple of the quantity it is relative to:
      scale  |s_dev - s_ref| <= scale * s_ref: FP32_SLOP for the fp32 arithmetic plus the storage rounding u
      elem   integer types: |W' - w| <= elem * s_dev = (0.5 + levels (FP32_SLOP + u)) s_dev: half a step, the fp32
             quotient's error at a tie and the stored scale's rounding, both times the largest code
      ztie   the zero point may be either neighbour where -lo / s lies within ztie = levels FP32_SLOP of a tie
      near   table / fp8: no finite entry is nearer to w / s_dev than the chosen one by more than near = FP32_SLOP
             max|table|
      e8m0   either neighbouring power of two where max|v| / fp8_max is within e8m0 = 2^-23 relative of one"""
    u = U[sname]
    b = dict(u=u, scale=FP32_SLOP + u)
    if wname in INT_BITS:
        levels = 2 ** INT_BITS[wname] - 1
        b.update(levels=levels, elem=0.5 + levels * (FP32_SLOP + u), ztie=levels * FP32_SLOP)
    else:
        b.update(near=FP32_SLOP * grid(wname)[1], e8m0=2.0 ** -23)
    return b


def _expand(a, K, g):
    return np.repeat(a, g, axis=0)[:K]


def check(w, group, wname, sname, asym, s_dev, z_dev, W_dev, fam=None):
    """Hold (s_dev [G, N] as stored, z_dev [G, N] in 0 .. levels or None, W_dev [K, N]) to the definition on input w.
    Raises AssertionError naming the first failing property; returns the largest err / bound of each."""
    w = np.asarray(w, np.float64)
    K, N = w.shape
    g, G = group_of(K, group)
    e8 = sname == "fp8_e8m0"
    ref = quantize(w, group, wname, asym, e8)
    b = bounds(wname, sname)
    s_dev, W_dev = np.asarray(s_dev, np.float64), np.asarray(W_dev, np.float64)
    assert s_dev.shape == (G, N) and W_dev.shape == (K, N)
    assert np.isfinite(s_dev).all() and np.isfinite(W_dev).all()
    rep = {}
    amax0 = np.stack([np.abs(w[gi * g:(gi + 1) * g]).max(0) == 0 for gi in range(G)])
    assert (s_dev[amax0] == 1.0).all(), "an all-zero group has scale 1"
    if e8:
        r, p = ref["r"], ref["s"]
        ok = s_dev == p
        ok |= (s_dev == p / 2) & (r <= (p / 2) * (1 + b["e8m0"]))
        ok |= (s_dev == 2 * p) & (r >= p * (1 - b["e8m0"]))
        assert ok.all(), "e8m0 scale is not the power of two demanded: %s" % (np.argwhere(~ok)[:4],)
        rep["scale"] = 0.0
    else:
        err = np.abs(s_dev - ref["s"]) / (b["scale"] * ref["s"])
        assert (err <= 1).all(), "scale off by %.3g of its bound at %s" % (err.max(), np.argwhere(err > 1)[:4])
        rep["scale"] = float(err.max())
    sk = _expand(s_dev, K, g)
    if wname in INT_BITS:
        err = np.abs(W_dev - w) / (b["elem"] * sk)
        assert (err <= 1).all(), "element off by %.4g of its bound (%.4g steps) at %s" % (
            err.max(), (np.abs(W_dev - w) / sk).max(), np.argwhere(err > 1)[:4])
        rep["elem"] = float(err.max())
        if asym:
            assert z_dev is not None
            z_dev = np.asarray(z_dev, np.int64)
            assert z_dev.min() >= 0 and z_dev.max() <= b["levels"]
            dz = np.abs(z_dev - ref["z"])
            near_tie = np.abs(np.abs(ref["zt"] - np.floor(ref["zt"])) - 0.5) <= b["ztie"]
            bad = (dz > 1) | ((dz == 1) & ~near_tie)
            assert not bad.any(), "zero point differs at %s" % (np.argwhere(bad)[:4],)
            rep["zp_moved"] = int((dz == 1).sum())
    else:
        tab, tmax = grid(wname)
        fin = tab[~np.isnan(tab)]
        x = W_dev / sk
        t = fin[np.abs(x[..., None] - fin).argmin(-1)]
        # W' = fl32(table[code] * s_dev): one fp32 product, 2^-24 relative (2^-23 allowed)
        assert (np.abs(x - t) <= 2.0 ** -23 * np.abs(t)).all(), "W' / s_dev is not a table value"
        y = w / sk
        excess = np.abs(y - t) - np.abs(y[..., None] - fin).min(-1)
        err = excess / b["near"]
        assert (err <= 1).all(), "a nearer entry exists: %.4g of the slop (%.4g of max|table|) at %s" % (
            err.max(), excess.max() / tmax, np.argwhere(err > 1)[:4])
        rep["near"] = float(err.max())
    if fam is not None:  # exact ties: the documented rule, exactly (the planted range makes the scale exactly 1)
        exact = wname in INT_BITS or wname in ("fp4_e2m1", "fp8_e4m3", "fp8_e5m2")
        cells = np.array([FAMILIES[f] == "ties" for f in fam.ravel()]).reshape(fam.shape)
        if exact and cells.any():
            assert (s_dev[cells] == 1.0).all(), "a tie cell's scale is exactly 1"
            mk = _expand(cells, K, g)
            assert np.array_equal(W_dev[mk], ref["deq"][mk]), "ties: half to even (integers) / lowest code (tables)"
            rep["ties"] = int(mk.sum())
    return rep
