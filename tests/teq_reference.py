"""TEQ's quantiser (Cheng et al. 2023, "TEQ: Trainable Equivalent Transformation for Quantization of LLMs") and the
gradient of its trainable scale, stated in float64: what `qbits.teq_forward / teq_grad` (csrc/woq_teq.hip) have to
compute. numpy, independent of the package; `autograd_gradients` is the same statement in torch float64, which is the
definition the closed form is held to (tests/test_teq_reference_cpu.py).

w [K, N] in working order, a [K] positive; one group = `group` consecutive k of one column (the last may be short;
group -1 = one per column); L = 2^bits - 1, qmax = 2^(bits-1) - 1, off = 2^(bits-1), rne = round half to even:

  u  = w[k,n] a[k]
  sym   s = max|u| / qmax (0 -> 1);  t = u / s;  c = clip(rne(t), -off, qmax);  deq = c s
  asym  hi = max(max u, 0), lo = min(min u, 0), s = (hi - lo) / L (0 -> 1), zf = -lo / s, z = clip(rne(zf), 0, L)
        t = u / s;  c = clip(rne(t) + z, 0, L);  q = c - z;  deq = q s
  W~ = deq / a[k]

a = 1 is the RTN rule of tests/quant_reference.py.

Gradient of sum(g W~) with respect to a, rne straight-through, clip passing inside its range (bounds included),
max / min passing to the one row that attains them, a group whose s was replaced by 1 giving nothing through s;
ga = g / a[k], un = "the code was not clipped":

  direct[k,n] = g (un ? w / a[k] : 0) - g deq / a[k]^2
  sym   DS = sum_k ga (un ? c - t : c);   E = DS sign(u*) w[k*,n] / qmax on row k* = argmax |u| of the group
  asym  DS = sum_k ga (un ? q - t : q + zf),  DLO = sum_k (un ? 0 : ga),  dhi = DS / L,  dlo = DLO - DS / L
        Ehi = dhi w[kmax,n] on row kmax where max u > 0;   Elo = dlo w[kmin,n] on row kmin where min u < 0
  da[k] = sum_n direct[k,n] + the E terms that land on row k
"""
import numpy as np

from tests import quant_reference as Q


def group_of(K, group):
    g = K if group <= 0 or group > K else group
    return g, (K + g - 1) // g


def consts(bits):
    return 2 ** bits - 1, 2 ** (bits - 1) - 1, 2 ** (bits - 1)  # L, qmax, off


def _groups(K, group):
    g = group_of(K, group)[0]
    return [slice(k0, min(K, k0 + g)) for k0 in range(0, K, g)]


def forward(w, a, group, bits, asym, dtype=np.float64):
    """-> dict: u, t, deq, W [K, N]; c, q [K, N] int64 (sym: q = c); un [K, N] = code not clipped; s, dead [G, N];
    z [G, N] int64 and zf [G, N] (asym, else zeros); rows [G, N] x 3 = kmax, kmin, kabs (absolute row indices: the first
    row that attains max u, min u, max |u|); mx, mn [G, N] = max u, min u"""
    w, a = np.asarray(w, dtype), np.asarray(a, dtype)
    K, N = w.shape
    L, qmax, off = consts(bits)
    u = w * a[:, None]
    G = group_of(K, group)[1]
    out = {name: np.zeros((K, N), dtype) for name in ("t", "deq")}
    out.update({name: np.zeros((K, N), np.int64) for name in ("c", "q")})
    out.update({name: np.zeros((G, N), dtype) for name in ("s", "zf", "mx", "mn")})
    out.update({name: np.zeros((G, N), np.int64) for name in ("z", "kmax", "kmin", "kabs")})
    out.update(u=u, un=np.zeros((K, N), bool), dead=np.zeros((G, N), bool))
    for gi, r in enumerate(_groups(K, group)):
        x = u[r]
        out["kmax"][gi], out["kmin"][gi] = x.argmax(0) + r.start, x.argmin(0) + r.start
        out["kabs"][gi] = np.abs(x).argmax(0) + r.start
        out["mx"][gi], out["mn"][gi] = x.max(0), x.min(0)
        if asym:
            hi, lo = np.maximum(x.max(0), dtype(0)), np.minimum(x.min(0), dtype(0))
            s = (hi - lo) / dtype(L)
        else:
            s = np.abs(x).max(0) / dtype(qmax)
        dead = s == 0
        s = np.where(dead, dtype(1), s)
        t = x / s
        if asym:
            zf = -lo / s
            z = np.clip(np.rint(zf), 0, L)
            rz = np.rint(t) + z
            c = np.clip(rz, 0, L)
            un = (rz >= 0) & (rz <= L)
            q = c - z
            out["zf"][gi], out["z"][gi] = zf, z.astype(np.int64)
        else:
            rz = np.rint(t)
            c = np.clip(rz, -off, qmax)
            un = (rz >= -off) & (rz <= qmax)
            q = c
        out["s"][gi], out["dead"][gi] = s, dead
        out["t"][r], out["c"][r], out["q"][r], out["un"][r] = t, c.astype(np.int64), q.astype(np.int64), un
        out["deq"][r] = q * s
    out["W"] = out["deq"] / a[:, None]
    return out


def gradients(w, a, g, group, bits, asym, fwd=None, scatter=True, dtype=np.float64):
    """The closed form -> (da [K], mag [K]): mag = the per-row sum of the absolute values of the terms da adds up, the
    products before any subtraction cancels: |g| |w / a| and |g| |deq / a^2| for direct, |ga| (|q| + |t|) (|q| + |zf|
    where clipped) inside DS and |ga| inside DLO, carried through E's factors. scatter=False leaves the E terms out (of
    da only). dtype=np.float32 restates it in fp32 with sequential sums (mag stays float64)."""
    f = fwd if fwd is not None and dtype == np.float64 else forward(w, a, group, bits, asym, dtype)
    w, a, g = np.asarray(w, dtype), np.asarray(a, dtype), np.asarray(g, dtype)
    K, N = w.shape
    L, qmax, _ = consts(bits)
    cols = np.arange(N)

    def total(x, axis):
        if dtype == np.float64:
            return x.sum(axis)
        return np.cumsum(x, axis=axis, dtype=dtype).take(-1, axis=axis)  # one rounding per addition, in order

    da, mag = np.zeros(K, dtype), np.zeros(K)
    for gi, r in enumerate(_groups(K, group)):
        aa, gg, ww = a[r, None], g[r], w[r]
        t, un, deq, q = f["t"][r], f["un"][r], f["deq"][r], f["q"][r].astype(dtype)
        dead = f["dead"][gi]
        ga = gg / aa
        direct = gg * np.where(un, ww / aa, dtype(0)) - gg * (deq / (aa * aa))
        m = (np.abs(gg) * (np.where(un, np.abs(ww / aa), 0) + np.abs(deq / (aa * aa)))).astype(np.float64)
        contrib = direct.copy()
        if asym:
            zf = f["zf"][gi]
            DS = total(ga * np.where(un, q - t, q + zf), 0)
            DLO = total(np.where(un, dtype(0), ga), 0)
            DSm = (np.abs(ga) * (np.abs(q) + np.where(un, np.abs(t), np.abs(zf)))).sum(0).astype(np.float64)
            DLOm = np.where(un, 0, np.abs(ga)).sum(0).astype(np.float64)
            dhi, dlo = DS / dtype(L), DLO - DS / dtype(L)
            for rows, live, e, em in ((f["kmax"][gi] - r.start, (f["mx"][gi] > 0) & ~dead, dhi, DSm / L),
                                      (f["kmin"][gi] - r.start, (f["mn"][gi] < 0) & ~dead, dlo, DLOm + DSm / L)):
                wk = ww[rows, cols]
                if scatter:
                    contrib[rows, cols] += np.where(live, e * wk, dtype(0))
                m[rows, cols] += np.where(live, em * np.abs(wk), 0)
        else:
            DS = total(ga * np.where(un, q - t, q), 0)
            DSm = (np.abs(ga) * (np.abs(q) + np.where(un, np.abs(t), 0))).sum(0).astype(np.float64)
            rows = f["kabs"][gi] - r.start
            wk = ww[rows, cols]
            sign = np.sign(f["u"][r][rows, cols])
            if scatter:
                contrib[rows, cols] += np.where(dead, dtype(0), DS * sign * wk / dtype(qmax))
            m[rows, cols] += np.where(dead, 0, DSm * np.abs(wk) / qmax)
        da[r], mag[r] = total(contrib, 1), m.sum(1)
    return da, mag


def autograd_gradients(w, a, g, group, bits, asym):
    """-> (da [K], W~ [K, N]) from torch autograd in float64: rne(x) written x + (round(x) - x).detach(), clip as
    torch.clamp, the range through amax / amin"""
    import torch

    D = torch.float64
    w, g = torch.tensor(np.asarray(w, np.float64), dtype=D), torch.tensor(np.asarray(g, np.float64), dtype=D)
    a = torch.tensor(np.asarray(a, np.float64), dtype=D, requires_grad=True)
    K = w.shape[0]
    L, qmax, off = consts(bits)

    def ste(x):
        return x + (torch.round(x) - x).detach()

    u = w * a[:, None]
    out = []
    for r in _groups(K, group):
        x = u[r]
        if asym:
            hi, lo = torch.clamp(x.amax(0), min=0), torch.clamp(x.amin(0), max=0)
            s = (hi - lo) / L
            s = torch.where(s == 0, torch.ones_like(s), s)
            z = torch.clamp(ste(-lo / s), 0, L)
            out.append((torch.clamp(ste(x / s) + z, 0, L) - z) * s)
        else:
            s = x.abs().amax(0) / qmax
            s = torch.where(s == 0, torch.ones_like(s), s)
            out.append(torch.clamp(ste(x / s), -off, qmax) * s)
    W = torch.cat(out) / a[:, None]
    (W * g).sum().backward()
    return a.grad.numpy(), W.detach().numpy()


# ---- inputs -------------------------------------------------------------------------------------------------------
def _near_half(x, width):
    return np.abs(np.abs(x - np.floor(x)) - 0.5) <= width


def ambiguous(w, a, group, bits, asym):
    """how many places of (w, a) fp32 and float64 arithmetic could disagree about: a t or a zf within
    FP32_SLOP * max(1, |.|) of a half-integer (the clip bounds' half-steps are such places), or a second row within
    FP32_SLOP (relative) of a group's max / min / max-magnitude"""
    f = forward(w, a, group, bits, asym)
    K = f["u"].shape[0]
    bad = int(_near_half(f["t"], Q.FP32_SLOP * np.maximum(1.0, np.abs(f["t"]))).sum())
    if asym:
        bad += int(_near_half(f["zf"], Q.FP32_SLOP * np.maximum(1.0, np.abs(f["zf"]))).sum())
    for r in _groups(K, group):
        x = f["u"][r]
        if x.shape[0] < 2:
            continue
        for v in ((x, -x) if asym else (np.abs(x),)):
            top = np.sort(v, axis=0)[-2:]  # the two largest
            bad += int(((top[1] - top[0] <= Q.FP32_SLOP * np.abs(top[1])) & (top[1] > 0)).sum())
    return bad


def inputs(K, N, group, bits, asym, seed=0):
    """-> (w, a, g), fp32 arrays: w [K, N] = N(0,1) with the first group of column 0 all zero (the s -> 1 cell), a [K]
    lognormal(0, 0.5), g = N(0,1); redrawn as a whole until `ambiguous` finds nothing."""
    g0 = group_of(K, group)[0]
    for attempt in range(1000):
        rng = np.random.default_rng([seed, attempt])
        w = rng.standard_normal((K, N)).astype(np.float32)
        w[:g0, 0] = 0.0
        a = rng.lognormal(0.0, 0.5, K).astype(np.float32)
        gout = rng.standard_normal((K, N)).astype(np.float32)
        if not ambiguous(w, a, group, bits, asym):
            return w, a, gout
    raise AssertionError("no unambiguous draw")
