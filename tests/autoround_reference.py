"""AutoRound's quantiser (Cheng et al. 2023, "Optimize Weight Rounding via Signed Gradient Descent"), stated in float64:
what `qbits.autoround_forward / autoround_step / autoround_codes` (csrc/woq_autoround.hip) have to compute. Pure numpy,
independent of the package.

One group = `group` consecutive k of one column of w [K, N] (the last may be short; group -1 = one per column), with
mn = min(min v, 0), mx = max(max v, 0); V [K, N] in [-0.5, 0.5], alpha / beta [G, N] in [0, 1];
L = 2^bits - 1, qmax = 2^(bits-1) - 1, off = 2^(bits-1), rne = round half to even:

  asym  lo = alpha mn, hi = beta mx, s = (hi - lo) / L (0 -> 1), z = clip(rne(-lo / s), 0, L)
        t = w / s + V, c = clip(rne(t) + z, 0, L), W~ = (c - z) s
  sym   amax = beta mx >= alpha (-mn) ? beta mx : alpha (-mn), s = amax / qmax (0 -> 1)
        t = w / s + V, c = clip(rne(t), -off, qmax), W~ = c s

V = 0, alpha = beta = 1 is the RTN rule of tests/quant_reference.py.

Gradients = autograd's of these expressions with rne(x) written (rne(x) - x).detach() + x and clip passing gradient
inside its range (bounds included, as torch.clamp); g = dL/dW~, q = c - z (asym) or c (sym):
  code not clipped   dV = g s,  ds += g (q - w / s)
  code clipped       dV = 0,    asym: ds += g (q - lo / s), dlo += g;   sym: ds += g c
  asym   dhi = ds / L, dlo -= ds / L, dalpha = dlo mn, dbeta = dhi mx
  sym    damax = ds / qmax, dbeta = damax mx where beta mx >= alpha (-mn), else dalpha = damax (-mn)
  a group whose s was replaced by 1 gives alpha and beta no gradient
(tests/test_autoround_reference_cpu.py holds them to torch.autograd.)

SignSGD: p <- clip(p - lr_t sign(grad)), sign(0) = 0, lr_t = lr (1 - t / iters).
"""
import numpy as np

WINDOW = 2.0 ** -20  # times L: how near a half-integer (in steps) counts as ambiguous between fp32 and float64


def group_of(K, group):
    g = K if group <= 0 or group > K else group
    return g, (K + g - 1) // g


def consts(bits):
    return 2 ** bits - 1, 2 ** (bits - 1) - 1, 2 ** (bits - 1)  # L, qmax, off


def _expand(a, K, g):
    return np.repeat(a, g, axis=0)[:K]


def forward(w, V, alpha, beta, group, bits, asym):
    """-> dict: mn, mx, s, replaced [G, N]; z [G, N] (asym, else zeros); zt = -lo / s (asym); lo [G, N]; beta_side
    [G, N] (sym: the side the maximum takes); t [K, N]; c [K, N] int64; q = c - z; clipped [K, N]; deq [K, N]"""
    w, V = np.asarray(w, np.float64), np.asarray(V, np.float64)
    alpha, beta = np.asarray(alpha, np.float64), np.asarray(beta, np.float64)
    K, N = w.shape
    g, G = group_of(K, group)
    L, qmax, off = consts(bits)
    mn, mx = np.empty((G, N)), np.empty((G, N))
    for gi in range(G):
        v = w[gi * g:min(K, (gi + 1) * g)]
        mn[gi], mx[gi] = np.minimum(v.min(0), 0.0), np.maximum(v.max(0), 0.0)
    out = dict(mn=mn, mx=mx)
    if asym:
        lo, hi = alpha * mn, beta * mx
        s = (hi - lo) / L
        side = np.zeros((G, N), bool)
    else:
        a, b = beta * mx, alpha * (-mn)
        side = a >= b
        s = np.where(side, a, b) / qmax
        lo = np.zeros((G, N))
    replaced = s == 0
    s = np.where(replaced, 1.0, s)
    if asym:
        zt = -lo / s
        z = np.clip(np.rint(zt), 0, L).astype(np.int64)
        cmin, cmax = 0, L
    else:
        zt = np.zeros((G, N))
        z = np.zeros((G, N), np.int64)
        cmin, cmax = -off, qmax
    sk, zk = _expand(s, K, g), _expand(z, K, g)
    t = w / sk + V
    rz = np.rint(t) + zk
    c = np.clip(rz, cmin, cmax).astype(np.int64)
    out.update(s=s, replaced=replaced, z=z, zt=zt, lo=lo, beta_side=side, t=t, c=c, q=c - zk,
               clipped=(rz < cmin) | (rz > cmax), deq=(c - zk) * sk)
    return out


def gradients(w, V, alpha, beta, gout, group, bits, asym, fwd=None):
    """-> dict: dV [K, N]; dalpha, dbeta [G, N]; sum_a, sum_b [G, N] = the sum of the absolute values of the terms each
    of them adds up (for an error bound); rows [G] = rows of each group; step_mask [K, N] = code not clipped"""
    f = fwd or forward(w, V, alpha, beta, group, bits, asym)
    w, gout = np.asarray(w, np.float64), np.asarray(gout, np.float64)
    K, N = w.shape
    g, G = group_of(K, group)
    L, qmax, _ = consts(bits)
    sk = _expand(f["s"], K, g)
    keep = ~f["clipped"]
    dV = np.where(keep, gout * sk, 0.0)
    if asym:
        los = _expand(f["lo"] / f["s"], K, g)
        term = gout * np.where(keep, f["q"] - w / sk, f["q"] - los)
    else:
        term = gout * np.where(keep, f["q"] - w / sk, f["q"].astype(np.float64))
    gclip = np.where(keep, 0.0, gout)
    ds, dabs, dlo, dloabs = (np.zeros((G, N)) for _ in range(4))
    rows = np.zeros(G, np.int64)
    for gi in range(G):
        r = slice(gi * g, min(K, (gi + 1) * g))
        rows[gi] = r.stop - r.start
        ds[gi], dabs[gi] = term[r].sum(0), np.abs(term[r]).sum(0)
        dlo[gi], dloabs[gi] = gclip[r].sum(0), np.abs(gclip[r]).sum(0)
    live = ~f["replaced"]
    mn, mx = f["mn"], f["mx"]
    if asym:
        dhi = ds / L
        dalpha, dbeta = (dlo - dhi) * mn, dhi * mx
        sum_a, sum_b = (dloabs + dabs / L) * np.abs(mn), dabs / L * np.abs(mx)
    else:
        dm, side = ds / qmax, f["beta_side"]
        dalpha, dbeta = np.where(side, 0.0, dm * (-mn)), np.where(side, dm * mx, 0.0)
        sum_a, sum_b = np.where(side, 0.0, dabs / qmax * np.abs(mn)), np.where(side, dabs / qmax * np.abs(mx), 0.0)
    z = np.zeros((G, N))
    return dict(dV=dV, dalpha=np.where(live, dalpha, z), dbeta=np.where(live, dbeta, z), sum_a=np.where(live, sum_a, z),
                sum_b=np.where(live, sum_b, z), rows=rows, step_mask=keep)


def sign_step(p, grad, lr, lo, hi):
    """p <- clip(p - lr sign(grad), lo, hi), sign(0) = 0"""
    return np.clip(np.asarray(p, np.float64) - lr * np.sign(grad), lo, hi)


def schedule(lr, t, iters):
    """the learning rate of iteration t of `iters`: linear decay to zero"""
    return lr * (1.0 - t / iters)


def default_lrs(lr, minmax_lr, iters):
    """(lr, minmax_lr) as the config defaults them: lr = 1 / iters, minmax_lr = lr"""
    lr = (1.0 / iters if iters else 0.0) if lr is None else lr
    return lr, (lr if minmax_lr is None else minmax_lr)


# ---- inputs -------------------------------------------------------------------------------------------------------
def _near_half(x, width):
    return np.abs(np.abs(x - np.floor(x)) - 0.5) <= width


def _side_tie(w, alpha, beta, group, bits):
    f = forward(w, np.zeros_like(w), alpha, beta, group, bits, False)
    a, b = beta * f["mx"], alpha * (-f["mn"])
    return (np.abs(a - b) <= WINDOW * np.maximum(np.abs(a), np.abs(b))) & ((a != 0) | (b != 0))


def inputs(K, N, group, bits, asym, seed=0):
    """-> (w, V, alpha, beta, g), fp32 arrays: w [K, N] = 0.05 N(0,1) with cell (0, 0) all zero, cell (0, 1) all
    positive and cell (G - 1, 2) all negative; V uniform in [-0.5, 0.5], a tenth of the elements at exactly +0.5 and a
    tenth at exactly -0.5; alpha / beta [G, N] uniform in [0.5, 1], a fifth at exactly 1; g = N(0,1).

    Then made unambiguous between fp32 and float64 arithmetic: every element whose float64 t lies within L * 2^-20 of
    a half-integer has its V moved by 0.01 towards 0 (repeated until none is left); sym: every group with
    |beta mx - alpha (-mn)| within 2^-20 relative of a tie gets beta = 1, alpha = 0.5; asym: every group whose zero
    point -lo / s lies within L * 2^-20 of a half-integer gets the same (the zero point enters every code of the
    group). Asserts that nothing ambiguous remains."""
    rng = np.random.default_rng(seed)
    g, G = group_of(K, group)
    L = consts(bits)[0]
    w = (0.05 * rng.standard_normal((K, N))).astype(np.float32)
    w[:g, 0] = 0.0
    w[:g, 1] = np.abs(w[:g, 1]) + np.float32(1e-3)
    w[(G - 1) * g:, 2] = -np.abs(w[(G - 1) * g:, 2]) - np.float32(1e-3)
    V = rng.uniform(-0.5, 0.5, (K, N)).astype(np.float32)
    pick = rng.random((K, N))
    V[pick < 0.1] = 0.5
    V[(pick >= 0.1) & (pick < 0.2)] = -0.5
    alpha = rng.uniform(0.5, 1.0, (G, N)).astype(np.float32)
    beta = rng.uniform(0.5, 1.0, (G, N)).astype(np.float32)
    alpha[rng.random((G, N)) < 0.2] = 1.0
    beta[rng.random((G, N)) < 0.2] = 1.0
    gout = rng.standard_normal((K, N)).astype(np.float32)

    if asym:
        bad = _near_half(forward(w, V, alpha, beta, group, bits, True)["zt"], L * WINDOW)
    else:
        bad = _side_tie(w, alpha, beta, group, bits)
    alpha[bad], beta[bad] = 0.5, 1.0
    for _ in range(100):
        near = _near_half(forward(w, V, alpha, beta, group, bits, asym)["t"], L * WINDOW)
        if not near.any():
            break
        V[near] = (V[near] - np.float32(0.01) * np.where(V[near] > 0, 1, -1)).astype(np.float32)

    f = forward(w, V, alpha, beta, group, bits, asym)
    assert not _near_half(f["t"], L * WINDOW).any()
    assert np.abs(V).max() <= 0.5
    if asym:
        assert not _near_half(f["zt"], L * WINDOW).any()
    else:
        assert not _side_tie(w, alpha, beta, group, bits).any()
    return w, V, alpha, beta, gout
