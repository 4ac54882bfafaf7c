"""GPTQ (Frantar et al. 2022; AutoGPTQ's `fasterquant`) stated in numpy float64, independent of the package: what
`qbits.gptq_sweep` (csrc/woq_gptq.hip) and `quantization/gptq.py gptq_quantize_weight` have to compute. The parameter
and code rule is `quant_reference`'s integer rule (bits in {2, 3, 4, 8}, sym or asym).

Working layout: w [K, N], row k = input feature k (Linear.weight.T); u [K, K] upper triangular with H^-1 = U^T U.
One block c0 <= j < c0 + B, every column on its own, j ascending:

    gid = col_group[j] if given else j // group
    at a group start (j % group == 0, parameters not given): (s, z) = the rule's parameters of the CURRENT
        w[j : min(j + group, K)] (rows of the block as updated so far, rows beyond it as they stand)
    code = the rule's code of w[j] under (s, z); d = its dequantised value; e = (w[j] - d) / u[j, j]
    w[k] -= e * u[j, k] for j < k < c0 + B;  w[j] = d

and after the block w[c0 + B:] -= u[c0 : c0 + B, c0 + B:]^T err. Codes here are the rule's: sym in [-off, qmax], asym in
[0, levels] with z in [0, levels] (the device stores asym codes and zero points shifted by -off).

`sweep_block` is that block, `quantize_weight` the whole algorithm, `lattice` / `correlated` the input families,
`replay_check` holds a device block to the definition given the device's own earlier errors.
"""
import numpy as np

try:
    from . import quant_reference as Q
except ImportError:  # imported as a top-level module
    import quant_reference as Q

WNAME = {4: "int4_clip", 8: "int8", 3: "int3_clip", 2: "int2_clip"}


def ranges(bits):
    """qmax, levels, off"""
    return 2 ** (bits - 1) - 1, 2 ** bits - 1, 2 ** (bits - 1)


def code_of(v, s, z, bits, asym):
    """the rule's code of values v under (s, z), and the dequantised value, in v's dtype"""
    qmax, levels, off = ranges(bits)
    r = np.rint(v / s)
    if asym:
        c = np.clip(r + z, 0, levels)
        return c.astype(np.int64), ((c - z) * s).astype(v.dtype)
    c = np.clip(r, -off, qmax)
    return c.astype(np.int64), (c * s).astype(v.dtype)


def sweep_block(w, u, c0, B, group, bits, asym, scale=None, zp=None, params_given=False, col_group=None,
                dtype=np.float64):
    """-> dict(w [K, N] after the block, q [K, N] int64 (rows of the block set), err [B, N], scale [G, N], zp [G, N] int64
    or None). `scale` / `zp` carry the parameters of earlier blocks (or all of them when params_given)."""
    w = np.array(w, dtype)
    u = np.asarray(u, dtype)
    K, N = w.shape
    g, G = Q.group_of(K, group)
    scale = np.ones((G, N)) if scale is None else np.array(scale, np.float64)
    zp = (np.zeros((G, N), np.int64) if zp is None else np.array(zp, np.int64)) if asym else None
    q = np.zeros((K, N), np.int64)
    err = np.zeros((B, N), dtype)
    for j in range(c0, c0 + B):
        gid = int(col_group[j]) if col_group is not None else j // g
        if not params_given and j % g == 0:
            r = Q.quantize(w[j:min(j + g, K)], -1, WNAME[bits], asym)
            scale[gid] = r["s"][0].astype(dtype)  # a float32 run keeps the scale it used
            if asym:
                zp[gid] = r["z"][0]
        s = scale[gid].astype(dtype)
        z = zp[gid].astype(dtype) if asym else 0
        v = w[j].copy()
        q[j], d = code_of(v, s, z, bits, asym)
        e = (v - d) / u[j, j]
        err[j - c0] = e
        w[j + 1:c0 + B] -= np.outer(u[j, j + 1:c0 + B], e)
        w[j] = d
    return dict(w=w, q=q, err=err, scale=scale, zp=zp)


def upper_factor(H):
    """float64 U, upper triangular, with H^-1 = U^T U"""
    Hinv = np.linalg.inv(np.asarray(H, np.float64))
    Hinv = (Hinv + Hinv.T) / 2
    return np.linalg.cholesky(Hinv).T.copy()


def prepare(w, H, group, bits, asym, damp_percent, desc_act, static_groups):
    """the steps before the sweep -> (W in working order, damped H in working order, perm or None, scale0, zp0)"""
    W = np.array(w, np.float64)
    H = np.array(H, np.float64)
    K = W.shape[0]
    dead = np.diag(H) == 0
    H[dead, dead] = 1.0
    W[dead] = 0.0
    scale0 = zp0 = None
    if static_groups:
        r = Q.quantize(W, group, WNAME[bits], asym)
        scale0, zp0 = r["s"], r["z"]
    perm = None
    if desc_act:
        perm = np.argsort(-np.diag(H), kind="stable")
        W, H = W[perm], H[perm][:, perm]
    H[np.arange(K), np.arange(K)] += damp_percent * np.mean(np.diag(H))
    return W, H, perm, scale0, zp0


def quantize_weight(w, H, bits, group, sym, blocksize=128, damp_percent=0.01, desc_act=False, static_groups=False):
    """the whole algorithm -> dict(q [K, N] original order, scale [G, N], zp or None, g_idx [K] or None, loss = sum
    err^2 / 2, deq [K, N] original order, Hd = the damped Hessian in original order)"""
    asym = not sym
    W, Hd, perm, scale, zp = prepare(w, H, group, bits, asym, damp_percent, desc_act, static_groups)
    K, N = W.shape
    g, G = Q.group_of(K, group)
    U = upper_factor(Hd)
    col_group = perm // g if (static_groups and desc_act) else None
    q = np.zeros((K, N), np.int64)
    loss = 0.0
    for c0 in range(0, K, blocksize):
        B = min(blocksize, K - c0)
        r = sweep_block(W, U, c0, B, group, bits, asym, scale, zp, static_groups, col_group)
        W, scale, zp = r["w"], r["scale"], r["zp"]
        q[c0:c0 + B] = r["q"][c0:c0 + B]
        W[c0 + B:] -= U[c0:c0 + B, c0 + B:].T @ r["err"]
        loss += float((r["err"] ** 2).sum()) / 2
    g_idx = None
    deq = W
    if desc_act:
        inv = np.argsort(perm)
        q, deq, Hd = q[inv], W[inv], Hd[inv][:, inv]
        if not static_groups:
            g_idx = (np.arange(K) // g)[inv]
    return dict(q=q, scale=scale, zp=zp, g_idx=g_idx, loss=loss, deq=deq, Hd=Hd)


def hessian_loss(w, deq, H):
    """tr(D^T H D), D = w - deq [K, N]: the layer's squared output error under the Hessian's inputs"""
    D = np.asarray(w, np.float64) - np.asarray(deq, np.float64)
    return float((D * (np.asarray(H, np.float64) @ D)).sum())


def dequantize(q, scale, zp, group, g_idx=None):
    """codes (the rule's domain) + parameters -> float64 [K, N]"""
    K = q.shape[0]
    g, _ = Q.group_of(K, group)
    gi = np.arange(K) // g if g_idx is None else np.asarray(g_idx)
    s = np.asarray(scale, np.float64)[gi]
    z = np.asarray(zp, np.float64)[gi] if zp is not None else 0.0
    return (np.asarray(q, np.float64) - z) * s


# ---- input families ------------------------------------------------------------------------------------------------
def lattice(K, N, group, bits=4, seed=0):
    """(w fp32 [K, N], u fp32 [K, K]) on which every operation of the sweep is exact in fp32 (sym):
      u: diagonal in {1, 2}; at most 3 entries above the diagonal per column, each +-1; the column of every group-start
         row and of every row with diagonal 2 is zero above the diagonal
      w: multiples of 2^-8 in [-5, 5]; each group's first row planted +-qmax, so every scale is exactly 1; an eighth
         of the other entries planted at k + 0.5 (exact rounding ties where the row takes no update)
    A row with diagonal 2 takes no update, so its error is a multiple of 2^-9, and so is everything after it."""
    rng = np.random.default_rng(seed)
    qmax = 2 ** (bits - 1) - 1
    g, G = Q.group_of(K, group)
    u = np.zeros((K, K), np.float32)
    two = rng.random(K) < 0.3
    u[np.arange(K), np.arange(K)] = np.where(two, 2.0, 1.0)
    for k in range(1, K):
        if k % g == 0 or two[k]:
            continue
        rows = rng.choice(k, size=min(k, int(rng.integers(0, 4))), replace=False)
        u[rows, k] = rng.choice([-1.0, 1.0], size=len(rows))
    w = (rng.integers(-5 * 256, 5 * 256 + 1, size=(K, N)) / 256.0).astype(np.float32)
    tie = rng.random((K, N)) < 0.125
    w[tie] = (rng.integers(-5, 5, size=int(tie.sum())) + 0.5).astype(np.float32)
    for gi in range(G):
        w[gi * g] = np.where(rng.random(N) < 0.5, -float(qmax), float(qmax))
    return w, u


def correlated(K, N, seed=0, tokens=1024):
    """(w fp32 [K, N] Gaussian, H fp32 [K, K] = 2 / tokens X^T X) with X = eight common factors with N(0, 1) loadings
    plus 0.5 N(0, 1) of its own per feature: strongly correlated inputs, the case GPTQ is for."""
    rng = np.random.default_rng(seed)
    load = rng.standard_normal((8, K))
    X = rng.standard_normal((tokens, 8)) @ load + 0.5 * rng.standard_normal((tokens, K))
    H = (2.0 / tokens) * (X.T @ X)
    w = (0.05 * rng.standard_normal((K, N))).astype(np.float32)
    return w, H.astype(np.float32)


# ---- a device block against the definition -----------------------------------------------------------------------
def replay_check(w0, u, c0, B, group, bits, asym, q_dev, scale_dev, zp_dev, err_dev, w_after, params_given=False,
                 col_group=None):
    """One swept block held to the definition with the device's own earlier errors as the givens, so nothing is
    amplified and a near tie may fall either way. w0 = the weight at the block's entry; q_dev / zp_dev in the rule's
    domain; scale_dev the fp32 values as float64. For each j, in float64,
        w_j = w0_j - sum_{c0 <= i < j} err_dev[i] u[i][j],   b_j = (j - c0 + 2) 2^-24 (|w0_j| + sum |err_dev[i]| |u[i][j]|)
    (b_j: the standard bound of an fp32 running sum of j - c0 fused updates, with two more roundings of room).
      code    a nearest level: |w_j / s - (code - z)| <= 0.5 + b_j / s, or the end code where w_j / s lies beyond it
      err     |err_dev[j] - (w_j - d_j) / u_jj| <= (b_j + 2^-23 |w_j - d_j|) / u_jj, d_j = (code - z) s
      scale   at a group start: the rule's scale of the replayed group within bounds()['scale'] + b / max|v| (sym;
              asym 2 b / (hi - lo): both ends of the range move by at most b), b the largest b_k of the group's rows
              at that step; the zero point within 0.5 + levels times that of -lo / s_dev
      w       on return row j is fl32(fl32(code - z) * s), exactly
    Returns the largest err / bound of each."""
    w0 = np.asarray(w0, np.float64)
    u = np.asarray(u, np.float64)
    err_dev = np.asarray(err_dev, np.float64)
    scale_dev = np.asarray(scale_dev, np.float64)
    K, N = w0.shape
    g, G = Q.group_of(K, group)
    qmax, levels, off = ranges(bits)
    lo_code, hi_code = (0, levels) if asym else (-off, qmax)
    srel = Q.bounds(WNAME[bits], "fp32")["scale"]
    rep = dict(code=0.0, err=0.0, scale=0.0, zp=0.0)
    cur = w0.copy()                     # rows of the block as replayed so far
    mag = np.abs(w0)                    # |w0_k| + sum |err_i| |u_ik|
    for j in range(c0, c0 + B):
        n_sum = j - c0
        gid = int(col_group[j]) if col_group is not None else j // g
        if not params_given and j % g == 0:
            k1 = min(j + g, K)
            v = cur[j:k1]
            b = ((n_sum + 2) * 2.0 ** -24 * mag[j:k1]).max(0)
            r = Q.quantize(v, -1, WNAME[bits], asym)
            s_ref = r["s"][0]
            span = (np.maximum(v.max(0), 0) - np.minimum(v.min(0), 0)) if asym else np.abs(v).max(0)
            rel = srel + (2.0 if asym else 1.0) * b / np.where(span == 0, 1.0, span)
            es = np.abs(scale_dev[gid] - s_ref) / (rel * s_ref)
            assert (es <= 1).all(), "row %d: scale off by %.3g of its bound" % (j, es.max())
            rep["scale"] = max(rep["scale"], float(es.max()))
            if asym:
                zt = -np.minimum(v.min(0), 0) / scale_dev[gid]
                ez = np.abs(zp_dev[gid] - np.clip(zt, 0, levels)) / (0.5 + levels * rel)
                assert (ez <= 1).all(), "row %d: zero point off by %.3g of its bound" % (j, ez.max())
                rep["zp"] = max(rep["zp"], float(ez.max()))
        s = scale_dev[gid]
        z = np.asarray(zp_dev[gid], np.float64) if asym else 0.0
        wj = cur[j]
        bj = (n_sum + 2) * 2.0 ** -24 * mag[j]
        code = np.asarray(q_dev[j], np.float64)
        assert (code >= lo_code).all() and (code <= hi_code).all(), "row %d: code out of range" % j
        x = wj / s + z
        slack = 0.5 + bj / s
        ok = np.abs(x - code) <= slack
        ok |= (code == hi_code) & (x >= hi_code - slack)
        ok |= (code == lo_code) & (x <= lo_code + slack)
        assert ok.all(), "row %d: code is not a nearest level at columns %s" % (j, np.argwhere(~ok)[:4].ravel())
        inner = (code > lo_code) & (code < hi_code)
        if inner.any():
            rep["code"] = max(rep["code"], float((np.abs(x - code) / slack)[inner].max()))
        d = (code - z) * s
        want = (wj - d) / u[j, j]
        tol = (bj + 2.0 ** -23 * np.abs(wj - d)) / u[j, j]
        ee = np.abs(err_dev[j - c0] - want)
        assert (ee <= tol).all(), "row %d: err off by %.3g of its bound" % (j, (ee / np.where(tol == 0, 1, tol)).max())
        rep["err"] = max(rep["err"], float((ee / np.where(tol == 0, 1.0, tol)).max()))
        d32 = (code - z).astype(np.float32) * scale_dev[gid].astype(np.float32)
        assert np.array_equal(np.asarray(w_after[j], np.float32), d32), "row %d: w is not code * s on return" % j
        cur[j + 1:c0 + B] -= np.outer(u[j, j + 1:c0 + B], err_dev[j - c0])
        mag[j + 1:c0 + B] += np.outer(np.abs(u[j, j + 1:c0 + B]), np.abs(err_dev[j - c0]))
    return rep
