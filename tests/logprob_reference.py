"""Reference for the log-probability record (csrc/woq_logprob.hip), numpy only.

`record_f64`: the specification. log_softmax over the given fp32 logits in float64, NaN logits weighing 0, and the 20
best ids by (logit descending, id ascending), padded with -1 / -inf. The order is pure comparisons of the fp32 values.

`logz_f32`: an fp32 restatement of the kernel's own summation order, used to size tolerances (how far fp32 arithmetic
of this shape lies from float64, measured on the reference alone): slices of 1024 ids, thread t of a slice adds ids
t, t + 256, t + 512, t + 768 in that order, a wave of 64 threads is summed as an xor butterfly (32, 16, .. 1), the four
waves are added in ascending order; the merge sums slice_sum * exp(slice_max - max) the same way over 1024 slots indexed
by slice (slot t adds slices t, t + 1024, ... in that order), then logZ = max + log(Z). A value equal to its maximum
weighs exactly 1.
"""
import numpy as np

TOP = 20
SLICE, THREADS = 1024, 256


def record_f64(logits, token):
    """-> (chosen float64, top_id int32 [20], top_lp float64 [20]) of fp32 `logits` [vocab] and the picked id."""
    x = np.asarray(logits, dtype=np.float32)
    ok = ~np.isnan(x)
    top_id = np.full(TOP, -1, dtype=np.int32)
    top_lp = np.full(TOP, -np.inf)
    if not ok.any():
        return np.nan, top_id, top_lp
    x64 = x.astype(np.float64)
    m = x64[ok].max()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w = np.where(ok, np.where(x64 == m, 1.0, np.exp(x64 - m)), 0.0)
        logz = m + np.log(w.sum())
        lp = x64 - logz
    ids = np.flatnonzero(ok)
    order = ids[np.lexsort((ids, -(x64[ids] + 0.0)))][:TOP]  # last key first: logit descending, then id ascending
    top_id[:len(order)] = order
    top_lp[:len(order)] = lp[order]
    return float(lp[int(token)]), top_id, top_lp


def _butterfly(v):
    """[..., 64] fp32 -> the wave's xor-butterfly sum (every lane ends with the same bits; lane 0 returned)"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(np.float32)
    return v[..., 0]


def _ordered(v):
    """[..., n] fp32 -> sum in ascending order"""
    z = v[..., 0].astype(np.float32)
    for i in range(1, v.shape[-1]):
        z = (z + v[..., i]).astype(np.float32)
    return z


def logz_f32(logits):
    """fp32 logZ in the kernel's summation order (NaN when no logit is a number)."""
    x = np.asarray(logits, dtype=np.float32)
    vocab = x.shape[0]
    n_slices = (vocab + SLICE - 1) // SLICE
    pad = np.full(n_slices * SLICE, np.nan, dtype=np.float32)
    pad[:vocab] = x
    s = pad.reshape(n_slices, SLICE // THREADS, THREADS)  # [slice][j][thread]: id = slice * 1024 + j * 256 + thread
    ok = ~np.isnan(s)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.where(ok, s, -np.inf).max(axis=(1, 2)).astype(np.float32)  # slice maxima (-inf: nothing, or only -inf)
        has = ok.any(axis=(1, 2))
        w = np.where(ok, np.where(s == m[:, None, None], np.float32(1), np.exp((s - m[:, None, None]).astype(np.float32))),
                     np.float32(0)).astype(np.float32)
        per_thread = _ordered(np.moveaxis(w, 1, 2))                       # [slice][thread]
        waves = _butterfly(per_thread.reshape(n_slices, THREADS // 64, 64))  # [slice][wave]
        slice_sum = _ordered(waves)                                        # [slice]
        if not has.any():
            return np.float32(np.nan)
        M = m[has].max()
        scale = np.where(m == M, np.float32(1), np.exp((m - M).astype(np.float32))).astype(np.float32)
        term = np.zeros(1024 * ((n_slices + 1023) // 1024), dtype=np.float32)
        term[:n_slices] = np.where(has, (slice_sum * scale).astype(np.float32), np.float32(0))
        acc = _ordered(term.reshape(-1, 1024).T)                           # thread t owns slices t, t + 1024, ...
        Z = _ordered(_butterfly(acc.reshape(16, 64)))
        return np.float32(M + np.log(Z, dtype=np.float32))


def record_f32(logits, token):
    """(chosen, top_lp [20]) as fp32 arithmetic of the kernel's shape gives them; ids are `record_f64`'s."""
    x = np.asarray(logits, dtype=np.float32)
    _, top_id, _ = record_f64(x, token)
    logz = logz_f32(x)
    with np.errstate(invalid="ignore"):
        chosen = np.float32(x[int(token)] - logz) if not np.isnan(logz) else np.float32(np.nan)
        top_lp = np.where(top_id >= 0, (x[np.maximum(top_id, 0)] - logz).astype(np.float32), -np.inf)
    return chosen, top_lp.astype(np.float32)


def deviation(logits, token):
    """largest |fp32 restatement - float64| over the record's finite values (0 when there is none)"""
    c64, _, t64 = record_f64(logits, token)
    c32, t32 = record_f32(logits, token)
    a = np.concatenate([[c64], t64])
    b = np.concatenate([[c32], t32]).astype(np.float64)
    fin = np.isfinite(a)
    assert (np.isfinite(b) == fin).all()
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0
