"""Reference for the scored prompt pass (csrc/woq_score.hip): numpy, torch only to convert bf16 bits.

`score_f64`: the specification. Final RMSNorm of each fp32 residual row in float64, a float64 product with the head's
weights converted exactly from their stored type, then `logprob_reference.record_f64` per row. A target outside
[0, vocab) gives chosen = NaN; the row's 20 ids are listed all the same.

`tolerance`: 4 x (A + B), from the reference alone.
  A = the largest deviation from float64, over the finite record values, of an all-fp32 restatement: fp32 norm,
      `np.float32` xn @ W.T, `record_f32` (the fp32 restatement of the record's own summation order);
  B = the largest change of those values when the float64 path multiplies hi + lo (xn split in the head's type,
      hi = cvt(xn), lo = cvt(xn - hi): what the kernel feeds the matrix cores) in place of xn.
The factor 4 is the margin the log-probability tests give their fp32 restatement.
"""
import numpy as np
import torch

from tests import logprob_reference as R


def weights_f64(W):
    """head weights (torch fp16 / bf16 tensor, or a numpy float16 array) -> (float64 [vocab, hidden], "fp16" | "bf16")"""
    if isinstance(W, torch.Tensor):
        kind = {torch.float16: "fp16", torch.bfloat16: "bf16"}[W.dtype]
        return W.detach().cpu().to(torch.float64).numpy(), kind
    assert W.dtype == np.float16
    return W.astype(np.float64), "fp16"


def _cvt(x64, kind):
    """float64 -> the head's 16-bit type (round to nearest even) -> float64"""
    if kind == "fp16":
        with np.errstate(over="ignore"):
            return x64.astype(np.float16).astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(x64)).to(torch.bfloat16).to(torch.float64).numpy()


def norm_f64(hidden_rows, norm_w, eps):
    x = np.asarray(hidden_rows, dtype=np.float32).astype(np.float64)
    inv = 1.0 / np.sqrt((x * x).mean(axis=1, keepdims=True) + float(eps))
    return x * inv * np.asarray(norm_w, dtype=np.float32).astype(np.float64)


def _records(logits, targets, record):
    """`record` per row -> chosen [M], top_id [M, 20], top_lp [M, 20] (float64)"""
    M, vocab = logits.shape
    chosen, top_id, top_lp = np.empty(M), np.empty((M, R.TOP), dtype=np.int32), np.empty((M, R.TOP))
    for r in range(M):
        t = int(targets[r])
        inside = 0 <= t < vocab
        out = record(logits[r], t if inside else 0)
        chosen[r] = out[0] if inside else np.nan
        if len(out) == 3:
            top_id[r], top_lp[r] = out[1], out[2]
        else:  # record_f32: ids are record_f64's
            top_id[r], top_lp[r] = R.record_f64(logits[r], 0)[1], out[1]
    return chosen, top_id, top_lp


def logits_f64(hidden_rows, norm_w, eps, W):
    """the fp32 rounding of the float64 logits [M, vocab] (what record_f64 takes)"""
    w64, _ = weights_f64(W)
    with np.errstate(invalid="ignore"):
        return (norm_f64(hidden_rows, norm_w, eps) @ w64.T).astype(np.float32)


def score_f64(hidden_rows, norm_w, eps, W, targets):
    """-> (chosen float64 [M], top_id int32 [M, 20], top_lp float64 [M, 20])"""
    return _records(logits_f64(hidden_rows, norm_w, eps, W), targets, R.record_f64)


def _max_dev(a, b):
    worst = 0.0
    for x, y in zip((a[0], a[2]), (b[0], b[2])):
        fin = np.isfinite(x) & np.isfinite(y)
        if fin.any():
            worst = max(worst, float(np.abs(x[fin] - y[fin]).max()))
    return worst


def tolerance_terms(hidden_rows, norm_w, eps, W, targets):
    """-> (A, B) of the module docstring"""
    w64, kind = weights_f64(W)
    base = score_f64(hidden_rows, norm_w, eps, W, targets)
    # A: everything in fp32
    x = np.asarray(hidden_rows, dtype=np.float32)
    nw = np.asarray(norm_w, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ss = (x * x).sum(axis=1, keepdims=True, dtype=np.float32)
        inv = (np.float32(1) / np.sqrt(ss / np.float32(x.shape[1]) + np.float32(eps))).astype(np.float32)
        xn32 = (x * inv * nw).astype(np.float32)
        lg32 = (xn32 @ w64.astype(np.float32).T).astype(np.float32)
    a = _max_dev(base, _records(lg32, targets, R.record_f32))
    # B: hi + lo in place of xn, float64 otherwise
    xn = norm_f64(hidden_rows, norm_w, eps)
    with np.errstate(invalid="ignore"):
        hi = _cvt(xn, kind)
        lo = _cvt(xn - hi, kind)
        lg = ((hi + lo) @ w64.T).astype(np.float32)
    b = _max_dev(base, _records(lg, targets, R.record_f64))
    return a, b


def tolerance(hidden_rows, norm_w, eps, W, targets):
    a, b = tolerance_terms(hidden_rows, norm_w, eps, W, targets)
    return 4 * (a + b)


def min_top_gap(logits_row, n=R.TOP + 1):
    """smallest difference between neighbours among the row's n largest logits (inf when it has fewer than 2 numbers)"""
    x = np.asarray(logits_row, dtype=np.float64)
    x = np.sort(x[~np.isnan(x)])[::-1][:n]
    return float(np.min(-np.diff(x))) if len(x) > 1 else np.inf
