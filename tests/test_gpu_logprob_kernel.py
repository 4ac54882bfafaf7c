"""The log-probability record's two launches (csrc/woq_logprob.hip) alone, through `woq_probe_logprobs`, against
tests/logprob_reference.py.

* `top_id` equals the float64 reference exactly: the order (logit descending, id ascending) is pure comparisons of the
  given fp32 values.
* `chosen` and `top_lp` lie within `tol` of float64, tol = 4 x the largest deviation of the fp32 restatement of the
  kernel's summation order (`logprob_reference.deviation`) from float64 over this file's own inputs: every vocabulary
  size, every input kind, every chosen token below. It is computed here, from the reference alone, and printed.
* -inf logits give -inf, NaN logits are never listed and give a NaN `chosen`, short lists pad with -1 / -inf, an all-NaN
  row gives chosen = NaN and every id -1.
"""
import functools

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import logprob_reference as R

pytestmark = pytest.mark.gpu

# 1: edge; 19: fewer than 20 (padding); 1000: divides nothing; the others: one slice, and the vocabularies in use
VOCABS = (1, 19, 64, 1000, 32000, 50257, 128256)
KINDS = ("normal", "ties", "neginf", "peak", "nan", "all_nan")


@functools.lru_cache(maxsize=None)
def _case(vocab, kind):
    """-> (logits fp32 [vocab], tuple of chosen ids): the best id, the worst id, a tied id, a -inf id, a NaN id where the
    row has one."""
    rng = np.random.default_rng(1000 * VOCABS.index(vocab) + KINDS.index(kind))
    x = (4 * rng.standard_normal(vocab)).astype(np.float32)
    some = min(max(1, vocab // 10), vocab - 1)  # "some" entries: at least one where the row can spare it
    extra = []
    if kind == "ties":
        x = (np.round(x * 4) / 4).astype(np.float32)  # 0.25 steps: many ties, id order decides
        vals, counts = np.unique(x, return_counts=True)
        if (counts > 1).any():
            extra.append(int(np.flatnonzero(x == vals[counts > 1][-1])[-1]))  # the last id of the best tied value
    elif kind == "neginf":
        hit = rng.choice(vocab, some, replace=False)
        x[hit] = -np.inf
        extra += [int(i) for i in hit[:1]]
    elif kind == "peak":
        x[int(rng.integers(vocab))] = np.float32(x.max() + 80)
    elif kind == "nan":
        hit = rng.choice(vocab, some, replace=False)
        x[hit] = np.nan
        extra += [int(i) for i in hit[:1]]
    elif kind == "all_nan":
        x[:] = np.nan
        return x, (0, vocab - 1)
    filled = np.where(np.isnan(x), np.inf, x)
    best = int(np.nanargmax(np.where(np.isnan(x), -np.inf, x)))
    worst = int(np.flatnonzero(filled == filled.min())[-1])  # lowest value that is a number, its last id
    return x, tuple(dict.fromkeys([best, worst] + extra))


@functools.lru_cache(maxsize=None)
def _tol():
    worst = max(R.deviation(_case(v, k)[0], t) for v in VOCABS for k in KINDS for t in _case(v, k)[1])
    assert 0 < worst < 1e-4  # fp32 over values up to ~100: a few ulp of 2^6 at most
    return 4 * worst


def _probe(x, tokens):
    """one probe call per chosen id, all asynchronous -> chosen [n], top_id [n, 20], top_lp [n, 20]"""
    dev, n = "cuda", len(tokens)
    lg = torch.from_numpy(x).to(dev)
    tok = torch.tensor(tokens, dtype=torch.int32, device=dev)
    chosen = torch.full((n,), 123.0, dtype=torch.float32, device=dev)
    top_id = torch.full((n, R.TOP), -7, dtype=torch.int32, device=dev)
    top_lp = torch.full((n, R.TOP), 123.0, dtype=torch.float32, device=dev)
    for j in range(n):
        L.probe_logprobs(lg, tok[j:j + 1], chosen[j:j + 1], top_id[j], top_lp[j])
    torch.cuda.synchronize()
    return chosen.cpu().numpy(), top_id.cpu().numpy(), top_lp.cpu().numpy()


def _close(got, want, tol, what):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    fin = np.isfinite(want)
    assert (np.isnan(got) == np.isnan(want)).all(), what
    assert (got[~fin & ~np.isnan(want)] == want[~fin & ~np.isnan(want)]).all(), what  # -inf stays -inf
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print("%s: max |kernel - float64| = %.3e (tol %.3e)" % (what, err, tol))
    assert np.isfinite(got[fin]).all() and err <= tol, what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("vocab", VOCABS)
def test_record_matches_the_float64_reference(vocab, kind):
    x, tokens = _case(vocab, kind)
    tol = _tol()
    chosen, top_id, top_lp = _probe(x, tokens)
    for j, t in enumerate(tokens):
        c64, id64, lp64 = R.record_f64(x, t)
        what = "vocab %d %s token %d" % (vocab, kind, t)
        assert (top_id[j] == id64).all(), what
        _close(top_lp[j], lp64, tol, what + " top_lp")
        _close(chosen[j], c64, tol, what + " chosen")
    # conventions, on the kernel's output itself
    n_num = int((~np.isnan(x)).sum())
    listed = min(n_num, R.TOP)
    assert (top_id[:, listed:] == -1).all() and np.isneginf(top_lp[:, listed:]).all()
    assert (top_id[:, :listed] >= 0).all() and not np.isnan(x[top_id[0, :listed]]).any()
    if kind == "all_nan":
        assert np.isnan(chosen).all() and (top_id == -1).all()
    if kind == "peak":
        assert abs(chosen[0]) <= tol and (top_lp[0, 1:listed] < -70).all()
    if kind == "neginf":
        for j, t in enumerate(tokens):
            assert np.isneginf(chosen[j]) == np.isneginf(x[t])
    if kind == "nan":
        for j, t in enumerate(tokens):
            assert np.isnan(chosen[j]) == np.isnan(x[t])
    if kind == "ties" and listed > 1:  # equal logits are listed in id order
        v = x[top_id[0, :listed]]
        assert (np.diff(v) <= 0).all() and (np.diff(top_id[0, :listed])[np.diff(v) == 0] > 0).all()
