"""The scored head alone (csrc/woq_score.hip: final norm as hi + lo rows, lm_head over all rows on the matrix cores, the
log-probability record per row), through `woq_probe_score_rows`, against tests/score_reference.py.

Inputs: hidden 256, rows N(0, 1) with the last row scaled by 30 (so the norm matters), head weights of sigma 0.08, seed 0.
Rows 1, 15, 16, 17, 70, 300: ragged against the 16-row MFMA and the 128-row output tile, 300 crosses the 256-row block.
Vocabularies 16 (fewer than 20 ids: the record pads), 1000 (below one 1024-id slice, ragged against the 128-id tile) and
2500 (ragged against tile and slice). The largest case runs with an fp16 and with a bf16 head.

* `chosen` and `top_lp` lie within `score_reference.tolerance` (4 x (A + B), computed from the reference alone and
  printed) of float64.
* `top_id` equals the reference for every row whose 21 largest reference logits are pairwise more than 2 x tolerance
  apart; the other rows are compared as sets of (id, log-probability), and at most 10 % of a case's rows may be such.
"""
import functools

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import logprob_reference as R
from tests import score_reference as S

pytestmark = pytest.mark.gpu

HIDDEN, EPS = 256, 1e-5
CASES = [  # rows, vocab, head type
    (1, 1000, "fp16"), (15, 16, "fp16"), (16, 2500, "bf16"), (17, 1000, "bf16"), (70, 16, "bf16"), (70, 2500, "fp16"),
    (300, 2500, "fp16"), (300, 2500, "bf16"),
]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _inputs(rows, vocab, kind):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((rows, HIDDEN)).astype(np.float32)
    x[-1] *= 30
    W = torch.from_numpy((0.08 * rng.standard_normal((vocab, HIDDEN))).astype(np.float32)).to(DTYPES[kind])
    norm_w = (1 + 0.1 * rng.standard_normal(HIDDEN)).astype(np.float32)
    targets = rng.integers(0, vocab, rows).astype(np.int32)
    return x, norm_w, W, targets


@functools.lru_cache(maxsize=None)
def _reference(rows, vocab, kind):
    """-> (score_f64's record, the reference logits, A, B), computed once per case"""
    x, norm_w, W, targets = _inputs(rows, vocab, kind)
    a, b = S.tolerance_terms(x, norm_w, EPS, W, targets)
    return S.score_f64(x, norm_w, EPS, W, targets), S.logits_f64(x, norm_w, EPS, W), a, b


def _probe(x, norm_w, W, targets, extra_rows=0, sentinel=123.0):
    dev, M = "cuda", x.shape[0]
    chosen = torch.full((M + extra_rows,), sentinel, dtype=torch.float32, device=dev)
    top_id = torch.full((M + extra_rows, R.TOP), -7, dtype=torch.int32, device=dev)
    top_lp = torch.full((M + extra_rows, R.TOP), sentinel, dtype=torch.float32, device=dev)
    L.probe_score_rows(torch.from_numpy(x).to(dev), torch.from_numpy(norm_w).to(dev), EPS, W.to(dev),
                       torch.from_numpy(targets).to(dev), chosen, top_id, top_lp)
    torch.cuda.synchronize()
    return chosen.cpu().numpy(), top_id.cpu().numpy(), top_lp.cpu().numpy()


def _check_rows(got, want, logits, tol, what, rows=None):
    """values within tol; ids equal where the reference's top 21 are well separated, as sets elsewhere (<= 10 % of rows)"""
    chosen, top_id, top_lp = got
    c64, id64, lp64 = want
    rows = range(len(c64)) if rows is None else rows
    worst, loose = 0.0, 0
    for r in rows:
        listed = id64[r] >= 0
        assert (top_id[r][~listed] == -1).all() and np.isneginf(top_lp[r][~listed]).all(), (what, r)
        assert np.isnan(chosen[r]) == np.isnan(c64[r]), (what, r)
        if not np.isnan(c64[r]):
            worst = max(worst, abs(float(chosen[r]) - c64[r]))
        if S.min_top_gap(logits[r]) > 2 * tol:
            assert (top_id[r] == id64[r]).all(), (what, r)
            if listed.any():
                worst = max(worst, float(np.abs(top_lp[r][listed] - lp64[r][listed]).max()))
        else:
            loose += 1
            assert set(top_id[r].tolist()) == set(id64[r].tolist()), (what, r)
            by_id = dict(zip(id64[r][listed].tolist(), lp64[r][listed].tolist()))
            worst = max([worst] + [abs(float(lp) - by_id[int(i)]) for i, lp in zip(top_id[r][listed], top_lp[r][listed])])
    print("%s: max |kernel - float64| = %.3e (tol %.3e), %d of %d rows compared as sets" % (what, worst, tol, loose, len(rows)))
    assert loose <= 0.1 * len(rows), what
    assert worst <= tol, what


@pytest.mark.parametrize("rows,vocab,kind", CASES)
def test_scored_rows_match_the_float64_reference(rows, vocab, kind):
    x, norm_w, W, targets = _inputs(rows, vocab, kind)
    want, logits, a, b = _reference(rows, vocab, kind)
    tol = 4 * (a + b)
    print("rows %d vocab %d %s: A = %.3e, B = %.3e, tolerance = %.3e" % (rows, vocab, kind, a, b, tol))
    assert 0 < tol < 1e-3
    got = _probe(x, norm_w, W, targets)
    _check_rows(got, want, logits, tol, "rows %d vocab %d %s" % (rows, vocab, kind))
    listed = min(vocab, R.TOP)
    assert (got[1][:, :listed] >= 0).all() and (got[1][:, :listed] < vocab).all()
    assert (got[1][:, listed:] == -1).all() and np.isneginf(got[2][:, listed:]).all()


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_special_rows_and_untouched_memory(kind):
    rows, vocab = 17, 1000
    x, norm_w, W, targets = (a.copy() if isinstance(a, np.ndarray) else a for a in _inputs(rows, vocab, kind))
    targets[0], targets[1] = -1, vocab
    x[2, 77] = np.nan
    want = S.score_f64(x, norm_w, EPS, W, targets)
    logits = S.logits_f64(x, norm_w, EPS, W)
    tol = S.tolerance(x, norm_w, EPS, W, targets)
    chosen, top_id, top_lp = _probe(x, norm_w, W, targets, extra_rows=3)
    # rows past M keep the sentinel
    assert (chosen[rows:] == 123.0).all() and (top_id[rows:] == -7).all() and (top_lp[rows:] == 123.0).all()
    got = (chosen[:rows], top_id[:rows], top_lp[:rows])
    # a target outside the vocabulary: chosen NaN, the row's top 20 still written
    for r in (0, 1):
        assert np.isnan(chosen[r]) and np.isnan(want[0][r])
        assert (top_id[r] == want[1][r]).all() or S.min_top_gap(logits[r]) <= 2 * tol
        assert np.isfinite(top_lp[r]).all()
    # one NaN in the hidden state: the norm makes the whole row NaN, the all-NaN record
    assert np.isnan(chosen[2]) and (top_id[2] == -1).all() and np.isneginf(top_lp[2]).all()
    assert np.isnan(want[0][2]) and (want[1][2] == -1).all()
    _check_rows(got, want, logits, tol, "special rows %s" % kind)
