"""The AWQ kernels alone (`qbits.awq_scale_delta`, `qbits.awq_clip_search`, csrc/woq_awq.hip) and the scale search
built on them (`quantization/awq.py search_scale`) against the float64 reference tests/awq_reference.py."""
import functools

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import qbits
from tests import awq_reference as A
from tests import gptq_reference as G
from tests import quant_reference as Q

pytestmark = pytest.mark.gpu

DELTA_SHAPES = [(256, 96, 64), (384, 200, 128), (200, 70, 32)]  # the last: a short final group and a ragged N
# the last two: K < group, one short group that still runs in its group's own kernel form
CLIP_SHAPES = [(256, 96, 32), (384, 200, 128), (200, 70, 64), (100, 200, 128), (48, 96, 64)]
EPS = 2.0 ** -24

# sum over the cells of losses[best], device over reference, on the six clip cases with K > group, measured on the
# MI355X (profiles/r16_awq.txt): the largest |ratio - 1| was 6.02e-8; the bound is 16 x that. A wrong Gram element or clamp
# moves the sum by tens of percent (RTN's is 1.45 to 2.2 times the best).
CLIP_SUM_MARGIN = 16 * 6.02e-8


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


# ---- delta ---------------------------------------------------------------------------------------------------------
DELTA_CASES = [(K, N, g, 4, asym) for (K, N, g) in DELTA_SHAPES for asym in (False, True)] + [(256, 96, 64, 8, True)]


@pytest.mark.parametrize("K,N,group,bits,asym", DELTA_CASES)
def test_scale_delta(K, N, group, bits, asym):
    w, _ = G.correlated(K, N, seed=K)
    a = np.random.default_rng(K + 1).lognormal(0.0, 1.0, K)
    wd = _dev(w)
    g, _ = Q.group_of(K, group)
    for r in (0.0, 0.35, 0.95):
        s32 = A.scale_of(a, round(r * A.N_GRID)).astype(np.float32)
        ref = A.scale_delta(w, s32, group, bits, asym)
        D = qbits.awq_scale_delta(wd, _dev(s32), group, bits, asym).cpu().numpy().astype(np.float64)
        W = w.astype(np.float64)
        # the code the device's value implies, on the reference's scale (asym: code - zero point)
        step = np.repeat(ref["qs"], g, axis=0)[:K]
        implied = np.rint((D + W) * s32[:, None].astype(np.float64) / step)
        want = np.rint(ref["back"] * s32[:, None].astype(np.float64) / step)
        agree = implied == want
        x = ref["x"]
        near_tie = np.abs(np.abs(x - np.floor(x)) - 0.5) <= Q.FP32_SLOP * np.maximum(1.0, np.abs(x))
        assert not (~agree & ~near_tie).any(), np.argwhere(~agree & ~near_tie)[:4]
        assert (~agree).mean() <= 1e-4
        err = np.abs(D - ref["D"])
        bound = 8 * EPS * (np.abs(W) + np.abs(W + ref["D"]))
        worst = (err / np.where(bound == 0, 1.0, bound))[agree].max()
        print("delta K=%d N=%d group=%d bits=%d asym=%d r=%.2f: codes differing %d, max |dD| %.3g, err / bound %.3f"
              % (K, N, group, bits, asym, r, int((~agree).sum()), err[agree].max(), worst))
        assert (err <= bound)[agree].all()
        if r == 0.0 and bits == 4:  # s = 1: the package's own RTN of the weight, exactly (an int8 blob dequantises
            # as two int4 planes, two products: not the one product of the rule)
            blob = qbits.quantize_to_packed_weight(wd, False, group, "fp32", A.WNAME[bits], "fp32", asym)
            deq = torch.empty(K, N, dtype=torch.float32, device="cuda")
            qbits.dequantize_packed_weight(blob, deq, False, "fp32", A.WNAME[bits], "fp32")
            assert np.array_equal(D.astype(np.float32), (deq - wd).cpu().numpy())


def test_scale_delta_one_group_per_column():
    w, _ = G.correlated(200, 70, seed=9)
    s32 = A.scale_of(np.random.default_rng(2).lognormal(0.0, 1.0, 200), 10).astype(np.float32)
    ref = A.scale_delta(w, s32, -1, 4, False)
    D = qbits.awq_scale_delta(_dev(w), _dev(s32), -1, 4, False).cpu().numpy().astype(np.float64)
    W = w.astype(np.float64)
    assert (np.abs(D - ref["D"]) <= 8 * EPS * (np.abs(W) + np.abs(W + ref["D"]))).mean() > 1 - 1e-4


# ---- clip ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clip_case(K, N, group, asym):
    """(w, H, reference, device results as numpy): one reference and one launch per case, shared by the tests"""
    w, H = G.correlated(K, N, seed=K)
    ref = A.clip_search(w, H, group, 4, asym)
    n_groups = (K + group - 1) // group
    losses = torch.full((A.N_CLIP, n_groups, N), float("nan"), device="cuda")
    w_out = torch.full((K, N), float("nan"), device="cuda")
    best, losses, w_out = qbits.awq_clip_search(_dev(w), _dev(H), group, 4, asym, A.N_GRID, A.N_CLIP, w_out=w_out,
                                                losses=losses)
    return w, H, ref, best.cpu().numpy(), losses.cpu().numpy().astype(np.float64), w_out.cpu().numpy()


@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("K,N,group", CLIP_SHAPES)
def test_clip_search(K, N, group, asym):
    w, H, ref, best, losses, w_out = _clip_case(K, N, group, asym)
    n_groups = (K + group - 1) // group
    assert best.shape == (n_groups, N) and losses.shape == (A.N_CLIP, n_groups, N) and w_out.shape == (K, N)
    # poisoned with NaN before the launch: every element was written
    assert np.isfinite(losses).all() and np.isfinite(w_out).all()
    assert best.min() >= 0 and best.max() < A.N_CLIP

    # the choice: the reference's wherever its runner-up is clearly behind
    clear = A.runner_up_gap(ref["losses"]) > 1e-5
    assert (~clear).mean() <= 1e-3
    differ = int((best != ref["best"]).sum())
    assert np.array_equal(best[clear], ref["best"][clear]), np.argwhere(clear & (best != ref["best"]))[:4]
    assert (ref["best"] > 0).mean() > 0.5  # most cells are clipped: the search is exercised

    # every candidate's loss within what fp32 allows, candidate 0 = the RTN loss; cells with a value at a rounding tie
    # may take the other code
    excess = np.abs(losses - ref["losses"]) / ref["fp32_bound"]
    ok = (excess <= 1) | ref["near_tie"]
    assert ref["near_tie"].mean() <= 1e-3
    assert ok.all(), (np.argwhere(~ok)[:4], excess[~ok][:4])
    picked = np.take_along_axis(losses, best[None].astype(np.int64), 0)[0]
    assert (picked <= losses[0]).all()
    assert np.array_equal(picked, losses.min(0))
    first = (losses == losses.min(0)).argmax(0)
    assert np.array_equal(best, first)  # the first minimum of the device's own losses

    ref_picked = np.take_along_axis(ref["losses"], ref["best"][None], 0)[0]
    ratio = picked.sum() / ref_picked.sum()
    print("clip K=%d N=%d group=%d asym=%d: %d cells, choices differing %d, clipped %.0f%%, RTN / best %.3f, "
          "largest loss err / bound %.3f, sum losses[best] dev / ref - 1 = %.3g"
          % (K, N, group, asym, best.size, differ, 100 * (best > 0).mean(), losses[0].sum() / picked.sum(),
             excess[~ref["near_tie"]].max(), ratio - 1))
    assert abs(ratio - 1) <= CLIP_SUM_MARGIN

    # the clamped weight: the reference's clamp to one fp32 rounding, untouched elements bit for bit
    same = np.repeat(best == ref["best"], group, axis=0)[:K]
    want = ref["w_out"]
    kept = want == w.astype(np.float64)
    assert np.array_equal(w_out[same & kept], w[same & kept])
    assert (np.abs(w_out.astype(np.float64) - want) <= EPS * (1 + 2.0 ** -20) * np.abs(want))[same].all()


def test_clip_search_takes_a_strided_gram_matrix_and_other_widths():
    """h as a view into a wider matrix (row stride > K); bits 8; fewer candidates"""
    K, N, group = 160, 70, 32
    w, H = G.correlated(K, N, seed=4)
    big = torch.zeros(K, K + 24, device="cuda")
    big[:, :K] = _dev(H)
    ref = A.clip_search(w, H, group, 8, True, n_cand=4)
    best, losses, _ = qbits.awq_clip_search(_dev(w), big[:, :K], group, 8, True, A.N_GRID, 4)
    assert tuple(losses.shape) == (4, K // group, N)
    excess = np.abs(losses.cpu().numpy().astype(np.float64) - ref["losses"]) / ref["fp32_bound"]
    assert ((excess <= 1) | ref["near_tie"]).all()
    clear = A.runner_up_gap(ref["losses"]) > 1e-5
    assert np.array_equal(best.cpu().numpy()[clear], ref["best"][clear])


def test_launchers_refuse_what_they_cannot_run():
    w = torch.zeros(128, 64, device="cuda")
    h = torch.eye(128, device="cuda")
    with pytest.raises(RuntimeError, match="QBits.*group"):
        qbits.awq_clip_search(w, h, 96, 4, False)
    with pytest.raises(RuntimeError, match="QBits.*bits"):
        qbits.awq_clip_search(w, h, 32, 5, False)
    with pytest.raises(RuntimeError, match="QBits.*n_cand"):
        qbits.awq_clip_search(w, h, 32, 4, False, n_grid=4, n_cand=5)
    with pytest.raises(RuntimeError, match="QBits"):
        qbits.awq_clip_search(w, h[:, :64], 32, 4, False)
    with pytest.raises(RuntimeError, match="QBits.*bits"):
        qbits.awq_scale_delta(w, torch.ones(128, device="cuda"), 32, 5, False)
    with pytest.raises(RuntimeError, match="QBits"):
        qbits.awq_scale_delta(w, torch.ones(64, device="cuda"), 32, 4, False)


# ---- the scale search end to end -----------------------------------------------------------------------------------
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("K,N,group", DELTA_SHAPES)
def test_scale_search_picks_the_reference_exponent(K, N, group, asym):
    from intel_extension_for_transformers_amd.transformers.llm.quantization.awq import search_scale

    w, X = A.salient(K, N, seed=K)
    H, a = A.stats(X)
    H, a = H.astype(np.float32), a.astype(np.float32)  # what the device is given
    ref = A.auto_scale([w], H, a, group, 4, asym)
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        best, s, losses = search_scale([_dev(w)], _dev(H), _dev(a), group, 4, asym)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
    srt = np.sort(ref["losses"])
    print("scale search K=%d N=%d group=%d asym=%d: best %d (reference %d), RTN / best %.2f, reference runner-up gap "
          "%.2e, largest |loss dev / ref - 1| %.2e" % (K, N, group, asym, best, ref["best"], losses[0] / losses[best],
                                                       (srt[1] - srt[0]) / srt[0],
                                                       np.abs(np.array(losses) / ref["losses"] - 1).max()))
    assert best == ref["best"] and best != 0
    assert np.allclose(s.cpu().numpy(), ref["s"], rtol=1e-5)
