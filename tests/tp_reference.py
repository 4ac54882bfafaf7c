"""Reference for the tensor-parallel exchange kernels (csrc/woq_comm.hip): numpy, the kernels' own specification.

`rank_ordered_sum`: allreduce_ll_kernel starts every element at fp32 0 and adds the ranks' values in rank order, each
add rounded to fp32 — `(fl32(0) + x_0) + x_1 ...`. fp32 addition of two fp32 values is correctly rounded in numpy and
on the device alike, so the comparison is bit for bit (NaN-ness where the sum is NaN: the payload is not specified).
Starting from +0 matters: `(+0) + (-0) = +0`, so a column every rank holds at -0 leaves as +0.

`greedy_pick`: tp_greedy_kernel's rule over the ranks' (max, local index) pairs — a pair takes part with the global
index `local + vocab_offset` unless its index is the 0x7fffffff sentinel (lm_head_kernel's "no number in these 16
rows"); the winner is the highest value, the lowest global index among equals; NaN never wins. No winner (nothing but
NaN, or -inf under the sentinel): token 0 and status bit 2 (value 4), the rule of the single-GPU tails.
`pairs_of` restates how lm_head_kernel folds 16 logits into one pair, so that a CPU test can hold `greedy_pick` to a
brute-force argmax over the whole row.
"""
import numpy as np

F32 = np.float32
SENTINEL = 0x7FFFFFFF
STATUS_NO_WINNER = 4


def rank_ordered_sum(xs):
    """xs: the ranks' fp32 vectors in rank order -> fp32 (0 + x_0) + x_1 + ..."""
    acc = np.zeros(np.asarray(xs[0]).shape, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for x in xs:
            x = np.asarray(x)
            assert x.dtype == F32
            acc = acc + x  # fp32 + fp32 -> fp32, round to nearest even
    assert acc.dtype == F32
    return acc


def same_bits(got, want):
    """bit for bit where `want` is a number or an infinity, NaN for NaN"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return bool(got.shape == want.shape and np.array_equal(np.isnan(got), nan)
                and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def specials(world=2):
    """-> `world` fp32 vectors whose element-wise rank-ordered sums walk the edges of fp32 addition: signed zeros,
    subnormals, the largest finite values (a pair that overflows, a pair that cancels), infinities of one and of both
    signs, NaN on either rank. Ranks beyond the second hold +0 (-0 in the all-minus-zero column)."""
    big, tiny, sub = np.finfo(F32).max, np.finfo(F32).tiny, F32(1e-42)
    least = np.nextafter(F32(0), F32(1))
    inf, nan = F32(np.inf), F32(np.nan)
    cols = [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (sub, sub), (sub, -sub), (-sub, -sub), (least, least),
            (least, -least), (tiny, -least), (tiny, -tiny), (big, big), (-big, -big), (big, -big), (big, 1.0),
            (big, F32(2.0 ** 103)), (big, F32(2.0 ** 102)), (inf, 1.0), (1.0, -inf), (inf, inf), (-inf, -inf),
            (inf, -inf), (-inf, inf), (inf, -big), (nan, 1.0), (1.0, nan), (nan, nan), (nan, inf), (1.0, -1.0),
            (1.0, F32(2.0 ** -24)), (1.0, F32(2.0 ** -24 + 2.0 ** -40)), (-1.5, sub)]
    out = [np.array([c[min(r, 1)] if r < 2 else 0.0 for c in cols], F32) for r in range(world)]
    for r in range(2, world):
        out[r][1] = -0.0
    return out


def pairs_of(logits, offset=0):
    """(max, lowest local index of it) of every 16 logits, as lm_head_kernel leaves them; a group without a number above
    -inf: (-inf, sentinel)"""
    lg = np.asarray(logits, F32)
    pm, pi = [], []
    for s in range(0, lg.size, 16):
        blk = lg[s:s + 16]
        ok = ~np.isnan(blk) & (blk > -np.inf)
        if ok.any():
            m = blk[ok].max()
            pm.append(m)
            pi.append(offset + s + int(np.flatnonzero(ok & (blk == m))[0]))
        else:
            pm.append(-np.inf)
            pi.append(SENTINEL)
    return np.array(pm, F32), np.array(pi, np.int32)


def greedy_pick(pmax, pidx, offsets):
    """pmax / pidx: per rank fp32 / int32 arrays of pairs, offsets: per rank vocab_offset -> (token, status bits)"""
    best, tok = -np.inf, SENTINEL
    for pm, pi, off in zip(pmax, pidx, offsets):
        for v, i in zip(np.asarray(pm, F32).tolist(), np.asarray(pi).tolist()):
            g = i if i == SENTINEL else i + int(off)
            if v > best or (v == best and g < tok):  # NaN compares false both ways
                best, tok = v, g
    if tok < 0 or tok == SENTINEL:
        return 0, STATUS_NO_WINNER
    return tok, 0
