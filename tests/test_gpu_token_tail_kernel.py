"""The greedy token tail alone (csrc/woq_ops.hip): `lm_head_kernel` with its per-workgroup (max, index) pairs, the three
argmax tails (`argmax_kernel` over logits and over pairs, `argmax_embed_kernel`) and `embed_kernel`, through
`woq_probe_lm_head` / `woq_probe_greedy_tail` / `woq_probe_embed`, against float64 (tests/xq_reference.py).

Inputs, seed 0: hidden state N(0, 1) with one element times 30, norm weights 1 + 0.1 N(0, 1), head weights of sigma 0.08,
embedding rows N(0, 1) * 0.5. The non-finite cases run through the probes only: no embedding row is ever looked up with
an unguarded token.
"""
import functools

import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from tests import xq_reference as X

pytestmark = pytest.mark.gpu

EPS, SENT = 1e-5, 777.0
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
# hidden 256: lanes 32..63 of the 512-element stride idle; 576: the second stride partial. vocab 16: one workgroup;
# 17: the second holds one row, three of its waves none; 1000: ragged against 16
LM_CASES = [(256, 16, "fp16"), (256, 17, "fp16"), (256, 17, "bf16"), (576, 17, "fp16"), (576, 1000, "fp16"),
            (256, 2500, "fp16"), (4096, 1000, "fp16"), (4096, 2500, "fp16"), (4096, 2500, "bf16")]


@functools.lru_cache(maxsize=None)
def _head(hidden, vocab, kind):
    rng = np.random.default_rng(0)
    x = rng.standard_normal(hidden).astype(np.float32)
    x[hidden // 3] *= 30
    norm_w = (1 + 0.1 * rng.standard_normal(hidden)).astype(np.float32)
    W = torch.from_numpy((0.08 * rng.standard_normal((vocab, hidden))).astype(np.float32)).to(DTYPES[kind])
    return x, norm_w, W


def _dev(a):
    return None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def _lm_head(x, norm_w, W, pairs=True):
    """-> (logits [vocab], pmax, pidx [(vocab + 15) / 16]); the memory behind each keeps its sentinel"""
    vocab, n = W.shape[0], (W.shape[0] + 15) // 16
    logits = torch.full((vocab + 5,), SENT, device="cuda")
    pmax = torch.full((n + 3,), SENT, device="cuda")
    pidx = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
    L.probe_lm_head(_dev(x), _dev(norm_w), EPS, _dev(W), logits, pmax if pairs else None, pidx if pairs else None)
    torch.cuda.synchronize()
    lg, pm, pi = logits.cpu().numpy(), pmax.cpu().numpy(), pidx.cpu().numpy()
    assert (lg[vocab:] == SENT).all(), "logits written past vocab"
    assert (pm[n if pairs else 0:] == SENT).all() and (pi[n if pairs else 0:] == -7).all(), "pairs written past the last"
    return lg[:vocab], pm[:n], pi[:n]


def _pairs_of(lg):
    """(max, lowest argmax) of every 16 logits; a group without a number: (-inf, 0x7fffffff)"""
    pm, pi = [], []
    for s in range(0, len(lg), 16):
        blk = lg[s:s + 16]
        ok = ~np.isnan(blk) & (blk > -np.inf)
        if ok.any():
            m = blk[ok].max()
            pm.append(m)
            pi.append(s + int(np.flatnonzero(ok & (blk == m))[0]))
        else:
            pm.append(-np.inf)
            pi.append(0x7FFFFFFF)
    return np.array(pm, np.float32), np.array(pi, np.int64)


@pytest.mark.parametrize("hidden,vocab,kind", LM_CASES)
def test_lm_head_against_float64(hidden, vocab, kind):
    x, norm_w, W = _head(hidden, vocab, kind)
    want = X.lm_head_f64(x, norm_w, EPS, W)
    a = X.lm_head_tolerance_terms(x, norm_w, EPS, W)
    lg, pm, pi = _lm_head(x, norm_w, W)
    worst = float(np.abs(lg - want).max())
    print("lm_head hidden %d vocab %d %s: A = %.3e, tolerance = %.3e, max |logit - float64| = %.3e (ratio %.3f)" % (
        hidden, vocab, kind, a, 4 * a, worst, worst / (4 * a)))
    assert 0 < a < 1e-3
    assert worst <= 4 * a
    wm, wi = _pairs_of(lg)
    assert np.array_equal(pm, wm) and np.array_equal(pi, wi)  # exactly, of the kernel's own logits
    lg2, _, _ = _lm_head(x, norm_w, W, pairs=False)  # without pairs: the same logits, nothing else written
    assert np.array_equal(lg, lg2)


def _tail(mode, vocab, logits=None, pmax=None, pidx=None, pos=3, max_ctx=64, embed=None, norm_w=None, status0=0):
    """one greedy tail -> dict(token, pos, log, status, step_seq, out, xo, ssq)"""
    token = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    posd = torch.full((1,), pos, dtype=torch.int32, device="cuda")
    log = torch.full((max_ctx + 2,), -9, dtype=torch.int32, device="cuda")
    status = torch.full((1,), status0, dtype=torch.int32, device="cuda")
    seq = torch.full((1,), 41, dtype=torch.int32, device="cuda")
    kw = {}
    if mode == 2:
        hidden = embed.shape[1]
        kw = dict(embed=embed, out=torch.full((hidden + 16,), SENT, device="cuda"), step_seq=seq, max_ctx=max_ctx)
        if norm_w is not None:
            kw.update(norm_w=norm_w, ssq_out=torch.full((hidden // 16 + 4,), SENT, device="cuda"),
                      xo=(torch.full((L.xq_limb_bytes(hidden),), 0x5A, dtype=torch.uint8, device="cuda"),
                          torch.full((hidden // 16 + 4,), SENT, device="cuda"),
                          torch.full((hidden // 16 + 4,), SENT, device="cuda")))
    L.probe_greedy_tail(mode, vocab, token, posd, logits=logits, pmax=pmax, pidx=pidx,
                        log=None if mode == 0 else log, status=None if mode == 0 else status, **kw)
    torch.cuda.synchronize()
    return dict(token=int(token.item()), pos=int(posd.item()), log=log.cpu().numpy(), status=int(status.item()),
                step_seq=int(seq.item()), **{k: v for k, v in kw.items() if k in ("out", "xo", "ssq_out")})


@functools.lru_cache(maxsize=None)
def _table(hidden, kind, rows=100):
    rng = np.random.default_rng(0)
    embed = torch.from_numpy((0.5 * rng.standard_normal((rows, hidden))).astype(np.float32)).to(DTYPES[kind])
    return embed, (1 + 0.1 * rng.standard_normal(hidden)).astype(np.float32)


def _all_tails(lg, pm, pi, want_token, want_status=0, what=""):
    """modes 0 (where it applies), 1 and 2 on the same logits / pairs: one token, the log, the position"""
    vocab = len(lg)
    embed, _ = _table(256, "fp16")
    res = {}
    if want_status == 0:
        res[0] = _tail(0, vocab, logits=_dev(lg))
    res[1] = _tail(1, vocab, pmax=_dev(pm), pidx=_dev(pi.astype(np.int32)))
    res[2] = _tail(2, vocab, pmax=_dev(pm), pidx=_dev(pi.astype(np.int32)), embed=_dev(embed))
    for mode, r in res.items():
        assert r["token"] == want_token, (what, mode, r["token"])
        assert r["pos"] == 4, (what, mode)
        if mode:
            assert r["log"][3] == want_token and (np.delete(r["log"], 3) == -9).all(), (what, mode)
            assert r["status"] == want_status, (what, mode, r["status"])
        else:
            assert (r["log"] == -9).all()
    assert res[2]["step_seq"] == 42 and res[1]["step_seq"] == 41
    return res


# ---- tie rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,where", [(33, 37, "one wave's row set"), (34, 35, "two waves of one workgroup"),
                                       (21, 70, "two workgroups")])
def test_ties_go_to_the_lowest_index(a, b, where):
    """rows a and b of the head are the same row, scaled so that they hold the largest logit"""
    x, norm_w, W = _head(256, 100, "fp16")
    base = X.lm_head_f64(x, norm_w, EPS, W)
    W = W.clone()
    W[a] = W[int(np.argmax(base))] * 2  # exact in fp16 here (no overflow at sigma 0.08): the largest logit, twice over
    W[b] = W[a]
    lg, pm, pi = _lm_head(x, norm_w, W)
    assert lg[a].tobytes() == lg[b].tobytes(), "the duplicated rows' logits are not bitwise equal"
    assert int(np.argmax(lg)) == a
    _all_tails(lg, pm, pi, a, what=where)
    # and the other way round within a workgroup's pairs: the lower index listed second still wins
    _all_tails(lg, pm[::-1].copy(), pi[::-1].copy(), a, what=where + " (pairs reversed)")


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("p,q,where", [(5, 9, "one wave"), (5, 70, "two waves"), (5, 5 + 1024, "one thread, two passes"),
                                       (700, 5 + 256, "mode 2: one thread, mode 1: two waves"), (2099, 3, "far apart")])
def test_tie_rule_over_many_candidates(p, q, where, order):
    """2100 candidates (more than one pass of the 1024- and the 256-thread reductions), the largest value at positions
    p and q; candidate indices ascending with the position or descending, so that the lower index is met first or
    last: every tail returns the lower index"""
    n = 2100
    rng = np.random.default_rng(0)
    pm = rng.standard_normal(n).astype(np.float32)
    pm[p] = pm[q] = 9.0
    at = np.arange(n) if order == "ascending" else np.arange(n)[::-1]
    pi = (16 * at + 3).astype(np.int32)
    want = int(min(pi[p], pi[q]))
    embed = torch.zeros(16 * n, 16, dtype=torch.float16, device="cuda")  # a row for every index mode 2 could pick
    for mode in (1, 2):
        r = _tail(mode, 16 * n, pmax=_dev(pm), pidx=_dev(pi), embed=embed if mode == 2 else None)
        assert r["token"] == want, (where, mode, r["token"])
    if order == "ascending":  # mode 0: candidate i is logit i
        r = _tail(0, n, logits=_dev(pm))
        assert r["token"] == min(p, q), (where, r["token"])


# ---- non-finite logits -------------------------------------------------------------------------------------------------
def test_nan_rows_are_skipped_and_a_nan_workgroup_loses():
    x, norm_w, W = _head(256, 100, "fp16")
    W = W.clone()
    W[5, 7] = float("nan")    # one row of workgroup 0
    W[32:48] = float("nan")   # all of workgroup 2
    lg, pm, pi = _lm_head(x, norm_w, W)
    assert np.isnan(lg[5]) and np.isnan(lg[32:48]).all() and np.isfinite(np.delete(lg, [5] + list(range(32, 48)))).all()
    wm, wi = _pairs_of(lg)
    assert np.array_equal(pm, wm) and np.array_equal(pi, wi)
    assert pi[2] == 0x7FFFFFFF and np.isneginf(pm[2]) and pi[0] != 5
    _all_tails(lg, pm, pi, int(np.nanargmax(lg)), what="NaN rows")


@pytest.mark.parametrize("fill", [float("nan"), float("-inf")], ids=["nan", "-inf"])
def test_no_winner_gives_token_0_and_status_bit_2_in_both_tails(fill):
    """every logit NaN, every logit -inf: the eager tail (mode 1) and the chained tail (mode 2) agree — token 0, status
    |= 4; the embedding row that mode 2 reads is row 0"""
    vocab = 100
    if np.isnan(fill):
        x, norm_w, W = _head(256, vocab, "fp16")
        x = x.copy()
        x[11] = np.nan  # the norm makes every logit NaN
        lg, pm, pi = _lm_head(x, norm_w, W)
        assert np.isnan(lg).all()
    else:
        lg = np.full(vocab, -np.inf, np.float32)
        pm, pi = _pairs_of(lg)
    assert (pi == 0x7FFFFFFF).all() and np.isneginf(pm).all()
    res = _all_tails(lg, pm, pi, 0, want_status=4, what="no winner")
    embed, _ = _table(256, "fp16")
    assert np.array_equal(res[2]["out"].cpu().numpy()[:256], embed[0].float().numpy())
    # the sticky status keeps earlier bits
    r = _tail(1, vocab, pmax=_dev(pm), pidx=_dev(pi.astype(np.int32)), status0=2)
    assert r["status"] == 6 and r["token"] == 0
    # mode 0 (the prompt pass's tail over logits) follows the same rule for the token
    token, posd = torch.full((1,), -5, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    L.probe_greedy_tail(0, vocab, token, posd, logits=_dev(lg))
    torch.cuda.synchronize()
    assert int(token.item()) == 0 and int(posd.item()) == 1


# ---- bookkeeping -------------------------------------------------------------------------------------------------------
def test_position_clamp_and_step_sequence():
    x, norm_w, W = _head(256, 100, "fp16")
    lg, pm, pi = _lm_head(x, norm_w, W)
    want = int(np.argmax(lg))
    embed, _ = _table(256, "fp16")
    pairs = dict(pmax=_dev(pm), pidx=_dev(pi.astype(np.int32)))
    r = _tail(2, 100, pos=63, max_ctx=64, embed=_dev(embed), **pairs)  # pos + 1 reaches max_ctx: clamped, flagged
    assert (r["token"], r["pos"], r["status"], r["step_seq"]) == (want, 63, 2, 42) and r["log"][63] == want
    r = _tail(2, 100, pos=62, max_ctx=64, embed=_dev(embed), **pairs)
    assert (r["token"], r["pos"], r["status"], r["step_seq"]) == (want, 63, 0, 42) and r["log"][62] == want
    r = _tail(1, 100, pos=0, **pairs)
    assert (r["token"], r["pos"], r["status"]) == (want, 1, 0) and r["log"][0] == want


# ---- embedding ---------------------------------------------------------------------------------------------------------
def _check_embedding(out, xo, ssq, row, norm_w, what):
    hidden = row.size
    o = out.cpu().numpy()
    assert np.array_equal(o[:hidden], row) and (o[hidden:] == SENT).all(), what
    if norm_w is None:
        return
    nb = hidden // 16
    limbs, u, sx = (t.cpu().numpy() for t in xo)
    want = X.encode((row * norm_w).astype(np.float32))
    assert np.array_equal(limbs[:nb * 48].view(np.int8).reshape(nb, 3, 16), want[0]), what
    assert np.array_equal(u[:nb], want[1]) and np.array_equal(sx[:nb], want[2]), what
    assert (limbs[nb * 48:] == 0x5A).all() and (u[nb:] == SENT).all() and (sx[nb:] == SENT).all(), what
    s = ssq.cpu().numpy()
    ref = X.block_ssq(row)
    assert (np.abs(s[:nb] - ref) <= X.SSQ_REL * ref).all() and (s[nb:] == SENT).all(), what


@pytest.mark.parametrize("with_xq", [True, False])
@pytest.mark.parametrize("kind", ["fp16", "bf16"])
@pytest.mark.parametrize("hidden", [256, 576])
def test_embedding_row_and_its_xq_form(hidden, kind, with_xq):
    """hidden 256: one workgroup of 256 columns; 576: three, the last partial. Mode 2 and woq_probe_embed."""
    embed, norm_w = _table(hidden, kind)
    g = norm_w if with_xq else None
    lgx, lgn, W = _head(256, 24, "fp16")
    lg, pm, pi = _lm_head(lgx, lgn, W)
    tok = int(np.argmax(lg))
    row = embed[tok].float().numpy()
    r = _tail(2, 24, pmax=_dev(pm), pidx=_dev(pi.astype(np.int32)), embed=_dev(embed), norm_w=_dev(g))
    assert r["token"] == tok and r["step_seq"] == 42
    _check_embedding(r["out"], r.get("xo"), r.get("ssq_out"), row, g, "mode 2 hidden %d %s" % (hidden, kind))
    # embed_kernel: the head of a step
    for pos, max_ctx, want_pos, want_status in ((5, 64, 5, 0), (64, 64, 63, 2), (70, 64, 63, 2)):
        out = torch.full((hidden + 16,), SENT, device="cuda")
        nb = hidden // 16
        xo = (torch.full((L.xq_limb_bytes(hidden),), 0x5A, dtype=torch.uint8, device="cuda"),
              torch.full((nb + 4,), SENT, device="cuda"), torch.full((nb + 4,), SENT, device="cuda")) if with_xq else None
        ssq = torch.full((nb + 4,), SENT, device="cuda") if with_xq else None
        seq = torch.full((1,), 41, dtype=torch.int32, device="cuda")
        posd = torch.full((1,), pos, dtype=torch.int32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        token = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        L.probe_embed(_dev(embed), token, out, norm_w=_dev(g), xo=xo, ssq_out=ssq, step_seq=seq, pos=posd,
                      max_ctx=max_ctx, status=status)
        torch.cuda.synchronize()
        assert (int(posd.item()), int(status.item()), int(seq.item()), int(token.item())) == (want_pos, want_status, 42, 7)
        _check_embedding(out, xo, ssq, embed[7].float().numpy(), g, "embed hidden %d %s pos %d" % (hidden, kind, pos))
