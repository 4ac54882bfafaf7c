"""tests/h2o_reference.py checked without a GPU: against the rolling cache's oracle operation where H2O must equal it,
against RoPE's own algebra in float64, against a hand-written selection, and run as a whole chain on the CPU oracle."""
import numpy as np

from oracle import woq_oracle as orc
from tests import h2o_reference as H
from tests.test_gpu_streaming_engine import DISCARD, KEEP, _oracle_shift

CFG = dict(hidden=256, inter=512, heads=4, kv_heads=2, head_dim=64, layers=2, vocab=384, eps=1e-5, theta=10000.0, window=0)


class _Caches:
    """what `evict` and `_oracle_shift` touch of an oracle"""

    def __init__(self, k, v, theta):
        self.k, self.v, self.cfg = [a.copy() for a in k], [a.copy() for a in v], dict(theta=theta)


def test_recent_that_leaves_only_the_oldest_rows_is_the_streaming_shift():
    rng = np.random.default_rng(1)
    for n_cached, kv_heads, D in [(32, 2, 64), (37, 1, 128)]:
        k = [rng.standard_normal((n_cached, kv_heads, D)).astype(np.float32) for _ in range(2)]
        v = [rng.standard_normal((n_cached, kv_heads, D)).astype(np.float32) for _ in range(2)]
        score = rng.random((2, kv_heads, n_cached))  # whatever the scores: the range holds exactly n_discard rows
        got, want = _Caches(k, v, 10000.0), _Caches(k, v, 10000.0)
        keep = [H.select(score[li], KEEP, DISCARD, n_cached - KEEP - DISCARD, n_cached) for li in range(2)]
        assert all(not m[:, KEEP:KEEP + DISCARD].any() and m.sum() == kv_heads * (n_cached - DISCARD) for m in keep)
        H.evict(got, keep)
        _oracle_shift(want, 10000.0)
        for li in range(2):
            assert got.k[li].dtype == np.float32 and got.k[li].shape == (n_cached - DISCARD, kv_heads, D)
            assert np.array_equal(got.k[li], want.k[li]) and np.array_equal(got.v[li], want.v[li])


def test_rotating_back_by_the_distance_is_the_rotation_of_the_destination():
    """rope(rope(x, p), -(p - q)) == rope(x, q) with another q per head: what a per-head distance relies on"""
    rng = np.random.default_rng(2)
    for D in (64, 128):
        x = rng.standard_normal((40, 3, D))
        p = rng.integers(0, 4096, 40)
        q = np.minimum(p[:, None], rng.integers(0, 4096, (40, 3)))  # a row never moves up
        assert (q != q[:, :1]).any()
        back = H.rope64(H.rope64(x, p[:, None]), -(p[:, None] - q))
        want = H.rope64(x, q)
        assert np.abs(back - want).max() <= 1e-12 * np.abs(want).max()
        for h in range(3):  # per head, each against its own scale
            assert np.abs(back[:, h] - want[:, h]).max() <= 1e-12 * np.abs(want[:, h]).max()
        # rope64 is orc.rope in float64 (the fp32 oracle op: fp32 angles of up to 4096 rad, hence 1e-3)
        assert np.abs(H.rope64(x, p[:, None]) - orc.rope(x.astype(np.float32), p)).max() <= 1e-3 * np.abs(x).max()


def test_select_breaks_ties_towards_the_lower_row_and_ignores_what_lies_outside_the_range():
    #            row: 0  1  2  3  4  5  6  7  8  9
    score = np.array([[0, 5, 1, 1, 3, 1, 0, 1, 0, 0],    # ties inside the range and with rows outside it
                      [9, 9, 2, 2, 2, 2, 2, 2, 0, 0]], np.float32)
    keep = H.select(score, 2, 3, 2, 10)  # the range is rows 2 .. 7; rows 0, 1 (sinks) and 8, 9 (recent) always stay
    want = np.ones((2, 10), bool)
    want[0, [6, 2, 3]] = False  # 0 at row 6, then the 1s of rows 2, 3 (not those of rows 5, 7; never row 0's, 8's, 9's 0)
    want[1, [2, 3, 4]] = False  # all equal: the three lowest rows
    assert np.array_equal(keep, want)
    assert np.array_equal(H.select(score, 2, 6, 2, 10)[:, 2:8], np.zeros((2, 6), bool))  # the whole range
    keep = H.select(score, 0, 1, 0, 9)  # the edges of the range are the edges of the cache; row 9 is not cached
    assert keep.shape == (2, 9) and np.flatnonzero(~keep[0]).tolist() == [0] and np.flatnonzero(~keep[1]).tolist() == [8]


def _oracle_only(seed=3):
    """a LlamaOracle of the tiny engine model's configuration over blobs packed on the CPU"""
    rng = np.random.default_rng(seed)
    H_, I, NH, KV, D = CFG["hidden"], CFG["inter"], CFG["heads"], CFG["kv_heads"], CFG["head_dim"]
    layers = []
    for _ in range(CFG["layers"]):
        ly = {}
        for n, (k, nn) in dict(q=(H_, NH * D), k=(H_, KV * D), v=(H_, KV * D), o=(NH * D, H_), gate=(H_, I), up=(H_, I),
                               down=(I, H_)).items():
            q, s, z = orc.rtn_quantize(rng.standard_normal((k, nn)).astype(np.float32) * 0.05, False, 128, False)
            ly[n] = orc.repack(q, s, z, None, 128, scale_type=orc.F16)
        ly["ln1"] = (1 + 0.1 * rng.standard_normal(H_)).astype(np.float32)
        ly["ln2"] = (1 + 0.1 * rng.standard_normal(H_)).astype(np.float32)
        layers.append(ly)
    embed = rng.standard_normal((CFG["vocab"], H_)).astype(np.float16).astype(np.float32)
    lm = (rng.standard_normal((CFG["vocab"], H_)) * 0.1).astype(np.float16).astype(np.float32)
    return orc.LlamaOracle(CFG, embed, layers, (1 + 0.1 * rng.standard_normal(H_)).astype(np.float32), lm)


def test_an_h2o_chain_on_the_oracle_alone_evicts_on_schedule_and_keeps_its_books():
    """the harness of tests/test_gpu_h2o_chain.py without the device: the oracle feeds its own argmax, `select` reads
    the ScoreBook. The score mass is conserved: G per query, less what the evicted rows took with them."""
    oracle = _oracle_only()
    ctx, n_keep, n_discard, recent, prompt = 32, 4, 7, 5, [7, 300, 12, 45, 99, 3]
    L, KV, G = CFG["layers"], CFG["kv_heads"], CFG["heads"] // CFG["kv_heads"]
    evictions, queries, dropped, tokens = 0, len(prompt), np.zeros((L, KV)), []
    with H.ScoreBook(L, CFG["heads"], KV, CFG["head_dim"], ctx) as book:
        oracle.forward_prompt(prompt[:4], 0)
        tok, p = int(oracle.forward_prompt(prompt[4:], 4).argmax()), len(prompt)
        for _ in range(45):
            if p == ctx:
                keep = [H.select(book.score[li], n_keep, n_discard, recent, ctx) for li in range(L)]
                assert all(m[:, n_keep:n_keep + n_discard].any() for m in keep)  # not the rolling cache's choice
                dropped += np.array([[book.score[li, h, :ctx][~keep[li][h]].sum() for h in range(KV)] for li in range(L)])
                low = [[book.score[li, h, n_keep:ctx - recent][keep[li][h, n_keep:ctx - recent]].min() for h in range(KV)]
                       for li in range(L)]
                H.evict(oracle, keep)
                book.gather(keep)
                p -= n_discard
                evictions += 1
                for li in range(L):
                    assert oracle.k[li].shape == oracle.v[li].shape == (p, KV, CFG["head_dim"])
                    assert not book.score[li, :, p:].any() and (book.score[li, :, :p] > 0).all()
                    # what stayed inside the range scored no less than anything that went
                    assert all(book.score[li, h, n_keep:p - recent].min() == low[li][h] for h in range(KV))
            logits = oracle.forward_token(tok, p)
            assert np.isfinite(logits).all()
            tok, p, queries = int(logits.argmax()), p + 1, queries + 1
            tokens.append(tok)
    assert orc.attn_decode.__name__ == "attn_decode" and orc.attn_prompt.__name__ == "attn_prompt"  # the wrappers are gone
    assert evictions == 3 and book.calls == L * (2 + 45)  # before steps 26, 33 and 40
    assert np.abs(book.score.sum(-1) + dropped - G * queries).max() <= 1e-9 * G * queries
    assert len(set(tokens)) > 4
