"""H2O heavy-hitter eviction (csrc/woq_h2o.hip, `Engine.h2o_evict`) restated in plain numpy, for the CPU oracle
(`oracle.woq_oracle.LlamaOracle`): which rows go (`select`), what the cache holds afterwards (`evict`) and the attention
each cached row has received (`ScoreBook`). No GPU code and nothing of the runtime: the GPU tests hold the engine to
this, and tests/test_h2o_reference_cpu.py holds this to the rolling cache's reference and to RoPE's own algebra.

Rows of one (layer, kv head) keep their order when they move down, and a K row that moves from row `src` to row `dst`
is rotated back by `src - dst` positions, so that it carries the rotation of the row it now sits in. After an eviction
every kv head holds another set of rows, hence the rotation per row AND per head."""
import numpy as np

from oracle import woq_oracle as orc


def select(score, n_keep, n_discard, recent, n_cached):
    """score [kv_heads, >= n_cached] -> bool keep mask [kv_heads, n_cached]: per head the `n_discard` lowest scores
    among rows [n_keep, n_cached - recent) go; a stable argsort, so of equal scores the lower row goes first."""
    score = np.asarray(score)
    lo, hi = n_keep, n_cached - recent
    assert 0 <= lo and n_discard >= 1 and lo + n_discard <= hi <= n_cached <= score.shape[1]
    keep = np.ones((score.shape[0], n_cached), bool)
    for h in range(score.shape[0]):
        keep[h, lo + np.argsort(score[h, lo:hi], kind="stable")[:n_discard]] = False
    return keep


def rope64(x, pos, theta=10000.0):
    """`orc.rope` in float64 with a position per leading index: x [..., D], pos broadcastable to x.shape[:-1]. The pair
    (d, d + D/2) turns by pos * theta^(-2 d / D)."""
    x = np.asarray(x, np.float64)
    half = x.shape[-1] // 2
    ang = np.asarray(pos, np.float64)[..., None] * theta ** (-2.0 * np.arange(half) / x.shape[-1])
    c, s = np.cos(ang), np.sin(ang)
    a, b = x[..., :half], x[..., half:]
    return np.concatenate([a * c - b * s, b * c + a * s], -1)


def moved(keep_row):
    """one head's keep mask -> (src, dst): the kept rows in order and the rows they land in"""
    src = np.flatnonzero(keep_row)
    return src, np.arange(src.size)


def evict(oracle, keep):
    """Apply keep[layer][kv head] (bool over the cached rows) to the oracle's caches `oracle.k[li]` / `oracle.v[li]`
    ([rows, kv_heads, D]): V rows gathered, K rows gathered and rotated by -(src - dst), one head's column at a time
    through `orc.rope` (a row that stays where it is is not touched). Every head must keep the same number of rows."""
    theta = oracle.cfg["theta"]
    for li in range(len(oracle.k)):
        k, v = oracle.k[li], oracle.v[li]
        assert np.shape(keep[li]) == (k.shape[1], k.shape[0]), (np.shape(keep[li]), k.shape)
        ks, vs = [], []
        for h in range(k.shape[1]):
            src, dst = moved(keep[li][h])
            col = np.array(k[src, h:h + 1], np.float32)
            far = src != dst
            if far.any():
                col[far] = orc.rope(col[far], -(src - dst)[far], theta)
            ks.append(col)
            vs.append(np.array(v[src, h:h + 1], np.float32))
        assert len({c.shape[0] for c in ks}) == 1, "every kv head keeps the same number of rows"
        oracle.k[li], oracle.v[li] = np.concatenate(ks, 1), np.concatenate(vs, 1)


class ScoreBook:
    """The H2O score of the oracle: while entered, `orc.attn_decode` and `orc.attn_prompt` also add the float64 softmax
    probability every cached row receives, summed over the queries of the call and the query heads of a kv group, to
    `score[layer, kv head, row]`. The layer is the call's index modulo `layers` (the oracle attends once per layer, in
    order). `logit` is the largest |q . k / sqrt(D)| seen, `calls` the attention calls counted. `gather(keep)` compacts the
    scores as an eviction compacts the cache."""

    def __init__(self, layers, heads, kv_heads, head_dim, rows):
        self.layers, self.kv_heads, self.group, self.head_dim = layers, kv_heads, heads // kv_heads, head_dim
        self.score = np.zeros((layers, kv_heads, rows))
        self.calls, self.logit = 0, 0.0
        self._saved = None

    def add(self, q, k, start):
        """q [T, heads, D] at positions start .. start + T - 1 over cache rows k [n, kv_heads, D]"""
        li, T, n = self.calls % self.layers, q.shape[0], k.shape[0]
        self.calls += 1
        s = np.einsum("tkgd,pkd->kgtp", q.reshape(T, self.kv_heads, self.group, self.head_dim).astype(np.float64),
                      k.astype(np.float64)) / np.sqrt(self.head_dim)
        vis = np.arange(n)[None, :] <= start + np.arange(T)[:, None]
        self.logit = max(self.logit, float(np.abs(s[..., vis]).max()))
        p = np.exp(np.where(vis, s, -np.inf))
        self.score[li, :, :n] += (p / p.sum(-1, keepdims=True)).sum((1, 2))

    def gather(self, keep):
        """keep[layer][kv head]: bool over the first n rows -> the kept scores move down in order, the rest is zero"""
        for li in range(self.layers):
            for h in range(self.kv_heads):
                src, dst = moved(keep[li][h])
                row = self.score[li, h].copy()
                self.score[li, h] = 0.0
                self.score[li, h, dst] = row[src]

    def __enter__(self):
        assert self._saved is None
        dec, pro = self._saved = (orc.attn_decode, orc.attn_prompt)
        orc.attn_decode = lambda q, k, v: (self.add(q[None], k, k.shape[0] - 1), dec(q, k, v))[1]
        orc.attn_prompt = lambda q, k, v, start, window=0: (self.add(q, k, start), pro(q, k, v, start, window))[1]
        return self

    def __exit__(self, *exc):
        orc.attn_decode, orc.attn_prompt = self._saved
        self._saved = None
        return False
