"""Rolling KV cache (StreamingLLM; reference docs/streamingllm.md and Neural Speed's `ctx_size`, `n_keep`, `n_discard`):
the request's configuration and its schedule, host arithmetic only (no torch, no device).

The cache keeps the first `n_keep` positions as attention sinks. When it is full (`ctx_size` positions) and tokens remain,
the `n_discard` positions after the sinks are dropped, the later rows move down (`WoqDecoderEngine.kv_shift`, K rows
rotated back to their new positions) and generation goes on at position `ctx_size - n_discard`: positions are counted
inside the cache, as in the reference.
"""


class StreamingConfig:
    """`ctx_size` = positions the request may hold (None: the engine's max_ctx); `n_keep` = sink positions that are never
    dropped; `n_discard` = positions dropped per shift (-1: `(ctx_size - n_keep) // 2`, the reference's "half")."""

    def __init__(self, ctx_size=None, n_keep=4, n_discard=-1):
        self.ctx_size = None if ctx_size is None else int(ctx_size)
        self.n_keep = int(n_keep)
        self.n_discard = int(n_discard)

    def resolve(self, max_ctx, n_prompt=0):
        """(ctx_size, n_keep, n_discard) for an engine with `max_ctx` positions and a prompt of `n_prompt` tokens, or
        ValueError: 0 <= n_keep, 1 <= n_discard, n_keep + n_discard <= ctx_size <= max_ctx and n_prompt < ctx_size."""
        ctx = int(max_ctx) if self.ctx_size is None else self.ctx_size
        keep = self.n_keep
        if keep < 0:
            raise ValueError("QBits: streaming n_keep (%d) must be >= 0" % keep)
        disc = (ctx - keep) // 2 if self.n_discard == -1 else self.n_discard
        if disc < 1:
            raise ValueError("QBits: streaming n_discard (%d) must be >= 1 (ctx_size %d, n_keep %d)" % (disc, ctx, keep))
        if keep + disc > ctx:
            raise ValueError("QBits: streaming n_keep (%d) + n_discard (%d) exceeds ctx_size (%d)" % (keep, disc, ctx))
        if ctx > int(max_ctx):
            raise ValueError("QBits: streaming ctx_size (%d) exceeds the engine's max_ctx (%d)" % (ctx, int(max_ctx)))
        if int(n_prompt) >= ctx:
            raise ValueError("QBits: prompt (%d) does not fit below the streaming ctx_size (%d)" % (int(n_prompt), ctx))
        return ctx, keep, disc

    def __repr__(self):
        return "StreamingConfig(ctx_size=%r, n_keep=%r, n_discard=%r)" % (self.ctx_size, self.n_keep, self.n_discard)


class H2OConfig(StreamingConfig):
    """H2O heavy-hitter eviction (reference kv_cache_compression/prune/h2o.py, docs/h2o.md) as a request option beside the
    rolling cache: the same `ctx_size`, `n_keep`, `n_discard` and schedule (`plan_stream`), but when the cache is full
    every (layer, kv head) drops the `n_discard` rows that received the least attention so far among rows
    `[n_keep, ctx_size - recent)`, ties to the older row (`WoqDecoderEngine.h2o_evict`). `recent` = the newest rows that
    are never dropped: a count, a ratio of `ctx_size` (a float below 1), or -1 = half of what `n_keep` and `n_discard`
    leave. `recent == ctx_size - n_keep - n_discard` is the rolling cache itself.

    `heavy_ratio` / `recent_ratio`: the reference's ratio spelling as remembered — UNVERIFIED against the reference tree,
    which this project has no copy of. Given (both), they set `recent = recent_ratio * ctx_size` and
    `n_discard = ctx_size - n_keep - recent - heavy_ratio * ctx_size`."""

    def __init__(self, ctx_size=None, n_keep=4, n_discard=-1, recent=-1, heavy_ratio=None, recent_ratio=None):
        StreamingConfig.__init__(self, ctx_size, n_keep, n_discard)
        if (heavy_ratio is None) != (recent_ratio is None):
            raise ValueError("QBits: H2O heavy_ratio and recent_ratio come together")
        self.recent = recent
        self.heavy_ratio = None if heavy_ratio is None else float(heavy_ratio)
        self.recent_ratio = None if recent_ratio is None else float(recent_ratio)

    def resolve(self, max_ctx, n_prompt=0):
        """(ctx_size, n_keep, n_discard, recent), or ValueError: StreamingConfig's rule, plus recent >= 0 and
        n_keep + n_discard + recent <= ctx_size."""
        ctx = int(max_ctx) if self.ctx_size is None else self.ctx_size
        disc, recent = self.n_discard, self.recent
        if self.heavy_ratio is not None:
            recent = int(self.recent_ratio * ctx)
            disc = ctx - self.n_keep - recent - int(self.heavy_ratio * ctx)
            if disc == -1:  # (-1 means "half" to the base rule; here it is a budget that does not fit)
                disc = -2
        ctx, keep, disc = StreamingConfig(ctx, self.n_keep, disc).resolve(max_ctx, n_prompt)
        if isinstance(recent, float) and recent < 1.0:
            recent = int(recent * ctx)
        recent = (ctx - keep - disc) // 2 if recent == -1 else int(recent)
        if recent < 0:
            raise ValueError("QBits: H2O recent (%d) must be >= 0" % recent)
        if keep + disc + recent > ctx:
            raise ValueError("QBits: H2O n_keep (%d) + n_discard (%d) + recent (%d) exceeds ctx_size (%d)"
                             % (keep, disc, recent, ctx))
        return ctx, keep, disc, recent

    def __repr__(self):
        return "H2OConfig(ctx_size=%r, n_keep=%r, n_discard=%r, recent=%r, heavy_ratio=%r, recent_ratio=%r)" % (
            self.ctx_size, self.n_keep, self.n_discard, self.recent, self.heavy_ratio, self.recent_ratio)


def h2o_from_keywords(h2o_config=None, ctx_size=None, n_keep=None, n_discard=None, recent=None, heavy_ratio=None,
                      recent_ratio=None):
    """An H2OConfig from `h2o_config` (an H2OConfig, or a dict of its arguments) or from the keywords; None when neither
    `h2o_config`, `recent` nor the ratios are given."""
    if isinstance(h2o_config, H2OConfig):
        return h2o_config
    if h2o_config is not None:
        return H2OConfig(**dict(h2o_config))
    if recent is None and heavy_ratio is None and recent_ratio is None:
        return None
    return H2OConfig(ctx_size, 4 if n_keep is None else n_keep, -1 if n_discard is None else n_discard,
                     -1 if recent is None else recent, heavy_ratio, recent_ratio)


def streaming_from_keywords(ctx_size=None, n_keep=None, n_discard=None, h2o_config=None, recent=None, heavy_ratio=None,
                            recent_ratio=None):
    """Neural Speed's three generate keywords -> a StreamingConfig, or None when none of them is given. With `h2o_config`
    (an H2OConfig or a dict of its arguments), `recent` or the two ratios: an H2OConfig (`h2o_from_keywords`)."""
    h2o = h2o_from_keywords(h2o_config, ctx_size, n_keep, n_discard, recent, heavy_ratio, recent_ratio)
    if h2o is not None:
        return h2o
    if ctx_size is None and n_keep is None and n_discard is None:
        return None
    return StreamingConfig(ctx_size, 4 if n_keep is None else n_keep, -1 if n_discard is None else n_discard)


def plan_stream(n_prompt, max_new_tokens, ctx_size=None, n_keep=0, n_discard=0, burst=16):
    """The decode schedule of one request after its prompt pass (which produced the first new token and left
    `n_prompt` rows in the cache): yields `("burst", p0, k)` = k chained steps, the first of which feeds cache position
    p0 (their tokens are token-log slots p0 .. p0 + k - 1), and `("shift", n_cached)` = drop `n_discard` positions
    after the `n_keep` sinks of a cache that holds `n_cached` rows; the next burst starts at `n_cached - n_discard`.
    `ctx_size` = None: no rolling cache, the plain bursts of `burst` steps. Otherwise a burst is clipped so that
    p0 + k <= ctx_size, and a shift is planned only when the cache is full (n_cached == ctx_size) and tokens remain.
    The burst sizes sum to max_new_tokens - 1; clipping changes where bursts end, never which steps run."""
    burst = max(1, int(burst))
    left = int(max_new_tokens) - 1
    p = int(n_prompt)
    if ctx_size is not None:
        ctx_size, n_keep, n_discard = int(ctx_size), int(n_keep), int(n_discard)
        if not (n_keep >= 0 and n_discard >= 1 and n_keep + n_discard <= ctx_size and p < ctx_size):
            raise ValueError("QBits: plan_stream needs 0 <= n_keep, 1 <= n_discard, n_keep + n_discard <= ctx_size "
                             "and n_prompt < ctx_size")
    while left > 0:
        k = min(burst, left)
        if ctx_size is not None:
            if p == ctx_size:
                yield ("shift", p)
                p -= n_discard
            k = min(k, ctx_size - p)
        yield ("burst", p, k)
        p += k
        left -= k


def plan_steps(plan):
    """A plan step by step: `("shift", n_cached)` as it stands, every burst as k `("step", p)` entries."""
    for ev in plan:
        if ev[0] == "burst":
            for j in range(ev[2]):
                yield ("step", ev[1] + j)
        else:
            yield ev
