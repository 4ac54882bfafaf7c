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


def streaming_from_keywords(ctx_size=None, n_keep=None, n_discard=None):
    """Neural Speed's three generate keywords -> a StreamingConfig, or None when none of them is given."""
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
