"""One request on the decode engine: prompt pass, first token, bursts of decode steps, a rolling KV cache between them.

Free functions over an engine (`WoqDecoderEngine`, or anything with its methods). Two drivers, because there are two
mechanisms: the CHAINED driver (`iter_generate`) lets the device chain token and position and reads the token log once
per burst; the HOST-FED driver (`iter_sampled`) runs logits-only steps, picks every token with a torch `DeviceSampler`
and sets the position itself. What they share is written once: the request scope (`_request`), the prompt pass, the
`logprobs` check, the record formatting and the eos cut. `generate`, `generate_sampled` and `iter_sampled_auto` are
built on the two iterators; so are `model.generate` (transformers/modeling/modeling_auto.py) and NeuralChat's stream
(neural_chat/models/base_model.py).
"""
import torch

from .. import _lib as L
from .streaming import plan_steps, plan_stream


# ---- the shared pieces ------------------------------------------------------------------------------------------------
def _request(engine, driver, prompt_ids, max_new_tokens, logprobs, streaming, *args):
    """The scope of one request around `driver(engine, ids, max_new_tokens, geometry, n_top, *args)`: everything that can
    refuse the request is checked before anything is launched, and with a rolling cache the request counts its dropped
    positions from 0 and leaves 0 behind however it ends (exhausted, closed, an exception) — one without `streaming`
    always runs with 0."""
    n_top = None if logprobs is None else _top_count(logprobs)
    ids = [int(t) for t in prompt_ids]
    geometry = engine._request_geometry(len(ids), max_new_tokens, streaming)
    if streaming is not None:
        engine.set_discarded(0)
    try:
        yield from driver(engine, ids, max_new_tokens, geometry, n_top, *args)
    finally:
        if streaming is not None:
            engine.set_discarded(0)


def _top_count(logprobs):
    """`logprobs` as the number of alternatives a record carries: 0 .. LOGPROB_TOP, or ValueError."""
    n_top = int(logprobs)
    if not 0 <= n_top <= L.LOGPROB_TOP:
        raise ValueError("`logprobs` is a count of alternatives in [0, %d]" % L.LOGPROB_TOP)
    return n_top


def _prompt_pass(engine, ids, max_new_tokens, chunk, ctx, tail):
    """The prompt in chunks of `chunk` tokens, then the attention regime of the context the request will reach. `tail`
    = which chunks may end on the chaining tail (`prefill(greedy=True)`: the pick, and with it the sampler's history
    mark and the record): "all", "last" or "none"."""
    n = len(ids)
    for s0 in range(0, n, chunk):
        engine.prefill(ids[s0:s0 + chunk], start_pos=s0, greedy=tail == "all" or (tail == "last" and s0 + chunk >= n))
    engine.tune_attn_for(n + max_new_tokens if ctx is None else min(ctx, n + max_new_tokens))


def _unpack_records(rows, n_top):
    """Rows `[token, chosen log-probability, n_top ids, n_top log-probabilities]` (floats, one per token) ->
    `(tokens, chosen_lps, top)` with `top` one list of `(id, log-probability)` pairs per token."""
    return ([int(r[0]) for r in rows], [r[1] for r in rows],
            [[(int(i), lp) for i, lp in zip(r[2:2 + n_top], r[2 + n_top:])] for r in rows])


def _records(engine, p0, k, n_top):
    """Rows p0 .. p0 + k - 1 of the token log and the three log-probability logs in ONE device-to-host copy."""
    chosen, top_id, top_lp = engine.logprob_log()
    rows = slice(p0, p0 + k)
    return _unpack_records(torch.cat([engine.token_log()[rows, None].double(), chosen[rows, None].double(),
                                      top_id[rows, :n_top].double(), top_lp[rows, :n_top].double()], dim=1).tolist(), n_top)


def _cut_at_eos(parts, eos):
    """`parts` = a burst's parallel lists, tokens first -> (the lists cut after the first id in `eos`, which is kept;
    whether there was one)."""
    stop = next((j + 1 for j, t in enumerate(parts[0]) if t in eos), None)
    return tuple(p[:stop] for p in parts), stop is not None


def _controls(presence_penalty, frequency_penalty, min_p, logit_bias):
    """(presence, frequency, min_p, {int id: float value}) with None = neutral"""
    return (float(presence_penalty or 0.0), float(frequency_penalty or 0.0), float(min_p or 0.0),
            {int(k): float(v) for k, v in dict(logit_bias or {}).items()})


def request_seed():
    """One 63-bit value from torch's default CPU generator: `torch.manual_seed` makes sampled requests reproducible."""
    return int(torch.randint(0, 2 ** 63 - 1, (1,)).item())


# ---- the chained driver -----------------------------------------------------------------------------------------------
def iter_generate(engine, prompt_ids, max_new_tokens, chunk=2048, burst=16, eos=(), logprobs=None, streaming=None):
    """Prompt pass + bursts of `burst` chained steps, yielding each burst's new tokens (the first one alone: it comes
    from the prompt pass's tail). With a sampler installed the prompt is marked in the history first and every
    token is the sampler's; without one this is the greedy chain. Stops after the first id in `eos` (kept).
    `logprobs` = N in 0..20: recording is on for this call (the previous state returns afterwards) and every burst
    is `(tokens, chosen_lps, top)` with `top` one list of N `(id, log-probability)` pairs per token, read back in
    the burst's one synchronisation. `streaming` = a StreamingConfig: the request runs over a rolling KV cache
    (`plan_stream`: bursts clipped at ctx_size, a `kv_shift` whenever the cache is full) and may be longer than
    the cache; tokens and records are read at cache positions."""
    return _request(engine, _chained, prompt_ids, max_new_tokens, logprobs, streaming, chunk, burst, eos)


def _chained(engine, ids, max_new_tokens, geometry, n_top, chunk, burst, eos):
    before = engine.logprobs_on
    if n_top is not None:  # recording is on for this request; the previous state returns afterwards
        engine.set_logprobs(True)
    try:
        yield from _chained_bursts(engine, ids, max_new_tokens, geometry, n_top, chunk, burst, eos)
    finally:
        if n_top is not None:
            engine.set_logprobs(before)


def _chained_bursts(engine, ids, max_new_tokens, geometry, n_top, chunk, burst, eos):
    n = len(ids)
    ctx, n_keep, n_discard = geometry
    if engine.sampler_installed:
        engine.mark_seen(ids, clear=True)
        if engine.controls_installed:
            engine.mark_counts([], clear=True)  # prompt tokens do not count: the penalties are over generated ids
        if engine.guide_installed:  # where the request's text starts: after the prompt for a bad-words guide
            engine.guide_reset(engine._guide.walk(engine._guide_prefix, engine._guide.prompt_state(ids)))
        engine.native_sampled_requests += 1
    # the sampled tail marks its pick in the history, so with a sampler only the last chunk may end on it: an earlier
    # chunk's throw-away token is neither prompt nor generated (the greedy argmax has no side effect) (and with
    # recording on only the last chunk's tail leaves a record)
    _prompt_pass(engine, ids, max_new_tokens, chunk, ctx, "last" if engine.sampler_installed or n_top is not None else "all")
    if max_new_tokens < 1:
        return
    eos = set(int(e) for e in eos)
    parts = ([int(engine.token.item())],)  # the prompt pass's token
    if n_top is not None:  # its record is row n - 1; the token log has no entry there (the prompt pass's pick does not log)
        parts += _records(engine, n - 1, 1, n_top)[1:]
    yield parts[0] if n_top is None else parts
    if parts[0][0] in eos:
        return
    if max_new_tokens > 1:
        engine.prepare_decode(greedy=True)  # a captured graph only in "graph" launch mode (engine.py LAUNCH)
    log = engine.token_log()
    for ev in plan_stream(n, max_new_tokens, ctx, n_keep, n_discard, burst):
        if ev[0] == "shift":  # the cache is full: drop n_discard positions, the device position follows
            engine.kv_shift(n_keep, n_discard, ev[1])
            continue
        _, p0, k = ev  # p0 = cache position the next step feeds
        engine.replay(k)
        # the burst's one host synchronisation: its slots of the token log, with the records in the same copy
        parts = (log[p0:p0 + k].tolist(),) if n_top is None else _records(engine, p0, k, n_top)
        parts, stopped = _cut_at_eos(parts, eos)  # a stop token is noticed at the end of its burst; the steps past it are dropped
        yield parts[0] if n_top is None else parts
        if stopped:
            return


def generate(engine, prompt_ids, max_new_tokens, chunk=2048, burst=16, sampler=None, logprobs=None, streaming=None):
    """`iter_generate` to the end -> the new tokens: the prompt goes through the prefill pass in chunks of `chunk`
    tokens, then bursts of `burst` steps chained on the device (one host read of the token log per burst). `sampler` =
    a dict of `set_sampler` arguments: the native sampler is installed for this call (removed afterwards). `logprobs` =
    N in 0..20: returns `(tokens, chosen_lps, top)` instead. `streaming` = a StreamingConfig: a rolling KV cache, so
    prompt + max_new_tokens may exceed the cache."""
    if sampler is not None:
        engine.set_sampler(**sampler)
    try:
        bursts = list(iter_generate(engine, prompt_ids, max_new_tokens, chunk=chunk, burst=burst, logprobs=logprobs,
                                    streaming=streaming))
    finally:
        if sampler is not None:
            engine.clear_sampler()
    if logprobs is None:
        return [t for b in bursts for t in b]
    return tuple([x for b in bursts for x in b[i]] for i in range(3))


# ---- the host-fed driver ----------------------------------------------------------------------------------------------
class DeviceSampler:
    """Next-token choice on the device from the engine's fp32 logits, with Hugging Face's semantics for the options the
    reference's NeuralChat passes by default (`neural_chat/config.py:400-409`: do_sample=True, temperature 0.1, top_k 40,
    top_p 0.75, repetition_penalty 1.1): RepetitionPenaltyLogitsProcessor over prompt + generated ids, then — when
    sampling — TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper (min_tokens_to_keep 1) and
    `torch.multinomial` on the softmax; argmax otherwise. Plain torch ops in HF's order (checked against the HF classes in
    tests/test_api_cpu.py); no host synchronisation — the caller reads tokens back in bursts."""

    def __init__(self, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, generator=None,
                 presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, logit_bias=None):
        """`logit_bias` ({token id: value}, HF's single-token `sequence_bias`, -inf = a suppressed token) is added ahead
        of the repetition penalty (where HF's SequenceBiasLogitsProcessor sits); `frequency_penalty` / `presence_penalty`
        (OpenAI's: `s - frequency * count`, then `s - presence`, over the ids GENERATED so far) follow it; `min_p` is HF's
        MinPLogitsWarper after top-p. The order of csrc/woq_sample.hip, every step one fp32 torch op."""
        self.presence, self.frequency, self.min_p, self.bias = _controls(presence_penalty, frequency_penalty, min_p,
                                                                         logit_bias)
        if not 0.0 <= self.min_p <= 1.0:
            raise ValueError("`min_p` has to be a float in the range [0, 1]")
        self._bias_dev = None
        self.do_sample = bool(do_sample)
        self.temperature = float(temperature if temperature is not None else 1.0)
        self.top_k = int(top_k or 0)
        self.top_p = float(top_p if top_p is not None else 1.0)
        self.penalty = float(repetition_penalty if repetition_penalty is not None else 1.0)
        self.generator = generator
        if self.do_sample and self.temperature <= 0:
            raise ValueError("`temperature` has to be a strictly positive float when sampling")

    def _adjusted(self, logits, history, generated):
        """bias, repetition penalty, frequency and presence penalty: a new tensor, or `logits` itself when all are off"""
        scores = logits
        if self.bias:
            if self._bias_dev is None or self._bias_dev[0].device != logits.device:
                self._bias_dev = (torch.tensor(list(self.bias), dtype=torch.int64, device=logits.device),
                                  torch.tensor(list(self.bias.values()), dtype=torch.float32, device=logits.device))
            scores = logits.clone()
            scores[self._bias_dev[0]] += self._bias_dev[1]
        if self.penalty != 1.0 and history.numel():
            scores = scores.clone() if scores is logits else scores
            picked = scores[history]
            scores[history] = torch.where(picked < 0, picked * self.penalty, picked / self.penalty)
        if (self.frequency != 0.0 or self.presence != 0.0) and generated is not None and generated.numel():
            counts = torch.bincount(generated, minlength=scores.numel())
            hit = counts > 0
            scores = torch.where(hit, scores - counts.to(torch.float32) * self.frequency, scores)
            scores = torch.where(hit, scores - self.presence, scores)
        return scores

    def processed(self, logits, history, generated=None):
        """logits fp32 [vocab]; history int64 [n] (prompt + generated so far); generated int64 [m] (the generated part
        alone: what the frequency / presence penalties count) -> the scores sampling draws from."""
        scores = self._adjusted(logits, history, generated)
        scores = scores.clone() if scores is logits else scores
        if not self.do_sample:
            return scores
        if self.temperature != 1.0:
            scores = scores / self.temperature
        if self.top_k > 0:
            k = min(self.top_k, scores.numel())
            kth = torch.topk(scores, k).values[-1]
            scores = scores.masked_fill(scores < kth, float("-inf"))
        if self.top_p < 1.0:
            sorted_scores, order = torch.sort(scores, descending=False)
            cum = sorted_scores.softmax(-1).cumsum(-1)
            drop = cum <= (1.0 - self.top_p)
            drop[-1] = False  # min_tokens_to_keep = 1
            scores = scores.masked_fill(torch.zeros_like(drop).scatter(0, order, drop), float("-inf"))
        if self.min_p > 0.0:
            scores = self._min_p_cut(scores)
        return scores

    def _min_p_cut(self, scores):
        """HF MinPLogitsWarper, min_tokens_to_keep 1: drop what is less likely than min_p x the likeliest token"""
        probs = scores.softmax(-1)
        drop = probs < self.min_p * probs.amax()
        drop[probs.argmax()] = False
        return scores.masked_fill(drop, float("-inf"))

    TIE_SLACK = 8  # candidates kept beyond top_k so that values tied with the k-th one survive like in HF's mask

    def __call__(self, logits, history, generated=None):
        if self.do_sample and 0 < self.top_k < logits.numel():
            return self._draw_top_k(logits, history, generated)
        scores = self.processed(logits, history, generated)
        if not self.do_sample:
            return scores.argmax().reshape(1)
        return torch.multinomial(scores.softmax(-1), 1, generator=self.generator)

    def _draw_top_k(self, logits, history, generated=None):
        """The same distribution as `processed` + softmax + multinomial when top_k is set, without sorting the whole
        vocabulary: after the top-k mask only the candidates matter (everything else has probability 0), so the
        temperature, the nucleus cut and the draw run on top_k (+ TIE_SLACK) values — a 32000-entry sort per token is
        most of what sampling costs otherwise (profiles/r04n_*). Ties beyond TIE_SLACK entries at the k-th value would
        be cut where HF keeps them all; fp32 logits do not tie in practice."""
        scores = self._adjusted(logits, history, generated)
        k2 = min(self.top_k + self.TIE_SLACK, scores.numel())
        vals, idx = torch.topk(scores, k2)  # descending
        if self.temperature != 1.0:
            vals = vals / self.temperature
        vals = vals.masked_fill(vals < vals[self.top_k - 1], float("-inf"))
        if self.top_p < 1.0:  # HF: ascending order, drop while the cumulative probability <= 1 - top_p, keep the last
            asc = vals.flip(0)
            drop = asc.softmax(-1).cumsum(-1) <= (1.0 - self.top_p)
            drop[-1] = False
            vals = vals.masked_fill(drop.flip(0), float("-inf"))
        if self.min_p > 0.0:
            vals = self._min_p_cut(vals)
        pick = torch.multinomial(vals.softmax(-1), 1, generator=self.generator)
        return idx[pick]


def iter_sampled(engine, prompt_ids, max_new_tokens, sampler, eos=(), burst=16, chunk=2048, logprobs=None,
                 streaming=None):
    """Prompt pass + decode steps with the next token chosen by `sampler` on the device (sampling and / or repetition
    penalty: the requests `generate`'s greedy chain does not cover). Every step is the engine's native step (logits
    only) followed by a dozen small torch kernels; nothing synchronises until `burst` tokens are read back (1 for a
    text stream). Yields each burst's new tokens; stops after the first id in `eos` (kept in the output, like HF).
    `logprobs` = N in 0..20: yields `(tokens, chosen_lps, top)` like `iter_generate`, the records computed here with
    `torch.log_softmax` + `torch.topk` over the raw logits (ties in whatever order topk leaves). `streaming` = a
    StreamingConfig: a rolling KV cache (`plan_stream`); the host sets the position of every step here, so the shifts
    leave the device position alone."""
    return _request(engine, _host_fed, prompt_ids, max_new_tokens, logprobs, streaming, sampler, chunk, burst, eos)


def _host_fed(engine, ids, max_new_tokens, geometry, n_top, sampler, chunk, burst, eos):
    n = len(ids)
    ctx, n_keep, n_discard = geometry
    # the cache position every step after the first token feeds, with the shifts between them
    steps = plan_steps(plan_stream(n, max_new_tokens, ctx, n_keep, n_discard, burst))
    dev = engine.device
    hist = torch.empty(n + max_new_tokens, dtype=torch.int64, device=dev)
    hist[:n] = torch.tensor(ids, dtype=torch.int64, device=dev)
    _prompt_pass(engine, ids, max_new_tokens, chunk, ctx, "none")
    eos = set(int(e) for e in eos)
    if n_top is not None:  # one `_unpack_records` row per token
        n_top = min(n_top, engine.cfg.vocab)
        rec = torch.empty(max(max_new_tokens, 1), 2 + 2 * n_top, dtype=torch.float64, device=dev)
    stopped, made, feed = False, 0, n  # feed = cache position of the next step (n + made until a shift)
    while not stopped and made < max_new_tokens:
        k = min(burst, max_new_tokens - made)
        for _ in range(k):
            if made > 0:
                ev = next(steps)
                if ev[0] == "shift":  # the cache is full: drop n_discard positions, then feed n_cached - n_discard
                    engine.kv_shift(n_keep, n_discard, ev[1], move_pos=False)
                    ev = next(steps)
                    engine.pos.fill_(ev[1])
                engine.step(greedy=False)  # logits of the token just chosen, at cache position ev[1]
                feed = ev[1] + 1
            tok = sampler(engine.logits, hist[:n + made], hist[n:n + made])
            if n_top is not None:  # the raw distribution's view of the pick and of its best ids
                lsm = torch.log_softmax(engine.logits, -1)
                rec[made, 0], rec[made, 1] = tok[0], lsm[tok[0]]
                if n_top:
                    best = torch.topk(engine.logits, n_top).indices
                    rec[made, 2:2 + n_top] = best
                    rec[made, 2 + n_top:] = lsm[best]
            hist[n + made] = tok[0]
            engine.token.copy_(tok.to(torch.int32))
            engine.pos.fill_(feed)
            made += 1
        # the burst's one host synchronisation
        parts = (hist[n + made - k:n + made].tolist(),) if n_top is None else _unpack_records(rec[made - k:made].tolist(), n_top)
        parts, stopped = _cut_at_eos(parts, eos)
        yield parts[0] if n_top is None else parts


def generate_sampled(engine, prompt_ids, max_new_tokens, sampler, eos=(), on_tokens=None, burst=16, chunk=2048):
    """`iter_sampled` to the end; `on_tokens(list)` receives each burst. Returns the new tokens."""
    out = []
    for new in iter_sampled(engine, prompt_ids, max_new_tokens, sampler, eos=eos, burst=burst, chunk=chunk):
        out += new
        if on_tokens is not None:
            on_tokens(new)
    return out


# ---- a sampling request on whichever driver takes it ------------------------------------------------------------------
def iter_sampled_auto(engine, prompt_ids, max_new_tokens, eos=(), burst=16, chunk=2048, do_sample=False,
                      temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, logprobs=None, presence_penalty=0.0,
                      frequency_penalty=0.0, min_p=0.0, logit_bias=None, seed=None, guide=None, streaming=None):
    """A sampling / repetition-penalty request: on the native sampler (chained bursts, graph replays) when
    `native_sampler_supports` says so, else `iter_sampled` with a `DeviceSampler`. The sampler is removed after the
    request, so the next greedy request runs the untouched greedy path: in a `finally` of this generator, which runs when
    the stream is exhausted, closed or collected — a consumer that stops early and keeps the generator alive should
    `close()` it. Installing and removing each drop the captured graphs, so a sampled request and the greedy request
    after it each pay one capture. `seed` = None: `request_seed()`; a given seed makes the request reproducible (on the
    torch sampler it seeds a device generator of the request's own). `guide` = a TokenGuide the request follows
    (`set_guide`); it runs on the native sampler only, so a request it cannot take raises. `streaming` = a
    StreamingConfig: the request runs over a rolling KV cache on either path."""
    pres, freq, min_p, bias = _controls(presence_penalty, frequency_penalty, min_p, logit_bias)
    opts = dict(do_sample=bool(do_sample), temperature=1.0 if temperature is None else temperature, top_k=top_k or 0,
                top_p=1.0 if top_p is None else top_p,
                repetition_penalty=1.0 if repetition_penalty is None else repetition_penalty,
                presence_penalty=pres, frequency_penalty=freq, min_p=min_p, logit_bias=bias)
    if opts["do_sample"] and float(opts["temperature"]) <= 0:
        raise ValueError("`temperature` has to be a strictly positive float when sampling")
    if guide is not None and not engine.native_sampler_supports(guide=guide, **opts):
        raise RuntimeError("QBits: a token guide runs on the native sampler, which does not take this request "
                           "(tensor parallel, another vocabulary, or sampling options it does not cover)")
    if not engine.native_sampler_supports(**opts):
        gen = None
        if seed is not None:
            gen = torch.Generator(device=engine.device)
            gen.manual_seed(int(seed) & (2 ** 63 - 1))
        yield from iter_sampled(engine, prompt_ids, max_new_tokens, DeviceSampler(generator=gen, **opts), eos=eos,
                                burst=burst, chunk=chunk, logprobs=logprobs, streaming=streaming)
        return
    try:  # (inside: the sampler may be installed already when the controls are refused)
        engine.set_sampler(seed=request_seed() if seed is None else int(seed), **opts)
        if guide is not None:
            engine.set_guide(guide)
        yield from iter_generate(engine, prompt_ids, max_new_tokens, chunk=chunk, burst=burst, eos=eos,
                                 logprobs=logprobs, streaming=streaming)
    finally:
        engine.clear_sampler()
