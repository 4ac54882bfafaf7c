"""The rolling KV cache inside the decode engine: the tiny model of tests/test_gpu_engine.py with max_ctx 32 and an fp16
cache generates 100 tokens after a 6-token prompt, dropping 14 positions behind 4 sinks whenever the cache is full.

The reference is the fp32 CPU oracle given the same operation after every shift,
`k = concat(k[:4], rope(k[18:], -14))`, `v` likewise, then stepped at the positions counted inside the cache. Every step's
logits meet the project's decode tolerance, 2e-3 * max|ref| + 1e-4, with equal argmax; the oracle keeps its own rows
throughout (no hand-back of device rows was needed: a row is re-rounded by at most one shift before it is dropped).
`generate(..., streaming=)` must reproduce that chain token for token in every launch mode and burst size, a seeded sampled
request must draw with the uniform of each token's ABSOLUTE index, and the log-probability records must describe each
step's logits."""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd import _lib as L
from oracle import woq_oracle as orc
from tests import kv_shift_reference as KR
from tests import logprob_reference as LR
from tests import sampler_reference as R
from tests.test_gpu_engine import _tiny

pytestmark = pytest.mark.gpu

PROMPT = [7, 300, 12, 45, 99, 3]
N_NEW = 100
CTX, KEEP, DISCARD = 32, 4, 14
SAMPLED = dict(do_sample=True, temperature=1.0, top_k=40)
SEED = 0x5EED0123456789


def _streaming():
    from intel_extension_for_transformers_amd.runtime.engine import StreamingConfig

    return StreamingConfig(ctx_size=CTX, n_keep=KEEP, n_discard=DISCARD)


@pytest.fixture(scope="module")
def tiny():
    eng, oracle, cfg = _tiny(128, False, "fp16", seed=3, max_ctx=CTX)
    return eng, oracle, cfg


def _oracle_shift(oracle, theta):
    for li in range(len(oracle.k)):
        rows = oracle.k[li].shape[0] - KEEP - DISCARD
        oracle.k[li] = np.concatenate([oracle.k[li][:KEEP],
                                       orc.rope(oracle.k[li][KEEP + DISCARD:], [-DISCARD] * rows, theta)], 0)
        oracle.v[li] = np.concatenate([oracle.v[li][:KEEP], oracle.v[li][KEEP + DISCARD:]], 0)


def _fp16_ulp(x):
    """the fp16 step at the magnitude of x (the subnormal step below 2^-14)"""
    _, e = np.frexp(np.abs(x).astype(np.float64))
    return np.ldexp(1.0, np.maximum(e - 1, -14) - 10)


@pytest.fixture(scope="module")
def chain(tiny):
    """The teacher-forced shifted chain: the prompt pass, then one logits-only step per token at cache positions, the
    host shifting the cache (device position untouched) when it is full, the oracle doing the same in fp32. Feeds the
    device's own argmax, so the tokens are what the greedy `generate` must produce. -> (tokens, shifts seen)"""
    eng, oracle, cfg = tiny
    oracle.reset()
    eng.clear_status()
    got = eng.prefill(PROMPT, greedy=False)[0].cpu().numpy()
    for i, t in enumerate(PROMPT):
        ref = oracle.forward_token(t, i)
    assert np.abs(got - ref).max() <= 1e-2 * np.abs(ref).max() and int(got.argmax()) == int(ref.argmax())  # (prompt pass: fp16 operands)
    tokens, p, shifts, worst = [int(got.argmax())], len(PROMPT), 0, 0.0
    while len(tokens) < N_NEW:
        if p == CTX:
            before = eng.kv_cache("k")[0].float().cpu().numpy()  # [layers][CTX][kv heads][D]: what the device holds
            v_before = KR.bits_of(eng.kv_cache("v")[0])
            eng.kv_shift(KEEP, DISCARD, CTX, move_pos=False)
            _oracle_shift(oracle, cfg["theta"])
            p -= DISCARD
            shifts += 1
            after = eng.kv_cache("k")[0].float().cpu().numpy()
            for li in range(cfg["layers"]):
                # the shift itself: the oracle's operation on the device's own stored rows, within 1 fp16 ulp
                want = orc.rope(before[li, KEEP + DISCARD:], [-DISCARD] * (CTX - KEEP - DISCARD), cfg["theta"])
                assert (np.abs(after[li, KEEP:p] - want) <= _fp16_ulp(want)).all(), (shifts, li)
                assert np.array_equal(after[li, :KEEP], before[li, :KEEP])
                # and against the oracle's own fp32 rows: 1 fp16 ulp, the fp16 storage rounding of the append (half an
                # ulp, carried through the rotation) and the decode tolerance of the projection that made the row
                ok = oracle.k[li]
                assert ok.shape[0] == p
                bound = 2 * _fp16_ulp(ok) + 2e-3 * np.abs(ok).max() + 1e-4
                assert (np.abs(after[li, :p] - ok) <= bound).all(), (shifts, li)
            v_after = KR.bits_of(eng.kv_cache("v")[0])
            assert np.array_equal(v_after[:, KEEP:p], v_before[:, KEEP + DISCARD:])
        t = tokens[-1]
        eng.token.fill_(t)
        eng.pos.fill_(p)
        eng.step(greedy=False)
        got = eng.logits.cpu().numpy()
        ref = oracle.forward_token(t, p)
        err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
        worst = max(worst, err / scale)
        assert err <= 2e-3 * scale + 1e-4, (len(tokens), p, shifts, err, scale)
        assert int(got.argmax()) == int(ref.argmax()), (len(tokens), p, shifts)
        tokens.append(int(got.argmax()))
        p += 1
    print("shifts %d, worst relative logit error vs the shifted oracle %.3e" % (shifts, worst))
    assert shifts == 6 and eng.status() == 0
    return tokens, shifts


def test_teacher_forced_chain_follows_the_shifted_oracle(chain):
    tokens, shifts = chain
    assert len(tokens) == N_NEW and len(set(tokens)) > 4


@pytest.mark.parametrize("launch,burst", [("graph", 16), ("graph", 5), ("eager", 16), ("eager", 5)])
def test_generate_streams_past_the_cache_and_equals_the_chain(tiny, chain, launch, burst):
    eng = tiny[0]
    eng.launch = launch
    eng.captured = False
    eng.clear_status()
    out = eng.generate(PROMPT, N_NEW, burst=burst, streaming=_streaming())
    assert eng.status() == 0 and eng.discarded() == 0  # the request's count returns to 0 for whatever runs next
    assert out == chain[0]
    assert sum(eng.iter_generate(PROMPT, N_NEW, burst=burst, streaming=_streaming()), []) == chain[0]
    # a request that fits runs the same with and without the keyword
    assert eng.generate(PROMPT, 20, burst=burst, streaming=_streaming()) == eng.generate(PROMPT, 20, burst=burst)


@pytest.mark.parametrize("launch", ["graph", "eager"])
def test_one_and_two_token_requests_return_the_chains_first_tokens(tiny, chain, launch):
    """`generate` shares the iterator's rule: decode is prepared (a graph captured) only when more than one token is
    asked for."""
    eng = tiny[0]
    eng.launch = launch
    eng.captured = False
    eng.clear_status()
    assert eng.generate(PROMPT, 1) == chain[0][:1] and eng.status() == 0
    assert eng.generate(PROMPT, 2) == chain[0][:2] and eng.status() == 0


def test_without_streaming_the_request_is_refused_as_before(tiny):
    eng = tiny[0]
    for call in (lambda: eng.generate(PROMPT, N_NEW), lambda: list(eng.iter_generate(PROMPT, N_NEW)),
                 lambda: eng.generate(PROMPT, N_NEW, sampler=dict(do_sample=False, repetition_penalty=1.2))):
        with pytest.raises(RuntimeError, match=r"QBits: prompt \(6\) \+ max_new_tokens \(100\) exceeds the engine's max_ctx \(32\)"):
            call()
    from intel_extension_for_transformers_amd.runtime.engine import StreamingConfig

    with pytest.raises(ValueError, match="QBits:"):
        eng.generate(PROMPT, N_NEW, streaming=StreamingConfig(ctx_size=64))  # beyond the engine's cache
    with pytest.raises(ValueError, match="QBits:"):
        eng.generate(list(range(32)), 4, streaming=_streaming())  # the prompt fills ctx_size


def test_torch_sampler_path_streams_the_same_greedy_tokens(tiny, chain):
    from intel_extension_for_transformers_amd.runtime.engine import DeviceSampler, iter_sampled

    eng = tiny[0]
    out = sum(iter_sampled(eng, PROMPT, N_NEW, DeviceSampler(do_sample=False), burst=7, streaming=_streaming()), [])
    assert out == chain[0] and eng.status() == 0


def _sampled(eng, burst, launch="graph"):
    eng.launch = launch
    eng.captured = False
    return eng.generate(PROMPT, N_NEW, burst=burst, sampler=dict(seed=SEED, **SAMPLED), streaming=_streaming())


def test_seeded_sampled_stream_draws_by_absolute_index(tiny):
    eng = tiny[0]
    n = len(PROMPT)
    eng.clear_status()
    eng.launch = "graph"
    eng.captured = False
    eng.set_sampler(seed=SEED, **SAMPLED)
    tokens, rows = [], []
    try:  # burst 1: the logits every token was drawn from are still in engine.logits when the burst is read
        for new in eng.iter_generate(PROMPT, N_NEW, burst=1, streaming=_streaming()):
            rows.append(eng.logits.cpu().numpy().copy())
            tokens += new
    finally:
        eng.clear_sampler()
    assert len(tokens) == N_NEW and eng.discarded() == 0
    history, needed_tol, repeats_if_cache_position = list(PROMPT), 0, 0
    for i, (t, lg) in enumerate(zip(tokens, rows)):
        ref = R.choose(R.scores_f32(lg, history, 1.0, SAMPLED["temperature"], True), SAMPLED["top_k"], 1.0)
        tol = 8 * ref.n_kept * R.TWO_M24
        u = R.uniform_at(SEED, n - 1 + i)  # token i of the stream: the counter is position fed + positions dropped
        assert ref.accepts(t, u, tol), (i, t, u, ref.pick(u))
        if ref.needs_tolerance(u, tol) or ref.boundary_margin < 100 * 8 * ref.n_candidates * R.TWO_M24:
            needed_tol += 1
        else:
            assert t == ref.pick(u), (i, t, u, ref.pick(u))
        history.append(t)
    assert needed_tol <= 4, needed_tol
    assert len(set(tokens)) > 8
    # launch mode and burst size do not change a token
    assert _sampled(eng, 16) == tokens
    assert _sampled(eng, 5) == tokens
    assert _sampled(eng, 16, "eager") == tokens
    assert eng.status() & ~8 == 0 and not eng.sampler_installed


def test_philox_words_at_a_cache_position_change_with_a_shift(tiny):
    """the sampling kernel with the engine's own `discarded` word: at one cache position the words before a shift are the
    existing reference's at that position, after it those of position + n_discard"""
    eng = tiny[0]
    cfg = L.sampler_config(seed=SEED, **SAMPLED)
    key = (SEED & R.MASK, (SEED >> 32) & R.MASK)
    logits = torch.randn(384, device=eng.device)
    seen = torch.zeros(12, dtype=torch.int32, device=eng.device)
    pos = torch.full((1,), 20, dtype=torch.int32, device=eng.device)
    tok = torch.zeros(1, dtype=torch.int32, device=eng.device)
    words = torch.zeros(4, dtype=torch.int32, device=eng.device)
    disc = L.lib().woq_engine_discarded_ptr(eng._h)

    def draw():
        L.probe_sample_stream(logits, seen, cfg, pos, disc, tok, philox_out=words)
        return [int(w) & R.MASK for w in words.tolist()]

    eng.set_discarded(0)
    eng.pos.fill_(CTX)
    before = draw()
    assert before == R.philox4x32_10((20, 0, 0, 0), key)  # discarded == 0: today's words
    eng.kv_shift(KEEP, DISCARD, CTX)
    assert eng.discarded() == DISCARD and int(eng.pos.item()) == CTX - DISCARD
    after = draw()
    assert after != before and after == R.philox4x32_10((20 + DISCARD, 0, 0, 0), key)
    eng.set_discarded(-1)  # uint32 wrap: 20 + 0xFFFFFFFF == 19
    assert draw() == R.philox4x32_10((19, 0, 0, 0), key)
    eng.set_discarded(0)
    L.probe_sample_stream(logits, seen, cfg, pos, None, tok, philox_out=words)  # a null pointer means 0
    assert [int(w) & R.MASK for w in words.tolist()] == before


def test_logprob_records_describe_each_steps_logits(tiny, chain):
    eng = tiny[0]
    eng.launch = "graph"
    eng.captured = False
    toks, lps, tops, rows = [], [], [], []
    for new, lp, top in eng.iter_generate(PROMPT, N_NEW, burst=1, logprobs=2, streaming=_streaming()):
        rows.append(eng.logits.cpu().numpy().copy())
        toks, lps, tops = toks + new, lps + lp, tops + top
    assert toks == chain[0] and not eng.logprobs_on
    tol = 4 * max(LR.deviation(lg, t) for lg, t in zip(rows, toks))
    assert 0 < tol < 4e-4
    worst = 0.0
    for t, lp, top, lg in zip(toks, lps, tops, rows):
        c64, id64, lp64 = LR.record_f64(lg, t)
        assert [i for i, _ in top] == id64[:2].tolist()
        worst = max(worst, abs(lp - c64), max(abs(v - w) for (_, v), w in zip(top, lp64[:2])))
    print("max |record - float64| = %.3e (tol %.3e)" % (worst, tol))
    assert worst <= tol
    # one burst size more: the records are read at cache positions whatever the burst
    got = eng.generate(PROMPT, N_NEW, burst=16, logprobs=2, streaming=_streaming())
    assert got[0] == toks and got[1] == lps and got[2] == tops


# ---- the public interfaces: model.generate's Neural Speed keywords and NeuralChat's GenerationConfig fields --------------
API_PROMPT = [5, 9, 33, 2, 71, 9, 9]


@pytest.fixture(scope="module")
def qmodel():
    import copy

    from intel_extension_for_transformers_amd.runtime.engine import optimize_transformers
    from intel_extension_for_transformers_amd.transformers import AutoModelForCausalLM, RtnConfig
    from tests.test_gpu_api import _tiny_llama

    fp = _tiny_llama()
    fp.generation_config.eos_token_id = None
    q = AutoModelForCausalLM.from_pretrained(copy.deepcopy(fp), quantization_config=RtnConfig(
        bits=4, group_size=32, compute_dtype="fp32", scale_dtype="fp32"), device_map="cuda")
    optimize_transformers(q, max_ctx=64)
    return q


def test_model_generate_takes_neural_speeds_keywords_and_builds_no_larger_engine(qmodel):
    from intel_extension_for_transformers_amd.runtime.engine import StreamingConfig

    eng = qmodel.woq_engine
    ids = torch.tensor([API_PROMPT], device="cuda")
    n = len(API_PROMPT)
    want = eng.generate(API_PROMPT, 150, streaming=StreamingConfig(64, 4, 20))
    out = qmodel.generate(ids, max_new_tokens=150, ctx_size=64, n_keep=4, n_discard=20)
    assert qmodel.woq_engine is eng and eng.cfg.max_ctx == 64  # the request ran on the engine at hand
    assert out.shape == (1, n + 150) and out[0, n:].tolist() == want
    # ctx_size alone: the engine's cache, 4 sinks, half of the rest dropped per shift
    assert qmodel.generate(ids, max_new_tokens=150, n_keep=4)[0, n:].tolist() == \
        eng.generate(API_PROMPT, 150, streaming=StreamingConfig(None, 4, -1))
    assert qmodel.woq_engine is eng
    # a sampled request with the keywords: reproducible, and on the native sampler
    count = eng.native_sampled_requests
    torch.manual_seed(11)
    a = qmodel.generate(ids, max_new_tokens=150, ctx_size=64, n_discard=20, **SAMPLED)
    torch.manual_seed(11)
    b = qmodel.generate(ids, max_new_tokens=150, ctx_size=64, n_discard=20, **SAMPLED)
    assert torch.equal(a, b) and a.shape == (1, n + 150) and eng.native_sampled_requests == count + 2
    assert eng.status() == 0 and eng.discarded() == 0 and not eng.sampler_installed
    with pytest.raises(ValueError, match="QBits:"):
        qmodel.generate(ids, max_new_tokens=150, ctx_size=64, n_keep=60, n_discard=20)
    with pytest.raises(RuntimeError, match="QBits: ctx_size / n_keep / n_discard need"):
        qmodel.generate(ids, max_new_tokens=150, ctx_size=64, num_beams=2)  # HF's loop has no rolling cache


def test_chatbot_routes_a_request_longer_than_the_cache_to_the_engine(tmp_path):
    from intel_extension_for_transformers_amd.neural_chat import GenerationConfig, PipelineConfig, build_chatbot
    from intel_extension_for_transformers_amd.runtime.engine import StreamingConfig
    from intel_extension_for_transformers_amd.transformers import RtnConfig
    from tests.test_gpu_api import _tiny_llama, _tiny_tokenizer

    d = tmp_path / "tiny-llama-chat"
    fp = _tiny_llama()
    fp.generation_config.eos_token_id = None
    fp.save_pretrained(str(d))
    _tiny_tokenizer(d, fp.config.vocab_size)
    bot = build_chatbot(PipelineConfig(model_name_or_path=str(d), device="cuda",
                                       optimization_config=RtnConfig(bits=4, group_size=128, scale_dtype="fp16")))
    eng = bot.engine
    assert eng is not None and eng.cfg.max_ctx == 256
    query = "w5 w17 w200 w3 w77"
    ids = bot.tokenizer(bot.prepare_prompt(query), return_tensors="pt").input_ids[0].tolist()
    # greedy, 300 new tokens in a 256-position cache: 4 sinks, ctx_size and n_discard by default (256, 126)
    cfg = GenerationConfig(max_new_tokens=300, do_sample=False, repetition_penalty=1.0, n_keep=4)
    want = eng.generate(ids, 300, streaming=StreamingConfig(None, 4, -1))
    eos = bot.tokenizer.eos_token_id
    want = want[:want.index(eos)] if eos in want else want
    text = bot.predict(query, config=cfg)
    assert text == bot.tokenizer.decode(want, skip_special_tokens=True) and len(text.split()) > 10
    assert "".join(bot.predict_stream(query, config=cfg)[0]) == text
    # the default sampled request with a seed, over a 64-position window
    cfg = GenerationConfig(max_new_tokens=300, ctx_size=64, n_keep=4, n_discard=20, seed=5)
    count = eng.native_sampled_requests
    a, b = bot.predict(query, config=cfg), bot.predict(query, config=cfg)
    assert a == b and len(a.split()) >= 1 and eng.native_sampled_requests == count + 2
    assert eng.status() & ~8 == 0 and eng.discarded() == 0 and not eng.sampler_installed
