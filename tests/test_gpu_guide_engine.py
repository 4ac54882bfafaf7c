"""The token guide inside the decode engine (the tiny quantised Llama of tests/test_gpu_sampler_controls_engine.py,
max_ctx 256): the guided pre-pass, the pick and the state's advance in the chaining tail of the prompt pass, eager steps,
the one-step graph and bursts. A synthetic `vocab_bytes` over the model's 320 ids (tests/guide_reference.py) with one id
as EOS.

* Guided greedy (a regex guide, a choices guide): with burst 1 and the saved logits every token is the argmax over the
  ids the guide's state allows (lowest id on ties), the state walked on the host; the same tokens in every launch mode and
  burst size; `guide_state()` = `walk(tokens)`. The patterns are ones the UNGUIDED greedy run violates within its first 4
  tokens (asserted on that run), so the guide bites.
* Guided seeded sampling: replayed step by step through the sampler references over the masked scores, acceptance rule
  and tolerance of tests/test_gpu_sampler_kernel.py; independent of launch mode and burst.
* Another guide or a reset keeps the captured graph; `clear_guide()` gives the plain greedy tokens back.
* `bad_words_ids` through `model.generate` runs on the engine and follows Hugging Face's rule, across the prompt boundary.
* With recording on, `chosen` is the RAW log-probability of the guided token (tests/logprob_reference.py).
"""
import numpy as np
import pytest
import torch

from intel_extension_for_transformers_amd.runtime.guide import TokenGuide
from tests import guide_reference as G
from tests import logprob_reference as LP
from tests import sampler_controls_reference as C
from tests import sampler_reference as R
from tests.test_gpu_sampler_controls_engine import PROMPT, SAMPLED, qmodel  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

N_NEW = 24
REGEX = r"(ab|ba|c)+\d{2,3}"
CHOICES = ["yes", "no", "maybe", "abcd"]
MODES = (("eager", 16), ("graph", 1), ("graph", 5), ("graph", 16))


def _vocab(eng):
    """the synthetic pieces padded with empty ones to the model's vocabulary -> (vocab_bytes, eos id)"""
    pieces, eos, _specials = G.synthetic_vocab()
    assert len(pieces) <= eng.cfg.vocab
    return pieces + [b""] * (eng.cfg.vocab - len(pieces)), eos


def _guided(eng, guide, n_new, eos, burst=16, launch="graph", rows=None, sampler=None, logprobs=None):
    """one request under `guide` -> (tokens, guide state afterwards); rows (a list) receives the logits of every step
    when burst == 1 (they are still in engine.logits when the burst is read)"""
    eng.launch = launch
    eng.captured = False
    if sampler is not None:
        eng.set_sampler(**sampler)
    eng.set_guide(guide)
    out = []
    try:
        for new in eng.iter_generate(PROMPT, n_new, burst=burst, eos=[eos], logprobs=logprobs):
            if rows is not None:
                assert burst == 1
                rows.append(eng.logits.cpu().numpy().copy())
            out.append(new)
        state = eng.guide_state()
        assert eng.guide_installed and eng.sampler_installed
    finally:
        eng.clear_guide()
        eng.clear_sampler()
    assert not eng.guide_installed and not eng.sampler_installed
    return out, state


def _violates_within(guide, tokens, n):
    try:
        guide.walk(tokens[:n])
    except ValueError:
        return True
    return False


@pytest.mark.parametrize("kind", ("regex", "choices"))
def test_guided_greedy_is_the_masked_argmax_in_every_launch_mode(qmodel, kind):  # noqa: F811
    eng = qmodel.woq_engine
    vb, eos = _vocab(eng)
    guide = (TokenGuide.from_regex(REGEX, vb, [eos]) if kind == "regex" else TokenGuide.from_choices(CHOICES, vb, [eos]))
    plain = eng.generate(PROMPT, N_NEW)
    assert _violates_within(guide, plain, 4), "the unguided run must violate the guide for the test to mean anything"
    rows = []
    bursts, state = _guided(eng, guide, N_NEW, eos, burst=1, rows=rows)
    tokens = sum(bursts, [])
    s = guide.start
    for i, (t, lg) in enumerate(zip(tokens, rows)):
        masked = G.masked_f32(lg, guide.table[s])
        assert t == int(np.flatnonzero(masked == np.nanmax(masked))[0]), (i, t)
        s = guide.walk([t], s)
    assert state == s == guide.walk(tokens)
    assert tokens != plain[:len(tokens)]
    if kind == "choices":
        assert tokens[-1] == eos and b"".join(vb[t] for t in tokens[:-1]).decode() in CHOICES
    for launch, burst in MODES:
        again, state = _guided(eng, guide, N_NEW, eos, burst=burst, launch=launch)
        assert sum(again, []) == tokens, (launch, burst)
        assert state == guide.walk(tokens), (launch, burst)  # steps run past EOS stay in the terminal state
    assert eng.status() == 0


def test_guided_seeded_sampling_step_by_step_and_across_launch_modes(qmodel):  # noqa: F811
    eng = qmodel.woq_engine
    vb, eos = _vocab(eng)
    guide = TokenGuide.from_regex(r"[a-z ]{1,40}(\d|[A-Z])*", vb, [eos])
    seed, n = 0x5EED0123456789, len(PROMPT)
    sampler = dict(seed=seed, **SAMPLED)
    rows = []
    bursts, state = _guided(eng, guide, N_NEW, eos, burst=1, rows=rows, sampler=sampler)
    tokens = sum(bursts, [])
    history, s, needed_tol = list(PROMPT), guide.start, 0
    zero = np.zeros(eng.cfg.vocab, np.int64)
    for i, (t, lg) in enumerate(zip(tokens, rows)):
        adj = G.masked_f32(C.adjusted_f32(lg, history, zero, SAMPLED["repetition_penalty"]), guide.table[s])
        ref = C.choose(R.scores_f32(adj, [], 1.0, SAMPLED["temperature"], True), SAMPLED["top_k"], SAMPLED["top_p"], 0.0)
        tol = 8 * ref.n_kept * R.TWO_M24
        u = R.uniform_at(seed, n - 1 + i)  # the position the step fed (the prompt pass fed n - 1)
        assert ref.accepts(t, u, tol), (i, t, u, ref.pick(u))
        if ref.needs_tolerance(u, tol) or ref.boundary_margin < 100 * 8 * ref.n_candidates * R.TWO_M24:
            needed_tol += 1
        else:
            assert t == ref.pick(u), (i, t, u, ref.pick(u))
        history.append(t)
        s = guide.walk([t], s)
    print("draws that needed the tolerance: %d of %d, distinct tokens %d" % (needed_tol, len(tokens), len(set(tokens))))
    assert needed_tol <= 2 and state == s and len(set(tokens)) > 2
    for launch, burst in MODES:
        again, state = _guided(eng, guide, N_NEW, eos, burst=burst, launch=launch, sampler=sampler)
        assert sum(again, []) == tokens and state == guide.walk(tokens), (launch, burst)
    assert eng.status() == 0


def test_another_guide_and_a_reset_keep_the_graph_and_clearing_restores_greedy(qmodel):  # noqa: F811
    eng = qmodel.woq_engine
    vb, eos = _vocab(eng)
    before = eng.generate(PROMPT, N_NEW)
    first = TokenGuide.from_choices(CHOICES, vb, [eos])
    second = TokenGuide.from_regex(r"[a-c]{20}\d", vb, [eos])  # more states than `first`: the engine's table grows
    assert second.n_states > first.n_states
    want_second = sum(_guided(eng, second, N_NEW, eos, launch="eager")[0], [])
    eng.launch = "graph"
    eng.captured = False
    eng.set_guide(first)
    try:
        assert eng.guide_installed and eng.sampler_installed and not eng.captured
        a = sum(eng.iter_generate(PROMPT, N_NEW, burst=4, eos=[eos]), [])
        assert eng.captured and eng.guide_state() == first.walk(a)
        eng.set_guide(second)
        assert eng.captured and eng.guide_state() == second.start
        b = sum(eng.iter_generate(PROMPT, N_NEW, burst=4, eos=[eos]), [])
        assert eng.captured and b == want_second and eng.guide_state() == second.walk(b)
        eng.guide_reset()
        assert eng.captured and eng.guide_state() == second.start
        eng.guide_reset(second.walk(b[:2]))
        assert eng.captured and eng.guide_state() == second.walk(b[:2])
    finally:
        eng.clear_guide()
    assert not eng.guide_installed and not eng.sampler_installed and not eng.captured
    assert eng.generate(PROMPT, N_NEW) == before
    # clear_sampler takes the guide along; a guide beside the caller's own sampler leaves that sampler installed
    eng.set_sampler(do_sample=False, repetition_penalty=1.2)
    eng.set_guide(first)
    eng.clear_guide()
    assert eng.sampler_installed and not eng.guide_installed
    eng.set_guide(first)
    eng.clear_sampler()
    assert not eng.sampler_installed and not eng.guide_installed
    with pytest.raises(RuntimeError, match="QBits"):
        eng.guide_state()
    wrong = TokenGuide(np.zeros((1, eng.cfg.vocab + 1), np.uint16))
    assert not eng.native_sampler_supports(guide=wrong) and eng.native_sampler_supports(guide=first)
    with pytest.raises(RuntimeError, match="QBits"):
        eng.set_guide(wrong)
    assert not eng.sampler_installed and eng.generate(PROMPT, N_NEW) == before
    assert eng.status() == 0


def _bad_words_reference(eng, words, n_new):
    """the engine under the bad-words guide with burst 1 -> tokens, each checked against Hugging Face's rule: the argmax
    of the saved logits over the ids that `hf_banned` leaves"""
    guide = TokenGuide.from_bad_words(words, eng.cfg.vocab)
    rows = []
    bursts, _state = _guided(eng, guide, n_new, eos=-1, burst=1, rows=rows)
    tokens = sum(bursts, [])
    for i, (t, lg) in enumerate(zip(tokens, rows)):
        masked = np.array(lg, dtype=np.float32)
        masked[sorted(G.hf_banned(words, PROMPT + tokens[:i]))] = -np.inf
        assert t == int(np.flatnonzero(masked == np.nanmax(masked))[0]), (i, t)
    return tokens


def test_bad_words_ids_through_model_generate_run_on_the_engine(qmodel):  # noqa: F811
    eng = qmodel.woq_engine
    ids = torch.tensor([PROMPT], device="cuda")
    g = qmodel.generate(ids, max_new_tokens=N_NEW)[0, len(PROMPT):].tolist()
    assert g == eng.generate(PROMPT, N_NEW)
    for words in ([[g[3], g[4]], [g[8]]], [[PROMPT[-1], g[0]]]):  # the second: a bigram across the prompt boundary
        count = eng.native_sampled_requests
        out = qmodel.generate(ids, max_new_tokens=N_NEW, bad_words_ids=words)[0, len(PROMPT):].tolist()
        assert eng.native_sampled_requests == count + 1, "the request left the engine"
        assert not eng.sampler_installed and not eng.guide_installed
        first = next(i for i in range(N_NEW) if g[i] in G.hf_banned(words, PROMPT + g[:i]))
        assert out[:first] == g[:first] and out[first] != g[first], (words, first)
        assert all(out[i] not in G.hf_banned(words, PROMPT + out[:i]) for i in range(N_NEW))
        assert out == _bad_words_reference(eng, words, N_NEW), words
    with pytest.raises(ValueError, match="guide"):
        qmodel.generate(ids, max_new_tokens=4, bad_words_ids=[[g[0]]], guide=TokenGuide.from_bad_words([[g[0]]], eng.cfg.vocab))
    # guide= on generate: a text guide ends the request with EOS
    vb, eos = _vocab(eng)
    out = qmodel.generate(ids, max_new_tokens=N_NEW, guide=TokenGuide.from_choices(CHOICES, vb, [eos]),
                          eos_token_id=eos)[0, len(PROMPT):].tolist()
    assert out[-1] == eos and b"".join(vb[t] for t in out[:-1]).decode() in CHOICES
    assert eng.status() == 0


def test_logprobs_describe_the_raw_distribution_at_the_guided_token(qmodel):  # noqa: F811
    eng = qmodel.woq_engine
    vb, eos = _vocab(eng)
    guide = TokenGuide.from_regex(REGEX, vb, [eos])
    rows = []
    bursts, _state = _guided(eng, guide, 12, eos, burst=1, rows=rows, logprobs=0)
    tokens = sum((b[0] for b in bursts), [])
    chosen = sum((b[1] for b in bursts), [])
    tol = 4 * max(LP.deviation(lg, t) for lg, t in zip(rows, tokens))
    assert 0 < tol < 4e-4
    raw_best = 0
    for t, c, lg in zip(tokens, chosen, rows):
        assert abs(c - LP.record_f64(lg, t)[0]) <= tol, (t, c)
        raw_best += int(t == int(np.argmax(lg)))
    assert raw_best < len(tokens)  # a guided token need not be the raw favourite: its raw log-probability is what counts
    assert not eng.logprobs_on and eng.status() == 0
