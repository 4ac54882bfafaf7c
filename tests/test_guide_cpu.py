"""The host builders of token guides (runtime/guide.py; numpy, no GPU) over the synthetic vocabulary of
tests/guide_reference.py (single bytes, multi-byte pieces, overlapping pieces, empty specials, one EOS).

* Regex and choices guides: random token sequences walk iff their bytes are a prefix of a match, and EOS is allowed at
  the end iff the bytes `re.fullmatch` the pattern; an accepting state is reachable from every reachable state; for
  patterns with a finite language every tokenisation of every member is accepted and a sequence that leaves the language's
  prefixes is rejected at the first offending token; unsupported constructs raise naming the construct.
* Bad-words guides against a restatement of Hugging Face's rule (and NoBadWordsLogitsProcessor itself when transformers
  imports) on random histories, with overlapping words and a word that is a suffix of another.
* The byte budget, `token_bytes` on stub tokenizers, the C-ABI names.
"""
import itertools
import os
import re

import numpy as np
import pytest

from intel_extension_for_transformers_amd.runtime.guide import BANNED, TokenGuide, token_bytes
from tests import guide_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECES, EOS, SPECIALS = G.synthetic_vocab()

# every supported operator: literals, escapes, `.`, classes with ranges / negation, \d \w \s, groups, |, * + ?, {m} {m,} {m,n}
PATTERNS = [
    r"abc",
    r"a|bc|abcd",
    r"(ab|ba|c)+\d{2,3}",
    r"a*b+c?",
    r"[a-c]{2}[^a-c]",
    r"\d+\.\d{1,2}",
    r"\w+\s\w*",
    r"yes|no|maybe",
    r"(?:ab){2,}",
    r"-?\d{1,3}(,\d{3})?",
    r"a.c",
    r"[\d_]+[^\d\s]",
    r"\{\"\w{1,4}\":(true|false|null)\}",
    r"é+a|€",
    r"x{3}|(yz){1,2}|\x41\n\t",
    r"[]a-]+\S\D\W",
]
FINITE = {  # pattern -> its language over the test alphabet, enumerated with `re` below
    r"a|bc|abcd": "abcd",
    r"[a-c]{2}[d1]?": "abcd1",
    r"yes|no|maybe": "yesnomayb",
    r"x{3}|(yz){1,2}|\x41\n\t": "xyzA\n\t",
    r"-?[12]{1,2}(,[12]{2})?": "-12,",
    r"a?b{1,2}(c|cd)": "abcd",
}
ALPHABET_IDS = [i for i, p in enumerate(PIECES) if p and all(b < 128 for b in p)] + \
    [i for i, p in enumerate(PIECES) if p in (b"\xc3\xa9", b"\xc3", b"\xa9", b"\xe2\x82\xac", b"\xe2\x82", b"\xac")]


def _matches(pattern, data):
    try:
        text = data.decode("utf-8")
    except UnicodeDecodeError:
        return False
    return re.fullmatch(pattern, text, re.ASCII) is not None


def _walk(guide, ids):
    try:
        return guide.walk(ids)
    except ValueError:
        return None


def _language(pattern, alphabet, max_len=6):
    out = []
    for n in range(max_len + 1):
        for combo in itertools.product(alphabet, repeat=n):
            s = "".join(combo)
            if re.fullmatch(pattern, s, re.ASCII):
                out.append(s.encode())
    return out


def _random_sequences(guide, rng, n, length=8):
    """half uniformly random over the alphabet's pieces, half random walks along allowed ids (so that long accepted
    prefixes occur), each cut at a random length"""
    for j in range(n):
        if j % 2:
            yield [int(t) for t in rng.choice(ALPHABET_IDS, rng.integers(0, length))]
            continue
        ids, s = [], guide.start
        for _ in range(rng.integers(0, 2 * length)):
            allowed = [int(t) for t in guide.allowed(s) if t != EOS]
            if not allowed or rng.random() < 0.1:
                ids.append(int(rng.choice(ALPHABET_IDS)))
                break
            ids.append(int(rng.choice(allowed)))
            s = guide.walk(ids[-1:], s)
        yield ids


def _check_no_dead_ends(guide):
    """from every state reachable from `start`, the terminal state (the one EOS leads to) is reachable"""
    succ = [set(int(t) for t in np.unique(row[row != BANNED])) for row in guide.table]
    reach, todo = {guide.start}, [guide.start]
    while todo:
        for t in succ[todo.pop()]:
            if t not in reach:
                reach.add(t)
                todo.append(t)
    terminal = {int(guide.table[s, EOS]) for s in reach if guide.table[s, EOS] != BANNED}
    assert len(terminal) == 1
    good = set(terminal)
    changed = True
    while changed:
        changed = False
        for s in reach - good:
            if succ[s] & good:
                good.add(s)
                changed = True
    assert good == reach == set(range(guide.n_states))  # and the table holds no unreachable state
    for s in reach:
        assert guide.allowed(s).size >= 1
    (t,) = terminal
    assert guide.allowed(t).tolist() == [EOS] and int(guide.table[t, EOS]) == t


@pytest.mark.parametrize("pattern", PATTERNS)
def test_regex_guides_accept_exactly_the_full_matches(pattern):
    guide = TokenGuide.from_regex(pattern, PIECES, [EOS])
    _check_no_dead_ends(guide)
    for sp in SPECIALS:
        assert (guide.table[:, sp] == BANNED).all()  # a token that spells nothing is never allowed
    rng = np.random.default_rng(len(pattern))
    accepted = walked = 0
    for ids in _random_sequences(guide, rng, 400):
        data = b"".join(PIECES[t] for t in ids)
        state = _walk(guide, ids)
        if state is None:
            assert not _matches(pattern, data), (pattern, data)
            continue
        walked += 1
        eos_ok = EOS in guide.allowed(state)
        assert eos_ok == _matches(pattern, data), (pattern, data)
        accepted += eos_ok
    assert walked > 50 and accepted > 0, (pattern, walked, accepted)


def _check_finite_language(guide, words):
    assert words
    prefixes = {w[:k] for w in words for k in range(len(w) + 1)}
    n_seg = 0
    for w in words:  # completeness: every tokenisation of every member
        for ids in G.segmentations(w, PIECES):
            n_seg += 1
            state = _walk(guide, ids)
            assert state is not None and EOS in guide.allowed(state), (w, ids)
            assert guide.allowed(guide.walk([EOS], state)).tolist() == [EOS]
    rng = np.random.default_rng(len(words))
    rejected = 0
    for ids in _random_sequences(guide, rng, 600, length=5):  # soundness: rejected at the first offending token
        data, state = b"", guide.start
        for j, t in enumerate(ids):
            data += PIECES[t]
            nxt = int(guide.table[state, t])
            assert (nxt != BANNED) == (data in prefixes), (data, ids[:j + 1])
            if nxt == BANNED:
                rejected += 1
                break
            state = nxt
        else:
            assert (EOS in guide.allowed(state)) == (data in set(words))
    assert rejected > 50 and n_seg >= len(words)


@pytest.mark.parametrize("pattern", list(FINITE))
def test_finite_regex_languages_are_complete_over_every_tokenisation(pattern):
    words = _language(pattern, FINITE[pattern])
    guide = TokenGuide.from_regex(pattern, PIECES, [EOS])
    _check_no_dead_ends(guide)
    _check_finite_language(guide, words)


def test_choices_guides_accept_every_tokenisation_of_the_choices_and_nothing_else():
    choices = ["yes", "no", "maybe", "abcd", "abc", "a\xe9", "12.5", "{\"a\":true}"]
    guide = TokenGuide.from_choices(choices, PIECES, [EOS])
    _check_no_dead_ends(guide)
    _check_finite_language(guide, [c.encode("utf-8") for c in choices])
    assert TokenGuide.from_choices([b"no"], PIECES, [EOS]).n_states == 4  # "", "n", "no", terminal
    with pytest.raises(ValueError, match="empty"):
        TokenGuide.from_choices([], PIECES, [EOS])


@pytest.mark.parametrize("pattern,construct", [
    (r"^abc", "anchor"), (r"abc$", "anchor"), (r"\bfoo", "anchor"), (r"a(?=b)", "look-around"), (r"(?<!a)b", "look-around"),
    (r"(a)\1", "back-reference"), (r"a*?", "lazy"), (r"a+?b", "lazy"), (r"a{1,2}?", "lazy"), (r"a*+", "possessive"),
    (r"(?i)abc", "flag"), (r"(?P<n>a)", "named group"), (r"[é-ü]", "non-ASCII"), (r"[^é]", "non-ASCII"),
    (r"(ab", "unbalanced"), (r"ab)", "unbalanced"), (r"a{2,1}", "n < m"), (r"*a", "nothing to repeat"), (r"[ab", "class"),
    (r"\p{L}", "escape"),
])
def test_unsupported_constructs_raise_naming_the_construct(pattern, construct):
    with pytest.raises(ValueError, match=re.escape(construct)):
        TokenGuide.from_regex(pattern, PIECES, [EOS])


def test_text_guides_need_eos_and_a_vocabulary_that_can_spell_the_text():
    with pytest.raises(ValueError, match="eos_ids"):
        TokenGuide.from_regex("a", PIECES, [])
    with pytest.raises(ValueError, match="eos_ids"):
        TokenGuide.from_choices(["a"], PIECES, ())
    with pytest.raises(ValueError, match="outside"):
        TokenGuide.from_regex("a", PIECES, [len(PIECES)])
    with pytest.raises(ValueError, match="spells"):
        TokenGuide.from_choices(["ab"], [b"a", b"c", b""], [2])
    # an id that leads only to a dead end is banned up front: "ab" or "ad" with no piece for "d"
    g = TokenGuide.from_regex("a(b|d)", [b"a", b"b", b"c", b""], [3])
    assert g.allowed(g.walk([0])).tolist() == [1]


def test_byte_budget_and_state_limit():
    big = [bytes([b]) for b in range(256)] * 8  # 2048 ids
    with pytest.raises(ValueError, match="budget"):
        TokenGuide.from_regex("a{300}", big, [5], max_bytes=1 << 20)
    assert TokenGuide.from_regex("a{100}", big, [5], max_bytes=1 << 20).n_states == 102
    with pytest.raises(ValueError, match="budget"):
        TokenGuide.from_bad_words([[1, 2, 3]] + [[4, i, 5] for i in range(300)], 2048, max_bytes=1 << 20)
    with pytest.raises(ValueError, match="budget"):
        TokenGuide(np.zeros((4, 1000), np.uint16), max_bytes=7999)
    with pytest.raises(ValueError, match="does not have"):
        TokenGuide(np.full((2, 4), 2, np.uint16))
    with pytest.raises(ValueError, match="65535"):
        TokenGuide(np.zeros((65536, 1), np.uint16))
    assert TokenGuide.from_regex("a{3}", [b"a", b""], [1]).table.dtype == np.uint16


BAD_WORDS = [[5, 6], [6, 7, 5, 6, 8], [9], [5, 6, 7], [6, 7], [7, 5], [3, 3, 3], [5, 6, 7, 5]]  # overlaps, suffixes, a single


def test_bad_words_guide_is_hugging_faces_rule_on_random_histories():
    vocab = 12
    guide = TokenGuide.from_bad_words(BAD_WORDS, vocab)
    assert guide.start == 0 and guide.eos_ids == ()
    rng = np.random.default_rng(3)
    hits = 0
    for _ in range(600):
        h = [int(t) for t in rng.integers(0, vocab, rng.integers(0, 12))]
        state = guide.prompt_state(h)  # a prompt may hold listed sequences: the automaton steps over them
        want = G.hf_banned(BAD_WORDS, h)
        assert set(range(vocab)) - set(guide.allowed(state).tolist()) == want, h
        hits += len(want) > 1
        legal = _walk(guide, h)  # a history that never completes a listed sequence walks the table itself
        if all(h[i] not in G.hf_banned(BAD_WORDS, h[:i]) for i in range(len(h))):
            assert legal == state
        else:
            assert legal is None
    assert hits > 100
    for bad in ([], [[]], [[1, vocab]], [[-1]]):
        with pytest.raises(ValueError):
            TokenGuide.from_bad_words(bad, vocab)
    with pytest.raises(ValueError, match="every id"):
        TokenGuide.from_bad_words([[0], [1]], 2)


def test_bad_words_guide_agrees_with_transformers_processor():
    transformers = pytest.importorskip("transformers")
    import torch

    vocab = 12
    guide = TokenGuide.from_bad_words(BAD_WORDS, vocab)
    proc = transformers.NoBadWordsLogitsProcessor(BAD_WORDS, eos_token_id=vocab + 5)
    rng = np.random.default_rng(4)
    for _ in range(200):
        # (histories no shorter than the longest word: the processor skips a word longer than the whole history, even
        # where the history ends with all of it but its last id — with a prompt in front that case does not arise)
        h = [int(t) for t in rng.integers(5, 8, rng.integers(5, 12))] if rng.random() < 0.5 else \
            [int(t) for t in rng.integers(0, vocab, rng.integers(5, 12))]
        scores = proc(torch.tensor([h]), torch.zeros(1, vocab))[0]
        banned = set(torch.nonzero(torch.isneginf(scores)).flatten().tolist())
        assert set(range(vocab)) - set(guide.allowed(guide.prompt_state(h)).tolist()) == banned, h


class _StubTokenizer:
    def __init__(self, pieces, special):
        self.pieces, self.all_special_ids = pieces, special

    def __len__(self):
        return len(self.pieces)

    def convert_ids_to_tokens(self, ids):
        return [self.pieces[i] for i in ids]


def test_token_bytes_on_sentencepiece_and_byte_level_pieces():
    sp = _StubTokenizer(["<unk>", "<s>", "</s>", "<0x0A>", "<0xE2>", "▁the", "▁", "é", "ab", None, "<0xZZ>"], [0, 1, 2])
    assert token_bytes(sp) == [b"", b"", b"", b"\n", b"\xe2", b" the", b" ", "é".encode(), b"ab", b"", b"<0xZZ>"]
    bl = _StubTokenizer(["<|endoftext|>", "Ġthe", "Ċ", "Ã©", "ab", "Ġ", "âĤ¬"], [0])
    assert token_bytes(bl) == [b"", b" the", b"\n", "é".encode(), b"ab", b" ", "€".encode()]
    # the bytes build a guide that spells text through them
    vb = token_bytes(sp)
    g = TokenGuide.from_choices([" the\n"], vb, [2])
    assert 2 in g.allowed(g.walk([5, 3])) and _walk(g, [3]) is None


def test_header_and_binding_name_the_guides_entry_points():
    from intel_extension_for_transformers_amd import _lib

    header = open(os.path.join(ROOT, "include", "woq_hip.h")).read()
    declared = set(re.findall(r"WOQ_API[^;(]*?\b(woq_\w+)\s*\(", header))
    new = {"woq_engine_set_guide", "woq_engine_guide_reset", "woq_engine_guide_state_ptr"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    exp = open(os.path.join(ROOT, "include", "woq_hip_experimental.h")).read()
    assert re.search(r"WOQ_API int woq_probe_guide\(", exp) and "woq_probe_guide" in _lib.EXPERIMENTAL_EXPORTS
    assert "#define WOQ_ABI_VERSION 4" in header and _lib.GUIDE_BANNED == BANNED == G.BANNED
