"""Reference pieces for the token guide (runtime/guide.py, csrc/woq_sample.hip `score_adjust_kernel<true>` and
`guide_advance_kernel`), shared by tests/test_guide_cpu.py and the GPU guide tests.

* `masked_f32`: step 5 of the score contract on top of tests/sampler_controls_reference.py: -inf where the state's row
  holds 0xFFFF, every other score untouched.
* `advance`: the state after a pick (the state stays on a banned pick).
* `synthetic_vocab`: about 300 pieces — the 256 single bytes, multi-byte pieces, overlapping pieces ("a", "ab", "abc"),
  a few empty specials and one EOS.
* `segmentations`: every way to spell a byte string with the vocabulary's pieces.
* `hf_banned`: Hugging Face's NoBadWordsLogitsProcessor rule, restated.
"""
import numpy as np

BANNED = 0xFFFF
NEG_INF = np.float32("-inf")


def masked_f32(scores, row):
    out = np.asarray(scores, dtype=np.float32).copy()
    out[np.asarray(row) == BANNED] = NEG_INF
    return out


def advance(table, state, token):
    """-> (state after the pick, status bit)"""
    nxt = int(table[state, token])
    return (state, 16) if nxt == BANNED else (nxt, 0)


def random_table(rng, n_states, vocab, ban=0.5):
    """uint16 [n_states][vocab]: about `ban` of each row banned, the rest random states; every row keeps an allowed id"""
    t = rng.integers(0, n_states, (n_states, vocab)).astype(np.uint16)
    t[rng.random((n_states, vocab)) < ban] = BANNED
    for s in range(n_states):
        if (t[s] == BANNED).all():
            t[s, rng.integers(0, vocab)] = rng.integers(0, n_states)
    return t


MULTI = [b"ab", b"abc", b"abcd", b"bc", b"cd", b"ba", b"aa", b"aaa", b"yes", b"no", b"ye", b"es", b"s ", b" y", b"maybe",
         b"may", b"be", b"12", b"123", b"23", b"0x", b"1.", b".5", b"-1", b"xy", b"yz", b"xyz", b"\xc3\xa9", b"\xc3",
         b"\xe2\x82\xac", b"\xe2\x82", b"a\xc3\xa9", b"\n\n", b" \t", b"__", b"a_", b"_1", b"A1", b"Zz", b"{\"", b"\":",
         b"true", b"false", b"tr", b"ue", b"fal", b"se", b"nu", b"ll", b"null"]


def synthetic_vocab():
    """-> (list[bytes], eos id, ids of the empty specials)"""
    pieces = [bytes([b]) for b in range(256)] + list(MULTI)
    specials = list(range(len(pieces), len(pieces) + 3))
    pieces += [b"", b"", b""]
    eos = len(pieces)
    pieces.append(b"")
    return pieces, eos, specials


def segmentations(text, pieces, limit=20000):
    """every list of ids whose pieces concatenate to `text` (bytes); stops with an AssertionError beyond `limit`"""
    by_first = {}
    for i, p in enumerate(pieces):
        if p:
            by_first.setdefault(p[0], []).append((i, p))
    out = []

    def rec(at, acc):
        if at == len(text):
            out.append(list(acc))
            assert len(out) <= limit
            return
        for i, p in by_first.get(text[at], ()):
            if text.startswith(p, at):
                acc.append(i)
                rec(at + len(p), acc)
                acc.pop()

    rec(0, [])
    return out


def hf_banned(words, history):
    """ids Hugging Face's NoBadWordsLogitsProcessor bans after `history`: t iff some word equals h[-k:] + [t]"""
    h, out = list(history), set()
    for w in words:
        k = len(w) - 1
        if k == 0 or (len(h) >= k and h[len(h) - k:] == list(w[:-1])):
            out.add(int(w[-1]))
    return out
