"""Token guides: deterministic automata over token ids that the native decode step follows on the device (constrained
decoding). Pure numpy, no GPU: the builders make the dense table `next[n_states][vocab]` of uint16 that
`WoqDecoderEngine.set_guide` uploads (0xFFFF = the id is banned in that state, anything else = the state after that id;
include/woq_hip.h woq_engine_set_guide).

  TokenGuide.from_regex(pattern, vocab_bytes, eos_ids)     full match of the generated text's UTF-8 bytes
  TokenGuide.from_choices(choices, vocab_bytes, eos_ids)   the text is one of the strings, in any tokenisation
  TokenGuide.from_bad_words(bad_words_ids, vocab)          Hugging Face's NoBadWordsLogitsProcessor

Text guides express completion with EOS: in an accepting state the `eos_ids` are allowed and lead to a terminal state
that allows only `eos_ids`, so the caller's EOS handling ends the request. Every builder prunes the states from which
no accepting state can be reached and bans the ids that lead to them: every reachable state keeps an allowed id.
`token_bytes(tokenizer)` gives the `vocab_bytes` of a Hugging Face tokenizer."""
import numpy as np

BANNED = 0xFFFF
MAX_STATES = 65535
DEFAULT_MAX_BYTES = 1 << 30


def _check_budget(n_states, vocab, max_bytes):
    if n_states > MAX_STATES:
        raise ValueError("the guide needs %d states; a token guide has at most %d" % (n_states, MAX_STATES))
    need = int(n_states) * int(vocab) * 2
    if need > int(max_bytes):
        raise ValueError("the guide's table (%d states x %d ids x 2 bytes = %d bytes) exceeds the budget of %d bytes"
                         % (n_states, vocab, need, int(max_bytes)))


class TokenGuide:
    """`table` np.uint16 [S][V], `start` the state of an empty text, `eos_ids` the ids that end a text guide."""

    def __init__(self, table, start=0, eos_ids=(), max_bytes=DEFAULT_MAX_BYTES):
        table = np.ascontiguousarray(table, dtype=np.uint16)
        if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError("a guide's table is [n_states >= 1][vocab >= 1]")
        _check_budget(table.shape[0], table.shape[1], max_bytes)
        if not 0 <= int(start) < table.shape[0]:
            raise ValueError("the start state is outside the table")
        if bool(((table != BANNED) & (table >= table.shape[0])).any()):
            raise ValueError("the table names a state it does not have")
        self.table, self.start, self.eos_ids = table, int(start), tuple(int(e) for e in eos_ids)
        self._goto = None  # from_bad_words: the automaton's own transition, which also steps over a listed sequence

    @property
    def n_states(self):
        return int(self.table.shape[0])

    @property
    def vocab(self):
        return int(self.table.shape[1])

    def allowed(self, state):
        """ids allowed in `state`, ascending (np.int64)"""
        return np.flatnonzero(self.table[int(state)] != BANNED)

    def walk(self, ids, state=None):
        """the state after `ids` from `state` (default: start); ValueError at the first banned id"""
        s = self.start if state is None else int(state)
        for j, t in enumerate(ids):
            nxt = int(self.table[s, int(t)])
            if nxt == BANNED:
                raise ValueError("id %d (index %d) is banned in state %d" % (int(t), j, s))
            s = nxt
        return s

    def prompt_state(self, prompt_ids):
        """The state a request starts in after its prompt. A bad-words guide matches across the prompt boundary and a
        prompt may itself hold a listed sequence, so it follows the automaton without the bans; a text guide constrains
        the generated text alone and starts at `start`."""
        if self._goto is None:
            return self.start
        s = self.start
        for t in prompt_ids:
            s = self._goto(s, int(t))
        return s

    # ---- builders ----------------------------------------------------------------------------------------------------
    @classmethod
    def from_regex(cls, pattern, vocab_bytes, eos_ids, max_bytes=DEFAULT_MAX_BYTES):
        """Texts whose UTF-8 bytes fully match `pattern`. Syntax: literals, escapes (\\n \\t \\r \\f \\v \\0 \\xNN and
        escaped punctuation), `.` (any code point but newline), classes with ranges and negation, \\d \\w \\s (ASCII)
        and their negations, groups `( )` / `(?: )`, `|`, `* + ?`, `{m}` `{m,}` `{m,n}`. Anything else (anchors,
        look-around, back-references, lazy or possessive quantifiers, flags, named groups, non-ASCII ranges) raises
        ValueError naming the construct."""
        dfa, accept = _regex_dfa(pattern)
        return cls._lifted(dfa, accept, vocab_bytes, eos_ids, max_bytes)

    @classmethod
    def from_choices(cls, choices, vocab_bytes, eos_ids, max_bytes=DEFAULT_MAX_BYTES):
        """Texts equal to one of `choices` (str or bytes), spelled by any sequence of tokens."""
        words = [c.encode("utf-8") if isinstance(c, str) else bytes(c) for c in choices]
        if not words:
            raise ValueError("`choices` is empty")
        rows, accept = [np.full(256, -1, np.int32)], [False]
        for w in words:
            s = 0
            for b in w:
                if rows[s][b] < 0:
                    rows[s][b] = len(rows)
                    rows.append(np.full(256, -1, np.int32))
                    accept.append(False)
                s = int(rows[s][b])
            accept[s] = True
        return cls._lifted(np.stack(rows), np.array(accept), vocab_bytes, eos_ids, max_bytes)

    @classmethod
    def _lifted(cls, dfa, accept, vocab_bytes, eos_ids, max_bytes):
        """byte DFA [S][256] (int32, -1 = no transition, state 0 = start) -> token guide"""
        eos = sorted(set(int(e) for e in eos_ids))
        V = len(vocab_bytes)
        if not eos:
            raise ValueError("a text guide needs a non-empty `eos_ids`: completion is expressed with EOS")
        if any(not 0 <= e < V for e in eos):
            raise ValueError("an EOS id is outside the vocabulary")
        S = int(dfa.shape[0])
        _check_budget(S + 1, V, max_bytes)  # before the lift allocates it (pruning can only shrink it)
        lens = np.array([len(b) for b in vocab_bytes], np.int64)
        lmax = max(int(lens.max()) if V else 0, 1)
        mat = np.zeros((V, lmax), np.uint8)
        for i, b in enumerate(vocab_bytes):
            if b:
                mat[i, :len(b)] = np.frombuffer(b, np.uint8)
        step = np.vstack([np.where(dfa < 0, S, dfa), np.full((1, 256), S)]).astype(np.int32)  # row S: the dead state
        T = S  # the terminal state's index in the unpruned table
        table = np.empty((S + 1, V), np.int32)
        block = max(1, (1 << 24) // max(V, 1))  # states per pass: bounds the [block][V] temporaries
        for s0 in range(0, S, block):
            cur = np.repeat(np.arange(s0, min(S, s0 + block), dtype=np.int32)[:, None], V, axis=1)
            for j in range(lmax):  # one gather per byte position over every (state, token) at once
                live = lens > j
                cur[:, live] = step[cur[:, live], mat[live, j][None, :]]
            table[s0:s0 + cur.shape[0]] = cur
        table[:S][table[:S] == S] = -1  # ran into the dead state
        table[:, lens == 0] = -1  # a token that spells nothing is never allowed by a text guide
        table[T] = -1
        acc = np.zeros(S + 1, bool)
        acc[:S] = np.asarray(accept, bool)
        acc[T] = True
        for e in eos:
            table[:, e] = np.where(acc, T, -1)
        return cls._pruned(table, 0, T, V, eos, max_bytes)

    @classmethod
    def _pruned(cls, table, start, final, V, eos, max_bytes):
        """int32 table (-1 = banned): keep the states on a path start -> ... -> final, ban the ids that leave them"""
        n = table.shape[0]
        succ = [np.unique(row[row >= 0]) for row in table]
        good = np.zeros(n, bool)
        good[final] = True
        changed = True
        while changed:  # states that can reach the final state
            changed = False
            for s in range(n):
                if not good[s] and succ[s].size and good[succ[s]].any():
                    good[s] = changed = True
        if not good[start]:
            raise ValueError("no sequence of tokens of this vocabulary spells a text the guide accepts")
        keep = np.zeros(n, bool)
        todo = [start]
        keep[start] = True
        while todo:
            s = todo.pop()
            for t in succ[s]:
                if good[t] and not keep[t]:
                    keep[t] = True
                    todo.append(int(t))
        new_id = np.full(n + 1, -1, np.int64)  # slot n: the banned entry
        order = np.flatnonzero(keep)
        order = np.concatenate([[start], order[order != start]])  # start becomes state 0
        new_id[order] = np.arange(order.size)
        _check_budget(order.size, V, max_bytes)
        out = new_id[np.where(table[order] < 0, n, table[order])]
        return cls(np.where(out < 0, BANNED, out).astype(np.uint16), 0, eos, max_bytes)

    @classmethod
    def from_bad_words(cls, bad_words_ids, vocab, max_bytes=DEFAULT_MAX_BYTES):
        """Hugging Face's NoBadWordsLogitsProcessor as an Aho-Corasick automaton over token ids: id t is banned after a
        history h iff some listed sequence equals h[-k:] + [t] (k = its length - 1; single-token words are banned
        everywhere). No EOS logic. `start` is the empty history; a request starts at `prompt_state(prompt_ids)`."""
        V = int(vocab)
        words = []
        for w in bad_words_ids:
            w = [int(t) for t in w]
            if not w or any(not 0 <= t < V for t in w):
                raise ValueError("`bad_words_ids` holds non-empty lists of ids inside the vocabulary")
            words.append(w)
        if not words:
            raise ValueError("`bad_words_ids` is empty")
        # trie of the sequences without their last id; out[node] = the ids that would complete a sequence there
        child, out = [{}], [set()]
        for w in words:
            s = 0
            for t in w[:-1]:
                if t not in child[s]:
                    child[s][t] = len(child)
                    child.append({})
                    out.append(set())
                s = child[s][t]
            out[s].add(w[-1])
        n = len(child)
        _check_budget(n, V, max_bytes)
        goto = np.zeros((n, V), np.uint16)  # the automaton without the bans: the longest suffix that is a trie node
        fail = [0] * n
        queue = [0]
        for s in queue:  # breadth first: a node's failure row is complete before the node's own
            if s:
                goto[s] = goto[fail[s]]
                out[s] |= out[fail[s]]  # sequences that end inside a longer one's prefix
            for t, c in child[s].items():
                fail[c] = int(goto[s, t]) if s else 0  # read before the child's edge overwrites it
                queue.append(c)
            for t, c in child[s].items():
                goto[s, t] = c
        table = goto.copy()
        for s in range(n):
            if out[s]:
                table[s, sorted(out[s])] = BANNED
        if bool((table == BANNED).all(axis=1).any()):
            raise ValueError("`bad_words_ids` bans every id of the vocabulary in some state")
        g = cls(table, 0, (), max_bytes)
        g._goto = lambda s, t: int(goto[s, t])
        return g


# ---- regular expressions over UTF-8 bytes: parser -> Thompson NFA -> subset construction --------------------------------
_ALL_ASCII = (1 << 128) - 1
_DIGIT = sum(1 << c for c in range(48, 58))
_WORD = _DIGIT | sum(1 << c for c in range(65, 91)) | sum(1 << c for c in range(97, 123)) | (1 << 95)
_SPACE = sum(1 << c for c in b" \t\n\r\f\v")
_SHORT = {"d": (_DIGIT, False), "w": (_WORD, False), "s": (_SPACE, False),
          "D": (_DIGIT, True), "W": (_WORD, True), "S": (_SPACE, True)}
_CTRL = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "0": 0, "a": 7}
# every UTF-8 encoded code point above U+007F, as byte ranges per position (RFC 3629: no overlongs, no surrogates)
_MULTIBYTE = [[(0xC2, 0xDF), (0x80, 0xBF)],
              [(0xE0, 0xE0), (0xA0, 0xBF), (0x80, 0xBF)], [(0xE1, 0xEC), (0x80, 0xBF), (0x80, 0xBF)],
              [(0xED, 0xED), (0x80, 0x9F), (0x80, 0xBF)], [(0xEE, 0xEF), (0x80, 0xBF), (0x80, 0xBF)],
              [(0xF0, 0xF0), (0x90, 0xBF), (0x80, 0xBF), (0x80, 0xBF)],
              [(0xF1, 0xF3), (0x80, 0xBF), (0x80, 0xBF), (0x80, 0xBF)],
              [(0xF4, 0xF4), (0x80, 0x8F), (0x80, 0xBF), (0x80, 0xBF)]]
_MAX_NFA = 200000


def _range_mask(lo, hi):
    return ((1 << (hi + 1)) - 1) ^ ((1 << lo) - 1)


class _Parser:
    """pattern -> tree of ("lit", bytes) | ("set", ascii_mask, any_multibyte, [bytes of single non-ASCII members]) |
    ("cat", [..]) | ("alt", [..]) | ("rep", node, m, n or None)"""

    def __init__(self, pattern):
        if not isinstance(pattern, str):
            raise ValueError("the pattern is a str")
        self.p, self.i = pattern, 0

    def fail(self, what):
        raise ValueError("unsupported in a guide's regular expression: %s (at offset %d of %r)" % (what, self.i, self.p))

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced `)`")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        parts = []
        while self.peek() not in ("", "|", ")"):
            parts.append(self.repeat())
        return ("cat", parts)

    def repeat(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "?":
                m, n = 0, 1
            elif c == "{":
                end = self.p.find("}", self.i)
                body = self.p[self.i + 1:end] if end > 0 else ""
                lo, sep, hi = body.partition(",")
                if not lo.isdigit() or (hi and not hi.isdigit()):
                    self.fail("`{` that is no {m}, {m,} or {m,n}")
                m = int(lo)
                n = m if not sep else (int(hi) if hi else None)
                if n is not None and n < m:
                    self.fail("a repetition {m,n} with n < m")
                self.i = end
            else:
                return node
            self.i += 1
            if self.peek() == "?":
                self.fail("lazy quantifier")
            if self.peek() == "+":
                self.fail("possessive quantifier")
            node = ("rep", node, m, n)

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] == ":":
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    self.fail("look-around")
                elif nxt[:1] == "P" or nxt[:1] == "<":
                    self.fail("named group")
                else:
                    self.fail("inline flag or group extension `(?`")
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced `(`")
            self.i += 1
            return node
        if c == "[":
            return self.klass()
        if c == ".":
            return ("set", _ALL_ASCII ^ (1 << 10), True, [])
        if c in "^$":
            self.i -= 1
            self.fail("anchor `%s` (a guide always matches the whole text)" % c)
        if c in "*+?{":
            self.i -= 1
            self.fail("a quantifier with nothing to repeat")
        if c == "\\":
            kind, val = self.escape()
            if kind == "set":
                mask, neg = val
                return ("set", (_ALL_ASCII ^ mask) if neg else mask, neg, [])
            return ("lit", val.encode("utf-8"))
        return ("lit", c.encode("utf-8"))

    def escape(self):
        """after a backslash -> ("set", (mask, negated)) | ("chr", str)"""
        c = self.peek()
        if c == "":
            self.fail("a trailing backslash")
        self.i += 1
        if c in _SHORT:
            return "set", _SHORT[c]
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(d not in "0123456789abcdefABCDEF" for d in h):
                self.fail("`\\x` without two hex digits")
            self.i += 2
            return "chr", chr(int(h, 16))
        if c in _CTRL:
            return "chr", chr(_CTRL[c])
        if c.isdigit():
            self.i -= 1
            self.fail("back-reference")
        if c in "bBAZ":
            self.i -= 1
            self.fail("anchor `\\%s`" % c)
        if c.isalnum():
            self.i -= 1
            self.fail("escape `\\%s`" % c)
        return "chr", c

    def klass(self):
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        mask, extra, first = 0, [], True
        while True:
            c = self.peek()
            if c == "":
                self.fail("unterminated class")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            self.i += 1
            if c == "\\":
                kind, val = self.escape()
                if kind == "set":
                    m, n = val
                    if n:
                        self.fail("a negated shorthand inside a class")
                    mask |= m
                    continue
                c = val
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.peek()
                self.i += 1
                if hi == "\\":
                    kind, hi = self.escape()
                    if kind == "set":
                        self.fail("a shorthand as the end of a range")
                if ord(c) > 127 or ord(hi) > 127:
                    self.fail("a class range over non-ASCII characters")
                if ord(hi) < ord(c):
                    self.fail("a reversed class range")
                mask |= _range_mask(ord(c), ord(hi))
            elif ord(c) < 128:
                mask |= 1 << ord(c)
            else:
                extra.append(c.encode("utf-8"))
        if neg:
            if extra:
                self.fail("a negated class with non-ASCII members")
            return ("set", _ALL_ASCII ^ mask, True, [])
        return ("set", mask, False, extra)


class _Nfa:
    def __init__(self):
        self.eps, self.edges = [], []  # per state: [targets], [(256-bit byte mask, target)]

    def state(self):
        if len(self.eps) >= _MAX_NFA:
            raise ValueError("the regular expression is too large for a guide (more than %d NFA states)" % _MAX_NFA)
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def seq(self, a, ranges):
        """a chain of byte-range edges from `a`; -> its last state"""
        for lo, hi in ranges:
            b = self.state()
            self.edges[a].append((_range_mask(lo, hi), b))
            a = b
        return a

    def build(self, node):
        """-> (entry, exit) of a fresh fragment"""
        kind = node[0]
        a = self.state()
        if kind == "lit":
            return a, self.seq(a, [(b, b) for b in node[1]])
        z = self.state()
        if kind == "set":
            _, mask, multibyte, extra = node
            if mask:
                self.edges[a].append((mask, z))
            for ranges in (_MULTIBYTE if multibyte else []):
                self.eps[self.seq(a, ranges)].append(z)
            for b in extra:
                self.eps[self.seq(a, [(x, x) for x in b])].append(z)
        elif kind == "cat":
            cur = a
            for part in node[1]:
                s, e = self.build(part)
                self.eps[cur].append(s)
                cur = e
            self.eps[cur].append(z)
        elif kind == "alt":
            for part in node[1]:
                s, e = self.build(part)
                self.eps[a].append(s)
                self.eps[e].append(z)
        else:  # rep: m copies, then n - m optional ones or a loop
            _, inner, m, n = node
            cur = a
            for _ in range(m):
                s, e = self.build(inner)
                self.eps[cur].append(s)
                cur = e
            if n is None:
                s, e = self.build(inner)
                self.eps[cur].append(s)
                self.eps[e].append(cur)
            else:
                for _ in range(n - m):
                    s, e = self.build(inner)
                    self.eps[cur].append(z)
                    self.eps[cur].append(s)
                    cur = e
            self.eps[cur].append(z)
        return a, z


def check_regex(pattern):
    """ValueError naming the construct when `from_regex` does not take `pattern` (syntax only: no vocabulary needed)"""
    _Parser(pattern).parse()


def _regex_dfa(pattern):
    """-> (int32 [S][256] with -1 = no transition, bool [S] accepting); state 0 is the start"""
    nfa = _Nfa()
    entry, final = nfa.build(_Parser(pattern).parse())

    def closure(states):
        seen, todo = set(states), list(states)
        while todo:
            for t in nfa.eps[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)

    first = closure([entry])
    index, rows, todo = {first: 0}, [], [first]
    while todo:
        cur = todo.pop()
        edges = [e for s in cur for e in nfa.edges[s]]
        row = np.full(256, -1, np.int32)
        cache = {}
        for b in range(256):
            key = tuple(t for m, t in edges if (m >> b) & 1)
            if not key:
                continue
            if key not in cache:
                nxt = closure(key)
                if nxt not in index:
                    index[nxt] = len(index)
                    todo.append(nxt)
                    if len(index) > 4 * MAX_STATES:
                        raise ValueError("the regular expression needs more than %d states" % MAX_STATES)
                cache[key] = index[nxt]
            row[b] = cache[key]
        rows.append((index[cur], row))
    dfa = np.empty((len(index), 256), np.int32)
    for i, row in rows:
        dfa[i] = row
    accept = np.zeros(len(index), bool)
    for states, i in index.items():
        accept[i] = final in states
    return dfa, accept


# ---- the bytes a tokenizer's ids spell -----------------------------------------------------------------------------
def _gpt2_byte_decoder():
    """GPT-2's printable stand-ins for the 256 bytes (byte-level BPE), inverted: character -> byte"""
    keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    chars, n = {}, 0
    for b in range(256):
        if b in keep:
            chars[chr(b)] = b
        else:
            chars[chr(256 + n)] = b
            n += 1
    return chars


def token_bytes(tokenizer):
    """list[bytes] of length vocab: what each id contributes to the text. SentencePiece pieces: `▁` is a space and
    `<0xNN>` that byte; byte-level BPE pieces go through the GPT-2 byte map; special and unknown ids give b"" (a text
    guide never allows those, except EOS)."""
    n = len(tokenizer)
    pieces = tokenizer.convert_ids_to_tokens(list(range(n)))
    special = set(int(i) for i in getattr(tokenizer, "all_special_ids", ()) or ())
    special |= set(int(i) for i in getattr(tokenizer, "added_tokens_decoder", {}) or {})
    dec = _gpt2_byte_decoder()
    plain = [p for i, p in enumerate(pieces) if isinstance(p, str) and i not in special]
    byte_level = any("Ġ" in p for p in plain) and not any("▁" in p for p in plain)
    out = []
    for i, p in enumerate(pieces):
        if i in special or not isinstance(p, str):
            out.append(b"")
        elif byte_level:
            out.append(bytes(dec[c] for c in p) if all(c in dec for c in p) else b"")
        elif len(p) == 6 and p.startswith("<0x") and p.endswith(">"):
            try:
                out.append(bytes([int(p[3:5], 16)]))
            except ValueError:
                out.append(p.encode("utf-8"))
        else:
            out.append(p.replace("▁", " ").encode("utf-8"))
    return out
