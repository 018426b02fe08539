"""Seeded generator of SPEC.md S5 regexes with matching examples, and of contents built
from them (shared by the CPU and GPU fuzz tests; a plain module, no fixtures).

A pattern is built as a small tree, so that the same tree can write the pattern text and
examples that match it by construction: at the minimum count of every repetition (the
common case), at random counts, or with one repetition given one copy fewer than its
minimum (a near miss).  Contents are noise over the words' own letters with examples and
mutated examples inserted.
"""
import random

# Literal words, 1-18 bytes, over a small alphabet.  Most hold a factor of >= 3 bytes (the
# prefilter is then usually on), several share a prefix (look-alikes), some hold '_' / '-'
# (short needles anchored on a rare byte) and two are >= 12 bytes (stride 8).
WORDS = [b"err", b"error", b"errno=", b"time", b"timeout", b"timer", b"stat", b"status=", b"tx-", b"tx-ab",
         b"k=v", b"ab", b"abab", b"to", b"x", b"e", b"user_id", b"pod-7", b"re_set", b"0123456789AB",
         b"deadline exceeded", b"took ", b"ms", b"rate=", b"a.b", b"beta", b"reset by peer"]
LONG_WORDS = [w for w in WORDS if len(w) >= 3]
NOISE = b"abertoxsmi01 =-_.KEdk7"

_LOWER = b"abdeikmorstx"
_CLASSES = [  # (pattern text, bytes an example draws from, whatever the case flag)
    (r"\d", b"0179"), (r"\w", b"ab0_Kx"), (r"\s", b" \t"), (r"\W", b" -=."), (".", b"ab0 -_K"),
    ("[a-c]", b"abc"), ("[^ab]", b"ert0 -_x"), ("[0-9a-f]", b"0a9fe"), ("[Kk]", b"Kk"),
    ("[[:alpha:]]", b"abKx"), ("[[:digit:]]", b"017"), ("[[:^alpha:]]", b"0 -=_"), ("[[:upper:]_]", b"KE_"),
    (r"[\d\s-]", b"0 -"),
]
_SPECIAL = b"\\.+*?()|[]{}^$"


def _esc(w: bytes) -> str:
    return "".join(("\\" + chr(c)) if c in _SPECIAL else chr(c) for c in w)


def _recase(rng, b: bytes) -> bytes:
    return bytes(c ^ 0x20 if (65 <= c <= 90 or 97 <= c <= 122) and rng.random() < 0.5 else c for c in b)


class _Lit:
    def __init__(self, text: bytes, pat: str, icase: bool):
        self.text, self.pat, self.icase = text, pat, icase

    def gen(self, rng, cx):
        return _recase(rng, self.text) if self.icase and rng.random() < 0.3 else self.text


class _Cls:
    def __init__(self, pat: str, draw: bytes):
        self.pat, self.draw = pat, draw

    def gen(self, rng, cx):
        return bytes([rng.choice(self.draw)])


class _Cat:
    def __init__(self, items, texts):
        self.items = items
        self.pat = "".join(texts)

    def gen(self, rng, cx):
        return b"".join(i.gen(rng, cx) for i in self.items)


class _Group:
    def __init__(self, opener: str, alts):
        self.alts = alts
        self.pat = opener + "|".join(a.pat for a in alts) + ")"

    def gen(self, rng, cx):
        return rng.choice(self.alts).gen(rng, cx)


class _Rep:
    def __init__(self, node, lo: int, hi, op: str):
        self.node, self.lo, self.hi = node, lo, hi  # hi None: unbounded
        self.pat = node.pat + op

    def gen(self, rng, cx):
        if cx.get("short") is self:
            n = self.lo - 1
        elif cx["mode"] == "min" or self.hi == self.lo:
            n = self.lo
        else:
            n = rng.randint(self.lo, self.lo + 2 if self.hi is None else min(self.hi, self.lo + 2))
        return b"".join(self.node.gen(rng, cx) for _ in range(n))


_REPS = [("*", 0, None), ("+", 1, None), ("?", 0, 1), ("{1}", 1, 1), ("{2}", 2, 2), ("{3}", 3, 3),
         ("{0,}", 0, None), ("{1,}", 1, None), ("{2,}", 2, None), ("{3,}", 3, None),
         ("{1,3}", 1, 3), ("{0,2}", 0, 2), ("{2,3}", 2, 3), ("{0,0}", 0, 0)]


class Pat:
    """One generated regex: `pattern` (bytes), whether it is anchored at the content's start
    (`bol`) / end (`eol`), and examples of it."""

    def __init__(self, root, bol: bool, eol: bool, reps):
        self.root, self.bol, self.eol = root, bol, eol
        self.pattern = root.pat.encode()
        self.shortable = [r for r in reps if r.lo >= 1]

    def example(self, rng, mode="min") -> bytes:
        """A text the pattern matches (for an anchored pattern: when placed at that end of the
        content).  mode "min": every repetition at its minimum count; "rand": random counts."""
        return self.root.gen(rng, {"mode": mode})

    def near_miss(self, rng):
        """An example with one repetition one copy short of its minimum (None: no repetition
        with a minimum)."""
        if not self.shortable:
            return None
        return self.root.gen(rng, {"mode": "min", "short": rng.choice(self.shortable)})


class _Builder:
    def __init__(self, rng):
        self.rng = rng
        self.reps = []

    def atom(self, depth, flag):
        rng = self.rng
        k = rng.random()
        if k < 0.16 and depth < 2:
            opener = rng.choice(["(", "(?:", "(?:", "(?i:", "(?P<g>"])
            inner = [flag[0] or opener == "(?i:"]  # flag changes inside stay inside
            alts = [self.concat(depth + 1, inner, rng.randint(1, 2)) for _ in range(rng.randint(1, 3))]
            if rng.random() < 0.15:
                alts.append(_Cat([], []))  # an empty alternative
            return _Group(opener, alts)
        if k < 0.21:
            w = rng.choice([b"a.b", b"k=v", b"x*", b"to", b"tx-ab"])
            return _Lit(w, "\\Q" + w.decode() + "\\E", flag[0])
        if k < 0.48:
            return _Cls(*rng.choice(_CLASSES))
        w = rng.choice(WORDS)
        if depth and len(w) > 7:
            w = rng.choice(WORDS)  # (long words mostly at the top: the 64-position budget)
        return _Lit(w, _esc(w), flag[0])

    def repeated(self, node):
        rng = self.rng
        if isinstance(node, _Lit) and len(node.text) > 1 and not node.pat.startswith("\\Q") and rng.random() < 0.8:
            # a repetition after a word binds to its last byte only
            head = _Lit(node.text[:-1], _esc(node.text[:-1]), node.icase)
            last = _Lit(node.text[-1:], _esc(node.text[-1:]), node.icase)
            return self._cat2(head, self.repeated(last))
        if isinstance(node, _Lit) and len(node.text) > 1:
            if node.pat.startswith("\\Q"):  # a repetition after \E takes the quoted text's last byte
                head = _Lit(node.text[:-1], "", node.icase)
                last = _Lit(node.text[-1:], node.pat, node.icase)
                return self._cat2(head, self.repeated(last))
            node = _Group("(?:", [node])
        if rng.random() < 0.06:  # `{01}`: leading zeros make it literal text, not a repetition
            return self._cat2(node, _Lit(b"{01}", "{01}", False))
        op, lo, hi = rng.choice(_REPS)
        if rng.random() < 0.2:
            op += "?"  # lazy: the same boolean match
        r = _Rep(node, lo, hi, op)
        self.reps.append(r)
        return r

    @staticmethod
    def _cat2(a, b):
        return _Cat([a, b], [a.pat, b.pat])

    def concat(self, depth, flag, n_items, need_word=False):
        rng = self.rng
        items, texts = [], []
        word_at = rng.randrange(n_items) if need_word else -1
        for k in range(n_items):
            if k == word_at:
                w = rng.choice(LONG_WORDS)
                a = _Lit(w, _esc(w), flag[0])
                if rng.random() < 0.25:
                    a = self.repeated(a)
            else:
                a = self.atom(depth, flag)
                if rng.random() < 0.4:
                    a = self.repeated(a)
            items.append(a)
            texts.append(a.pat)
            if rng.random() < 0.07:  # a flag group: holds for the rest of this group
                f = rng.choice(["(?i)", "(?-i)", "(?s)"])
                texts.append(f)
                if f != "(?s)":
                    flag[0] = f == "(?i)"
                whole = isinstance(a, (_Cls, _Group, _Rep)) or (isinstance(a, _Lit) and len(a.text) == 1)
                if whole and rng.random() < 0.4:  # a repetition after the flag group takes the item before it
                    op, lo, hi = rng.choice(_REPS)
                    r = _Rep(items[-1], lo, hi, f + op)
                    self.reps.append(r)
                    items[-1] = r
                    texts.append(op)
        return _Cat(items, texts)


def pattern(rng) -> Pat:
    """One random pattern of the S5 subset (nesting to depth 2)."""
    b = _Builder(rng)
    flag = [False]
    lead = ""
    if rng.random() < 0.15:
        lead, flag[0] = "(?i)", True
    bol = rng.random() < 0.1
    eol = rng.random() < 0.1
    items = []
    if rng.random() < 0.12:  # an unbounded prefix: no bound on the match start before any factor
        op, lo, hi = rng.choice([("+", 1, None), ("*", 0, None), ("{2,}", 2, None)])
        items.append(_Rep(_Cls(*rng.choice(_CLASSES)), lo, hi, op))
        b.reps.append(items[0])
    items.append(b.concat(0, flag, rng.randint(1, 4), need_word=rng.random() < 0.8))
    texts = ([lead, rng.choice(["^", "\\A"]) if bol else ""] + [i.pat for i in items]
             + [rng.choice(["$", "\\z"]) if eol else ""])
    root = _Cat(items, texts)
    return Pat(root, bol, eol, b.reps)


def corrupt(rng, pat: bytes) -> bytes:
    """The pattern with one byte dropped, doubled or replaced by a syntax byte (it may then
    lie outside the subset: the compilers must agree on that too)."""
    if not pat:
        return pat
    k = rng.randrange(len(pat))
    op = rng.randrange(3)
    if op == 0:
        return pat[:k] + pat[k + 1:]
    if op == 1:
        return pat[:k] + pat[k:k + 1] + pat[k:]
    return pat[:k] + bytes([rng.choice(b"()[]{}*+?|\\^$-,:ab0")]) + pat[k + 1:]


def noise(rng, n: int) -> bytes:
    return bytes(rng.choice(NOISE) for _ in range(n))


def fragment(rng, p: Pat) -> bytes:
    """An example of p as is, or mutated: one byte changed / dropped, re-cased, cut at the
    front or the back, or one repetition short of its minimum."""
    ex = p.example(rng, "min" if rng.random() < 0.6 else "rand")
    k = rng.random()
    if k < 0.5 or not ex:
        return ex
    if k < 0.6:
        i = rng.randrange(len(ex))
        return ex[:i] + bytes([rng.choice(NOISE)]) + ex[i + 1:]
    if k < 0.7:
        i = rng.randrange(len(ex))
        return ex[:i] + ex[i + 1:]
    if k < 0.78:
        return _recase(rng, ex)
    if k < 0.86:
        c = rng.randint(1, max(1, len(ex) // 2))
        return ex[c:] if rng.random() < 0.5 else ex[:-c]
    nm = p.near_miss(rng)
    return ex if nm is None else nm


def content(rng, pats, max_noise=40) -> bytes:
    """Noise with 0-3 fragments of `pats` inserted (a pattern anchored at the content's start
    or end mostly gets its fragment there)."""
    s = noise(rng, rng.randint(0, max_noise)) if rng.random() < 0.85 else b""
    for _ in range(rng.choice([0, 1, 1, 1, 2, 3])):
        p = rng.choice(pats)
        f = fragment(rng, p)
        if p.bol and p.eol and rng.random() < 0.6:
            s = f
        elif p.bol and rng.random() < 0.7:
            s = f + s
        elif p.eol and rng.random() < 0.7:
            s = s + f
        else:
            k = rng.randint(0, len(s))
            s = s[:k] + f + s[k:]
    return s


def pattern_set(rng, max_rx=3, max_lit=1):
    """(literals, [Pat]) of one --grep / --match set: 1..max_rx regexes, 0..max_lit literals."""
    pats = [pattern(rng) for _ in range(rng.randint(1, max_rx))]
    lits = [rng.choice(LONG_WORDS) for _ in range(rng.randint(0, max_lit))]
    return lits, pats
