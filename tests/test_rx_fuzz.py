"""The pattern compiler (klf_patterns.cpp: parser, {m,n} expansion, Glushkov tables, required
factors and their match-start bounds, prefilter placement) fuzzed on the host against
Python re (the Python oracle's translation) with the C oracle's regex leg as a second
reference.  Patterns, examples that match by construction and near misses come from
tests/rxfuzz.py; nothing here derives an expectation from the code under test."""
import functools
import json
import random
import re
import subprocess
import sys
from pathlib import Path

import pytest

import c_oracle as co
import klf_oracle as po
import rxfuzz
from klogs_amd import engine as E

ROOT = Path(__file__).resolve().parent.parent
SEEDS = range(8)
SETS_PER_SEED = 36
CONTENTS_PER_SET = 40


def _py(pat):
    """The Python oracle's compiled pattern, or None when it is outside the subset."""
    try:
        return po.Pattern("regex", pat)
    except (po.PatternError, re.error):
        return None


@functools.lru_cache(maxsize=None)
def _corpus(seed):
    """The seed's pattern sets with their contents and the reference's answers:
    (sets, stats); a set = (literals, [Pat], [reference pattern], [(content, want)])."""
    rng = random.Random(7000 + seed)
    sets, st = [], dict(generated=0, refused=0, contents=0, matched=0)
    for _ in range(SETS_PER_SEED):
        lits, pats = rxfuzz.pattern_set(rng)
        st["generated"] += 1
        refs = [_py(p.pattern) for p in pats]
        assert all(refs), [p.pattern for p in pats]  # the generator stays inside the subset
        rc, _, err = E.debug_compile(lits, [p.pattern for p in pats])
        assert rc in (0, E.KLF_ETOOBIG), (pats, err)
        if rc:
            st["refused"] += 1
            continue
        cs = []
        for _ in range(CONTENTS_PER_SET):
            s = rxfuzz.content(rng, pats)
            want = any(l in s for l in lits) or any(r.matches(s) for r in refs)
            cs.append((s, want))
            st["contents"] += 1
            st["matched"] += want
        sets.append((lits, pats, refs, cs))
    return sets, st


@pytest.mark.parametrize("seed", range(4))
def test_compile_agrees_with_the_oracles(seed):
    """Generated patterns and one-byte corruptions of them: the two oracles and the product
    accept or reject together (the product may refuse with KLF_ETOOBIG what needs more than
    64 positions), and an accepted corruption matches like the reference."""
    rng = random.Random(8000 + seed)
    n_ok = n_big = n_rej = 0
    for k in range(300):
        pat = rxfuzz.pattern(rng).pattern
        if k % 2:
            pat = rxfuzz.corrupt(rng, pat)
        ref = _py(pat)
        assert (co.rx_error(pat) is None) == (ref is not None), pat
        rc, _, err = E.debug_compile([], [pat])
        if ref is None:
            assert rc == E.KLF_EPATTERN, (pat, rc, err)
            n_rej += 1
            continue
        assert rc in (0, E.KLF_ETOOBIG), (pat, rc, err)
        n_ok += 1
        if rc:
            n_big += 1
            continue
        for _ in range(6):
            s = rxfuzz.noise(rng, rng.randint(0, 12))
            want = ref.matches(s)
            assert co.rx_match(pat, s) == want, (pat, s)
            assert E.debug_match(s, match=[pat]) == want, (pat, s)
    assert n_ok >= 200 and n_rej >= 10, (n_ok, n_rej)
    assert n_big <= 0.10 * n_ok, (n_big, n_ok)


@pytest.mark.parametrize("seed", SEEDS)
def test_glushkov_tables_random(seed):
    """The compiled tables' recurrence on the host: every pattern alone and every set (1-3
    regexes, 0-1 literals) decide each content as the reference does."""
    sets, _ = _corpus(seed)
    for lits, pats, refs, cs in sets:
        match = [p.pattern for p in pats]
        for s, want in cs:
            assert E.debug_match(s, grep=lits, match=match) == want, (lits, match, s)
            for p, r in zip(pats, refs):
                w1 = r.matches(s)
                assert co.rx_match(p.pattern, s) == w1, (p.pattern, s)
                assert E.debug_match(s, match=[p.pattern]) == w1, (p.pattern, s)


@pytest.mark.parametrize("seed", SEEDS)
def test_prefilter_random(seed):
    """The prefiltered decision (samples at every phase of the stride, bitmap, buckets,
    literal hits final, factor hits -> the NFA over its window) equals the reference."""
    sets, _ = _corpus(seed)
    for lits, pats, refs, cs in sets:
        match = [p.pattern for p in pats]
        for s, want in cs:
            got, info = E.debug_prefilter(s, grep=lits, match=match, phase=0)
            assert got == want, (lits, match, s, 0, info)
            for ph in range(1, 16 if info["stride"] >= 6 else 4):
                got, _ = E.debug_prefilter(s, grep=lits, match=match, phase=ph)
                assert got == want, (lits, match, s, ph, info)


def _occurrences(text, alts, loose):
    t = bytes(c | 0x20 for c in text) if loose else text
    out = []
    for a in alts:
        k = t.find(a)
        while k >= 0:
            out.append(k)
            k = t.find(a, k + 1)
    return out


@functools.lru_cache(maxsize=None)
def _window_stats(seed):
    """Checks the bound of every pattern of the seed; returns (bounded, unbounded, factor-less,
    matches checked) at the longest factor choice."""
    rng = random.Random(9000 + seed)
    bounded = unbounded = none = checked = 0
    for _ in range(60):
        p = rxfuzz.pattern(rng)
        if E.debug_compile([], [p.pattern])[0]:
            continue
        rx = re.compile(po.go_regex_to_python(p.pattern), re.DOTALL)
        texts = []
        for k in range(6):
            ex = p.example(rng, "min" if k < 3 else "rand")
            texts.append((b"" if p.bol else rxfuzz.noise(rng, rng.randint(0, 9))) + ex
                         + (b"" if p.eol else rxfuzz.noise(rng, rng.randint(0, 9))))
        for want in (0, 4, 6, 10):
            f = E.debug_factors(p.pattern, want)
            if want == 0:
                none += f is None
                bounded += f is not None and f[1] is not None
                unbounded += f is not None and f[1] is None
            if f is None:
                continue
            alts, pre, loose = f
            for s in texts:
                for start in range(len(s) + 1):
                    m = rx.search(s, start)
                    if m is None:
                        break
                    occ = _occurrences(s[m.start():m.end()], alts, loose)
                    # every match holds one of the required factors ...
                    assert occ, (p.pattern, want, alts, s, m.span())
                    # ... the first of them within `pre` bytes of the match's start
                    if pre is not None:
                        assert min(occ) <= pre, (p.pattern, want, alts, pre, s, m.span())
                    checked += 1
    return bounded, unbounded, none, checked


@pytest.mark.parametrize("seed", SEEDS)
def test_window_bounds_random(seed):
    """What k_nfa_win rests on: a match of a regex whose factor set has a bounded `pre` holds
    a factor occurrence at most `pre` bytes after the match's start (the leftmost match and
    the match found from every later start), at every factor-length preference."""
    assert _window_stats(seed)[3] > 100


def test_generator_is_not_trivial():
    """The shares the fuzz rests on, over all seeds (conditions on the generator, each from
    the reference or the compile's own report, none from a compared answer)."""
    tot = dict(generated=0, refused=0, contents=0, matched=0)
    on = compared = 0
    for seed in SEEDS:
        sets, st = _corpus(seed)
        for k in tot:
            tot[k] += st[k]
        for lits, pats, _, _ in sets:
            compared += 1
            on += E.debug_prefilter(b"", grep=lits, match=[p.pattern for p in pats])[1]["on"]
    b = u = n = 0
    for seed in SEEDS:
        wb, wu, wn, _ = _window_stats(seed)
        b, u, n = b + wb, u + wu, n + wn
    print(f"sets {tot['generated']} refused {tot['refused']} compared {compared} prefilter on {on}; "
          f"contents {tot['contents']} matched {tot['matched']}; patterns bounded {b} unbounded {u} no factor {n}")
    assert tot["refused"] <= 0.10 * tot["generated"], tot
    assert on >= 0.50 * compared, (on, compared)
    assert b >= 0.40 * (b + u + n) and u >= 0.10 * (b + u + n), (b, u, n)
    assert 0.25 * tot["contents"] <= tot["matched"] <= 0.75 * tot["contents"], tot
    assert compared >= 250 and tot["contents"] >= 10000, (compared, tot)


KNOWN = [  # pattern, texts at the minimum count (match), the next-shorter text (no match)
    (rb"x{1,}ab", [b"xab", b"xxab"], b"ab"),
    (rb"x{2,}ab", [b"xxab", b"xxxab"], b"xab"),
    (rb"x{3,}ab", [b"xxxab"], b"xxab"),
    (rb"^x{2,}$", [b"xx", b"xxx", b"xxxx"], b"x"),
    (rb"(?:ab){1,}", [b"ab", b"abab"], b"a"),
    (rb"(?:0123456789AB){2,}", [b"0123456789AB" * 2, b"0123456789AB" * 3], b"0123456789AB"),
    (rb"\d{3,}ms", [b"123ms", b"took 1234ms"], b"12ms"),
    (rb"(?i)(?:k=v){2,}", [b"K=Vk=v", b"k=vK=VK=v"], b"K=V"),
    (rb"^(?:x{1,}y){2}$", [b"xyxy", b"xxyxy"], b"xyy"),
    (rb"^a{01}$", [b"a{01}"], b"a"),                 # leading zeros: literal text, as in Go
    (rb"^\Qab\E+$", [b"ab", b"abbb"], b"abab"),      # the repetition takes the last quoted byte
    (rb"^ab(?i)*$", [b"a", b"abb"], b"aB"),          # ... or the item before a flag group
    (rb"^a(?)b+$", [b"ab", b"abb"], b"a"),           # an empty flag group is nothing, as in Go
]


@pytest.mark.parametrize("pat", [rb"[[:uper:]]", rb"[[:^alph::]]", rb"[[:foo:]_]+x", rb"a[[:alpha:b]c:]"])
def test_unknown_class_names_are_refused(pat):
    """Go reads a class name from `[:` to the next `:]`, wherever that is, and refuses a name
    it does not know: both oracle legs and the product do the same."""
    with pytest.raises(po.PatternError):
        po.Pattern("regex", pat)
    assert co.rx_error(pat) is not None
    assert E.debug_compile([], [pat])[0] == E.KLF_EPATTERN


@pytest.mark.parametrize("pat,yes,no", KNOWN)
def test_repeat_known_answers(pat, yes, no):
    ref = po.Pattern("regex", pat)
    for s in yes + [no]:
        want = s != no
        assert ref.matches(s) is want and co.rx_match(pat, s) is want, (pat, s)
        assert E.debug_match(s, match=[pat]) is want, (pat, s)
        for ph in range(4):
            assert E.debug_prefilter(s, match=[pat], phase=ph)[0] is want, (pat, s, ph)
        pad = b"-- " + s + b" --"
        if not pat.startswith(b"^"):
            assert E.debug_match(pad, match=[pat]) is ref.matches(pad), (pat, pad)
            assert E.debug_prefilter(pad, match=[pat])[0] is ref.matches(pad), (pat, pad)


# Positions of the documented expansion (SPEC.md S5: x{m,n} n copies, x{n,} max(n, 1) copies)
LIMIT = [(rb"a{64}", 64), (rb"a{65}", 65), (rb"(?:a{1,}){32}", 32), (rb"(?:a{1,}){33}", 33),
         (rb"(?:a{1,}){64}", 64), (rb"(?:a{1,}){65}", 65), (rb"(?:a{2,}){32}", 64), (rb"(?:a{2,}){33}", 66),
         (rb"(?:abcdefgh{1,}){8}", 64), (rb"(?:abcdefgh+){8}", 64), (rb"(?:abcdefgh+){9}", 72),
         (rb"(?:abcdefgh{1,}){9}", 72), (rb"(?:a{2,3}){21}", 63), (rb"(?:a{2,3}){22}", 66),
         (rb"(?:ab{0,}){32}", 64), (rb"(?:ab{0,}c){22}", 66)]
LIMIT_TEXTS = [b"", b"a" * 31, b"a" * 32, b"a" * 33, b"a" * 42, b"a" * 63, b"a" * 64, b"a" * 65, b"a" * 66,
               b"abcdefgh" * 8, b"abcdefg" * 8 + b"abcdefgh", b"abcdefghh" * 9, b"abcdefgh" * 7, b"ab" * 32,
               b"a" * 32 + b"b", b"abc" * 22, b"abc" * 21 + b"ab", b"xx" + b"a" * 64 + b"yy"]

_LIMIT_CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r]
from klogs_amd import engine as E
pats, texts = json.loads(sys.stdin.read())
out = []
for p in pats:
    p = bytes.fromhex(p)
    rc = E.debug_compile([], [p])[0]
    row = [rc]
    if rc == 0:
        for t in texts:
            t = bytes.fromhex(t)
            row.append([E.debug_match(t, match=[p]), E.debug_prefilter(t, match=[p])[0]])
    out.append(row)
print(json.dumps(out))
"""


def test_position_limit_is_exact():
    """Patterns at and just past 64 positions either compile and match like the reference or
    are refused with KLF_ETOOBIG, the boundary exactly at 64 positions of the documented
    expansion.  In a child process: a compile that writes past its tables shows as this
    test's failure."""
    child = _LIMIT_CHILD % (str(ROOT), str(ROOT / "oracle"))
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=120,
                       input=json.dumps([[p.hex() for p, _ in LIMIT], [t.hex() for t in LIMIT_TEXTS]]))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rows = json.loads(r.stdout)
    assert len(rows) == len(LIMIT)
    for (pat, npos), row in zip(LIMIT, rows):
        if npos > 64:
            assert row[0] == E.KLF_ETOOBIG, (pat, npos, row[0])
            continue
        assert row[0] == 0, (pat, npos, row[0])
        # a repetition of a repetition of one byte sends Python re's backtracking into
        # exponential time on runs of that byte: there the C oracle's regex leg (a lazy DFA,
        # linear time, its own parser) is the only reference; elsewhere both are
        nested = re.search(rb"a\{\d,\d?\}\)\{", pat) is not None
        ref = None if nested else po.Pattern("regex", pat)
        for t, got in zip(LIMIT_TEXTS, row[1:]):
            want = co.rx_match(pat, t)
            if ref is not None:
                assert ref.matches(t) is want, (pat, t)
            assert got == [want, want], (pat, t, got)
