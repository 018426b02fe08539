"""The exact gram-table probe of small needle sets (kQfExact, klf_kernels.hpp qf_exact_slot /
klf_patterns.cpp place_tables) on the host: when it is offered and chosen, that its table
passes the probed grams and nothing else, and that the prefiltered decision under it equals
the full matcher's and Python re / bytes.Contains at every sample phase."""
import functools
import random

import numpy as np
import pytest

import test_prefilter as tp
from klogs_amd import engine as E
from klogs_amd import synth

EXACT = 6  # kQfExact
MAX_GRAMS = 192  # kQfExactMaxGrams
SIX = [b"ab_cd1", b"Xy.z9w", b"qr=stu"]     # stride 4, 3-byte grams: the window is the whole needle
SEVEN = [b"ab_cd1e", b"Xy.z9wv", b"qr=stuw"]  # stride 4, 4-byte grams: likewise


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for k in ("KLF_QF_EXACT", "KLF_QF_TUNE", "KLF_QF_TWO", "KLF_QF_ANCHOR", "KLF_QF_QMAX"):
        monkeypatch.delenv(k, raising=False)


def force(monkeypatch, mode="force"):
    monkeypatch.setenv("KLF_QF_EXACT", mode)


def grams_of(needles, q):
    """The grams a stride-4 layout probes for needles of q + 3 bytes: all four of each."""
    assert all(len(n) == q + 3 for n in needles)
    return {int.from_bytes(n[k:k + q], "little") for n in needles for k in range(4)}


# ---- the layout choice on the C5 set ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def c5_data():
    return (synth.generate(synth.LONGJSON, 1, 0, 1 << 20), synth.generate(synth.LONGJSON, 1, 1, 16 << 20))


def test_c5_set_takes_the_exact_probe(monkeypatch):
    rx = synth.c5_regexes()
    sample, data = c5_data()
    ex = E.debug_prefilter_hits(sample, data, match=rx)
    print("exact:", ex)
    force(monkeypatch, "0")
    bl = E.debug_prefilter_hits(sample, data, match=rx)
    print("bloom:", bl)
    assert (ex["stride"], ex["k"], ex["anchor"]) == (4, EXACT, None) and ex["mul"] and f" k={EXACT} " in ex["layout"], ex
    assert (bl["stride"], bl["q"], bl["k"], bl["anchor"], bl["mul"]) == (4, 3, 2, None, 0), bl
    assert ex["verified"] == bl["verified"] > 0
    assert ex["probes"] == bl["probes"] and ex["bitmap_hits"] <= bl["bitmap_hits"]
    assert 0 < ex["grams"] <= MAX_GRAMS


def test_not_offered_without_statistics_or_at_another_stride(monkeypatch):
    """Untuned layouts keep their kind; so does a tuned layout at stride 8."""
    assert E.debug_prefilter(b"", grep=SIX)[1]["k"] == 2
    assert E.debug_prefilter_hits(b"", b"", grep=SIX)["k"] == 2
    sample = synth.generate(synth.TEXT, 4, 0, 60_000)
    h = E.debug_prefilter_hits(sample, b"", grep=[b"0123456789ABC", b"a longer needle"])
    assert h["stride"] == 8 and h["k"] == 2 and h["mul"] == 0, h
    assert E.debug_prefilter_hits(sample, b"", grep=SIX)["k"] == EXACT
    force(monkeypatch)
    h = E.debug_prefilter_hits(b"", b"", grep=[b"0123456789ABC", b"a longer needle"])
    assert h["stride"] == 8 and h["k"] == 2, h


# ---- exactness: the table passes the probed grams and nothing else ---------------------------
def test_q3_table_passes_exactly_its_grams(monkeypatch):
    """Every 3-byte value once, as the low bytes of an aligned dword (the top byte, which a
    3-byte gram does not cover, is 0): the hits are the distinct probed grams."""
    force(monkeypatch)
    data = np.arange(1 << 24, dtype="<u4").tobytes()
    h = E.debug_prefilter_hits(b"", data, grep=SIX)
    assert (h["stride"], h["q"], h["k"]) == (4, 3, EXACT), h
    assert h["probes"] == 1 << 24
    assert h["grams"] == len(grams_of(SIX, 3)) == 12
    assert h["bitmap_hits"] == h["grams"], h
    data = (np.arange(1 << 16, dtype="<u4") | 0xFF000000).astype("<u4").tobytes()  # (the table's own top byte)
    h = E.debug_prefilter_hits(b"", data, grep=SIX)
    assert h["bitmap_hits"] == sum(g < (1 << 16) for g in grams_of(SIX, 3)), h


def test_q4_table_passes_exactly_its_grams(monkeypatch):
    """A million random dwords, every probed gram and all its one-byte neighbours."""
    force(monkeypatch)
    grams = grams_of(SEVEN, 4)
    rng = np.random.default_rng(5)
    near = [g ^ ((g ^ (v << (8 * b))) & (0xFF << (8 * b))) for g in sorted(grams) for b in range(4) for v in range(256)]
    dw = np.concatenate([rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64), np.array(near, dtype=np.uint64)])
    h = E.debug_prefilter_hits(b"", dw.astype("<u4").tobytes(), grep=SEVEN)
    assert (h["stride"], h["q"], h["k"]) == (4, 4, EXACT), h
    assert h["grams"] == len(grams) == 12 and h["probes"] == len(dw)
    want = int(np.isin(dw, np.array(sorted(grams), dtype=np.uint64)).sum())
    assert want >= 4 * len(grams)  # (each gram is its own neighbour in all four byte positions)
    assert h["bitmap_hits"] == want, (h, want)


# ---- decision parity under the forced exact probe ---------------------------------------------
def contents(rng, inserts, n=200, maxlen=50):
    out = []
    for _ in range(n):
        s = tp._text(rng, rng.randint(0, maxlen))
        for _ in range(rng.randint(0, 2)):
            k = rng.randint(0, len(s))
            s = s[:k] + rng.choice(inserts) + s[k:]
        out.append(s)
    return out + list(inserts)


def near_misses(needles):
    return [n[:-1] for n in needles] + [n[1:] for n in needles] + [n[:-1] + b"#" for n in needles]


@pytest.mark.parametrize("length,q", [(6, 3), (7, 4)])
@pytest.mark.parametrize("seed", range(3))
def test_literal_sets(monkeypatch, length, q, seed):
    force(monkeypatch)
    rng = random.Random(40 + seed)
    lits = [tp._text(rng, length + (rng.randint(0, 6) if i else 0)) for i in range(rng.randint(2, 30))]
    info = tp._check(lits, [], contents(rng, lits + near_misses(lits)))
    assert (info["stride"], info["q"], info["k"]) == (4, q, EXACT) and info["mul"], info


RX_SETS = [
    [rb"timeout after \d+ms", rb"(?i)panic: [a-z]+", rb"status=(500|502|503)"],
    [rb"user_id=u\d{4,6}", rb"(?i)OOMkill(ed|_score)", rb"tx-[0-9a-f]{4}-done!"],
    [rb"(?i)error: (disk|net)\w* full", rb"\Qa.b*c.d-e\E", rb"abcdef.defghi"],
]
RX_INSERTS = [b"timeout after 123ms", b"timeout after ms", b"PANIC: xyz", b"panic: 1", b"status=502", b"status=302",
              b"user_id=u12345", b"user_id=u12", b"oomKILLED", b"OOMkill_", b"tx-0a9f-done!", b"tx-0a9-done!",
              b"ERROR: disk0 full", b"Error: Network full", b"error: full", b"a.b*c.d-e", b"a.b*c.d-f", b"abcdefXdefghi",
              b"abcdef.defghi", b"abcdefdefghi"]


@pytest.mark.parametrize("idx", range(len(RX_SETS)))
def test_regex_sets(monkeypatch, idx):
    force(monkeypatch)
    info = tp._check([], RX_SETS[idx], contents(random.Random(60 + idx), RX_INSERTS, 300, 40))
    assert info["on"] and (info["stride"], info["k"]) == (4, EXACT), info


@pytest.mark.parametrize("idx", range(len(tp.RX_SETS)))
def test_regex_sets_of_any_stride(monkeypatch, idx):
    """The forced kind changes nothing where it does not apply (factors too short for stride 4)."""
    force(monkeypatch)
    info = tp._check([], tp.RX_SETS[idx], contents(random.Random(70 + idx), RX_INSERTS, 100, 40))
    assert info["k"] == EXACT or info["stride"] != 4 or info["anchor"] is not None, info


def test_needles_that_differ_in_their_last_byte(monkeypatch):
    force(monkeypatch)
    lits = [b"abcde" + bytes([c]) for c in b"XYZ012"]
    info = tp._check(lits, [], contents(random.Random(80), lits + [b"abcde", b"abcdeW", b"bcdeX", b"deX"]))
    assert (info["q"], info["k"]) == (3, EXACT), info
    lits = [b"abcdef" + bytes([c]) for c in b"XYZ012"]  # 4-byte grams "defX", "defY", ...: one slot, never apart
    info = tp._check(lits, [], contents(random.Random(81), lits + [b"abcdef", b"abcdefW", b"bcdefX", b"defX"]))
    assert (info["stride"], info["q"], info["k"]) == (4, 4, 2), info


def test_q4_needles_sharing_three_bytes_elsewhere(monkeypatch):
    """4-byte grams with common first three bytes, in longer needles: a window that avoids the
    pair is fine, a refusal is fine, a wrong decision is not."""
    force(monkeypatch)
    lits = [b"xyzabcdQrstuv", b"mnoabcdRrstuv", b"abcdSlongerneedle"]
    info = tp._check(lits, [], contents(random.Random(82), lits + [b"abcdQ", b"abcdR", b"abcdS", b"abcd"]))
    assert info["k"] in (2, EXACT), info


def test_too_many_grams_fall_back(monkeypatch):
    force(monkeypatch)
    rng = random.Random(90)
    lits = sorted({tp._text(rng, 7) for _ in range(600)})
    h = E.debug_prefilter_hits(b"", b"", grep=lits)
    assert h["grams"] > MAX_GRAMS and h["k"] != EXACT and h["mul"] == 0, h
    info = tp._check(lits, [], contents(rng, lits[:20] + near_misses(lits[:20]), 60))
    assert info["k"] != EXACT


def test_placement_is_deterministic(monkeypatch):
    sample, data = c5_data()
    rx = synth.c5_regexes()
    a = E.debug_prefilter_hits(sample, data[:1 << 20], match=rx)
    b = E.debug_prefilter_hits(sample, data[:1 << 20], match=rx)
    assert a == b and a["k"] == EXACT
    # the table itself: the same values pass in both compiles, over every 3-byte value
    if a["q"] == 3:
        every = np.arange(1 << 24, dtype="<u4").tobytes()
        ha, hb = (E.debug_prefilter_hits(sample, every, match=rx) for _ in range(2))
        assert ha == hb and ha["mul"] == a["mul"]
