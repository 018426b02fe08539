"""klf_result_field_stats (SPEC.md S4f: the statistics of a numeric field of a finished run): the
reference the GPU tests compare against, written from the S4f text with Python's big integers, a
by-hand table that pins it, the host helper klf_field_value against it, and the library's new
ABI entries.  No GPU here."""
import ctypes as C
import functools
import random
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from klogs_amd import engine as E
from test_window_ref import WindowRef

ROOT = Path(__file__).resolve().parent.parent
HIT, MISS, BAD = E.FIELD_HIT, E.FIELD_MISS, E.FIELD_BAD
LIMIT = 1 << 62
U64, U32 = (1 << 64) - 1, (1 << 32) - 1
SEPARATORS = b' \t=:"'
UNITS = [(b"ns", 1), (b"us", 10**3), (b"\xc2\xb5s", 10**3), (b"\xce\xbcs", 10**3), (b"ms", 10**6), (b"s", 10**9),
         (b"m", 6 * 10**10), (b"h", 36 * 10**11)]


def _digit(c, p):
    return p < len(c) and 0x30 <= c[p] <= 0x39


def _number(c, p):
    """The number at c[p:]: (integer digits, fraction digits, the offset behind it), or None when
    no digit stands there.  A '.' is taken only with a digit behind it."""
    q = p
    while _digit(c, q):
        q += 1
    if q == p:
        return None
    ip, fr = c[p:q], b""
    if q < len(c) and c[q] == 0x2E and _digit(c, q + 1):
        r = q + 1
        while _digit(c, r):
            r += 1
        fr, q = c[q + 1:r], r
    return ip, fr, q


def field_value(content: bytes, key: bytes, decimals: int = 0, duration: bool = False):
    """(class, value) of one content by S4f; the value is 0 unless the class is HIT."""
    i = content.find(key)  # step 1: the first occurrence alone
    if i < 0:
        return MISS, 0
    p = i + len(key)
    skipped = 0
    while skipped < 4 and p < len(content) and content[p] in SEPARATORS:  # step 2
        p += 1
        skipped += 1
    sign = 1
    if p < len(content) and content[p] in b"+-":  # step 3
        sign = -1 if content[p] == 0x2D else 1
        p += 1
    if not duration:  # step 4
        num = _number(content, p)
        if num is None:
            return BAD, 0
        ip, fr, _ = num
        mag = int(ip + (fr + b"0" * decimals)[:decimals])
    else:  # step 5
        mag = 0
        while True:
            num = _number(content, p)
            if num is None:
                return BAD, 0
            ip, fr, p = num
            unit = max((u for u in UNITS if content.startswith(u[0], p)), key=lambda u: len(u[0]), default=None)
            if unit is None:
                return BAD, 0
            mag += int(ip) * unit[1] + int((fr + b"0" * 9)[:9]) * unit[1] // 10**9
            p += len(unit[0])
            if not _digit(content, p):
                break
    if mag >= LIMIT:  # (every term is non-negative: an intermediate at 2^62 means the total is)
        return BAD, 0
    return HIT, sign * mag


def quantile(values, q):
    """Nearest rank: of the ascending values the one at index max(1, ceil(q n / 10000)) - 1."""
    a = sorted(values)
    if not a:
        return 0
    return a[max(1, -(-q * len(a) // 10000)) - 1]


def _row(lines, bad, vals):
    """One klf_field_row as a dict; vals = [(value, stream, line)] of the hits."""
    row = dict(lines=lines, hits=len(vals), bad=bad, min=0, max=0, sum_lo=0, sum_hi=0, min_line=U64, max_line=U64,
               min_stream=U32, max_stream=U32)
    if vals:
        total = sum(v for v, _, _ in vals)
        lo, hi = min(v for v, _, _ in vals), max(v for v, _, _ in vals)
        at_lo = min((s, l) for v, s, l in vals if v == lo)
        at_hi = min((s, l) for v, s, l in vals if v == hi)
        row.update(min=lo, max=hi, sum_lo=total & U64, sum_hi=total >> 64, min_stream=at_lo[0], min_line=at_lo[1],
                   max_stream=at_hi[0], max_line=at_hi[1])
    return row


def row_sum(row):
    return (int(row["sum_hi"]) << 64) + int(row["sum_lo"])


class FieldRef(WindowRef):
    """WindowRef plus the S4f class and value of every line."""

    def __init__(self, data: bytes, grep=(), match=()):
        super().__init__(data, grep, match)
        self._fields = {}

    def content(self, i):
        """S1's content of line i without its terminating '\\n' (a parsed line: it has a space)."""
        s, e = self.lines[i]
        c = self.data[s:e].split(b" ", 1)[1]
        return c[:-1] if c.endswith(b"\n") else c

    def fields(self, key, decimals, duration):
        """[(class, value) or None for an unparsed line] of every line, computed once per option set."""
        k = (key, decimals, duration)
        if k not in self._fields:
            self._fields[k] = [field_value(self.content(i), key, decimals, duration) if self.parsed[i] else None
                               for i in range(self.n_lines)]
        return self._fields[k]

    def field_stats(self, g, key, decimals=0, duration=False, quantiles=()):
        return field_stats([self], [g], key, decimals, duration, quantiles)


def field_stats(refs, flags, key, decimals=0, duration=False, quantiles=()):
    """(rows, qvals) over the streams `refs` with H flags `flags`: one row per stream, then the
    row over all of them; qvals[i] = the quantiles of row i."""
    per = []
    for s, (ref, g) in enumerate(zip(refs, flags)):
        f = ref.fields(key, decimals, duration)
        lines, bad, vals = 0, 0, []
        for i in range(ref.n_lines):
            if not (g[i] and ref.parsed[i]):
                continue
            lines += 1
            cls, v = f[i]
            if cls == HIT:
                vals.append((v, s, i))
            elif cls == BAD:
                bad += 1
        per.append((lines, bad, vals))
    per.append((sum(p[0] for p in per), sum(p[1] for p in per), [x for p in per for x in p[2]]))
    rows = [_row(*p) for p in per]
    qvals = [[quantile([v for v, _, _ in p[2]], q) for q in quantiles] for p in per]
    return rows, qvals


def fixed(v, decimals):
    """A fixed-point value as a decimal with `decimals` fraction digits."""
    if not decimals:
        return b"%d" % v
    return (b"-" if v < 0 else b"") + b"%d.%0*d" % (abs(v) // 10**decimals, decimals, abs(v) % 10**decimals)


CLI_QUANTILES = (5000, 9000, 9900)  # p50, p90, p99


def render_stats_tsv(rows, qvals, names, decimals):
    """stats.tsv of klogs-filter --stat: names[i] = (pod, container) of stream i."""
    out = []
    for i, (row, qv) in enumerate(zip(rows, qvals)):
        pod, cont = names[i] if i < len(names) else ("*", "*")
        cols = [pod.encode(), cont.encode(), b"%d" % row["lines"], b"%d" % row["hits"], b"%d" % row["bad"]]
        if row["hits"]:
            mp, mc = names[row["max_stream"]]
            cols += [fixed(row["min"], decimals), fixed(row["max"], decimals), fixed(row_sum(row), decimals)]
            cols += [fixed(q, decimals) for q in qv]
            cols.append(b"%s/%s:%d" % (mp.encode(), mc.encode(), row["max_line"] + 1))
        else:
            cols += [b"-"] * 7
        out.append(b"\t".join(cols) + b"\n")
    return b"".join(out)


# ------------------------------------------------------------------ the by-hand table ---

P62 = 4611686018427387904  # 2^62
K64 = b"k" * 63 + b"="
PLAIN, DUR = False, True

# (content, key, decimals, duration, class, value)
BY_HAND = [
    # where the key stands
    (b"lat=12 rest", b"lat", 0, PLAIN, HIT, 12),                 # at offset 0
    (b"request lat", b"lat", 0, PLAIN, BAD, 0),                  # at the very end: C ends first
    (b"lat=x lat=5", b"lat", 0, PLAIN, BAD, 0),                  # twice: the first occurrence is bad and decides
    (b"lat=7 lat=x", b"lat", 0, PLAIN, HIT, 7),
    (b"request la", b"lat", 0, PLAIN, MISS, 0),                  # the tail is a proper prefix of the key
    (b"x latency=5", b"lat", 0, PLAIN, BAD, 0),                  # the key is a proper prefix of the tail's word
    (b"aaab=3", b"aab", 0, PLAIN, HIT, 3),                       # the occurrence begins inside a failed attempt
    (b"nothing here", b"lat", 0, PLAIN, MISS, 0),
    (b"", b"lat", 0, PLAIN, MISS, 0),
    (b"la", b"lat", 0, PLAIN, MISS, 0),
    # 0 to 5 separator bytes
    (b"lat12", b"lat", 0, PLAIN, HIT, 12),
    (b"lat 12", b"lat", 0, PLAIN, HIT, 12),
    (b"lat\t=12", b"lat", 0, PLAIN, HIT, 12),
    (b'"lat": 12,', b"lat", 0, PLAIN, HIT, 12),
    (b'lat = "12"', b"lat", 0, PLAIN, HIT, 12),
    (b'lat = ":12', b"lat", 0, PLAIN, BAD, 0),                   # the fifth is not skipped
    # sign, leading zeros
    (b"lat=-12", b"lat", 0, PLAIN, HIT, -12),
    (b"lat=+12", b"lat", 0, PLAIN, HIT, 12),
    (b"lat=--12", b"lat", 0, PLAIN, BAD, 0),
    (b"lat=-", b"lat", 0, PLAIN, BAD, 0),
    (b"lat=- 3", b"lat", 0, PLAIN, BAD, 0),
    (b"lat= -3", b"lat", 0, PLAIN, HIT, -3),
    (b"lat=000123", b"lat", 0, PLAIN, HIT, 123),
    (b"lat=-0", b"lat", 0, PLAIN, HIT, 0),
    # '.' with and without digits; what follows the number is ignored
    (b"lat=12.", b"lat", 0, PLAIN, HIT, 12),
    (b"lat=12.x", b"lat", 2, PLAIN, HIT, 1200),
    (b"lat=.5", b"lat", 1, PLAIN, BAD, 0),
    (b"lat=12.5", b"lat", 0, PLAIN, HIT, 12),
    (b"lat=-12.99", b"lat", 0, PLAIN, HIT, -12),                 # cut toward zero
    (b"lat=-0.5", b"lat", 0, PLAIN, HIT, 0),
    (b"lat=12.5.7", b"lat", 1, PLAIN, HIT, 125),
    (b"lat=12ms", b"lat", 0, PLAIN, HIT, 12),
    (b"lat=1e5", b"lat", 0, PLAIN, HIT, 1),
    (b"lat=5\r", b"lat", 0, PLAIN, HIT, 5),
    # each D with a longer and a shorter fraction
    (b"v=3.14159265358979", b"v", 0, PLAIN, HIT, 3),
    (b"v=3.14159265358979", b"v", 1, PLAIN, HIT, 31),
    (b"v=3.14159265358979", b"v", 2, PLAIN, HIT, 314),
    (b"v=3.14159265358979", b"v", 3, PLAIN, HIT, 3141),
    (b"v=3.14159265358979", b"v", 4, PLAIN, HIT, 31415),
    (b"v=3.14159265358979", b"v", 5, PLAIN, HIT, 314159),
    (b"v=3.14159265358979", b"v", 6, PLAIN, HIT, 3141592),
    (b"v=3.14159265358979", b"v", 7, PLAIN, HIT, 31415926),
    (b"v=3.14159265358979", b"v", 8, PLAIN, HIT, 314159265),
    (b"v=3.14159265358979", b"v", 9, PLAIN, HIT, 3141592653),
    (b"v=-2.5", b"v", 0, PLAIN, HIT, -2),
    (b"v=-2.5", b"v", 1, PLAIN, HIT, -25),
    (b"v=-2.5", b"v", 2, PLAIN, HIT, -250),
    (b"v=-2.5", b"v", 3, PLAIN, HIT, -2500),
    (b"v=-2.5", b"v", 4, PLAIN, HIT, -25000),
    (b"v=-2.5", b"v", 5, PLAIN, HIT, -250000),
    (b"v=-2.5", b"v", 6, PLAIN, HIT, -2500000),
    (b"v=-2.5", b"v", 7, PLAIN, HIT, -25000000),
    (b"v=-2.5", b"v", 8, PLAIN, HIT, -250000000),
    (b"v=-2.5", b"v", 9, PLAIN, HIT, -2500000000),
    # 2^62 - 1 and 2^62; a 30-digit run
    (b"n=4611686018427387903", b"n", 0, PLAIN, HIT, P62 - 1),
    (b"n=4611686018427387904", b"n", 0, PLAIN, BAD, 0),
    (b"n=-4611686018427387903", b"n", 0, PLAIN, HIT, -(P62 - 1)),
    (b"n=-4611686018427387904", b"n", 0, PLAIN, BAD, 0),
    (b"n=4611686018427387.903", b"n", 3, PLAIN, HIT, P62 - 1),
    (b"n=4611686018427387.904", b"n", 3, PLAIN, BAD, 0),
    (b"n=4611686018427387904", b"n", 9, PLAIN, BAD, 0),
    (b"n=123456789012345678901234567890", b"n", 0, PLAIN, BAD, 0),
    (b"n=000000000000000000000000000042", b"n", 0, PLAIN, HIT, 42),
    (b"n=000000000000000000000000000042.5", b"n", 2, PLAIN, HIT, 4250),
    # every unit, both micro signs, m against ms
    (b"d=7ns", b"d", 0, DUR, HIT, 7),
    (b"d=7us", b"d", 0, DUR, HIT, 7000),
    (b"d=7\xc2\xb5s", b"d", 0, DUR, HIT, 7000),
    (b"d=7\xce\xbcs", b"d", 0, DUR, HIT, 7000),
    (b"d=7ms", b"d", 0, DUR, HIT, 7000000),
    (b"d=7s", b"d", 0, DUR, HIT, 7000000000),
    (b"d=7m", b"d", 0, DUR, HIT, 420000000000),
    (b"d=7h", b"d", 0, DUR, HIT, 25200000000000),
    (b"d=1m5s", b"d", 0, DUR, HIT, 65000000000),
    (b"d=1ms5s", b"d", 0, DUR, HIT, 5001000000),
    (b"d=1mx", b"d", 0, DUR, HIT, 60000000000),
    (b"d=1m s", b"d", 0, DUR, HIT, 60000000000),
    (b"d=7\xc2s", b"d", 0, DUR, BAD, 0),
    (b"d=7\xce\xb5s", b"d", 0, DUR, BAD, 0),
    (b"d=7\xc2\xb5", b"d", 0, DUR, BAD, 0),
    (b"d=7n", b"d", 0, DUR, BAD, 0),
    (b"d=7u5", b"d", 0, DUR, BAD, 0),
    # compound durations, a missing unit, fractions
    (b"took=1m30.5s", b"took", 0, DUR, HIT, 90500000000),
    (b"took=250ms", b"took", 0, DUR, HIT, 250000000),
    (b"took=1.5h", b"took", 0, DUR, HIT, 5400000000000),
    (b"took=12.s", b"took", 0, DUR, BAD, 0),
    (b"took=1h2m3s4ms5us6ns.", b"took", 0, DUR, HIT, 3723004005006),
    (b"took=15", b"took", 0, DUR, BAD, 0),
    (b"took=1h30", b"took", 0, DUR, BAD, 0),
    (b"took=-1.5s", b"took", 0, DUR, HIT, -1500000000),
    (b"took=1s-2s", b"took", 0, DUR, HIT, 1000000000),          # a sign only before the first component
    (b"took=0.0000000019s", b"took", 0, DUR, HIT, 1),           # the first 9 fraction digits
    (b"took=0.9999999999ns", b"took", 0, DUR, HIT, 0),
    (b"took=2.5us", b"took", 0, DUR, HIT, 2500),
    (b"took=1.7ns", b"took", 0, DUR, HIT, 1),
    (b"took=.5s", b"took", 0, DUR, BAD, 0),
    (b"took=4611686018427387903ns", b"took", 0, DUR, HIT, P62 - 1),
    (b"took=4611686018427387904ns", b"took", 0, DUR, BAD, 0),
    (b"took=4611686018427387903ns1ns", b"took", 0, DUR, BAD, 0),  # the total reaches 2^62
    (b"took=1281023h", b"took", 0, DUR, HIT, 4611682800000000000),
    (b"took=1281024h", b"took", 0, DUR, BAD, 0),
    (b"took=123456789012345678901234567890h", b"took", 0, DUR, BAD, 0),
    # a 64-byte key, a 1-byte key, keys holding \x00 and bytes >= 0x80
    (b"x" + K64 + b"5", K64, 0, PLAIN, HIT, 5),
    (b"x" + K64[1:] + b"5", K64, 0, PLAIN, MISS, 0),
    (b"a=5", b"=", 0, PLAIN, HIT, 5),
    (b"a==7", b"=", 0, PLAIN, HIT, 7),
    (b"ab\x00\xff\x80=9", b"\x00\xff\x80", 0, PLAIN, HIT, 9),
    (b"ab\x00\xff\x81=9", b"\x00\xff\x80", 0, PLAIN, MISS, 0),
    (b"t\xc2\xb5 3.25", b"\xc2\xb5", 1, PLAIN, HIT, 32),
]


def test_reference_on_the_by_hand_table():
    assert len(BY_HAND) >= 40 and len(K64) == 64
    for content, key, decimals, duration, cls, value in BY_HAND:
        assert field_value(content, key, decimals, duration) == (cls, value), (content, key, decimals, duration)
    assert {d for _, _, d, dur, _, _ in BY_HAND if not dur} == set(range(10))
    assert {c for *_, c, _ in BY_HAND} == {HIT, MISS, BAD}


def _value(content, key, decimals, duration):
    """(rc, value) of one klf_field_value call; the content sits at the end of its buffer."""
    lib = E.lib()
    src = C.create_string_buffer(content, len(content) or 1)
    kb = C.create_string_buffer(key, len(key) or 1)
    v = C.c_int64(12345)
    rc = lib.klf_field_value(C.addressof(src), len(content), C.addressof(kb), len(key), decimals,
                             E.FIELD_DURATION if duration else 0, C.byref(v))
    return rc, v.value


def test_field_value_on_the_by_hand_table():
    for content, key, decimals, duration, cls, value in BY_HAND:
        assert _value(content, key, decimals, duration) == (cls, value), (content, key, decimals, duration)
        assert E.field_value(content, key, decimals, duration) == (cls, value)


RANDOM_TOKENS = [b"lat", b"lat", b"lat=", b"la", b"l", b"t", b"at", b" ", b"=", b":", b'"', b"\t", b"-", b"+", b".",
                 b"0", b"1", b"7", b"9", b"12", b"305", b"n", b"u", b"m", b"s", b"h", b"ms", b"ns", b"\xc2\xb5",
                 b"\xce\xbc", b"x", b"99999999999", b"4611686018427387904"]


def random_content(rng):
    shape = rng.randrange(6)
    if shape >= 4:  # mostly well formed: a number, often with a fraction and a unit, then anything
        num = rng.choice([b"0", b"7", b"12", b"0305", b"99999999999"]) + rng.choice([b"", b".5", b".125", b".", b".0009"])
        more = rng.choice([b"", b"", b"30s", b"5", b"2.5ms", b"x"])
        return (rng.choice([b"", b"x ", b"la l t "]) + b"lat" + rng.choice([b"", b"=", b": ", b'="', b'": "'])
                + rng.choice([b"", b"", b"-", b"+"]) + num + rng.choice([b"", b"ms", b"s", b"m", b"h", b"us", b"ns",
                                                                         b"\xc2\xb5s", b"\xce\xbcs", b" "]) + more)
    if shape == 0:  # anything
        return b"".join(rng.choice(RANDOM_TOKENS) for _ in range(rng.randrange(0, 14)))
    head = b"".join(rng.choice([b"x", b" ", b"la", b"l", b"t", b"7"]) for _ in range(rng.randrange(0, 6)))
    if shape == 1:  # no key at all
        return head.replace(b"lat", b"l-t") + rng.choice([b"", b"la", b"l", b"12"])
    seps = b"".join(rng.choice([b" ", b"=", b":", b'"', b"\t"]) for _ in range(rng.choice([0, 1, 1, 2, 3, 4, 5])))
    body = b"".join(rng.choice([b"1", b"20", b"305", b".", b"5", b"ms", b"s", b"m", b"h", b"us", b"ns", b"\xc2\xb5s",
                                b"\xce\xbcs", b"-", b"x", b"0"]) for _ in range(rng.randrange(0, 8)))
    return head + b"lat" + seps + rng.choice([b"", b"", b"-", b"+"]) + body


def test_field_value_equals_the_reference_on_random_contents():
    rng = random.Random(2025)
    seen = {HIT: 0, MISS: 0, BAD: 0}
    n = 6000
    for _ in range(n):
        content = random_content(rng)
        duration = rng.random() < 0.5
        decimals = 0 if duration else rng.randrange(10)
        want = field_value(content, b"lat", decimals, duration)
        assert _value(content, b"lat", decimals, duration) == want, (content, decimals, duration)
        seen[want[0]] += 1
    assert all(c >= n // 10 for c in seen.values()), seen


def test_quantile_and_tie_rules_by_hand():
    vals = [(5, 0, 0), (-3, 0, 1), (9, 0, 2), (5, 1, 0), (9, 1, 1), (-3, 1, 2), (7, 1, 3)]  # (value, stream, line)
    a = [v for v, _, _ in vals]
    assert sorted(a) == [-3, -3, 5, 5, 7, 9, 9]
    # n = 7: q n / 10000 -> rank: 0 -> 1 (clamped), 1 -> 1, 1428 -> 1, 1429 -> 2, 5000 -> 4, 7142 -> 5, 7143 -> 6
    want = {0: -3, 1: -3, 1428: -3, 1429: -3, 2857: -3, 2858: 5, 5000: 5, 5714: 5, 5715: 7, 7142: 7, 7143: 9, 9999: 9,
            10000: 9}
    for q, v in want.items():
        assert quantile(a, q) == v, q
    assert quantile([], 5000) == 0 and quantile([4], 0) == quantile([4], 10000) == 4
    row = _row(9, 1, vals)
    assert row == dict(lines=9, hits=7, bad=1, min=-3, max=9, sum_lo=29, sum_hi=0, min_stream=0, min_line=1,
                       max_stream=0, max_line=2)  # ties: the lowest (stream, line)
    neg = _row(2, 0, [(-5, 0, 0), (2, 0, 1)])
    assert (neg["sum_lo"], neg["sum_hi"]) == (U64 - 2, -1) and row_sum(neg) == -3
    big = _row(8, 0, [(P62 - 1, 0, i) for i in range(8)])
    assert big["sum_hi"] == 1 and row_sum(big) == 8 * (P62 - 1)
    empty = _row(3, 3, [])
    assert empty == dict(lines=3, hits=0, bad=3, min=0, max=0, sum_lo=0, sum_hi=0, min_line=U64, max_line=U64,
                         min_stream=U32, max_stream=U32)
    assert fixed(-1234, 3) == b"-1.234" and fixed(5, 2) == b"0.05" and fixed(-5, 0) == b"-5" and fixed(-5, 2) == b"-0.05"


def test_field_ref_by_hand():
    ts = b"2024-10-22T00:00:%02dZ "
    lines = [ts % 0 + b"GET /a lat=12ms\n", b"junk lat=99\n", ts % 2 + b"GET /b lat=7ms\n", ts % 3 + b"GET /c lat=\n",
             ts % 4 + b"POST /d\n", ts % 5 + b"GET /e lat=12"]
    ref = FieldRef(b"".join(lines), grep=[b"GET"])
    rows, qv = ref.field_stats(ref.gprime(), b"lat=", quantiles=(0, 5000, 10000))
    assert rows[0] == rows[1] == dict(lines=4, hits=3, bad=1, min=7, max=12, sum_lo=31, sum_hi=0, min_stream=0,
                                      min_line=2, max_stream=0, max_line=0)
    assert qv == [[7, 12, 12], [7, 12, 12]]
    every = FieldRef(b"".join(lines))
    rows, _ = every.field_stats(every.gprime(), b"lat=")
    assert (rows[0]["lines"], rows[0]["hits"], rows[0]["bad"]) == (5, 3, 1)  # the unparseable line is not in H
    assert render_stats_tsv(*ref.field_stats(ref.gprime(), b"lat=", 2, False, CLI_QUANTILES), [("p", "c")], 2) == \
        b"p\tc\t4\t3\t1\t7.00\t12.00\t31.00\t12.00\t12.00\t12.00\tp/c:1\n" \
        b"*\t*\t4\t3\t1\t7.00\t12.00\t31.00\t12.00\t12.00\t12.00\tp/c:1\n"


# ------------------------------------------------------------- the inputs of the GPU tests ---

def _ts(i):
    return b"2024-10-22T%02d:%02d:%02d.%09dZ " % (i // 3600 % 24, i // 60 % 60, i % 60, i % 1000)


BIG_N = 20_000


@functools.lru_cache(maxsize=None)
def big_streams():
    """Three streams, the first of BIG_N lines (> 2 chunks of 8192): about a third of the lines
    carry lat= with values of both signs and beyond 32 bits, some carry the key without a value,
    every third line holds HIT, and the last stream ends in a fragment."""
    rng = random.Random(17)

    def line(i, s):
        r = rng.random()
        tag = b"HIT " if i % 3 == 0 else b""
        if r < 0.30:
            v = rng.choice([rng.randrange(-50, 50), rng.randrange(-(1 << 40), 1 << 40), rng.randrange(1 << 33, 1 << 50),
                            -rng.randrange(1 << 33, 1 << 50), 7])
            return _ts(i) + tag + b"GET /api/%d ERR_CONN_RESET lat=%d.%03dms\n" % (s, v, rng.randrange(1000))
        if r < 0.36:
            return _ts(i) + tag + b"GET /api/%d timeout lat=%s\n" % (s, rng.choice([b"", b"NaN", b"-", b"=====1"]))
        if r < 0.45:
            return _ts(i) + tag + b"took=%dm%d.%ds total\n" % (rng.randrange(90), rng.randrange(60), rng.randrange(1000))
        return _ts(i) + tag + b"handler %d ok, %d rows\n" % (rng.randrange(100), rng.randrange(1000))

    a = b"".join(line(i, 0) for i in range(BIG_N))
    b = b"".join(line(i, 1) for i in range(3000))
    c = b"".join(line(i, 2) for i in range(700))[:-1]
    return (a, b, c)


def cli_bodies():
    """(pod, container, body) of the CLI test: three small bodies, the last without a hit."""
    rng = random.Random(5)
    out = []
    for k, (pod, cont) in enumerate((("pod-0", "app"), ("pod-0", "sidecar"), ("pod-1", "app"))):
        lines = []
        for i in range(400):
            if k < 2 and i % 3 == 0:
                lines.append(_ts(i) + b"req e lat=%d.%02d took=%dms\n" % (rng.randrange(-20, 5000), rng.randrange(100),
                                                                           rng.randrange(3000)))
            elif i % 7 == 0:
                lines.append(_ts(i) + b"req e lat=? took=soon\n")
            else:
                lines.append(_ts(i) + b"idle e %d\n" % i)
        out.append((pod, cont, b"".join(lines)))
    return out


def test_big_streams_shape():
    refs = [FieldRef(s) for s in big_streams()]
    assert refs[0].n_lines == BIG_N > 2 * 8192 and all(r.n_parsed == r.n_lines for r in refs)
    rows, _ = field_stats(refs, [r.gprime() for r in refs], b"lat=", 3)
    assert all(r["hits"] > 100 and r["bad"] > 10 for r in rows) and rows[3]["hits"] > 5000
    assert rows[3]["min"] < -(1 << 33) and rows[3]["max"] > (1 << 33)
    rows, _ = field_stats(refs, [r.gprime() for r in refs], b"took=", 0, True)
    assert rows[3]["hits"] > 1000 and rows[3]["bad"] == 0


# ------------------------------------------- the extractor header in a stand-alone program ---

HOST_CHECK = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "klf_fieldval.hpp"
static std::vector<uint8_t> unhex(const char* s) {
  std::vector<uint8_t> v;
  if (s[0] == '-') return v;
  for (; s[0] && s[1]; s += 2) { char b[3] = {s[0], s[1], 0}; v.push_back((uint8_t)strtoul(b, nullptr, 16)); }
  return v;
}
int main(int argc, char** argv) {  // lines: content-hex key-hex decimals flags class value
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char c[4096], k[256];
  unsigned dec, flags;
  int cls, bad = 0, n = 0;
  long long want;
  while (fscanf(f, "%4095s %255s %u %u %d %lld", c, k, &dec, &flags, &cls, &want) == 6) {
    const std::vector<uint8_t> cv = unhex(c), kv = unhex(k);
    uint8_t* heap = (uint8_t*)malloc(cv.size() ? cv.size() : 1);  // exactly the content: a read past it is caught
    if (!cv.empty()) memcpy(heap, cv.data(), cv.size());
    klf::FieldHostBytes src{heap};
    int64_t v = 0;
    const int got = klf::field_classify(src, cv.size(), kv.data(), (uint32_t)kv.size(), dec, flags, &v);
    if (got != cls || (got == klf::kFieldHit && v != want)) { printf("case %d: class %d value %lld\n", n, got, (long long)v); ++bad; }
    free(heap);
    ++n;
  }
  printf("%d cases, %d wrong\n", n, bad);
  return bad ? 1 : 0;
}
"""


def test_extractor_header_stands_alone_under_sanitizers(tmp_path):
    """klf_fieldval.hpp in a program of its own (no HIP, no library), built with the address and
    undefined-behaviour sanitizers where the compiler has them: the by-hand table and the random
    contents, each in a heap block of exactly its length."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    rng = random.Random(7)
    cases = list(BY_HAND)
    for _ in range(1500):
        content = random_content(rng)
        duration = rng.random() < 0.5
        decimals = 0 if duration else rng.randrange(10)
        cases.append((content, b"lat", decimals, duration) + field_value(content, b"lat", decimals, duration))
    (tmp_path / "cases.txt").write_text("".join(
        "%s %s %d %d %d %d\n" % (c.hex() or "-", k.hex(), d, 1 if dur else 0, cls, v) for c, k, d, dur, cls, v in cases))
    (tmp_path / "check.cpp").write_text(HOST_CHECK)
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'klogs_amd' / 'csrc'}",
            str(tmp_path / "check.cpp"), "-o", str(tmp_path / "check")]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program still checks the table
        subprocess.run(base, check=True)
    r = subprocess.run([str(tmp_path / "check"), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 wrong" % len(cases) in r.stdout


# ---------------------------------------------------------------- the library (no device) ---

SYMBOLS = ("klf_result_field_stats", "klf_field_value")


def test_library_exports_field_stats():
    lib = E.lib()
    hdr = (ROOT / "include" / "klf.h").read_text()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in E.SIGNATURES, name
        assert name in hdr, name
    for name in ("klf_field_opts", "klf_field_row", "KLF_FIELD_DURATION", "KLF_FIELD_MAX_KEY", "KLF_FIELD_MAX_QUANTILES",
                 "KLF_FIELD_HIT", "KLF_FIELD_MISS", "KLF_FIELD_BAD"):
        assert name in hdr, name
    assert C.sizeof(E._FieldOpts) == 32 and C.sizeof(E._FieldRow) == 80 and E.FIELD_ROW.itemsize == 80
    assert [E.FIELD_ROW.fields[f][1] for f, _ in E._FieldRow._fields_] == \
        [getattr(E._FieldRow, f).offset for f, _ in E._FieldRow._fields_]
    assert re.search(r"#define KLF_FIELD_DURATION 1u\b", hdr) and E.FIELD_DURATION == 1
    assert re.search(r"#define KLF_FIELD_MAX_KEY 64u\b", hdr) and E.FIELD_MAX_KEY == 64
    assert re.search(r"#define KLF_FIELD_MAX_QUANTILES 16u\b", hdr) and E.FIELD_MAX_QUANTILES == 16
    for name, v in (("HIT", 0), ("MISS", 1), ("BAD", 2)):
        assert re.search(r"#define KLF_FIELD_%s %d\b" % (name, v), hdr) and getattr(E, "FIELD_" + name) == v


class Opts:
    """A klf_field_opts with the buffers it points to kept alive."""

    def __init__(self, key=b"lat=", decimals=0, flags=0, quantiles=(), key_len=None, null_key=False, null_q=False,
                 n_quantiles=None):
        self.kb = C.create_string_buffer(key, len(key) or 1)
        self.q = (C.c_uint16 * max(1, len(quantiles)))(*quantiles)
        self.o = E._FieldOpts(None if null_key else C.addressof(self.kb), None if null_q else C.addressof(self.q),
                              len(key) if key_len is None else key_len, decimals,
                              len(quantiles) if n_quantiles is None else n_quantiles, flags)


# every option the call refuses with KLF_EINVAL (also used on a live result by the GPU tests)
BAD_OPTS = {
    "null key": dict(null_key=True),
    "empty key": dict(key=b""),
    "key of 65 bytes": dict(key=b"k" * 65),
    "key_len 2^32 - 1": dict(key_len=0xFFFFFFFF),
    "decimals 10": dict(decimals=10),
    "decimals with a duration": dict(decimals=1, flags=1),
    "unknown flag": dict(flags=2),
    "unknown flags": dict(flags=0x80000001),
    "17 quantiles": dict(quantiles=tuple(range(17))),
    "a quantile above 10000": dict(quantiles=(5000, 10001)),
    "null quantiles": dict(quantiles=(5000,), null_q=True),
}


def test_field_stats_bad_arguments_are_einval_without_a_device():
    lib = E.lib()
    rows = (E._FieldRow * 4)()
    qv = (C.c_int64 * 64)()
    ok = Opts()
    assert lib.klf_result_field_stats(None, C.byref(ok.o), rows, qv, None) == E.KLF_EINVAL
    assert lib.klf_result_field_stats(None, None, rows, qv, None) == E.KLF_EINVAL
    assert lib.klf_result_field_stats(None, C.byref(ok.o), None, qv, None) == E.KLF_EINVAL
    for name, kw in BAD_OPTS.items():
        o = Opts(**kw)
        assert lib.klf_result_field_stats(None, C.byref(o.o), rows, qv, None) == E.KLF_EINVAL, name
    # klf_field_value
    src, key, v = C.create_string_buffer(b"lat=5"), C.create_string_buffer(b"lat="), C.c_int64(77)
    a, k = C.addressof(src), C.addressof(key)
    assert lib.klf_field_value(a, 5, k, 4, 0, 0, C.byref(v)) == HIT and v.value == 5
    assert lib.klf_field_value(None, 0, k, 4, 0, 0, C.byref(v)) == MISS and v.value == 0  # an empty content
    for args in ((None, 5, k, 4, 0, 0), (a, 5, None, 4, 0, 0), (a, 5, k, 0, 0, 0), (a, 5, k, 65, 0, 0),
                 (a, 5, k, 4, 10, 0), (a, 5, k, 4, 1, 1), (a, 5, k, 4, 0, 2)):
        assert lib.klf_field_value(*args, C.byref(v)) == E.KLF_EINVAL, args
    assert lib.klf_field_value(a, 5, k, 4, 0, 0, None) == E.KLF_EINVAL
    with pytest.raises(E.KlfError):
        E.field_value(b"lat=5", b"", 0)
