"""klf_result_field_stats on the GPU (SPEC.md S4f): the statistics of a numeric field of a
finished run, against the reference of tests/test_fieldstats_ref.py.  Every call is compared in
full and exactly: all rows, all quantile values, and `lines` against the result's own counts."""
import os
import subprocess

import numpy as np
import pytest

from klogs_amd import engine as E
from klogs_amd import host as H
from klogs_amd import synth
from test_fieldstats_ref import (BAD_OPTS, BIG_N, CLI_QUANTILES, HIT, P62, U32, U64, FieldRef, Opts, big_streams,
                                 cli_bodies, field_stats, render_stats_tsv, row_sum, _ts)
from test_gpu_regroup import PATTERN_SETS
from test_gpu_window import SMALL, _based_streams

pytestmark = pytest.mark.gpu

QS = (0, 1, 5000, 9999, 10000)
FIELDS = [name for name, _ in E._FieldRow._fields_]


def as_dicts(rows):
    return [{f: int(r[f]) for f in FIELDS} for r in rows]


class Session:
    """One engine run over `streams`; every field_stats call is checked in full against the reference."""

    def __init__(self, streams, grep=(), match=(), since=None, tail=-1):
        self.streams = streams
        self.patterned = bool(list(grep) or list(match))
        self.refs = [FieldRef(s, grep, match) for s in streams]
        self.eng = E.Engine(0, grep=grep, match=match)
        self.eng.set_streams(len(streams))
        for i, s in enumerate(streams):
            if s:
                self.eng.stage(i, s)
        self.r = self.eng.run(since=since, tail=tail, n_streams=len(streams))
        self.g = [r.gprime() for r in self.refs]  # the set self.r was selected from
        self.size_key = "matched" if self.patterned else "parsed"  # |H| among the result's counts

    def check(self, key, decimals=0, duration=False, quantiles=QS, r=None, g=None, size_key=None):
        """One call on r (default: the session's result, selected from the flags g), checked in
        full; returns (rows, qvals) as the reference has them."""
        r = r or self.r
        g = g or self.g
        want_rows, want_q = field_stats(self.refs, g, key, decimals, duration, quantiles)
        rows, qv = r.field_stats(key, decimals, duration, quantiles)
        tag = (key, decimals, duration)
        assert rows.dtype == E.FIELD_ROW and len(rows) == len(self.streams) + 1
        got = as_dicts(rows)
        assert got == want_rows, (tag, [(i, a, b) for i, (a, b) in enumerate(zip(got, want_rows)) if a != b][:3])
        assert qv.shape == (len(self.streams) + 1, len(quantiles)) and qv.dtype == np.int64
        assert qv.tolist() == want_q, (tag, [(i, a, b) for i, (a, b) in enumerate(zip(qv.tolist(), want_q)) if a != b][:3])
        sizes = [r.stream_counts(i)[size_key or self.size_key] for i in range(len(self.streams))]
        assert [x["lines"] for x in got] == sizes + [sum(sizes)], tag
        assert r.field_ms >= 0
        return want_rows, want_q

    def close(self):
        self.r.free()
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


GRID = [(0, False), (3, False), (9, False), (0, True)]


# ------------------------------------------------------------------ 1. small, adversarial ---

def _with_fields(lines, fields):
    """`lines` with b" " + fields[i] behind line i's content (None: the line stays as it is)."""
    out = []
    for ln, f in zip(lines, list(fields) + [None] * len(lines)):
        if f is None:
            out.append(ln)
        elif ln.endswith(b"\n"):
            out.append(ln[:-1] + b" " + f + b"\n")
        else:
            out.append(ln + b" " + f)
    return out


# stream 0: SMALL (20 lines, 17 parsed) with negative values, the maximum of all streams at line 7
# (again at line 13 and in stream 1: the lowest (stream, line) wins), values that differ only above
# bit 32, durations
SMALL_FIELDS = [b"lat=-12.5 took=1m30.5s", b"lat=4294967297", None, b"lat=1", b"lat=8589934593.25 took=250ms",
                b"lat=-4294967296", b"lat=x", b"lat=99999999999", None, b"lat=0.125 took=1.5h", None, b"took=12.s",
                b"lat=-0.0009", b"lat=99999999999 took=7us", b"lat=17179869185", b"lat=5", None, b"lat=",
                b"lat=+3.1415926535 took=1h2m3s", b"lat=-7"]
STREAM_A = _with_fields(SMALL, SMALL_FIELDS)
# stream 1: every hit has the same value (no sort pass moves anything) ...
STREAM_SAME = [_ts(i) + (b"HIT " if i % 2 else b"") + b"lat=99999999999 took=5ms\n" for i in range(21)]
# ... 2: exactly one hit; 3: only bad lines; 4: only misses
STREAM_ONE = [_ts(i) + b"HIT nothing\n" for i in range(5)] + [_ts(5) + b"HIT lat=42 took=42ns\n"] + \
             [_ts(i) + b"HIT nothing\n" for i in range(6, 9)]
STREAM_BAD = [_ts(i) + b"HIT lat=%s took=%s\n" % (x, x) for i, x in enumerate([b"", b"abc", b"-", b".5", b"=====1"])]
STREAM_MISS = [_ts(i) + b"HIT la t=%d\n" % i for i in range(7)]


@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_small_adversarial(gpu, grep):
    streams = [b"".join(x) for x in (STREAM_A, STREAM_SAME, STREAM_ONE, STREAM_BAD, STREAM_MISS)]
    with Session(streams, grep=grep) as s:
        assert s.refs[0].n_lines == 20 and s.refs[0].n_parsed == 17
        for decimals, duration in GRID:
            for key in (b"lat=", b"took="):
                s.check(key, decimals, duration)
        rows, qv = s.check(b"lat=", 3)
        assert rows[1]["hits"] == rows[1]["lines"] and rows[1]["min"] == rows[1]["max"] == 99999999999000
        assert rows[2]["hits"] == 1 and (rows[2]["min_line"], rows[2]["max_line"]) == (5, 5)
        assert rows[3]["hits"] == 0 and rows[3]["bad"] == rows[3]["lines"] == 5 and rows[3]["max_line"] == U64
        assert rows[4]["hits"] == rows[4]["bad"] == 0 and rows[4]["lines"] == 7 and rows[4]["max_stream"] == U32
        # the maximum stands in streams 0 (twice) and 1: the lowest (stream, line) of them
        assert rows[5]["max"] == 99999999999000 and (rows[5]["max_stream"], rows[5]["max_line"]) == (0, 7)
        assert rows[5]["min"] < 0 and qv[5][0] == rows[5]["min"] and qv[5][4] == rows[5]["max"]
        if not grep:
            assert {4294967297000, 8589934593250, 17179869185000, -4294967296000} <= \
                {v for _, v in (f for f in s.refs[0].fields(b"lat=", 3, False) if f) if v}
            assert rows[0]["bad"] >= 2 and rows[0]["min"] == -4294967296000
        s.check(b"lat=", 0, False, ())          # no quantiles
        s.check(b"took=", 0, True, (10000, 0, 5000, 5000) * 4)  # sixteen, any order, duplicates
        s.check(b"t", 0, False)                 # a 1-byte key


# ------------------------------------------------------------------------------ 2. seams ---

def _seam_streams():
    """Stream 0's length is a multiple of 256 and it ends, unterminated, in "... lat=12"; stream 1
    begins with "34 ...": nothing behind a content's end may count."""
    first = _ts(0) + b"a lat=7\n" + _ts(1) + b"9 after a terminated line lat=5\r\n"
    pad = -(len(first) + len(_ts(2)) + len(b" lat=12")) % 256
    first += _ts(2) + b"e" * pad + b" lat=12"
    assert len(first) % 256 == 0
    second = b"34 no timestamp here\n" + _ts(3) + b"x lat=34\n"
    return [first, second]


def _tail_streams(tail, head):
    """A stream of a multiple of 256 bytes whose fragment ends in `tail`, then one that begins with `head`."""
    first = _ts(0) + b"a lat=1\n"
    pad = -(len(first) + len(_ts(1)) + len(tail)) % 256
    first += _ts(1) + b"e" * pad + tail
    assert len(first) % 256 == 0
    return [first, head + b" rest of the line\n" + _ts(2) + b"b lat=3\n"]


def test_seams(gpu):
    with Session(_seam_streams()) as s:
        for decimals, duration in GRID:
            s.check(b"lat=", decimals, duration)
        rows, _ = s.check(b"lat=")
        assert (rows[0]["hits"], rows[0]["min"], rows[0]["max"], row_sum(rows[0])) == (3, 5, 12, 24)  # 12, not 1234
        assert (rows[0]["max_line"], rows[1]["hits"], rows[1]["max"]) == (2, 1, 34)
    with Session(_tail_streams(b" lat=", b"56")) as s:  # a fragment ends in the key alone: bad
        rows, _ = s.check(b"lat=")
        assert (rows[0]["hits"], rows[0]["bad"]) == (1, 1)
    with Session(_tail_streams(b" la", b"t=56")) as s:  # ... in a proper prefix of the key whose rest opens the next stream: a miss
        rows, _ = s.check(b"lat=")
        assert (rows[0]["hits"], rows[0]["bad"], rows[0]["lines"]) == (1, 0, 2)
    with Session(_tail_streams(b" took=1", b"m5s")) as s:  # a duration's unit must not come from the next stream
        rows, _ = s.check(b"took=", 0, True)
        assert (rows[0]["hits"], rows[0]["bad"]) == (0, 1)
        s.check(b"took=", 0, False)
    with Session(_tail_streams(b" took=1m", b"s")) as s:  # "1m" stays a minute
        rows, _ = s.check(b"took=", 0, True)
        assert (rows[0]["hits"], rows[0]["max"]) == (1, 60 * 10**9)


def test_load_boundaries(gpu):
    """The key and the number each astride a 16-byte load boundary of their content, at every
    alignment: contents of 0..47 bytes of filler, then the field, then the next line's digits."""
    lines, k = [], 0
    for fill in range(48):
        for field in (b"latency_ms=1234567.891", b"took=1h2m3.5s"):
            lines.append(_ts(k) + b"f" * fill + field + b"\n")
            lines.append(_ts(k + 1) + b"f" * fill + field + b" z\n")
            k += 2
    with Session([b"".join(lines), b"".join(lines[5:])]) as s:
        rows, _ = s.check(b"latency_ms=", 3)
        assert rows[0]["hits"] == 96 and rows[0]["min"] == rows[0]["max"] == 1234567891
        rows, _ = s.check(b"took=", 0, True)
        assert rows[0]["hits"] == 96 and rows[0]["min"] == rows[0]["max"] == 3723500000000
        s.check(b"f" * 16 + b"l", 0)
        s.check(b"ms=1234567.", 2)


# ------------------------------------------------- 3. stream boundaries inside a bitmap word ---

def _field_based_streams():
    """_based_streams (about three lines a stream, many streams without bytes) with a field behind
    most lines; the values fall with the stream number, so the extremes lie in different streams."""
    out, k = [], 0
    for i, s in enumerate(_based_streams()):
        lines = s.split(b"\n")
        for j, ln in enumerate(lines):
            k += 1
            if ln and k % 5:
                lines[j] = ln + (b" lat=%d.%d" % (1000 - 3 * i + j, k % 10) if k % 11 else b" lat=oops")
        out.append(b"\n".join(lines))
    return out


@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_stream_boundaries_in_a_word(gpu, grep):
    streams = _field_based_streams()
    with Session(streams, grep=grep) as s:
        assert sum(r.n_lines for r in s.refs) < 1200  # ~3 lines a stream: several streams per word
        rows, _ = s.check(b"lat=", 1)
        n = len(streams)
        assert rows[n]["hits"] > (20 if grep else 400) and rows[n]["bad"] > (1 if grep else 20)
        assert rows[n]["min_stream"] != rows[n]["max_stream"]
        assert sum(1 for r in rows[:n] if r["hits"]) > (15 if grep else 150)  # rows are per stream
        assert any(r["lines"] == 0 for r in rows[:n]) and sum(r["hits"] for r in rows[:n]) == rows[n]["hits"]
        s.check(b"lat=", 0)
        s.check(b"lat=", 0, True)  # every line with the key is bad: a bare number


# ------------------------------------------- 4. more than two chunks, and a wave's rounds ---

BIG_CASES = {"no patterns": {}, "literal": dict(grep=[b"HIT"]), "regex set": PATTERN_SETS["regex set"]}


@pytest.fixture(scope="module", params=list(BIG_CASES))
def big_session(gpu, request):
    s = Session(list(big_streams()), **BIG_CASES[request.param])
    s.name = request.param
    yield s
    s.close()


def test_chunks_and_rounds(big_session):
    s = big_session
    assert BIG_N > 2 * 8192
    rows, qv = s.check(b"lat=", 3)
    assert all(r["hits"] > 0 for r in rows)  # hits in every stream
    assert rows[3]["hits"] >= 1000 and rows[3]["min"] < -(1 << 32) and rows[3]["max"] > (1 << 32)
    distinct = {f[1] for ref, g in zip(s.refs, s.g) for i, f in enumerate(ref.fields(b"lat=", 3, False))
                if f and g[i] and f[0] == HIT}
    assert len(distinct) >= 100
    first = s.r.field_stats(b"lat=", 3, False, QS)
    again = s.r.field_stats(b"lat=", 3, False, QS)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    s.check(b"lat=", 9)  # the large values leave 62 bits with nine decimals: bad
    if s.name != "regex set":
        assert s.check(b"took=", 0, True)[0][3]["hits"] > (100 if s.name == "literal" else 1000)
    s.check(b"took=", 0, False)


# ------------------------------------------- 4a. the sort at its block boundaries ---

SIXTEEN = (0, 1, 100, 500, 1000, 2500, 3333, 5000, 6667, 7500, 9000, 9500, 9900, 9990, 9999, 10000)


def _sort_size_streams(n_hits):
    """n_hits lines with a value over two streams, a few lines without the key or with a bad value
    between them.  The values: small ones of either sign, every fifth beyond 2^32 (either sign),
    every fourth the same 42: both stages of the sort move items, and ties exist."""
    lines = []
    for i in range(n_hits):
        v = (i * 7919) % 2003 - 1000
        if i % 5 == 0:
            v += (1 + i % 7) * (1 << 32) * (1 if i % 2 else -1)
        if i % 4 == 3:
            v = 42
        lines.append(b"req %d lat=%d done\n" % (i, v))
        if i % 97 == 50:
            lines.append(b"no field in this line\n")
        if i % 101 == 60:
            lines.append(b"lat=oops\n")
    lines = [_ts(k) + ln for k, ln in enumerate(lines)]
    cut = max(1, len(lines) * 2 // 5)
    return [b"".join(lines[:cut]), b"".join(lines[cut:])]


@pytest.mark.parametrize("n_hits", [1, 2047, 2048, 2049, 4097])  # one item; T - 1, T, T + 1, 2 T + 1 for kTlSortBlock
def test_sort_sizes(gpu, n_hits):
    with Session(_sort_size_streams(n_hits)) as s:
        rows, qv = s.check(b"lat=", quantiles=SIXTEEN)
        assert rows[2]["hits"] == n_hits and len(qv[2]) == 16
        if n_hits > 1:
            assert rows[0]["hits"] and rows[1]["hits"] and rows[2]["bad"] and rows[2]["lines"] > n_hits + rows[2]["bad"]
            assert rows[2]["min"] < -(1 << 32) and rows[2]["max"] > (1 << 32) and 42 in qv[2]


# --------------------------------------------------------------- 5. a sum beyond 64 bits ---

def test_sum_beyond_64_bits(gpu):
    big = P62 - 1
    up = b"".join(_ts(i) + b"n=%d\n" % (big - i) for i in range(8))
    down = b"".join(_ts(i) + b"n=-%d\n" % (big - 2 * i) for i in range(8))
    mixed = b"".join(_ts(i) + b"n=%d\n" % ((big - 10 - i) * (1 if i % 2 else -1)) for i in range(8))
    with Session([up, down, mixed]) as s:
        rows, _ = s.check(b"n=")
        assert rows[0]["sum_hi"] == 1 and row_sum(rows[0]) == 8 * big - 28
        assert rows[1]["sum_hi"] == -2 and row_sum(rows[1]) == -(8 * big - 56)
        assert row_sum(rows[2]) == -4 and rows[2]["sum_hi"] == -1 and rows[2]["hits"] == 8  # cancels to a small sum
        assert row_sum(rows[3]) == 24 and rows[3]["hits"] == 24 and rows[3]["min"] == -big and rows[3]["max"] == big
        s.check(b"n=", 1)  # every line bad


# ------------------------------------------------------------------------ 6. long lines ---

def test_long_lines(gpu):
    body = bytes(97 + (k * 7) % 26 for k in range(70_000))
    a = _ts(0) + b"short lat=1\n" + _ts(1) + body + b" lat=123.456 end\n" + _ts(2) + body + b"\n" + _ts(3) + b"lat=2\n"
    b = _ts(0) + body + b" lat=77"  # the field at the very end of an unterminated long line
    with Session([a, b]) as s:
        assert max(e - b_ for r in s.refs for b_, e in r.lines) > 70_000
        rows, _ = s.check(b"lat=", 2)
        assert (rows[0]["lines"], rows[0]["hits"], rows[0]["max"], rows[0]["max_line"]) == (4, 3, 12345, 1)
        assert (rows[1]["hits"], rows[1]["max"]) == (1, 7700)
        s.check(b"lat=", 0, True)
        s.check(body[-64:], 0)  # a 64-byte key
        s.check(b"zz", 0)       # a key that is nowhere


# ------------------------------------------------------------- 7. composition, read-only ---

def _composition_streams():
    out = []
    for seed, (kind, size) in enumerate(((synth.TEXT, 200_000), (synth.ADVERSARIAL, 5000))):
        data = synth.generate(kind, 31 + seed, seed, size, permille=60, drop_final_nl=bool(seed))
        lines = data.split(b"\n")
        for j in range(len(lines)):
            if lines[j] and j % 3 == 0:
                lines[j] += b" latency_ms=%d.%d took=%dms" % ((j * 37) % 5000 - 100, j % 10, (j * 91) % 700)
        out.append(b"\n".join(lines))
    return out


def test_composition_and_read_only(gpu):
    streams = _composition_streams()
    a, b = (synth.T0 + 900, 0), (synth.T0 + 2000, 0)
    with Session(streams, grep=[synth.NEEDLE, b"cache miss"], since=(synth.T0 + 600, 0), tail=3) as s:
        r = s.r

        def state(x):
            return [(x.stream(i).out, x.match_bits(i), x.group_bits(i), x.stream(i).counts) for i in range(2)]

        before = state(r)
        first = s.check(b"latency_ms=", 1)
        assert first[0][2]["hits"] > 10
        r.histogram((synth.T0, 0), 60 * 10**9, 30)
        with r.groups(5, True) as gr:
            assert len(gr) > 0
        assert s.check(b"latency_ms=", 1) == first  # stats, histogram, groups, stats again
        s.check(b"took=", 0, True)
        assert state(r) == before
        lib = E.lib()
        rows, qv = (E._FieldRow * 3)(), (E.C.c_int64 * 48)()
        for name, kw in BAD_OPTS.items():
            o = Opts(**kw)
            assert lib.klf_result_field_stats(r._p, E.C.byref(o.o), rows, qv, None) == E.KLF_EINVAL, name
        ok = Opts(quantiles=(5000,))
        assert lib.klf_result_field_stats(r._p, None, rows, qv, None) == E.KLF_EINVAL
        assert lib.klf_result_field_stats(r._p, E.C.byref(ok.o), None, qv, None) == E.KLF_EINVAL
        assert lib.klf_result_field_stats(r._p, E.C.byref(ok.o), rows, None, None) == E.KLF_EINVAL  # quantiles without qvals
        assert lib.klf_result_field_stats(r._p, E.C.byref(ok.o), rows, qv, None) == E.KLF_OK
        assert state(r) == before
        r1 = r.retail(-1)  # a re-tail: H is unchanged
        assert s.check(b"latency_ms=", 1, r=r1) == first
        r2 = r1.window(a, b)  # stats over G''
        g2 = [ref.cut(a, b) for ref in s.refs]
        cut = s.check(b"latency_ms=", 1, r=r2, g=g2)
        assert 0 < cut[0][2]["lines"] < first[0][2]["lines"]
        with pytest.raises(E.KlfError) as ei:  # r1 is not the latest any more
            r1.field_stats(b"latency_ms=")
        assert ei.value.code == E.KLF_ESTATE
        r3 = r2.regroup(0, 0, True)  # stats over G': what else is in there
        g3 = [ref.group(0, 0, True) for ref in s.refs]
        inv = s.check(b"latency_ms=", 1, r=r3, g=g3)
        assert inv[0][2]["lines"] + first[0][2]["lines"] == sum(ref.n_parsed for ref in s.refs)
        assert inv[0][2]["hits"] > first[0][2]["hits"]
        for x in (r, r1, r2, r3):
            x.free()
        s.r = s.eng.run(since=None, tail=1, n_streams=2)
        assert s.check(b"latency_ms=", 1) == first


# ---------------------------------------------------------------------------- 8. empty ---

def test_empty_and_streams_without_bytes(gpu):
    streams = [b"".join(STREAM_A), b"".join(STREAM_ONE)]
    empty_row = dict(lines=0, hits=0, bad=0, min=0, max=0, sum_lo=0, sum_hi=0, min_line=U64, max_line=U64, min_stream=U32,
                     max_stream=U32)
    with Session(streams, grep=[b"matches nothing at all"]) as s:
        rows, qv = s.check(b"lat=")
        assert rows == [empty_row] * 3 and qv == [[0] * 5] * 3
    # streams without bytes among streams with bytes: the rows are indexed by stream id
    streams = [b"", b"".join(STREAM_ONE), b"", b"", b"".join(STREAM_A), b""]
    with Session(streams) as s:
        rows, _ = s.check(b"lat=", 2)
        assert [r["hits"] > 0 for r in rows] == [False, True, False, False, True, False, True]
        assert rows[0] == rows[2] == rows[5] == empty_row
        assert (rows[6]["max_stream"], rows[6]["max_line"]) == (4, 7) and rows[1]["max_stream"] == 1
        s.check(b"took=", 0, True)
        rows_only, qv = s.r.field_stats(b"lat=", 2)  # n_quantiles = 0 with qvals = NULL
        assert qv.shape == (7, 0) and [int(x) for x in rows_only["hits"]] == [r["hits"] for r in rows]
    with Session([b"", b"junk lat=5\n", b""]) as s:  # no parsed line
        rows, _ = s.check(b"lat=")
        assert rows == [empty_row] * 4
    eng = E.Engine(0)
    eng.set_streams(2)
    r = eng.run(n_streams=2)  # no stream has bytes
    rows, qv = r.field_stats(b"lat=", 0, False, (5000,))
    assert [{f: int(x[f]) for f in FIELDS} for x in rows] == [empty_row] * 3 and qv.tolist() == [[0]] * 3
    r.free()
    eng.close()


# ------------------------------------------------------------------------------- 9. CLI ---

def test_cli_stat(gpu, tmp_path):
    bodies, rows = cli_bodies(), []
    for pod, cname, data in bodies:
        f = tmp_path / f"body_{pod}_{cname}.log"
        f.write_bytes(data)
        rows.append((pod, "container", cname, str(f)))
    m = tmp_path / "manifest.tsv"
    m.write_text("".join("\t".join(r) + "\n" for r in rows))
    now = synth.T0 + synth.SPAN + 1
    base = ["--grep", "e", "-t", "20", "--now", str(now), "--no-color", str(m)]
    cases = (("plain", []), ("lat", ["--stat", "lat=", "--stat-decimals", "2"]), ("int", ["--stat", "lat="]),
             ("took", ["--stat", "took=", "--stat-duration"]))
    for name, extra in cases:
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / name)] + extra + base, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
    names = sorted(H.log_file_name(p, c) for p, c, _ in bodies)
    assert sorted(os.listdir(tmp_path / "plain")) == names  # without --stat: no stats.tsv
    refs = [FieldRef(data, grep=[b"e"]) for _, _, data in bodies]
    flags = [ref.gprime() for ref in refs]
    pc = [(p, c) for p, c, _ in bodies]
    for name, key, decimals, duration in (("lat", b"lat=", 2, False), ("int", b"lat=", 0, False), ("took", b"took=", 0, True)):
        assert sorted(os.listdir(tmp_path / name)) == sorted(names + ["stats.tsv"])
        for nm in names:
            assert (tmp_path / name / nm).read_bytes() == (tmp_path / "plain" / nm).read_bytes() != b"", nm
        want_rows, want_q = field_stats(refs, flags, key, decimals, duration, CLI_QUANTILES)
        assert want_rows[0]["hits"] > 100 and want_rows[2]["hits"] == 0 and want_rows[2]["bad"] > 10  # taken before --tail 20
        got = (tmp_path / name / "stats.tsv").read_bytes()
        assert got == render_stats_tsv(want_rows, want_q, pc, decimals)
        assert got.count(b"\n") == 4 and got.splitlines()[2].endswith(b"\t-\t-\t-\t-\t-\t-\t-") and b"\n*\t*\t" in got
    # usage errors: an empty key or one over 64 bytes, D outside 0..9, both sub-flags, a sub-flag without --stat
    for extra in (["--stat", ""], ["--stat", "k" * 65], ["--stat", "lat=", "--stat-decimals", "10"],
                  ["--stat", "lat=", "--stat-decimals", "-1"], ["--stat", "lat=", "--stat-decimals", "x"],
                  ["--stat", "lat=", "--stat-decimals", "2", "--stat-duration"], ["--stat-decimals", "2"],
                  ["--stat-duration"]):
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / "none")] + extra + base, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 1 and "usage:" in r.stderr, extra
    assert not (tmp_path / "none").exists()
