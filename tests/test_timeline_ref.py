"""klf_result_timeline (SPEC.md S4d: the emitted lines of all streams of a finished run in one
chronological sequence): the reference the GPU tests compare against, its self-check against the
oracle over every input the GPU tests use, and the library's new ABI entries.  No GPU here."""
import ctypes as C
import datetime
import random
from pathlib import Path

import pytest

import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import synth
from test_gpu_hist import SHUF_N, _shuffled_streams
from test_gpu_regroup import PATTERN_SETS
from test_gpu_window import SMALL, _based_streams
from test_window_ref import WindowRef

ROOT = Path(__file__).resolve().parent.parent
GZ = po.GO_ZERO_TIME


class TimelineRef(WindowRef):
    """WindowRef plus E: the lines of a selection g (flags per line: S4's G) that S4's tail rule
    and S3's since emit, restated line by line."""

    def base_flags(self):
        """G of a plain run: the matching lines, or every line on an engine without patterns."""
        return list(self.m) if self.patterned else [True] * self.n_lines

    def emitted(self, g, tail=-1, since=GZ):
        """Flags per line: the line is in E."""
        glist = [i for i in range(self.n_lines) if g[i]]
        e = [False] * self.n_lines
        if tail < -1 or tail == 0:
            return e
        start = 0
        if tail > 0:  # the start rank: max(0, T - n) over the newline-terminated lines of G
            terminated = sum(1 for i in glist if self.data[self.lines[i][0]:self.lines[i][1]].endswith(b"\n"))
            start = max(0, terminated - tail)
        counted = 0
        for i in glist[start:]:
            if tail > 0 and counted == tail:  # the stop: n parsed lines were counted
                break
            if self.ts[i] is None:  # unparseable: skipped, not counted
                continue
            counted += 1  # counted whether or not since drops it
            if tuple(self.ts[i]) >= tuple(since):
                e[i] = True
        # (the fragment rule follows: a trailing fragment is the last line of G, reached only
        # when fewer than n parsed lines were counted before it)
        return e

    def render(self, i, tag=b"", timestamps=False):
        s, e = self.lines[i]
        line = self.data[s:e]
        sp = line.index(b" ") + 1  # (a line of E is parsed: it has a space)
        return tag + (line[:sp] if timestamps else b"") + line[sp:] + (b"" if line.endswith(b"\n") else b"\n")


def merged(refs, flags, tags=None, timestamps=False):
    """(entries, bytes) of the timeline over the streams `refs` with E flags `flags`: entries are
    (sec, nsec, stream, line, off) tuples in timeline order."""
    keys = sorted((ref.ts[i][0], ref.ts[i][1], s, i) for s, (ref, e) in enumerate(zip(refs, flags))
                  for i in range(ref.n_lines) if e[i])
    out = bytearray()
    entries = []
    for sec, nsec, s, i in keys:
        entries.append((sec, nsec, s, i, len(out)))
        out += refs[s].render(i, tags[s] if tags is not None else b"", timestamps)
    return entries, bytes(out)


def stream_output(ref, e):
    """The invariant's right side from the reference: E's contents in input order."""
    return b"".join(ref.data[ref.lines[i][0]:ref.lines[i][1]].split(b" ", 1)[1] for i in range(ref.n_lines) if e[i])


# ------------------------------------------------------------- the inputs of the GPU tests ---

def _ts(sec, nsec=0):
    """The canonical prefix of synth.T0 + sec."""
    return b"2024-10-22T%02d:%02d:%02d.%09dZ " % (sec // 3600, sec // 60 % 60, sec % 60, nsec)


def small_streams():
    """Three streams over the SMALL lines: all of them (ending in a fragment with content), the
    reversed terminated ones ending in a fragment without content, and a terminated rotation."""
    a = b"".join(SMALL)
    b = b"".join(reversed(SMALL[:-1])) + b"2024-10-22T00:00:05.000000000Z "
    c = b"".join(SMALL[7:-1] + SMALL[:7])
    return [a, b, c]


def tie_streams():
    """Four streams whose lines all carry one instant, written four ways; ties inside a stream."""
    same = [b"2024-10-22T00:00:05.500000000Z ", b"2024-10-22T05:30:05.5+05:30 ", b"2024-10-22T00:00:05,5Z ",
            b"2024-10-21T23:00:05.500000000-01:00 "]
    return [b"".join(same[(s + j) % 4] + b"stream %d line %d HIT\n" % (s, j) for j in range(40 + s)) for s in range(4)]


def two_instant_streams():
    """Three streams of 300 lines alternating between two instants: ties across and inside."""
    lines = [b"2024-10-22T00:00:0%d.000000000Z s%%d l%d\n" % (j % 2, j) for j in range(300)]
    return [b"".join(ln % st for ln in lines) for st in range(3)]


YEARS = (1, 1969, 1970, 2024, 2099, 2100, 9999)


def range_streams():
    """Years on both sides of the epoch and of the fast parser's range, in two interleaved
    streams, descending in one of them."""
    lines = [b"%04d-%02d-%02dT%02d:00:00.%09dZ year %d k %d\n" % (y, 1 + k % 12, 1 + k, k, k * 111111111, y, k)
             for y in YEARS for k in range(3)]
    return [b"".join(lines[0::2]), b"".join(reversed(lines[1::2]))]


def digit_keys():
    """Instants around a base that differ from it in one key byte alone: nsec bytes 0..3 and sec
    bytes 0..4.  Years 0000..9999 keep |sec| below 2^38, so sec bytes 5..7 of the key only change
    together, with the sign: a few negative seconds stand for them."""
    base_sec, base_nsec = 0x0110203040, 0x01010101
    keys = {(base_sec, base_nsec), (-1, base_nsec), (-0x10203040, base_nsec), (-62135596800, 0)}
    for byte in range(4):
        for v in (0x00, 0x02, 0x03, 0x3A if byte == 3 else 0xFE):
            keys.add((base_sec, (base_nsec & ~(0xFF << (8 * byte))) | (v << (8 * byte))))
    for byte in range(5):
        for v in (0x00, 0x02, 0x03, 0x3A) if byte == 4 else (0x00, 0x03, 0x80, 0xFF):
            keys.add(((base_sec & ~(0xFF << (8 * byte))) | (v << (8 * byte)), base_nsec))
    assert all(-62135596800 <= sec <= 253402300799 and 0 <= nsec < 10**9 for sec, nsec in keys)
    return sorted(keys)


def digit_streams():
    """digit_keys as canonical lines, shuffled (fixed seed) into three streams."""
    keys = digit_keys()
    random.Random(5).shuffle(keys)
    lines = []
    for sec, nsec in keys:
        d = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=sec)
        lines.append(b"%04d-%02d-%02dT%02d:%02d:%02d.%09dZ key %d %d\n"
                     % (d.year, d.month, d.day, d.hour, d.minute, d.second, nsec, sec, nsec))
    return [b"".join(lines[k::3]) for k in range(3)]


SORT_T = 2048  # the scatter's items per block (klf_analysis.hpp kTlSortBlock)
SORT_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, SORT_T - 1, SORT_T, SORT_T + 1, 4095, 4096, 4097,
              8191, 8192, 8193, 20000)
assert 2 * SORT_T + 1 in SORT_SIZES


def sort_streams(n):
    """n lines: one shuffled stream (fixed seed; seconds and nanoseconds both vary) and one
    ascending stream with the rest."""
    a = n // 2
    secs = list(range(a))
    random.Random(n).shuffle(secs)
    first = b"".join(_ts(x % 86400, (x * 7919) % 10**9) + b"shuffled %d\n" % i for i, x in enumerate(secs))
    second = b"".join(_ts((3 * i) % 86400, i % 1000) + b"ascending %d\n" % i for i in range(n - a))
    return [first, second]


def long_line_streams():
    """One 100 KB line between short ones; the first stream's length is a multiple of 256, so the
    next stream follows it directly in the batch."""
    head = _ts(10) + b"short before\n"
    tail = _ts(5) + b"short after, earlier\n"
    body = _ts(7) + bytes(33 + (k * 7) % 90 for k in range(100_000)) + b"\n"
    first = head + body + tail
    pad = -(len(first) + len(_ts(8)) + 1) % 256
    first += _ts(8) + b"p" * pad + b"\n"
    assert len(first) % 256 == 0
    second = _ts(6) + b"next stream, first line\n" + _ts(9, 1) + b"next stream, fragment"
    return [first, second]


def mode_streams():
    return [synth.generate(synth.TEXT, 21, 0, 150_000, permille=20),
            synth.generate(synth.JSON, 22, 1, 120_000, permille=20, drop_final_nl=True),
            synth.generate(synth.ADVERSARIAL, 23, 2, 6000, permille=40, drop_final_nl=True)]


MODE_SINCE = (synth.T0 + 900, 0)


def patternless_streams():
    return [synth.generate(synth.TEXT, 71, 0, 200_000),
            synth.generate(synth.ADVERSARIAL, 72, 1, 4000, drop_final_nl=True)]


def which_set_streams():
    return [synth.generate(synth.JSON, 41, 0, 300_000, permille=30),
            synth.generate(synth.ADVERSARIAL, 42, 1, 5000, permille=40, drop_final_nl=True)]


def cli_bodies():
    """(pod, container, body) of the CLI test: two pods of two containers."""
    out = []
    for p in range(2):
        for cname in ("app", "sidecar"):
            out.append((f"pod-{p}", cname, synth.generate(synth.JSON, 61 + p, p * 2 + len(cname), 150_000 + 3000 * p,
                                                          permille=100, drop_final_nl=(cname == "sidecar"))))
    return out


# (name, streams, patterns, since, tails): every run of tests/test_gpu_timeline.py
def gpu_inputs():
    yield "small", small_streams(), {}, GZ, (-1, 0, 1, 5)
    yield "small HIT", small_streams(), dict(grep=[b"HIT"]), GZ, (-1, 0, 1, 5)
    yield "ties", tie_streams(), {}, GZ, (-1, 3)
    yield "key range", range_streams(), {}, GZ, (-1,)
    yield "digits", digit_streams(), {}, GZ, (-1,)
    yield "two instants", two_instant_streams(), {}, GZ, (-1,)
    for n in SORT_SIZES:
        yield f"sort {n}", sort_streams(n), {}, GZ, (-1,)
    yield "tiny", _based_streams(), {}, GZ, (-1, 2)
    yield "tiny HIT", _based_streams(), dict(grep=[b"HIT"]), GZ, (-1, 2)
    yield "shuffled", _shuffled_streams(), {}, GZ, (-1,)
    yield "long line", long_line_streams(), {}, GZ, (-1, 2)
    for name, pats in PATTERN_SETS.items():
        yield f"modes {name}", mode_streams(), pats, MODE_SINCE, (5,)
    yield "patternless", patternless_streams(), {}, (synth.T0 + 300, 0), (-1,)
    yield "which set", which_set_streams(), dict(grep=[synth.NEEDLE]), (synth.T0 + 600, 0), (3, -1)
    yield "cli", [b for _, _, b in cli_bodies()], dict(grep=[synth.NEEDLE]), GZ, (20,)


@pytest.mark.parametrize("case", list(gpu_inputs()), ids=lambda c: c[0])
def test_reference_equals_the_oracle(case):
    """E's contents are read_logs' output and |E| is _count_selected, for every GPU test input:
    only then is the reference trusted."""
    name, streams, pats, since, tails = case
    emitted = 0
    for data in streams:
        ref = TimelineRef(data, **pats)
        g = ref.base_flags()
        gfile = b"".join(data[s:e] for (s, e), f in zip(ref.lines, g) if f)
        for tail in tails:
            e = ref.emitted(g, tail, since)
            assert stream_output(ref, e) == po.read_logs(gfile, tail, since), (name, tail)
            assert sum(e) == po._count_selected(gfile, tail, since), (name, tail)
            assert all(ref.ts[i] is not None for i in range(ref.n_lines) if e[i])
            emitted += sum(e)
    if name not in ("sort 0", "modes never"):
        assert emitted > 0, name


def test_reference_on_regrouped_and_windowed_selections():
    """The same over G' and G'' (what klf_regroup and klf_window select from)."""
    for data in which_set_streams() + small_streams():
        ref = TimelineRef(data, grep=[synth.NEEDLE, b"HIT"])
        a, b = (synth.T0 + 900, 0), (synth.T0 + 2000, 0)
        for g in (ref.group(2, 1), ref.cut(a, b, 1, 1), ref.group(0, 0, True)):
            gfile = b"".join(data[s:e] for (s, e), f in zip(ref.lines, g) if f)
            for tail in (-1, 0, 1, 4):
                e = ref.emitted(g, tail, (synth.T0 + 600, 0))
                assert stream_output(ref, e) == po.read_logs(gfile, tail, (synth.T0 + 600, 0))
                assert sum(e) == po._count_selected(gfile, tail, (synth.T0 + 600, 0))


def test_merge_by_hand():
    t = b"2024-10-22T00:00:%02d.%09dZ "
    s0 = t % (2, 0) + b"b\n" + b"junk\n" + t % (1, 5) + b"a late\n" + t % (3, 0) + b"frag"
    s1 = b"2024-10-22T05:30:02+05:30 tie with b\n" + t % (1, 4) + b"first\n" + t % (9, 0)
    refs = [TimelineRef(s0), TimelineRef(s1)]
    flags = [r.emitted(r.base_flags()) for r in refs]
    assert flags == [[True, False, True, True], [True, True, True]]
    ent, out = merged(refs, flags)
    assert [(s, l) for _, _, s, l, _ in ent] == [(1, 1), (0, 2), (0, 0), (1, 0), (0, 3), (1, 2)]
    assert out == b"first\na late\nb\ntie with b\nfrag\n\n"
    assert [o for *_, o in ent] == [0, 6, 13, 15, 26, 31]
    ent, out = merged(refs, flags, tags=[b"A ", b""], timestamps=True)
    assert out.startswith(t % (1, 4) + b"first\nA " + t % (1, 5) + b"a late\n")
    assert out.endswith(b"A " + t % (3, 0) + b"frag\n" + t % (9, 0) + b"\n")
    # tail 1 on stream 1: the last terminated line is the start; the fragment follows only
    # because the rule has counted one parsed line by then -- it is not emitted
    assert refs[1].emitted(refs[1].base_flags(), 1) == [False, True, False]
    # an unparseable terminated line in the window lets the fragment through
    r = TimelineRef(t % (1, 0) + b"x\n" + b"junk\n" + t % (2, 0) + b"frag")
    assert r.emitted(r.base_flags(), 1) == [False, False, True]
    assert r.emitted(r.base_flags(), 2) == [True, False, True]


def test_digit_streams_cover_every_key_byte():
    refs = [TimelineRef(s) for s in digit_streams()]
    assert all(r.n_parsed == r.n_lines for r in refs)
    keys = sorted({tuple(ts) for r in refs for ts in r.ts})
    assert keys == digit_keys()  # the lines parse back to the keys they were made from
    assert any(sec < 0 for sec, _ in keys)

    def key_bytes(k):
        return k[1].to_bytes(4, "little") + (k[0] + (1 << 63)).to_bytes(8, "little")

    differ = set()
    for a in keys:
        for b in keys:
            d = [i for i in range(12) if key_bytes(a)[i] != key_bytes(b)[i]]
            if len(d) == 1:
                differ.add(d[0])
    assert differ == set(range(9)), differ  # one byte alone: nsec 0..3 and sec 0..4
    assert {key_bytes(k)[9:] for k in keys} == {b"\0\0\x80", b"\xff\xff\x7f"}  # sec bytes 5..7: the sign
    years = {int(r.data[r.lines[i][0]:r.lines[i][0] + 4]) for r in [TimelineRef(s) for s in range_streams()]
             for i in range(r.n_lines)}
    assert years == set(YEARS)


# ---------------------------------------------------------------- the library (no device) ---

SYMBOLS = ("klf_result_timeline", "klf_timeline_entries", "klf_timeline_bytes", "klf_timeline_write",
           "klf_timeline_ms", "klf_timeline_free")


def test_library_exports_timeline():
    lib = E.lib()
    hdr = (ROOT / "include" / "klf.h").read_text()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in E.SIGNATURES, name
        assert name in hdr, name
    for name in ("klf_timeline_opts", "klf_timeline_entry", "KLF_TIMELINE_TIMESTAMPS", "KLF_TIMELINE_MAX_TAG"):
        assert name in hdr, name
    assert C.sizeof(E._TimelineOpts) == 24
    assert E.TIMELINE_ENTRY.itemsize == 32
    assert (E.TIMELINE_TIMESTAMPS, E.TIMELINE_MAX_TAG) == (1, 1024)


def timeline_opts(tags=None, tag_off=None, flags=0, reserved=0):
    """(klf_timeline_opts, the buffers it points into)"""
    o = E._TimelineOpts()
    keep = []
    if tags is not None:
        buf = C.create_string_buffer(tags, len(tags) or 1)
        o.tags = C.addressof(buf)
        keep.append(buf)
    if tag_off is not None:
        arr = (C.c_uint32 * len(tag_off))(*tag_off)
        o.tag_off = C.addressof(arr)
        keep.append(arr)
    o.flags, o._reserved = flags, reserved
    return o, keep


# every option the call refuses with KLF_EINVAL on a result of two streams (also used on a live
# result by the GPU tests)
BAD_OPTS = {
    "unknown flag": dict(flags=2),
    "unknown flags": dict(flags=0x80000001),
    "reserved": dict(reserved=1),
    "tags without tag_off": dict(tags=b"ab"),
    "tag_off descends": dict(tags=b"abcd", tag_off=[0, 3, 2]),
    "tag too long": dict(tags=b"x" * 1030, tag_off=[0, 1025, 1030]),
}


def test_timeline_bad_arguments_are_einval_without_a_device():
    lib = E.lib()
    out = C.c_void_p()
    o, keep = timeline_opts()
    assert lib.klf_result_timeline(None, C.byref(o), C.byref(out)) == E.KLF_EINVAL
    assert lib.klf_result_timeline(None, None, C.byref(out)) == E.KLF_EINVAL
    assert lib.klf_result_timeline(None, C.byref(o), None) == E.KLF_EINVAL
    for name, kw in BAD_OPTS.items():
        o, keep = timeline_opts(**kw)
        assert lib.klf_result_timeline(None, C.byref(o), C.byref(out)) == E.KLF_EINVAL, name
    assert out.value is None
    n, p, ms = C.c_uint64(), C.c_void_p(), C.c_double()
    assert lib.klf_timeline_entries(None, C.byref(p), C.byref(n)) == E.KLF_EINVAL
    assert lib.klf_timeline_bytes(None, C.byref(p), C.byref(n)) == E.KLF_EINVAL
    assert lib.klf_timeline_write(None, 1, C.byref(n)) == E.KLF_EINVAL
    assert lib.klf_timeline_ms(None, C.byref(ms)) == E.KLF_EINVAL
    lib.klf_timeline_free(None)  # like free(NULL)
