"""klf_records on the GPU (SPEC.md S4h): whole multi-line records over a finished run, against the
reference of tests/test_records_ref.py.  Each case is one engine run and then many calls; every
call is compared in full and exactly, per stream: the output bytes, matched / selected /
out_bytes, the unchanged lines / parsed / since_ok, group_bits, and match_bits still M; and the
heads / continuations of records_info against the reference's classification."""
import os
import random
import subprocess

import numpy as np
import pytest

import c_oracle as co
import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import host as H
from klogs_amd import synth
from test_gpu_regroup import CARRY_N, PATTERN_SETS, _tiny_streams, ts
from test_records_ref import FRAGMENT, HAND_OPTS, HAND_STREAMS, RecordsRef, lib_flags, opts, raw_opts
from test_timeline_ref import merged
from test_window_ref import OPEN_HI, OPEN_LO

pytestmark = pytest.mark.gpu

GZ = po.GO_ZERO_TIME
COUNT_KEYS = ("lines", "parsed", "since_ok")
INDENT = opts(indent=True)
WHOLE = opts(head_mode=True)  # head mode without prefixes: each stream one record


def opt(t):
    """A reference bound as Result.records takes it (None = open)."""
    return None if t in (OPEN_LO, OPEN_HI) else t


def inv(o):
    return dict(o, invert=not o["invert"])


class Session:
    """One engine run over `streams`; every records call is checked in full against the reference."""

    def __init__(self, streams, grep=(), match=(), since=None, tail=-1, refs=None, run=None):
        self.streams = streams
        self.since = since
        self.refs = refs if refs is not None else [RecordsRef(s, grep, match) for s in streams]
        self.mbits = [r.m_bits() for r in self.refs]
        self.eng = E.Engine(0, grep=grep, match=match)
        if run is None:
            self.eng.set_streams(len(streams))
            for i, s in enumerate(streams):
                if s:
                    self.eng.stage(i, s)
            self.r = self.eng.run(since=since, tail=tail, n_streams=len(streams))
        else:
            self.r = run(self.eng)
        self.base = [self.r.stream_counts(i) for i in range(len(streams))]
        self.memo = {}

    def flags(self, o, frm=OPEN_LO, until=OPEN_HI):
        return [r.cut(o, frm, until) for r in self.refs]

    def sizes(self, o, frm=OPEN_LO, until=OPEN_HI):
        """(|G''|, |M|, parsed lines) over all streams, by the reference."""
        return (sum(map(sum, self.flags(o, frm, until))), sum(sum(r.m) for r in self.refs),
                sum(r.n_parsed for r in self.refs))

    def check_flags(self, r, g, tail=-1, what=""):
        """Result r against the selection flags g (per stream) tailed with `tail`."""
        for i, ref in enumerate(self.refs):
            key = (i, ref.pack(g[i]), tail)  # (many calls select the same lines)
            if key not in self.memo:
                self.memo[key] = ref.emit(g[i], tail, self.since or GZ)
            out, n, gbits, nsel = self.memo[key]
            tag = (what, i, tail)
            so = r.stream(i)
            assert so.out == out, tag
            c = so.counts
            assert (c["matched"], c["selected"], c["out_bytes"]) == (n, nsel, len(out)), (tag, c)
            for k in COUNT_KEYS:
                assert c[k] == self.base[i][k], (tag, k, c, self.base[i])
            assert r.group_bits(i) == gbits, tag
            assert r.match_bits(i) == self.mbits[i], tag

    def records(self, o, frm=OPEN_LO, until=OPEN_HI, tail=-1):
        pre = o["head"] if o["head_mode"] else o["cont"]
        old, self.r = self.r, self.r.records(cont=pre, from_=opt(frm), until=opt(until), tail=tail, flags=lib_flags(o))
        old.free()
        self.check_flags(self.r, self.flags(o, frm, until), tail, ("records", tuple(o.items()), frm, until))
        heads, conts, ms = self.r.records_info()
        want = [ref.class_counts(o) for ref in self.refs]
        assert (heads, conts) == (sum(h for h, _ in want), sum(c for _, c in want)), (o, heads, conts)
        assert heads + conts == sum(r.n_parsed for r in self.refs) and ms >= 0.0
        return self.r

    def close(self):
        self.r.free()
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---------------------------------------------------------------------- 1. small adversarial ---

SMALL_SINCE = po.parse_line(b"2024-10-22T00:00:03Z x")[0]


@pytest.mark.parametrize("since", [None, SMALL_SINCE])
@pytest.mark.parametrize("grep", [b"ERROR", b"at", b"NEEDLE", b"ValueError"])
def test_small_adversarial(gpu, grep, since):
    """The by-hand streams of the reference file, every option set plain and inverted."""
    with Session(HAND_STREAMS, grep=[grep], since=since) as s:
        assert sum(r.n_lines for r in s.refs) == 31 and sum(r.n_parsed for r in s.refs) == 28
        assert not HAND_STREAMS[4].endswith(b"\n")
        seen = set()
        for o in HAND_OPTS + [WHOLE]:
            for oo in (o, inv(o)):
                for tail in (-1, 0, 1, 3):
                    s.records(oo, tail=tail)
                seen.add(s.sizes(oo)[0])
        assert len(seen) >= 4


# ----------------------------------------------------- 2. stream boundaries inside a bitmap word ---

def _tiny_record_streams():
    """_tiny_streams' shape (about 300 streams of 0..5 lines, some empty, some ending in a
    fragment, some lines unparseable), with every stream's first line and about half of the others
    shaped like a continuation."""
    rng = random.Random(11)
    out = []
    for s in _tiny_streams():
        lines = s.split(b"\n")
        body = []
        for j, ln in enumerate(lines):
            if ln and b" " in ln and (j == 0 or rng.random() < 0.5):
                head, rest = ln.split(b" ", 1)
                ln = head + b" \t" + rest
            body.append(ln)
        out.append(b"\n".join(body))
    return out


def test_stream_boundaries_in_a_word(gpu):
    streams = _tiny_record_streams()
    with Session(streams, grep=[b"HIT"]) as s:
        assert len(streams) == 300 and any(not x for x in streams) and sum(r.n_lines for r in s.refs) < 1200
        first_cont = sum(1 for r in s.refs if r.n_parsed and r.is_cont(INDENT)[[i for i in range(r.n_lines) if r.parsed[i]][0]])
        last_rec_hit = sum(1 for r in s.refs if r.n_parsed and any(r.m[i] for i in r.record_list(INDENT)[-1]))
        assert first_cont > 150 and last_rec_hit > 60
        m, nm, parsed = s.sizes(INDENT)
        assert nm < m < parsed
        for o in (INDENT, inv(INDENT), WHOLE, inv(WHOLE), opts(cont=[b"\tq"]), opts(head=[b"HIT", b"quiet 1"])):
            s.records(o)
            s.records(o, tail=2)


# ---------------------------------------------------------------- 3. word and chunk carries ---

# heads of layout 1: records that end or start at lines 31 / 32 / 33 and 8191 / 8192 / 8193, and one
# from 8200 over the rest of chunk 1, all of chunk 2 and into chunk 3
HEADS_1 = (0, 20, 31, 32, 33, 50, 64, 96, 8000, 8191, 8192, 8193, 8200, 24600, 24700, CARRY_N - 1)
# heads of layout 2: records split exactly at the chunk edges, one a single line
HEADS_2 = (0, 8192, 16384, 16385, 24576)
CARRY_CASES = {
    "left carry through a chunk without a start": (HEADS_1, (8200, 31, 8191, 40)),
    "right carry from the record's last line": (HEADS_1, (24599, 32, 8192, 49, CARRY_N - 1)),
    "ends of records at word and chunk edges": (HEADS_1, (30, 7999, 8190, 8199, 24699)),
    "back to back at a chunk edge, the second matched": (HEADS_2, (12000,)),
    "back to back at a chunk edge, the first matched in its last line": (HEADS_2, (8191, 16384)),
    "one match at line 0": (HEADS_2, (0,)),
    "one match at the last line": (HEADS_2, (CARRY_N - 1,)),
    "no match": (HEADS_2, ()),
}


@pytest.mark.parametrize("name", list(CARRY_CASES))
def test_word_and_chunk_carries(gpu, name):
    heads, hits = CARRY_CASES[name]
    big = b"".join(ts(i) + (b"" if i in heads else b"\t") + (b"HIT %05d padding .....\n" if i in hits else b"line %05d padding ....\n") % i
                   for i in range(CARRY_N))
    second = b"".join(ts(i) + (b"HIT second\n" if i == 0 else b"\tsecond %d\n" % i) for i in range(40))
    with Session([big, second], grep=[b"HIT"]) as s:
        ref = s.refs[0]
        assert [i for i, m in enumerate(ref.m) if m] == sorted(hits) and ref.n_parsed == ref.n_lines == CARRY_N
        assert [r[0] for r in ref.record_list(INDENT)] == list(heads)
        g = ref.group(INDENT)
        if name.startswith("left carry"):
            assert all(g[8200:24600]) and not g[24600] and g[31] and not g[30] and not g[32] and g[8191] and not g[8192]
        if name.startswith("right carry"):
            assert all(g[8200:24600]) and not g[8199] and g[32] and not g[31] and g[8192] and not g[8191] and all(g[33:50]) and not g[50]
        if name.startswith("back to back at a chunk edge, the second"):
            assert sum(g) == 8192 and all(g[8192:16384])
        if name.startswith("back to back at a chunk edge, the first"):
            assert sum(g) == 8193 and all(g[0:8192]) and g[16384] and not g[8192] and not g[16385]
        for o in (INDENT, inv(INDENT), WHOLE, inv(WHOLE)):
            s.records(o)
        s.records(INDENT, tail=7)
        assert s.sizes(WHOLE)[0] == (CARRY_N + 40 if hits else 40)  # the second stream's own match selects it whole


# ------------------------------------------------------------------------------- 4. seams ---

def _seam_layout(abut):
    """Three streams in tests/seams.py' device layout (bases at multiples of 256, klf_layout's):
    stream 0 ends in the fragment '... Caused b', stream 1 in a fragment with an empty content.
    abut: their lengths are multiples of 256 and the next stream's first bytes ('y: x', then a
    space) lie right behind them; else the pads behind them begin with those bytes."""
    from seams import ALIGN, SLACK, Layout

    def fit(lines, last, tail_bytes):
        body = b"".join(lines) + last
        if abut:  # a filler line behind the first one brings the length to a multiple of 256
            pad = (-(len(body) + len(ts(7)) + 1)) % ALIGN
            body = lines[0] + ts(7) + b"f" * pad + b"\n" + b"".join(lines[1:]) + last
            assert len(body) % ALIGN == 0
        return body

    s0 = fit([ts(1) + b"ERROR boom\n", ts(2) + b"\tat a.b(C.java:1)\n", ts(3) + b"INFO next HIT\n"], ts(4) + b"Caused b", b"y: x")
    s1 = fit([b"y: x is what was cut off\n", ts(5) + b"ERROR again HIT\n", ts(6) + b"\tat d.e(F.java:2)\n"], ts(8), b" ")
    s2 = b" an indented first line without a timestamp\n" + ts(9) + b"INFO last\n"
    streams = [s0, s1, s2]
    bases, pos = [], 0
    for x in streams:
        bases.append(pos)
        pos = (pos + len(x) + ALIGN - 1) // ALIGN * ALIGN
    buf = bytearray(b" " * (pos + SLACK))
    for b, x in zip(bases, streams):
        buf[b:b + len(x)] = x
    if not abut:
        buf[bases[0] + len(s0):bases[0] + len(s0) + 4] = b"y: x"
    assert bytes(buf[bases[0] + len(s0):bases[0] + len(s0) + 4]) == b"y: x" and buf[bases[1] + len(s1)] == 0x20
    return Layout("R", bytes(buf), bases, [len(x) for x in streams])


@pytest.mark.parametrize("abut", [True, False])
def test_seams(gpu, abut):
    """The classification is that of the bytes inside the line only: 'Caused b' is no 'Caused by:'
    whatever lies behind the stream, and an empty content is neither indented nor 'y'."""
    import torch
    lay = _seam_layout(abut)
    d = torch.from_numpy(np.frombuffer(lay.buf, dtype=np.uint8).copy()).to("cuda")
    torch.cuda.synchronize()
    with Session(lay.streams(), grep=[b"HIT"], run=lambda eng: eng.run_device(d.data_ptr(), lay.bases, lay.lens)) as s:
        r0, r1 = s.refs[0], s.refs[1]
        assert r0.c[-1] == b"Caused b" and r1.c[-1] == b"" and not r1.parsed[0]
        caused = opts(indent=True, cont=[b"Caused by:"])
        assert r0.is_cont(caused)[-1] is False and r1.is_cont(caused)[-1] is False  # heads: records of their own
        # each follows a matching record, which it would join if it were taken for a continuation
        assert r0.group(caused)[-2:] == [True, False] and r1.group(caused)[-2:] == [True, False]
        for o in (caused, inv(caused), opts(indent=True, cont=[b"Caused by: x"]), opts(cont=[b"Caused b"]),
                  opts(cont=[b"Caused by"]), opts(blank=True), opts(indent=True, blank=True), opts(head=[b" "]),
                  opts(head=[b"Caused by:", b"ERROR", b"INFO"]), opts(cont=[b" "])):
            s.records(o)
            s.records(o, tail=2)
        assert r1.group(opts(indent=True, blank=True))[-1] is True and r1.group(opts(cont=[b" "]))[-1] is False
    del d


# -------------------------------------- 5. every pattern mode, from a run with a partial index ---

def _indented(data, seed):
    """`data` with an indented block of 1..4 lines behind about every sixth line (the block's lines
    repeat the line's own timestamp)."""
    rng = random.Random(seed)
    out = []
    for ln in data.split(b"\n"):
        out.append(ln)
        stamp = ln.split(b" ", 1)[0]
        if b" " in ln and len(stamp) <= 40 and rng.random() < 0.17:
            for k in range(rng.randrange(1, 5)):
                out.append(stamp + (b" \tat frame %d" % k if k % 2 == 0 else b"   caused by timeout backoff %d" % k))
    return b"\n".join(out)


@pytest.mark.parametrize("name", list(PATTERN_SETS))
def test_pattern_modes_from_a_partial_index(gpu, name):
    pats = PATTERN_SETS[name]
    streams = [_indented(synth.generate(synth.TEXT, 21, 0, 100_000, permille=20), 1),
               _indented(synth.generate(synth.JSON, 22, 1, 90_000, permille=20, drop_final_nl=True), 2),
               _indented(synth.generate(synth.ADVERSARIAL, 23, 2, 600, permille=40, drop_final_nl=True), 3)]
    assert all(len(x) <= 150_000 for x in streams)
    frm, until = (synth.T0 + 1200, 0), (synth.T0 + 2700, 0)
    with Session(streams, since=(synth.T0 + 900, 0), tail=5, **pats) as s:
        m, nm, parsed = s.sizes(INDENT)
        if name == "never":
            assert m == nm == 0
        elif name == "all":
            assert m == nm == parsed
        else:
            assert s.r.index_mode() != "full"  # the call builds the rest of the index
            assert nm < m < parsed
        for tail in (-1, 5):
            s.records(INDENT, tail=tail)
            s.records(inv(INDENT), frm, until, tail=tail)
        s.records(opts(head=[b"{", b"I", b"E", b"W"]), tail=5)


# ------------------------------------------------- 6. trailing fragment and drop_final_nl ---

def test_trailing_fragment_ends_the_last_record(gpu):
    json = _indented(synth.generate(synth.JSON, 31, 0, 60_000, permille=30, drop_final_nl=True), 4)
    json += b"\n" + ts(1) + b"ERROR the last head " + synth.NEEDLE + b"\n" + ts(2) + b"\tat the.last(Frame.java:9)"
    streams = [json, FRAGMENT, synth.generate(synth.TEXT, 32, 1, 40_000, permille=30, drop_final_nl=True)]
    with Session(streams, grep=[synth.NEEDLE, b"ERROR"], match=[b"(?i)timeout [a-z]+="]) as s:
        assert not any(x.endswith(b"\n") for x in streams)
        g = s.refs[0].group(INDENT)
        assert g[-1] and g[-2] and not s.refs[0].m[-1]  # the fragment is selected through its head
        for o in (INDENT, inv(INDENT), WHOLE):
            for tail in (-1, 1, 2, 9):
                s.records(o, tail=tail)
        s.records(INDENT)
        assert s.r.stream(0).out.endswith(b"ERROR the last head " + synth.NEEDLE + b"\n\tat the.last(Frame.java:9)")


# --------------------------------------------------------------------------- 7. output growth ---

def test_output_growth(gpu, monkeypatch):
    monkeypatch.setenv("KLF_DEBUG_OUT_INIT", "4096")
    n = 10_000
    a = b"".join(ts(i) + (b"HIT once\n" if i == 1234 else b"\tat frame %d of a very long trace\n" % i) for i in range(n))
    b = b"".join(ts(i) + b"line %d of the second stream\n" % i for i in range(n))
    assert len(a) + len(b) <= 1_500_000
    with Session([a, b], grep=[b"HIT"]) as s:
        assert [len(s.r.stream(i).out) for i in range(2)] == [len(b"HIT once\n"), 0]
        r = s.records(INDENT)  # the orphans ahead of the match are a record of their own
        assert s.sizes(INDENT) == (n - 1234, 1, 2 * n)
        so = r.stream(0)
        assert so.counts["matched"] == so.counts["selected"] == n - 1234 and len(so.out) > 100_000
        r = s.records(inv(INDENT))
        assert r.stream(1).counts["selected"] == n and len(r.stream(1).out) > 100_000


# ----------------------------------------------------------------- 8. chaining and state ---

def test_chaining_and_state(gpu):
    # stream 0: a head every sixth line, every fifth of them matching, a second apart (a record's
    # lines differ in their instants, so a window can hold a record's tail without its head)
    traces = b"".join(ts(i) + ((b"ERROR request %d failed " % i + (synth.NEEDLE if i % 30 == 0 else b"quietly")) if i % 6 == 0
                               else b"\tat frame %d lat=%d" % (i, i % 97)) + b"\n" for i in range(3000))
    streams = [traces,
               _indented(synth.generate(synth.ADVERSARIAL, 42, 1, 500, permille=40, drop_final_nl=True), 6),
               _indented(synth.generate(synth.TEXT, 43, 2, 100_000, permille=0), 7)]
    since = (synth.T0 + 600, 0)
    with Session(streams, grep=[synth.NEEDLE], since=since, tail=3) as s:
        ref = s.refs[0]
        assert not any(s.refs[2].m) and sum(ref.m) > 10
        # a window that holds lines of a record whose match lies ahead of it
        g = ref.group(INDENT)
        k = next(i for i in range(720, ref.n_lines) if ref.m[i] and i + 2 < ref.n_lines and g[i + 1] and not ref.m[i + 1] and
                 ref.ts[i + 1] > ref.ts[i])  # (behind the run's since)
        frm, until = ref.ts[k + 1], (ref.ts[k + 1][0] + 400, 0)
        assert not (tuple(frm) <= tuple(ref.ts[k]) < tuple(until)) and ref.cut(INDENT, frm, until)[k + 1]
        matched_inside = [r.cut(opts(), frm, until) for r in s.refs]
        assert sum(map(sum, matched_inside)) < s.sizes(INDENT, frm, until)[0] < s.sizes(INDENT)[0]
        s.records(INDENT, frm, until)        # the match outside lends its record's lines inside
        s.records(INDENT, frm, OPEN_HI, tail=4)
        s.records(inv(INDENT), OPEN_LO, until, tail=4)
        s.records(INDENT, until, frm)        # from > until: empty
        r = s.records(INDENT, frm, until, tail=2)
        # the analyses of the new result work on G''
        g2 = s.flags(INDENT, frm, until)
        total = sum(map(sum, g2))
        counts, outside = r.histogram((synth.T0, 0), 60 * 10**9, 64)
        assert int(counts.sum()) + int(outside.sum()) == total
        with r.groups(4) as gr:
            assert gr.n_lines == total
        rows, _ = r.field_stats(b"lat")
        assert int(rows[-1]["lines"]) == total
        e = [rf.emitted(gi, 2, since) for rf, gi in zip(s.refs, g2)]
        want_ent, want_bytes = merged(s.refs, e, None, True)
        tl = r.timeline(timestamps=True)
        try:
            assert [tuple(int(x) for x in row) for row in tl.entries.tolist()] == want_ent and tl.bytes == want_bytes
            assert len(want_ent) >= 2
        finally:
            tl.free()
        stale = s.r
        s.r = s.r.retail(-1)                 # re-tails over G''
        s.check_flags(s.r, g2, -1, "retail")
        assert s.r.records_info()[:2] == (0, 0)
        for touch in (lambda: stale.records(indent=True), lambda: stale.stream(0), lambda: stale.retail(1)):
            with pytest.raises(E.KlfError) as ei:
                touch()
            assert ei.value.code == E.KLF_ESTATE
        stale.free()
        s.records(INDENT)
        s.records(opts(cont=[b"\tat frame 1"]))  # a second call does not compound: from M again
        assert s.sizes(opts(cont=[b"\tat frame 1"]))[0] < s.sizes(INDENT)[0]
        old, s.r = s.r, s.r.regroup(1, 1, False, -1)  # records -> regroup: from M
        old.free()
        s.check_flags(s.r, [rf.group(1, 1) for rf in s.refs], -1, "regroup")
        s.records(INDENT, tail=1)
        old, s.r = s.r, s.r.window((synth.T0 + 900, 0), None)  # records -> window: from M
        old.free()
        s.check_flags(s.r, [rf.cut((synth.T0 + 900, 0), OPEN_HI) for rf in s.refs], -1, "window")
        s.records(INDENT)
        old, s.r = s.r, s.r.around(0, 0)     # records -> around: from M (equal instants: the blocks share their line's)
        old.free()
        assert all(s.r.match_bits(i) == s.mbits[i] for i in range(3)) and s.r.around_counts()[0] == s.sizes(INDENT)[1]
        s.records(inv(INDENT))
        s.records(opts())                    # no flags, no prefixes: klf_retail over M
        old, s.r = s.r, s.eng.run(since=since, tail=3, n_streams=len(streams))  # the next run is untouched
        old.free()
        for i, data in enumerate(streams):
            out, lo, bits, cn = co.filter_stream(data, since, 3, [synth.NEEDLE])
            so = s.r.stream(i)
            assert so.out == out and so.counts["matched"] == cn["matched"]
            assert s.r.match_bits(i) == bits == s.r.group_bits(i)
        assert s.r.records_info() == (0, 0, 0.0)


# ------------------------------------------------------------------------------ 9. errors ---

def _raw_records(eng, r, o, tail=-1):
    out = E.C.c_void_p()
    rc = E.lib().klf_records(eng._h, r._p, E.C.byref(o) if o is not None else None, tail, E.C.byref(out))
    assert not out.value or rc == E.KLF_OK
    return rc


def test_errors(gpu):
    from test_records_ref import BAD_OPTS
    data = synth.generate(synth.JSON, 51, 0, 60_000, permille=50)
    for grep in ((), (synth.NEEDLE,)):
        with E.Engine(0, grep=grep) as eng:
            eng.set_streams(1)
            eng.stage(0, data)
            r = eng.run(tail=-1, n_streams=1)
            for name, kw in BAD_OPTS.items():
                o, keep = raw_opts(**kw)
                assert _raw_records(eng, r, o) == E.KLF_EINVAL, name
                assert b"klf_records" in E.lib().klf_last_error(eng._h), name
            good, keep = raw_opts()
            assert _raw_records(eng, r, None) == E.KLF_EINVAL
            assert _raw_records(eng, r, good, tail=-2) == E.KLF_EINVAL
            assert E.lib().klf_records(eng._h, r._p, E.C.byref(good), -1, None) == E.KLF_EINVAL
            assert E.lib().klf_records(eng._h, None, E.C.byref(good), -1, E.C.byref(E.C.c_void_p())) == E.KLF_EINVAL
            if not grep:  # records of what?
                assert _raw_records(eng, r, good) == E.KLF_EINVAL
                assert b"no patterns" in E.lib().klf_last_error(eng._h)
                with pytest.raises(E.KlfError) as ei:
                    r.records(indent=True)
                assert ei.value.code == E.KLF_EINVAL
                assert r.stream(0).out == po.filter_stream(data, GZ, -1, ()).out  # the engine still serves its run
                r.free()
                continue
            # no device work before the argument checks: prev is still the latest and untouched
            assert r.stream(0).out == po.filter_stream(data, GZ, -1, po.compile_patterns(grep)).out
            r2 = r.records(head=[b"no line starts like this"])  # one record: the whole stream
            assert r2.stream(0).counts["matched"] == r2.stream(0).counts["parsed"]
            with pytest.raises(E.KlfError) as ei:  # r is not the latest any more
                r.records(indent=True)
            assert ei.value.code == E.KLF_ESTATE
            r.free()
            r2.free()
            r3 = eng.run(tail=2, n_streams=1)  # after the errors the engine still runs
            assert r3.stream(0).out == po.filter_stream(data, GZ, 2, po.compile_patterns(grep)).out
            r3.free()


# --------------------------------------------------------------------------------- 10. CLI ---

def test_cli_record_flags(gpu, tmp_path):
    bodies = []
    for p in range(2):
        for cname in ("app", "sidecar"):
            data = _indented(synth.generate(synth.JSON if cname == "app" else synth.TEXT, 61 + p, p * 2 + len(cname),
                                            60_000 + 3000 * p, permille=60, drop_final_nl=(cname == "sidecar")), 8 + p)
            f = tmp_path / f"body_{p}_{cname}.log"
            f.write_bytes(data)
            bodies.append((f"pod-{p}", cname, data, str(f)))
    m = tmp_path / "manifest.tsv"
    m.write_text("".join("\t".join((p, "container", c, f)) + "\n" for p, c, _, f in bodies))
    now = synth.T0 + synth.SPAN + 1
    tailv = ["--now", str(now), "--no-color", str(m)]
    grep = ["--grep", synth.NEEDLE.decode()]
    refs = [RecordsRef(data, grep=[synth.NEEDLE]) for _, _, data, _ in bodies]
    until = po.parse_line(b"2024-10-22T00:40:00.5Z x")[0]
    since, tail5, rej = H.lop_opts("40m", 5, (now, 0))
    assert not rej and tail5 == 5
    cases = {
        "indent": (["--record-indent"], INDENT, OPEN_LO, OPEN_HI, -1, GZ),
        "blank_cont": (["--record-blank", "--record-cont", "\tat", "--record-cont", "  caused by", "-t", "3"],
                       opts(blank=True, cont=[b"\tat", b"  caused by"]), OPEN_LO, OPEN_HI, 3, GZ),
        "head": (["--record-head", "{", "--record-head", "I", "--record-head", "E", "--record-head", "W", "-s", "40m", "-t", "5"],
                 opts(head=[b"{", b"I", b"E", b"W"]), OPEN_LO, OPEN_HI, 5, since),
        "invert_cut": (["--record-indent", "--record-invert", "--until", "2024-10-22T00:40:00.5Z"], inv(INDENT), OPEN_LO, until, -1, GZ),
    }
    for name, (flags, o, frm, unt, tail, snc) in cases.items():
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / name)] + grep + flags + tailv, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        g = [ref.cut(o, frm, unt) for ref in refs]
        assert sum(map(sum, g)) > 0 and sum(map(sum, g)) != sum(sum(ref.m) for ref in refs)
        assert sorted(os.listdir(tmp_path / name)) == sorted(H.log_file_name(p, c) for p, c, _, _ in bodies)
        for (p, c, _, _), ref, gi in zip(bodies, refs, g):
            assert (tmp_path / name / H.log_file_name(p, c)).read_bytes() == ref.emit(gi, tail, snc)[0], (name, p, c)
    # usage errors exit as the --around ones do
    for flags in (["--record-indent"],                                       # no --grep / --match
                  grep + ["--record-indent", "-C", "2"], grep + ["--record-indent", "-A", "1"],
                  grep + ["--record-blank", "-B", "1"], grep + ["--record-cont", "x", "--invert-match"],
                  grep + ["--record-indent", "--around", "1s"], grep + ["--record-invert", "--around-before", "1s"],
                  grep + ["--record-head", "x", "--around-after", "1s"],
                  grep + ["--record-head", "x", "--record-cont", "y"], grep + ["--record-head", "x", "--record-indent"],
                  grep + ["--record-head", "x", "--record-blank"], grep + ["--record-cont", ""],
                  grep + ["--record-cont", "x" * 33], grep + ["--record-cont", "x"] * 9):
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / "none")] + flags + tailv, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 1 and "usage:" in r.stderr, flags
