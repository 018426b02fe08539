"""klf_around on the GPU (SPEC.md S4g): time context across streams over a finished run, against
the reference of tests/test_around_ref.py.  Each case is one engine run and then many calls;
every call is compared in full and exactly, per stream: the output bytes, matched / selected /
out_bytes, the unchanged lines / parsed / since_ok, group_bits, and match_bits still M."""
import datetime
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
from test_around_ref import MAX_NS, AroundRef, ns_of
from test_gpu_regroup import CARRY_HITS, CARRY_N, PATTERN_SETS, _tiny_streams
from test_gpu_window import SMALL, SMALL_MID
from test_hist_ref import HistRef
from test_timeline_ref import TimelineRef, merged
from test_window_ref import OPEN_HI, OPEN_LO

pytestmark = pytest.mark.gpu

GZ = po.GO_ZERO_TIME
COUNT_KEYS = ("lines", "parsed", "since_ok")
NS = 10**9
MS = 10**6
AR_BLOCK = 2048  # anchors per block of the interval merge (klf_analysis.hpp kArBlock) and of a radix pass (kTlSortBlock)


def opt(t):
    """A reference bound as Result.around takes it (None = open)."""
    return None if t in (OPEN_LO, OPEN_HI) else t


def stamp(t_ns):
    """The canonical prefix of the instant t_ns (nanoseconds since the epoch, any year 1..9999)."""
    sec, nsec = divmod(t_ns, NS)
    d = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=sec)
    return b"%04d-%02d-%02dT%02d:%02d:%02d.%09dZ " % (d.year, d.month, d.day, d.hour, d.minute, d.second, nsec)


T0 = synth.T0 * NS  # 2024-10-22T00:00:00Z


class Session:
    """One engine run over `streams`; every around is checked in full against the reference."""

    def __init__(self, streams, grep=(), match=(), since=None, tail=-1, refs=None, run=None):
        self.streams = streams
        self.since = since
        self.refs = refs if refs is not None else [TimelineRef(s, grep, match) for s in streams]
        self.ar = AroundRef(streams, refs=self.refs)
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

    def flags(self, before, after, frm=OPEN_LO, until=OPEN_HI):
        return self.ar.cut(before, after, frm, until)

    def sizes(self, before, after, frm=OPEN_LO, until=OPEN_HI):
        """(|G''|, |M|, parsed lines) over all streams, by the reference."""
        return (sum(map(sum, self.flags(before, after, frm, until))), sum(sum(r.m) for r in self.refs),
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

    def around(self, before=0, after=0, frm=OPEN_LO, until=OPEN_HI, tail=-1):
        old, self.r = self.r, self.r.around(before, after, opt(frm), opt(until), tail)
        old.free()
        self.check_flags(self.r, self.flags(before, after, frm, until), tail, ("around", before, after, frm, until))
        n, k = self.r.around_counts()
        assert n == len(self.ar.anchors()) and (1 <= k <= n if n else k == 0), (n, k)
        return self.r

    def close(self):
        self.r.free()
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def intervals(anchors, before, after):
    """K by the definition: an anchor opens an interval iff its gap to the one ahead exceeds the span."""
    return sum(1 for i, a in enumerate(anchors) if i == 0 or a - anchors[i - 1] > before + after)


# ------------------------------------------------------------------ 1. adversarial prefixes ---

DURATIONS = (0, 1, 999_999_999, NS, NS + 1, 40 * 60 * NS, MAX_NS)


@pytest.mark.parametrize("since", [None, SMALL_MID])
def test_adversarial_prefixes(gpu, since):
    streams = [b"".join(SMALL[k::3]) for k in range(3)]  # (the fragment ends stream 1)
    with Session(streams, grep=[b"HIT"], since=since) as s:
        assert sum(r.n_lines for r in s.refs) == 20 and sum(r.n_parsed for r in s.refs) == 17
        assert len(s.ar.anchors()) == 9 and s.ar.anchors()[0] < -62 * 10**18  # year 0000: below -2^63 ns
        seen = set()
        for before in DURATIONS:
            for after in DURATIONS:
                for tail in (-1, 0, 1, 7):
                    s.around(before, after, tail=tail)
                seen.add(s.sizes(before, after)[0])
        assert min(seen) == s.sizes(0, 0)[0] < max(seen) == 17 and len(seen) >= 4  # from the equal instants to all


# ---------------------------------------------------------------------- 2. edge exactness ---

@pytest.mark.parametrize("before,after", [(700 * MS, 800 * MS), (NS + 700 * MS, 59 * NS + 800 * MS), (300 * MS, 699_999_999),
                                          (0, 0), (1, 1)])
def test_edge_exactness(gpu, before, after):
    """One anchor at .3 s: a - before borrows from the second (.3 < .7) and a + after carries
    into the next (.3 + .8); the 300 ms / 699 999 999 ns pair does neither (ends .0 and
    .999999999)."""
    a = T0 + 300 * MS
    one = stamp(a) + b"HIT the anchor\n"
    other = b"".join(stamp(t) + b"%d\n" % k for k, t in enumerate((a + after, a + after + 1, a - before, a - before - 1)))
    with Session([one, other], grep=[b"HIT"]) as s:
        assert s.flags(before, after) == [[True], [True, False, True, False]]
        for tail in (-1, 1):
            s.around(before, after, tail=tail)
        assert s.r.around_counts() == (1, 1)


# ---------------------------------------------------------------------- 3. equal instants ---

def test_equal_instants(gpu):
    a = T0 + 5 * NS + 123_456_789
    s0 = stamp(a - 7) + b"quiet\n" + stamp(a) + b"HIT\n" + stamp(a + 7) + b"quiet\n"
    s1 = stamp(a + 1) + b"one ns behind\n" + stamp(a) + b"same instant, no match\n" + stamp(a - 1) + b"one ns ahead\n" + \
        b"2024-10-22T01:00:05.123456789+01:00 same instant, with a zone\n"
    with Session([s0, s1], grep=[b"HIT"]) as s:
        assert s.flags(0, 0) == [[False, True, False], [False, True, False, True]]
        s.around(0, 0)
        assert s.r.stream(1).out == b"same instant, no match\nsame instant, with a zone\n"
        s.around(0, 0, tail=1)


# ---------------------------------------------------------------------- 4. interval merge ---

def test_interval_merge_gaps(gpu):
    """before + after = 500 ns.  Anchors exactly 500 ns apart share an end point and merge; 501
    ns apart their intervals are neighbours without an instant between them and do not merge;
    502 ns apart they leave a hole of one instant, and a line there is out."""
    before, after = 300, 200
    base = [T0 + k * NS for k in range(3)]
    gaps = (500, 501, 502)
    anchors = sorted(b + d for b, g in zip(base, gaps) for d in (0, g))
    s0 = b"".join(stamp(t) + b"HIT %d\n" % k for k, t in enumerate(anchors))
    probes = []
    for b, g in zip(base, gaps):
        probes += [b - before - 1, b - before, b + after, b + after + 1, b + g - before - 1, b + g - before,
                   b + g + after, b + g + after + 1]
    s1 = b"".join(stamp(t) + b"probe %d\n" % k for k, t in enumerate(probes))
    with Session([s0, s1], grep=[b"HIT"]) as s:
        g = s.flags(before, after)[1]
        assert g[0:8] == [False, True, True, True, True, True, True, False]     # 500: one interval
        assert g[8:16] == [False, True, True, True, True, True, True, False]    # 501: neighbours, every instant covered
        assert g[16:24] == [False, True, True, False, False, True, True, False]  # 502: b + 201 is the hole
        assert probes[19] == probes[20] == base[2] + 201
        s.around(before, after)
        assert s.r.around_counts() == (6, 5) == (6, intervals(s.ar.anchors(), before, after))
        s.around(before, after + 1)
        assert s.r.around_counts() == (6, 4)
        s.around(before + 1, after + 1, tail=3)
        assert s.r.around_counts() == (6, 3)


def _seam_streams(n):
    """n anchors, one per second from T0 on, in a fixed shuffled order, with a few more streams'
    lines around the first, the block-seam and the last anchors: 100 ms behind one and 1 ns
    further, the same ahead of one, and in the middle between two."""
    secs = list(range(n))
    random.Random(n).shuffle(secs)
    s0 = b"".join(stamp(T0 + x * NS) + b"HIT %d\n" % i for i, x in enumerate(secs))
    marks = sorted({k for k in (0, 1, AR_BLOCK - 2, AR_BLOCK - 1, AR_BLOCK, AR_BLOCK + 1, 2 * AR_BLOCK - 1, 2 * AR_BLOCK,
                                n - 2, n - 1, n) if k >= 0})
    probes = []
    for k in marks:
        t = T0 + k * NS
        probes += [t + 100 * MS, t + 100 * MS + 1, t - 100 * MS, t - 100 * MS - 1, t + 500 * MS]
    random.Random(n + 1).shuffle(probes)
    s1 = b"".join(stamp(t) + b"probe %d\n" % i for i, t in enumerate(probes[0::2]))
    s2 = b"".join(stamp(t) + b"probe %d\n" % i for i, t in enumerate(probes[1::2]))
    return [s0, s1, s2]


# 5. sort sizes (the radix passes' block seams) and 4.'s head-block seams, one run per size
@pytest.mark.parametrize("n", [0, 1, AR_BLOCK - 1, AR_BLOCK, AR_BLOCK + 1, 2 * AR_BLOCK + 1])
def test_sort_and_head_block_seams(gpu, n):
    with Session(_seam_streams(n), grep=[b"HIT"]) as s:
        assert len(s.ar.anchors()) == n and s.ar.anchors() == sorted(s.ar.anchors())
        s.around(100 * MS, 100 * MS)  # every anchor its own interval
        assert s.r.around_counts() == (n, n)
        if n > 1:
            m, nm, parsed = s.sizes(100 * MS, 100 * MS)
            assert nm < m < parsed
        s.around(400 * MS, 600 * MS)  # gap == span: all anchors in one interval
        assert s.r.around_counts() == (n, min(n, 1))
        s.around(400 * MS, 600 * MS - 1, tail=5)  # one ns less: every anchor its own again
        assert s.r.around_counts() == (n, n)
        s.around(0, 0, tail=1)
        if n == 0:  # no anchor: a valid empty selection
            assert all(s.r.stream(i).out == b"" and s.r.group_bits(i) == bytes(len(s.mbits[i])) for i in range(3))


# -------------------------------------------------------------------------- 6. walk seams ---

@pytest.fixture(scope="module")
def carry_session(gpu):
    big = b"".join(stamp(T0 + i * NS) + (b"HIT %05d padding .....\n" if i in CARRY_HITS else b"line %05d padding ....\n") % i
                   for i in range(CARRY_N))
    second = b"".join(stamp(T0 + i * 8 * NS + 500 * MS) + b"second %d\n" % i for i in range(CARRY_N // 8))
    s = Session([big, second], grep=[b"HIT"])
    assert [i for i, m in enumerate(s.refs[0].m) if m] == list(CARRY_HITS) and not any(s.refs[1].m)
    yield s
    s.close()


@pytest.mark.parametrize("before,after", [(0, 0), (500 * MS, 500 * MS), (31 * NS, 33 * NS), (8191 * NS, 0), (0, 8193 * NS),
                                          (20000 * NS, 20000 * NS)])
def test_word_and_chunk_seams(carry_session, before, after):
    s = carry_session
    s.around(before, after)
    s.around(before, after, tail=7)
    if before + after:
        m, nm, parsed = s.sizes(before, after)
        assert nm < m and sum(s.flags(before, after)[1]) > 0  # the anchor-less stream gets lines
        assert (m == parsed) == (before == 20000 * NS)


def test_stream_boundaries_in_a_word(gpu):
    streams = _tiny_streams()
    with Session(streams, grep=[b"HIT"]) as s:
        assert len(streams) == 300 and sum(r.n_lines for r in s.refs) < 1200
        m, nm, parsed = s.sizes(2 * NS, 2 * NS)
        assert nm < m < parsed
        gained = sum(1 for r, g in zip(s.refs, s.flags(2 * NS, 2 * NS)) if sum(g) > sum(r.m))
        assert gained > 50  # many streams get lines from their neighbours' anchors
        for before, after in ((2 * NS, 2 * NS), (0, 0), (60 * NS, 0), (0, 5 * NS)):
            s.around(before, after)
            s.around(before, after, tail=2)


# ----------------------------------------------------------------- 7. unordered timestamps ---

def test_unordered_timestamps(gpu):
    n = 600
    perm = list(range(n))
    random.Random(7).shuffle(perm)
    down = b"".join(stamp(T0 + (n - 1 - i) * NS) + (b"HIT down %d\n" if i % 97 == 3 else b"down %d\n") % i for i in range(n))
    shuf = b"".join(stamp(T0 + x * NS + 250 * MS) + (b"HIT shuf %d\n" if i % 131 == 5 else b"shuf %d\n") % i
                    for i, x in enumerate(perm))
    up = b"".join(stamp(T0 + i * NS + 750 * MS) + b"up %d\n" % i for i in range(n))
    with Session([down, shuf, up], grep=[b"HIT"]) as s:
        for before, after in ((0, 0), (250 * MS, 0), (0, 750 * MS), (2 * NS, 3 * NS)):
            s.around(before, after)
            s.around(before, after, tail=4)
        m, nm, parsed = s.sizes(2 * NS, 3 * NS)
        assert nm < m < parsed and sum(s.flags(2 * NS, 3 * NS)[2]) > 0


# -------------------------------------- 8. every pattern mode, from a run with a partial index ---

@pytest.mark.parametrize("name", list(PATTERN_SETS))
def test_pattern_modes_from_a_partial_index(gpu, name):
    pats = PATTERN_SETS[name]
    streams = [synth.generate(synth.TEXT, 21, 0, 150_000, permille=20),
               synth.generate(synth.JSON, 22, 1, 120_000, permille=20, drop_final_nl=True),
               synth.generate(synth.ADVERSARIAL, 23, 2, 6000, permille=40, drop_final_nl=True)]
    frm, until = (synth.T0 + 1200, 0), (synth.T0 + 2700, 0)
    with Session(streams, since=(synth.T0 + 900, 0), tail=5, **pats) as s:
        m, nm, parsed = s.sizes(2 * NS, NS)
        if name == "never":
            assert m == nm == 0
        elif name == "all":
            assert m == nm == parsed
        else:
            assert s.r.index_mode() != "full"  # the around builds the rest of the index
            assert nm < m < parsed
        for tail in (-1, 5):
            s.around(2 * NS, NS, tail=tail)
            s.around(2 * NS, NS, frm, until, tail=tail)


# --------------------------------------------------------------------------- 9. output growth ---

def test_output_growth(gpu, monkeypatch):
    monkeypatch.setenv("KLF_DEBUG_OUT_INIT", "4096")
    n = 10_000
    a = b"".join(stamp(T0 + i * NS) + (b"HIT once\n" if i == 1234 else b"line %d of the first stream\n" % i) for i in range(n))
    b = b"".join(stamp(T0 + i * NS + 500 * MS) + b"line %d of the second stream\n" % i for i in range(n))
    with Session([a, b], grep=[b"HIT"]) as s:
        assert [len(s.r.stream(i).out) for i in range(2)] == [len(b"HIT once\n"), 0]
        r = s.around(n * NS, n * NS)
        assert s.sizes(n * NS, n * NS) == (2 * n, 1, 2 * n)
        for i in range(2):
            so = r.stream(i)
            assert so.counts["matched"] == so.counts["parsed"] == so.counts["selected"] == n
            assert len(so.out) > 100_000


# ----------------------------------------------------------------- 10. window cut and state ---

def test_window_cut_and_state(gpu):
    streams = [synth.generate(synth.JSON, 41, 0, 300_000, permille=30),
               synth.generate(synth.ADVERSARIAL, 42, 1, 5000, permille=40, drop_final_nl=True),
               synth.generate(synth.TEXT, 43, 2, 100_000, permille=0)]
    since = (synth.T0 + 600, 0)
    with Session(streams, grep=[synth.NEEDLE], since=since, tail=3) as s:
        anchors = s.ar.anchors()
        assert not any(s.refs[2].m) and len(anchors) > 10
        a = anchors[len(anchors) // 2]
        frm, until = divmod(a + 1, NS), divmod(a + 20 * NS, NS)  # opens 1 ns behind an anchor
        inside = [x for x in anchors if a < x < a + 20 * NS]
        lent = AroundRef(streams, refs=s.refs)
        lent._anchors = inside  # what the anchors inside the window alone would select
        d = 5 * NS
        assert sum(map(sum, lent.cut(d, d, frm, until))) < s.sizes(d, d, frm, until)[0] < s.sizes(d, d)[0]
        s.around(d, d, frm, until)           # closed on both sides: the anchor outside lends context inside
        s.around(d, d, frm, OPEN_HI, tail=4)
        s.around(d, d, OPEN_LO, until, tail=4)
        s.around(d, d, until, frm)           # from > until: empty
        s.around(d, d, frm, until, tail=2)
        stale = s.r
        s.r = s.r.retail(-1)                 # re-tails over G''
        s.check_flags(s.r, s.flags(d, d, frm, until), -1, "retail")
        for touch in (lambda: stale.around(d, d), lambda: stale.stream(0), lambda: stale.retail(1)):
            with pytest.raises(E.KlfError) as ei:
                touch()
            assert ei.value.code == E.KLF_ESTATE
        stale.free()
        s.around(d, 0)
        s.around(0, d)                       # a second around does not compound: from M again
        assert s.sizes(0, d)[0] < s.sizes(d, d)[0]
        old, s.r = s.r, s.r.regroup(1, 1, False, -1)  # around -> regroup: from M
        old.free()
        s.check_flags(s.r, [ref.group(1, 1) for ref in s.refs], -1, "regroup")
        s.around(d, d, tail=1)
        old, s.r = s.r, s.r.window((synth.T0 + 900, 0), None)  # around -> window: from M
        old.free()
        s.check_flags(s.r, [ref.cut((synth.T0 + 900, 0), OPEN_HI) for ref in s.refs], -1, "window")
        s.around(d, d)
        old, s.r = s.r, s.eng.run(since=since, tail=3, n_streams=len(streams))  # the next run is untouched
        old.free()
        for i, data in enumerate(streams):
            out, lo, bits, cn = co.filter_stream(data, since, 3, [synth.NEEDLE])
            so = s.r.stream(i)
            assert so.out == out and so.counts["matched"] == cn["matched"]
            assert s.r.match_bits(i) == bits == s.r.group_bits(i)
        assert s.r.around_counts() == (0, 0)


# ------------------------------------------------------------- 11. analyses on the result ---

def test_timeline_and_histogram_of_the_result(gpu):
    n = 300  # an anchor every second; a stream 50 ms behind each; a stream 400 ms ahead of every third
    streams = [b"".join(stamp(T0 + k * NS) + b"HIT %d\n" % k for k in range(n)),
               b"".join(stamp(T0 + k * NS + 50 * MS) + b"behind %d\n" % k for k in range(n)),
               b"".join(stamp(T0 + 3 * k * NS + 600 * MS) + b"ahead %d\n" % k for k in range(n // 3))]
    with Session(streams, grep=[b"HIT"], since=(synth.T0 + 20, 0)) as s:
        assert [sum(g) for g in s.flags(100 * MS, 100 * MS)] == [n, n, 0]
        assert [sum(g) for g in s.flags(NS, 0)] == [n, n - 1, n // 3]
        frm, until = (synth.T0 + 10, 0), (synth.T0 + 250, 500 * MS)
        for args, tail in (((100 * MS, 100 * MS), -1), ((NS, 0, frm, until), 40)):
            g = s.flags(*args)
            r = s.around(*args, tail=tail)
            e = [ref.emitted(gi, tail, s.since) for ref, gi in zip(s.refs, g)]
            want_ent, want_bytes = merged(s.refs, e, None, True)
            assert len(want_ent) > 20 and len({x[2] for x in want_ent}) >= 2  # entries of several streams
            tl = r.timeline(timestamps=True)
            try:
                assert [tuple(int(x) for x in row) for row in tl.entries.tolist()] == want_ent
                assert tl.bytes == want_bytes
            finally:
                tl.free()
            origin, w, n = (synth.T0 - 5, 0), 7 * NS + 1, 50
            counts, outside = r.histogram(origin, w, n)
            for i, ref in enumerate(s.refs):
                b, lo, hi = HistRef.hist(ref, g[i], origin, w, n)
                assert counts[i].tolist() == b and (int(outside[i, 0]), int(outside[i, 1])) == (lo, hi), i
                assert lo + sum(b) + hi == sum(g[i]) == r.stream_counts(i)["matched"]


# ------------------------------------------------------------------------------- 12. seams ---

@pytest.mark.parametrize("name,buf", [("A", None), ("B", b"0")])
def test_stream_cut_inside_a_prefix(gpu, name, buf):
    """tests/seams.py: streams that end inside a timestamp prefix with the rest right behind them
    (layout A: the next stream's first bytes; layout B: the pad, here overwritten with '0'),
    through run_device.  k_ar_keys and k_ar_build read 32 bytes at each line start: what lies
    past a stream's end must not decide."""
    import torch
    from test_gpu_seams import LAYOUTS, SETS, window_refs
    lay = LAYOUTS[name]
    grep, match = SETS["needle"]
    refs = window_refs(name, "needle")
    assert sum(1 for x in lay.seams if x.cls == "prefix_cut" and 0 < x.k < 31) > 3  # streams ending inside a prefix
    raw = lay.buf if buf is None else lay.filled(buf)
    d = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to("cuda")
    torch.cuda.synchronize()
    with Session(lay.streams(), grep=grep, match=match, refs=refs,
                 run=lambda eng: eng.run_device(d.data_ptr(), lay.bases, lay.lens)) as s:
        m, nm, parsed = s.sizes(2 * NS, 2 * NS)
        assert 0 < nm < m < parsed
        assert any(r.n_parsed < r.n_lines for r in refs)  # cut prefixes: unparseable last lines
        s.around(2 * NS, 2 * NS)
        s.around(0, 0, tail=3)
        s.around(60 * NS, 60 * NS, tail=9)
        cut = (300 * NS, 200 * NS, lay.frm, lay.until)  # the anchors behind `until` lend context inside
        assert 0 < s.sizes(*cut)[0] < s.sizes(*cut[:2])[0]
        s.around(*cut)
        s.around(MAX_NS, MAX_NS)
    del d


# ------------------------------------------------------------------------------ 13. errors ---

def _opts(before=0, after=0, frm=OPEN_LO, until=OPEN_HI, flags=0, reserved=0, from_res=0, until_res=0):
    o = E._AroundOpts()
    o.from_.sec, o.from_.nsec, o.from_._reserved = frm[0], frm[1], from_res
    o.until.sec, o.until.nsec, o.until._reserved = until[0], until[1], until_res
    o.before_ns, o.after_ns, o.flags, o._reserved = before, after, flags, reserved
    return o


def _raw_around(eng, r, opts, tail=-1):
    out = E.C.c_void_p()
    rc = E.lib().klf_around(eng._h, r._p, E.C.byref(opts) if opts is not None else None, tail, E.C.byref(out))
    assert not out.value or rc == E.KLF_OK
    return rc


def test_errors(gpu):
    data = synth.generate(synth.JSON, 51, 0, 60_000, permille=50)
    t = (synth.T0 + 1500, 0)
    bad = [_opts(flags=1), _opts(flags=0x80000000), _opts(reserved=7), _opts(from_res=1), _opts(until_res=1),
           _opts(frm=(t[0], -1)), _opts(frm=(t[0], NS)), _opts(until=(t[0], -1)), _opts(until=(t[0], NS)),
           _opts(before=MAX_NS + 1), _opts(after=MAX_NS + 1), _opts(before=(1 << 64) - 1)]
    for grep in ((), (synth.NEEDLE,)):
        with E.Engine(0, grep=grep) as eng:
            eng.set_streams(1)
            eng.stage(0, data)
            r = eng.run(tail=-1, n_streams=1)
            for o in bad:
                assert _raw_around(eng, r, o) == E.KLF_EINVAL
                assert b"klf_around" in E.lib().klf_last_error(eng._h)
            assert _raw_around(eng, r, None) == E.KLF_EINVAL
            assert _raw_around(eng, r, _opts(), tail=-2) == E.KLF_EINVAL
            assert E.lib().klf_around(eng._h, r._p, E.C.byref(_opts()), -1, None) == E.KLF_EINVAL
            assert E.lib().klf_around(eng._h, None, E.C.byref(_opts()), -1, E.C.byref(E.C.c_void_p())) == E.KLF_EINVAL
            if not grep:  # anchors need a pattern
                assert _raw_around(eng, r, _opts(NS, NS)) == E.KLF_EINVAL
                assert b"no patterns" in E.lib().klf_last_error(eng._h)
                with pytest.raises(E.KlfError) as ei:
                    r.around(NS, NS)
                assert ei.value.code == E.KLF_EINVAL
                r.free()
                continue
            # no device work before the argument checks: prev is still the latest and untouched
            assert r.stream(0).out == po.filter_stream(data, GZ, -1, po.compile_patterns(grep)).out
            r2 = r.around(MAX_NS, MAX_NS)  # (the maximum is legal)
            assert r2.stream(0).counts["matched"] == r2.stream(0).counts["parsed"]
            with pytest.raises(E.KlfError) as ei:  # r is not the latest any more
                r.around(NS, NS)
            assert ei.value.code == E.KLF_ESTATE
            r.free()
            r2.free()


# --------------------------------------------------------------------------------- 14. CLI ---

def test_cli_around_flags(gpu, tmp_path):
    api = b"".join(stamp(T0 + i * NS + 40 * MS) + (b"ERR_CONN_RESET upstream %d\n" if i in (100, 101, 400) else b"GET /%d 200\n") % i
                   for i in range(600))
    sidecar = b"".join(stamp(T0 + i * NS) + (b"restarting %d\n" if i % 100 == 0 else b"tick %d\n") % i for i in range(600))
    db = b"".join(stamp(T0 + i * 7 * NS + 600 * MS) + b"checkpoint %d\n" % i for i in range(80)) + b"half a line"
    bodies = [("pod-0", "api", api), ("pod-0", "sidecar", sidecar), ("pod-1", "db", db)]
    rows = []
    for pod, cname, data in bodies:
        f = tmp_path / f"body_{pod}_{cname}.log"
        f.write_bytes(data)
        rows.append((pod, "container", cname, str(f)))
    m = tmp_path / "manifest.tsv"
    m.write_text("".join("\t".join(r) + "\n" for r in rows))
    now = synth.T0 + 3600
    tailv = ["--now", str(now), "--no-color", str(m)]
    grep = ["--grep", "ERR_CONN_RESET"]
    refs = [TimelineRef(data, grep=[b"ERR_CONN_RESET"]) for _, _, data in bodies]
    ar = AroundRef(None, refs=refs)
    tags = [f"{p}/{c} ".encode() for p, c, _ in bodies]
    until = po.parse_line(b"2024-10-22T00:06:40.5Z x")[0]
    cases = {
        "both": (["--around", "500ms", "--merge"], (500 * MS, 500 * MS), -1),
        "sides": (["--around", "500ms", "--around-before", "2s", "--around-after", "0", "--merge", "-t", "3"], (2 * NS, 0), 3),
        "cut": (["--around-after", "6s", "--until", "2024-10-22T00:06:40.5Z", "--merge"], (0, 6 * NS, OPEN_LO, until), -1),
    }
    for name, (flags, args, tail) in cases.items():
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / name)] + grep + flags + tailv, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        g = ar.cut(*args)
        assert sum(map(sum, g)) > sum(sum(ref.m) for ref in refs) and sum(g[1]) > 0 and sum(g[2]) > 0
        for (p, c, _), ref, gi in zip(bodies, refs, g):
            assert (tmp_path / name / H.log_file_name(p, c)).read_bytes() == ref.emit(gi, tail, GZ)[0], (name, p, c)
        e = [ref.emitted(gi, tail, GZ) for ref, gi in zip(refs, g)]
        assert (tmp_path / name / "merged.log").read_bytes() == merged(refs, e, tags)[1], name
    assert b"pod-0/sidecar restarting 100\npod-0/api ERR_CONN_RESET upstream 100\n" in (tmp_path / "both" / "merged.log").read_bytes()
    # usage errors exit as the --from ones do
    for flags in (["--around", "500ms"],                                  # no --grep / --match
                  grep + ["--around", "-1s"], grep + ["--around", "soon"], grep + ["--around-before", "-1ns"],
                  grep + ["--around-after", "9223372036854775807ns"],    # above 2^62 - 1
                  grep + ["--around", "1s", "-C", "2"], grep + ["--around", "1s", "-A", "1"],
                  grep + ["--around", "1s", "-B", "1"], grep + ["--around-after", "1s", "--invert-match"]):
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / "none")] + flags + tailv, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 1 and "usage:" in r.stderr, flags
        assert not (tmp_path / "none").exists()
