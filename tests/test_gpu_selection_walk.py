"""The three consumers of the selected-line walk (klf_analysis.hip walk_publish / walk_rounds:
k_tw_build, k_hist, k_tl_keys) held against each other on one batch: the window's selection, the
histogram's table and the timeline's entries of the same result must describe the same lines, so
a divergence of one of them fails here even where each still matches its own reference case."""
import random
import time

import pytest

from klogs_amd import engine as E
from test_hist_ref import NS, HistRef, shift

pytestmark = pytest.mark.gpu

# Six streams, in two orders.  "word 0": three streams share bitmap word 0 and a fourth starts in
# it.  "chunk edge": the first stream ends one line past a kMatchChunk (8,192 lines) edge, and the
# three short streams share the word behind it.  8,301 lines: no multiple of 32.
ORDERS = {"word 0": (3, 1, 1, 40, 8193, 63), "chunk edge": (8193, 3, 1, 1, 40, 63)}
N_BUCKETS = 61
T_LO, T_HI = 946684800, 3786912000  # 2000-01-01 .. 2090-01-01: the canonical lines' instants

# global line index -> a valid prefix off the canonical shape, or no prefix at all
SPECIAL = {
    1: b"2031-05-06T07:08:09.123456789+02:00 offset zone HIT\n",
    2: b"no timestamp at all HIT\n",
    20: b"2044-01-02T03:04:05.5Z one fraction digit\n",
    47: b"2150-01-01T00:00:00.000000001Z a year past 2099 HIT\n",
    4000: b"2050-06-07T08:09:10Z no fraction HIT\n",
    8192: b"1969-12-31T23:59:59.999999999Z a year before 1970\n",
    8193: b"2061-02-03T04:05:06.1234-07:30 offset zone, four fraction digits HIT\n",
    8199: b"neither here\n",
    8300: b"2077-08-09T10:11:12.000000000+00:00 a zero offset spelled out HIT\n",
}
UNPARSABLE = (2, 8199)


def _streams(order):
    """Canonical lines with instants drawn from a fixed seed (shuffled across and inside the
    streams), about one in three holding the literal, and the lines of SPECIAL."""
    rng = random.Random(5)
    out, g = [], 0
    for n in ORDERS[order]:
        lines = []
        for _ in range(n):
            sec, nsec, hit = rng.randrange(T_LO, T_HI), rng.randrange(NS), rng.random() < 1 / 3
            line = b"%s.%09dZ %s %d\n" % (time.strftime("%Y-%m-%dT%H:%M:%S", time.gmtime(sec)).encode(), nsec,
                                          b"HIT" if hit else b"line", g)
            lines.append(SPECIAL.get(g, line))
            g += 1
        out.append(b"".join(lines))
    return out


def _popcount(bits: bytes) -> int:
    return sum(bin(b).count("1") for b in bits)


def _set_lines(bits: bytes):
    return [8 * i + k for i, b in enumerate(bits) for k in range(8) if b >> k & 1]


def _timeline(r):
    tl = r.timeline(tags=[b"%d " % i for i in range(r.n_streams)])
    try:
        return [(int(s), int(ns), int(st), int(ln)) for s, ns, st, ln, _ in tl.entries.tolist()]
    finally:
        tl.free()


def _table(r, origin, width):
    counts, outside = r.histogram(origin, width, N_BUCKETS)
    return [[int(x) for x in row] for row in counts.tolist()], [[int(x) for x in row] for row in outside.tolist()]


@pytest.mark.parametrize("grep", [(), (b"HIT",)], ids=["no patterns", "one literal"])
@pytest.mark.parametrize("order", list(ORDERS))
def test_window_histogram_and_timeline_agree(gpu, order, grep):
    streams = _streams(order)
    n = len(streams)
    refs = [HistRef(s, grep) for s in streams]
    assert [r.n_lines for r in refs] == list(ORDERS[order]) and sum(ORDERS[order]) == 8301
    flat = [t for r in refs for t in r.ts]
    assert [i for i, t in enumerate(flat) if t is None] == list(UNPARSABLE)
    sel = [r.gprime() for r in refs]  # M, or without patterns the parsed lines
    want = [sum(g) for g in sel]
    if grep:  # about one line in three: a wave's 2,048 lines take a partial round at the least
        assert 2500 < sum(want) < 3100
    else:     # every parsed line: 32 rounds a wave
        assert sum(want) == 8301 - len(UNPARSABLE)
    inst = [t for t in flat if t is not None]
    origin, end = min(inst), shift(max(inst), 1)  # [origin, end) holds every instant
    assert origin[0] < 0 and end[0] > 5_600_000_000  # 1969 and 2150
    width = -(-((end[0] - origin[0]) * NS + end[1] - origin[1]) // N_BUCKETS)

    with E.Engine(0, grep=grep) as eng:
        eng.set_streams(n)
        for i, s in enumerate(streams):
            eng.stage(i, s)
        r = eng.run(since=None, tail=-1, n_streams=n)
        w = h = None
        try:
            table, outside = _table(r, origin, width)
            ent = _timeline(r)
            w = r.window(origin, end)  # (r is stale from here on)
            wbits = [w.group_bits(i) for i in range(n)]

            # per-stream line counts: the three, and the oracle's
            got_w = [_popcount(b) for b in wbits]
            got_h = [sum(row) + sum(out) for row, out in zip(table, outside)]
            got_t = [sum(1 for e in ent if e[2] == i) for i in range(n)]
            assert got_w == got_h == got_t == want, (got_w, got_h, got_t, want)
            assert got_w == [w.stream_counts(i)["selected"] for i in range(n)]
            # the timeline's entries, bucketed here, are the histogram's table
            mine = [[0] * N_BUCKETS for _ in range(n)]
            for sec, nsec, st, _ in ent:
                mine[st][((sec - origin[0]) * NS + nsec - origin[1]) // width] += 1
            assert mine == table and outside == [[0, 0]] * n
            assert table == [ref.hist(g, origin, width, N_BUCKETS)[0] for ref, g in zip(refs, sel)]
            assert sum(1 for k in range(N_BUCKETS) if any(row[k] for row in table)) > 20
            # its (stream, line) set is the window's selection, which is the oracle's
            assert sorted((st, ln) for _, _, st, ln in ent) == [(i, l) for i in range(n) for l in _set_lines(wbits[i])]
            assert wbits == [ref.pack(g) for ref, g in zip(refs, sel)]
            assert [(sec, nsec) for sec, nsec, _, _ in ent] == sorted(refs[st].ts[ln] for _, _, st, ln in ent)
            # the same two over the window's own bitmap
            assert _table(w, origin, width) == (table, outside) and _timeline(w) == ent

            if grep:  # the inverted selection through the regroup kernels, then the walk
                h = w.regroup(invert=True)
                inv, out = _table(h, origin, width)
                assert [sum(row) for row in inv] == [ref.n_parsed - sum(ref.m) for ref in refs]
                assert inv == [ref.hist(ref.group(0, 0, True), origin, width, N_BUCKETS)[0] for ref in refs]
                assert out == [[0, 0]] * n
        finally:
            for x in (h, w, r):
                if x is not None:
                    x.free()
