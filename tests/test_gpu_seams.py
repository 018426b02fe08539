"""Input stream seams on the GPU: results must not depend on the bytes behind a stream.

tests/seams.py cuts one text T into streams that end inside a timestamp prefix, a needle, a
regex match, a long line, right before a newline; the completion sits right behind each end
(layout A: it is the next stream's first bytes; layout B: it is the stale pad up to the next
256-byte base), and tests/test_seams_ref.py shows on the host that reading it changes the
answer.  Here the buffer is uploaded as it is and run with klf_run_device, and every stream
is compared exactly with the oracle of its own bytes T[base:base+len]: output, line
offsets, match bits, every count.  The C oracle for literals and no patterns, the Python
oracle for sets with a regex; each expectation is computed once (seams.expected)."""
import numpy as np
import pytest

import klf_oracle as po
import seams
from klogs_amd import engine as E
from test_window_ref import WindowRef

pytestmark = pytest.mark.gpu

S = seams.build()
LAYOUTS = {"A": S.A, "B": S.B}
SETS = seams.pattern_sets()
GZ = po.GO_ZERO_TIME
BOTH = pytest.mark.parametrize("name", ["A", "B"])


@pytest.fixture(scope="module")
def dev(gpu):
    """The two layouts' buffers in HBM, plus layout B with its pads and slack overwritten."""
    import torch
    bufs = {"A": S.A.buf, "B": S.B.buf, "B\\n": S.B.filled(b"\n"), "B0": S.B.filled(b"0"), "B ": S.B.filled(b" ")}
    out = {k: torch.from_numpy(np.frombuffer(v, dtype=np.uint8).copy()).to("cuda") for k, v in bufs.items()}
    torch.cuda.synchronize()
    yield out


def compare(r, name, sname, since, tail, want=None):
    """Result r, stream by stream, against the oracle of layout `name`'s own streams."""
    want = want if want is not None else seams.expected(name, sname, since, tail)
    patterned = any(SETS[sname])
    for i, w in enumerate(want):
        tag = (name, sname, since, tail, i)
        so = r.stream(i)
        assert so.out == w["out"], tag
        assert r.lines(i).tolist() == w["lines"], tag
        if patterned:
            assert r.match_bits(i) == w["bits"], tag
        assert so.counts == w["counts"], tag


def run_check(dev, name, sname, since=None, tail=-1, buf=None):
    lay = LAYOUTS[name]
    grep, match = SETS[sname]
    with E.Engine(0, grep=grep, match=match) as eng:
        r = eng.run_device(dev[buf or name].data_ptr(), lay.bases, lay.lens, since=since, tail=tail)
        try:
            compare(r, name, sname, since, tail)
        finally:
            r.free()


# ---- no patterns ------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("since,tail", [(None, -1), ("mid", -1), (None, 1), (None, 3), ("mid", 100)])
def test_no_patterns(dev, name, since, tail):
    run_check(dev, name, "none", LAYOUTS[name].mid if since else None, tail)


@BOTH
def test_no_patterns_short_fuse_ranges(dev, monkeypatch, name):
    monkeypatch.setenv("KLF_DEBUG_FUSE_RANGE", "8")
    run_check(dev, name, "none")


# ---- one literal ------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("win", ["0", "1"])
@pytest.mark.parametrize("tail", [-1, 1, 5])
def test_one_literal(dev, monkeypatch, name, win, tail):
    monkeypatch.setenv("KLF_WIN_INDEX", win)
    run_check(dev, name, "needle", None, tail)


# ---- literal sets -----------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("sname,stride", [("lit2", 2), ("lit4", 4), ("lit6", 6), ("lit8", 8)])
def test_literal_sets(dev, name, sname, stride):
    info = E.debug_prefilter(b"", grep=SETS[sname][0])[1]
    assert info["on"] and info["stride"] == stride, info
    for tail in (-1, 2):
        run_check(dev, name, sname, None, tail)


@BOTH
def test_anchored_short_needle(dev, monkeypatch, name):
    monkeypatch.setenv("KLF_QF_ANCHOR", "force")
    info = E.debug_prefilter(b"", grep=SETS["anch"][0])[1]
    assert info["stride"] == 8 and info["anchor"] is not None, info
    for tail in (-1, 2):
        run_check(dev, name, "anch", None, tail)


# ---- regex sets -------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("win", ["0", "1"])
def test_regex_set(dev, monkeypatch, name, win):
    """c5_regexes() + took \\d+ms + the unbounded ERR_\\w+ (k_verify, k_nfa_win, k_nfa)."""
    monkeypatch.setenv("KLF_WIN_INDEX_RX", win)
    assert E.debug_prefilter(b"", match=SETS["rx"][1])[1]["on"]
    for tail in (-1, 2):
        run_check(dev, name, "rx", None, tail)


@BOTH
def test_mixed_set(dev, name):
    for since, tail in ((None, -1), (LAYOUTS[name].mid, 3)):
        run_check(dev, name, "mixed", since, tail)


@BOTH
def test_prefilter_off(dev, name):
    grep, match = SETS["off"]
    assert not E.debug_prefilter(b"", grep=grep, match=match)[1]["on"]  # k_match decides every line
    for tail in (-1, 2):
        run_check(dev, name, "off", None, tail)


@BOTH
def test_pattern_counts(dev, name):
    lay = LAYOUTS[name]
    grep, match = SETS["rx"]
    pats = po.compile_patterns(grep, match)
    with E.Engine(0, grep=grep, match=match) as eng:
        r = eng.run_device(dev[name].data_ptr(), lay.bases, lay.lens, pattern_counts=True)
        try:
            compare(r, name, "rx", None, -1)
            for i, s in enumerate(lay.streams()):
                assert r.pattern_counts(i) == po.pattern_counts(s, pats), (name, i)
        finally:
            r.free()


# ---- transforms of a finished run -------------------------------------------------------------

_refs = {}


def window_refs(name, sname):
    """One WindowRef per stream; the match set M comes from the expectation already computed."""
    if (name, sname) not in _refs:
        out = []
        for s, w in zip(LAYOUTS[name].streams(), seams.expected(name, sname)):
            ref = WindowRef(s)
            if w["bits"] is not None:
                ref.patterned = True
                ref.m = [bool(w["bits"][l >> 3] >> (l & 7) & 1) for l in range(ref.n_lines)]
            out.append(ref)
        _refs[name, sname] = out
    return _refs[name, sname]


def check_transform(r, refs, base, want, tag):
    for i, ref in enumerate(refs):
        out, n, gbits, nsel = want(ref)
        so = r.stream(i)
        assert so.out == out, (tag, i)
        c = so.counts
        assert (c["matched"], c["selected"], c["out_bytes"]) == (n, nsel, len(out)), (tag, i, c)
        for k in ("lines", "parsed", "since_ok"):
            assert c[k] == base[i][k], (tag, i, k)
        assert r.group_bits(i) == gbits, (tag, i)
        if ref.patterned:
            assert r.match_bits(i) == ref.pack(ref.m), (tag, i)


@pytest.mark.parametrize("name,buf", [("A", "A"), ("B", "B"), ("B", "B\\n"), ("B", "B0"), ("B", "B ")])
@pytest.mark.parametrize("sname", ["needle", "rx"])
def test_regroup_and_window(dev, name, buf, sname):
    """Context lines stop at the stream's end, the inverted match takes the final fragments,
    and the window reads each selected line's first 32 bytes (tw_line_in), also of a final
    fragment shorter than that.  Bounds are instants of seam lines.  Layout B also with its
    pads and slack overwritten (the filler leg)."""
    lay = LAYOUTS[name]
    grep, match = SETS[sname]
    refs = window_refs(name, sname)
    lo, hi = (E.TIME_MIN_SEC, 0), (E.TIME_MAX_SEC, 0)
    with E.Engine(0, grep=grep, match=match) as eng:
        r = eng.run_device(dev[buf].data_ptr(), lay.bases, lay.lens)
        base = [r.stream_counts(i) for i in range(len(refs))]
        steps = [
            ("regroup(2,2)", lambda r: r.regroup(2, 2), lambda f: f.regroup(2, 2)),
            ("regroup(invert)", lambda r: r.regroup(invert=True), lambda f: f.regroup(0, 0, True)),
            ("regroup(1,3,tail=4)", lambda r: r.regroup(1, 3, tail=4), lambda f: f.regroup(1, 3, False, 4)),
            ("window", lambda r: r.window(lay.frm, lay.until, tail=5), lambda f: f.window(lay.frm, lay.until, tail=5)),
            ("window+context", lambda r: r.window(lay.frm, lay.until, 2, 2),
             lambda f: f.window(lay.frm, lay.until, 2, 2)),
            ("window(from,invert)", lambda r: r.window(lay.frm, None, invert=True),
             lambda f: f.window(lay.frm, hi, invert=True)),
            ("window(until,invert,context)", lambda r: r.window(None, lay.until, 1, 1, invert=True, tail=7),
             lambda f: f.window(lo, lay.until, 1, 1, True, 7)),
        ]
        try:
            for tag, go, want in steps:
                old, r = r, go(r)
                old.free()
                check_transform(r, refs, base, want, (name, sname, tag))
        finally:
            r.free()


@pytest.mark.parametrize("name,buf", [("A", "A"), ("B", "B"), ("B", "B\\n"), ("B", "B0"), ("B", "B ")])
def test_window_without_patterns(dev, name, buf):
    """G' = the parsed lines: every final fragment with a whole prefix is read by the window."""
    lay = LAYOUTS[name]
    refs = window_refs(name, "none")
    hi = (E.TIME_MAX_SEC, 0)
    with E.Engine(0) as eng:
        r = eng.run_device(dev[buf].data_ptr(), lay.bases, lay.lens)
        base = [r.stream_counts(i) for i in range(len(refs))]
        try:
            for tag, go, want in [
                ("window", lambda r: r.window(lay.frm, lay.until), lambda f: f.window(lay.frm, lay.until)),
                ("window(from,tail)", lambda r: r.window(lay.frm, None, tail=2), lambda f: f.window(lay.frm, hi, tail=2)),
            ]:
                old, r = r, go(r)
                old.free()
                check_transform(r, refs, base, want, (name, tag))
        finally:
            r.free()


# ---- the filler leg: layout B's streams, everything outside them overwritten ------------------

@pytest.mark.parametrize("byte", ["\\n", "0", " "])
@pytest.mark.parametrize("sname,since,tail", [("none", None, -1), ("none", None, 3), ("none", "mid", 100),
                                              ("needle", None, -1), ("needle", None, 5), ("lit2", None, -1), ("lit4", None, -1),
                                              ("lit6", None, -1), ("lit8", None, -1), ("rx", None, -1),
                                              ("rx", None, 2), ("off", None, -1), ("anch", None, -1),
                                              ("mixed", None, -1), ("mixed", "mid", 3)])
def test_filler_behind_streams(dev, monkeypatch, byte, sname, since, tail):
    if sname == "anch":
        monkeypatch.setenv("KLF_QF_ANCHOR", "force")
        assert E.debug_prefilter(b"", grep=SETS["anch"][0])[1]["anchor"] is not None
    run_check(dev, "B", sname, S.B.mid if since else None, tail, buf="B" + byte)


# ---- the counter-check: the same bytes inside the streams --------------------------------------

@BOTH
@pytest.mark.parametrize("sname", ["none", "needle", "lit6", "rx"])
def test_bytes_behind_count_once_they_belong(dev, name, sname):
    """The same buffer with the streams declared 64 bytes longer: the device answers as the
    oracle of the longer streams does, which test_seams_ref shows to differ at every seam.  So
    the completions behind the ends are live for the device paths too, and the equalities
    above hold because the kernels stop at the end, not because the features went unseen.
    The streams are kept apart as klf_layout keeps them (a one-pass result is laid out like
    its input): every third stream is lengthened per run and the others are declared empty."""
    lay = LAYOUTS[name]
    grep, match = SETS[sname]
    n = len(lay.lens)
    over = [seams.oracle(lay.stream(i, seams.OVER), sname) for i in range(n)]
    empty = seams.oracle(b"", sname)
    exact = seams.expected(name, sname)
    mine = [s for s in lay.seams if s.expect and s.expect[0] == sname]
    assert mine and all(over[s.stream]["counts"] != exact[s.stream]["counts"] or
                        over[s.stream]["out"] != exact[s.stream]["out"] for s in mine)
    with E.Engine(0, grep=grep, match=match) as eng:
        for phase in range(3):
            lens = [lay.lens[i] + seams.OVER if i % 3 == phase else 0 for i in range(n)]
            ends = [(lay.bases[i], lay.bases[i] + lens[i]) for i in range(n) if lens[i]]
            assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))
            r = eng.run_device(dev[name].data_ptr(), lay.bases, lens)
            try:
                compare(r, name, sname, None, -1, want=[over[i] if i % 3 == phase else empty for i in range(n)])
            finally:
                r.free()


# ---- the staged leg: the real stale-pad path ---------------------------------------------------

@pytest.mark.parametrize("sname", ["none", "needle", "rx"])
def test_staged_after_a_larger_batch(gpu, sname):
    """klf_run never clears pads or slack and the batch buffer only grows: stage
    seams.staged_first() as one stream and run, reset, then stage layout B's and layout A's
    pieces on the same engine.  klf_stage places them as klf_layout does, B's pieces where
    they lay in the first batch, so every pad holds the bytes that were cut off and A's
    pieces abut (test_seams_ref simulates the buffer and finds every seam hostile in it)."""
    grep, match = SETS[sname]
    first, pieces = seams.staged_first(), seams.staged_pieces()
    want = seams.expected("B", sname) + seams.expected("A", sname)
    with E.Engine(0, grep=grep, match=match) as eng:
        eng.stage(0, first)
        r = eng.run(n_streams=1)
        w = seams.oracle(first, sname)
        assert r.stream(0).out == w["out"] and r.stream(0).counts == w["counts"]
        r.free()
        eng.reset()
        eng.set_streams(len(pieces))
        for i, p in enumerate(pieces):
            if p:
                eng.stage(i, p)
        r = eng.run(n_streams=len(pieces))
        try:
            compare(r, "B+A", sname, None, -1, want=want)
        finally:
            r.free()


@pytest.mark.parametrize("sname", ["none", "needle", "rx"])
def test_follow_after_a_larger_flush(gpu, sname):
    """The same through a follow session, the long-lived engine of the product: one flush over
    seams.staged_first() (it ends in a newline: nothing is carried), then one over every piece,
    each on its own stream id; the final flush stages the open fragments too, so the batch is
    the staged leg's.  Per stream the output is the oracle's with tail -1."""
    from klogs_amd import follow
    grep, match = SETS[sname]
    first, pieces = seams.staged_first(), seams.staged_pieces()
    want = seams.expected("B", sname) + seams.expected("A", sname)
    with E.Engine(0, grep=grep, match=match) as eng, follow.Follow(eng) as fw:
        fw.feed(0, first)
        assert fw.flush() == {0: seams.oracle(first, sname)["out"]} and fw.open_bytes(0) == 0
        for i, p in enumerate(pieces):
            fw.feed(i, p)
        got = fw.flush(final=True)
    assert got == {i: w["out"] for i, w in enumerate(want) if w["counts"]["lines"]}
