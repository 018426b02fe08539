"""klf_result_timeline on the GPU (SPEC.md S4d): the emitted lines of all streams of a finished
run in one chronological sequence, against the reference of tests/test_timeline_ref.py.  Every
timeline is compared in full and exactly: the entry records, the merged bytes, the invariant
against the result's own per-stream output, and the entry count against the selected lines."""
import os
import subprocess

import pytest

import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import host as H
from klogs_amd import synth
from test_timeline_ref import (BAD_OPTS, GZ, MODE_SINCE, PATTERN_SETS, SHUF_N, SORT_SIZES, SORT_T, TimelineRef,
                               _based_streams, _shuffled_streams, cli_bodies, digit_keys, digit_streams,
                               long_line_streams, merged, mode_streams, patternless_streams, range_streams,
                               small_streams, sort_streams, stream_output, tie_streams, timeline_opts,
                               two_instant_streams, which_set_streams)

pytestmark = pytest.mark.gpu


class Session:
    """One engine run over `streams`; every timeline is checked in full against the reference."""

    def __init__(self, streams, grep=(), match=(), since=None, tail=-1):
        self.streams = streams
        self.since = since if since is not None else GZ
        self.tail = tail
        self.refs = [TimelineRef(s, grep, match) for s in streams]
        self.eng = E.Engine(0, grep=grep, match=match)
        self.eng.set_streams(len(streams))
        for i, s in enumerate(streams):
            if s:
                self.eng.stage(i, s)
        self.r = self.eng.run(since=since, tail=tail, n_streams=len(streams))
        self.g = [r.base_flags() for r in self.refs]  # the set self.r was selected from

    def flags(self, g=None, tail=None):
        g = g or self.g
        tail = self.tail if tail is None else tail
        return [ref.emitted(gi, tail, self.since) for ref, gi in zip(self.refs, g)]

    def check(self, r=None, g=None, tail=None, tags=None, timestamps=False):
        """One timeline of r (default: the session's result, selected from the flags g with
        `tail`), checked in full; returns the reference's entries."""
        r = r or self.r
        e = self.flags(g, tail)
        want_ent, want_bytes = merged(self.refs, e, tags, timestamps)
        tl = r.timeline(tags=tags, timestamps=timestamps)
        try:
            ent = tl.entries
            assert ent.dtype == E.TIMELINE_ENTRY
            got = [tuple(int(x) for x in row) for row in ent.tolist()]
            assert len(got) == len(want_ent) == len(tl), (len(got), len(want_ent))
            assert got == want_ent, [(k, a, b) for k, (a, b) in enumerate(zip(got, want_ent)) if a != b][:6]
            assert tl.size == len(want_bytes)
            data = tl.bytes
            assert data == want_bytes, _first_difference(data, want_bytes)
            selected = [r.stream_counts(i)["selected"] for i in range(len(self.streams))]
            assert len(got) == sum(selected) and selected == [sum(x) for x in e]
        finally:
            tl.free()
        if tags is None and not timestamps:  # the invariant, from the GPU's own entries and bytes
            ends = [o for *_, o in got[1:]] + [len(data)]
            for i, ref in enumerate(self.refs):
                mine = sorted((line, data[off:end]) for (_, _, s, line, off), end in zip(got, ends) if s == i)
                out = r.stream(i).out
                assert out == stream_output(ref, e[i])
                # (the stream's unterminated fragment is emitted: its entry brings the "\n")
                frag = bool(self.streams[i]) and not self.streams[i].endswith(b"\n") and \
                    any(line == ref.n_lines - 1 for line, _ in mine)
                assert b"".join(x for _, x in mine) == out + (b"\n" if frag else b""), i
        else:
            self.check(r, g, tail)
        return want_ent

    def close(self):
        self.r.free()
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return (len(a), len(b), k, a[max(0, k - 40):k + 40], b[max(0, k - 40):k + 40])


# ------------------------------------------------------------------ 1. small, adversarial ---

SMALL_TAGS = [None, [b"", b"", b""], [b"a/b ", b"", b"pod-with-a-longer-name/container-1 "],
              [b"x" * 1024, b"y", b"zz"]]


@pytest.mark.parametrize("tail", [-1, 0, 1, 5])
@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_small_adversarial(gpu, grep, tail):
    streams = small_streams()
    with Session(streams, grep=grep, tail=tail) as s:
        assert [r.n_lines for r in s.refs] == [20, 20, 19] and s.refs[0].n_parsed == 17
        e = s.flags()
        if tail in (-1, 5) and not grep:
            assert e[0][-1] and e[1][-1]  # both fragments are emitted, with and without content
            ent, data = merged(s.refs, e)
            k = [i for i, x in enumerate(ent) if x[2:4] == (1, 19)][0]
            assert 0 < k < len(ent) - 1  # the empty fragment sits mid-timeline and renders as "\n"
            assert data[ent[k][4]:ent[k + 1][4]] == b"\n"
            k = [i for i, x in enumerate(ent) if x[2:4] == (0, 19)][0]
            assert k < len(ent) - 1 and data[ent[k][4]:ent[k + 1][4]] == b"fragment HIT\n"
        for tags in SMALL_TAGS:
            for timestamps in (False, True):
                s.check(tags=tags, timestamps=timestamps)


# ------------------------------------------------------------------ 2. ties and stability ---

def test_ties_and_stability(gpu):
    with Session(tie_streams()) as s:
        ent = s.check()
        assert len({(sec, nsec) for sec, nsec, *_ in ent}) == 1  # one instant: every pass is skipped
        assert [(st, ln) for _, _, st, ln, _ in ent] == [(st, ln) for st in range(4) for ln in range(40 + st)]
        s.check(tags=[b"0 ", b"1 ", b"2 ", b"3 "], timestamps=True)
        r2 = s.r.retail(3)
        s.r.free()
        s.r = r2
        ent = s.check(tail=3)
        assert [(st, ln) for _, _, st, ln, _ in ent] == [(st, 37 + st + k) for st in range(4) for k in range(3)]
    # two instants, each tied across and inside the streams: one pass runs, the ties keep their order
    with Session(two_instant_streams()) as s:
        ent = s.check()
        assert [(st, ln) for _, _, st, ln, _ in ent[:450]] == [(st, ln) for st in range(3) for ln in range(0, 300, 2)]


# ----------------------------------------------------------------------------- 3. key range ---

def test_key_range(gpu):
    with Session(range_streams()) as s:
        ent = s.check()
        assert ent[0][0] < -62_000_000_000 and ent[-1][0] > 253_000_000_000
        s.check(timestamps=True)
    with Session(digit_streams()) as s:
        ent = s.check()
        assert [(sec, nsec) for sec, nsec, *_ in ent] == digit_keys()
        s.check(tags=[b"a ", b"b ", b"c "])


# ----------------------------------------------------------------------------- 4. sort sizes ---

@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_sizes(gpu, n):
    assert SORT_T == 2048  # klf_analysis.hpp kTlSortBlock: T - 1, T, T + 1 and 2 T + 1 are in the list
    with Session(sort_streams(n)) as s:
        ent = s.check()
        assert len(ent) == n
        if n == 20000:
            s.check(tags=[b"shuffled ", b"ascending "], timestamps=True)


# ------------------------------------------------------------------------------- 5. shuffled ---

def test_shuffled(gpu):
    with Session(_shuffled_streams()) as s:
        ent = s.check()
        assert len(ent) == 3 * SHUF_N
        secs = [sec for sec, *_ in ent]
        assert secs == sorted(secs) and len(set(secs)) >= SHUF_N


# ------------------------------------------------- 6. stream boundaries inside a bitmap word ---

@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_stream_boundaries_in_a_word(gpu, grep):
    streams = _based_streams()
    with Session(streams, grep=grep) as s:
        assert sum(r.n_lines for r in s.refs) < 1200  # ~3 lines a stream: several streams per word
        ent = s.check()
        assert len({st for _, _, st, _, _ in ent}) > (10 if grep else 150)
        s.check(tags=[b"%d " % i for i in range(len(streams))])
        r2 = s.r.retail(2)
        s.r.free()
        s.r = r2
        s.check(tail=2)


# ------------------------------------------------------------------------- 7. one long line ---

def test_one_long_line(gpu):
    with Session(long_line_streams()) as s:
        assert len(s.streams[0]) % 256 == 0 and max(e - b for b, e in s.refs[0].lines) > 100_000
        s.check()
        s.check(tags=[b"first ", b"second "], timestamps=True)
        r2 = s.r.retail(2)
        s.r.free()
        s.r = r2
        s.check(tail=2)


# -------------------------------------- 8. every pattern mode, from a run with a partial index ---

@pytest.mark.parametrize("name", list(PATTERN_SETS))
def test_pattern_modes_from_a_partial_index(gpu, name):
    with Session(mode_streams(), since=MODE_SINCE, tail=5, **PATTERN_SETS[name]) as s:
        ent = s.check()
        assert len(ent) <= 15 and (len(ent) > 0) == (name != "never")
        s.check(tags=[b"text ", b"json ", b"adv "], timestamps=True)


@pytest.fixture(params=["sparse", "dense", None])
def compact(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("KLF_COMPACT", raising=False)
    else:
        monkeypatch.setenv("KLF_COMPACT", request.param)
    return request.param


def test_patternless_engine(gpu, compact):
    with Session(patternless_streams(), since=(synth.T0 + 300, 0)) as s:
        if compact is None:
            assert s.r.compaction() == "one_pass"
        c = s.r.stream_counts(1)
        assert c["parsed"] < c["lines"]
        ent = s.check()
        assert len(ent) > 1000
        s.check(tags=[b"t ", b"a "], timestamps=True)


# ------------------------------------------------------------- 9. which set, and read-only ---

def test_which_set_and_read_only(gpu):
    since = (synth.T0 + 600, 0)
    a, b = (synth.T0 + 900, 0), (synth.T0 + 2000, 0)
    with Session(which_set_streams(), grep=[synth.NEEDLE], since=since, tail=3) as s:
        r = s.r

        def state(x):
            return [(x.stream(i).out, x.match_bits(i), x.group_bits(i), x.stream(i).counts) for i in range(2)]

        before = state(r)
        e1 = s.check()
        s.check(timestamps=True)  # repeated with other options
        assert before == state(r)
        r2 = r.window(a, b, 1, 1)  # r was still the latest: no KLF_ESTATE
        g2 = [ref.cut(a, b, 1, 1) for ref in s.refs]
        assert s.check(r=r2, g=g2, tail=-1) != e1  # E follows G''
        with pytest.raises(E.KlfError) as ei:  # r is not the latest any more
            r.timeline()
        assert ei.value.code == E.KLF_ESTATE
        r.free()
        r3 = r2.regroup(2, 1, tail=4)
        g3 = [ref.group(2, 1) for ref in s.refs]
        e3 = s.check(r=r3, g=g3, tail=4)
        r4 = r3.retail(1)
        e4 = s.check(r=r4, g=g3, tail=1)
        assert 0 < len(e4) < len(e3)
        keep = r4.timeline(tags=[b"A ", b"B "])
        kept = (keep.entries.tolist(), keep.bytes)
        r5 = r4.retail(-1)
        want = [ref.regroup(2, 1, False, -1, since)[0] for ref in s.refs]
        assert [r5.stream(i).out for i in range(2)] == want  # the timelines in between changed nothing
        s.check(r=r5, g=g3, tail=-1)
        for x in (r2, r3, r4, r5):
            x.free()
        # a timeline outlives the next run and a reset
        late = s.eng.run(since=None, tail=1, n_streams=2)
        assert (keep.entries.tolist(), keep.bytes) == kept
        late.free()
        s.eng.reset()
        for i, d in enumerate(s.streams):
            s.eng.stage(i, d)
        assert (keep.entries.tolist(), keep.bytes) == kept
        with open(os.devnull, "wb") as f:
            assert keep.write(f.fileno()) == len(kept[1])
        keep.free()
        s.r = s.eng.run(since=since, tail=3, n_streams=2)
        s.tail = 3
        assert s.check() == e1


def test_errors_on_a_live_result(gpu):
    with Session(small_streams()[:2], grep=(b"HIT",)) as s:
        lib = E.lib()
        out = E.C.c_void_p()
        for name, kw in BAD_OPTS.items():
            o, keep = timeline_opts(**kw)
            assert lib.klf_result_timeline(s.r._p, E.C.byref(o), E.C.byref(out)) == E.KLF_EINVAL, name
            assert out.value is None
        o, keep = timeline_opts()
        assert lib.klf_result_timeline(s.r._p, None, E.C.byref(out)) == E.KLF_EINVAL
        assert lib.klf_result_timeline(s.r._p, E.C.byref(o), None) == E.KLF_EINVAL
        o, keep = timeline_opts(tags=None, tag_off=[5, 1, 0])  # null tags: tag_off is ignored
        assert lib.klf_result_timeline(s.r._p, E.C.byref(o), E.C.byref(out)) == E.KLF_OK
        lib.klf_timeline_free(out)
        s.check()  # the result is as it was
    with Session([b"", b"junk\n", b""]) as s:  # no emitted line: a valid empty timeline
        assert s.check(tags=[b"a", b"b", b"c"]) == []
    eng = E.Engine(0)
    eng.set_streams(2)
    r = eng.run(n_streams=2)  # no stream has bytes
    tl = r.timeline()
    assert len(tl) == 0 and tl.bytes == b"" and tl.size == 0 and tl.write(1) == 0
    tl.free()
    r.free()
    eng.close()


# ----------------------------------------------------------------------------- 10. write ---

def test_write(gpu, tmp_path):
    with Session(_shuffled_streams()[:2] + long_line_streams()) as s:
        tags = [b"a ", b"", b"long ", b"d "]
        tl = s.r.timeline(tags=tags, timestamps=True)
        path = tmp_path / "merged.log"
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            assert tl.write(fd) == tl.size  # the device path: no host view was taken yet
        finally:
            os.close(fd)
        data = tl.bytes
        assert path.read_bytes() == data == merged(s.refs, s.flags(), tags, True)[1]
        fd = os.open(path, os.O_WRONLY | os.O_APPEND)
        try:
            assert tl.write(fd) == len(data)  # now from the host copy, appended
        finally:
            os.close(fd)
        assert path.read_bytes() == data + data
        assert tl.ms > 0
        rd, wr = os.pipe()
        os.close(rd)
        with pytest.raises(E.KlfError) as ei:  # (Python ignores SIGPIPE: write(2) fails with EPIPE)
            tl.write(wr)
        os.close(wr)
        assert ei.value.code == E.KLF_EIO
        tl.free()


# ------------------------------------------------------------------------------- 11. CLI ---

def test_cli_merge(gpu, tmp_path):
    bodies, rows = cli_bodies(), []
    for pod, cname, data in bodies:
        f = tmp_path / f"body_{pod}_{cname}.log"
        f.write_bytes(data)
        rows.append((pod, "container", cname, str(f)))
    m = tmp_path / "manifest.tsv"
    m.write_text("".join("\t".join(r) + "\n" for r in rows))
    now = synth.T0 + synth.SPAN + 1
    base = ["--grep", synth.NEEDLE.decode(), "-t", "20", "--now", str(now), "--no-color", str(m)]
    dirs = {"plain": [], "merge": ["--merge"], "stamps": ["--merge", "--merge-timestamps"]}
    for name, extra in dirs.items():
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / name)] + extra + base, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
    names = sorted(H.log_file_name(p, c) for p, c, _ in bodies)
    assert sorted(os.listdir(tmp_path / "plain")) == names
    refs = [TimelineRef(data, grep=[synth.NEEDLE]) for _, _, data in bodies]
    flags = [ref.emitted(ref.base_flags(), 20, GZ) for ref in refs]
    tags = [f"{p}/{c} ".encode() for p, c, _ in bodies]
    assert [sum(f) for f in flags] == [20] * 4  # (each body holds 28 matches or more: the tail binds)
    for name, stamps in (("merge", False), ("stamps", True)):
        assert sorted(os.listdir(tmp_path / name)) == sorted(names + ["merged.log"])
        for nm in names:
            assert (tmp_path / name / nm).read_bytes() == (tmp_path / "plain" / nm).read_bytes() != b"", nm
        assert (tmp_path / name / "merged.log").read_bytes() == merged(refs, flags, tags, stamps)[1]
    # built from the result that gets written: after the window
    r = subprocess.run([str(H.CLI), "-p", str(tmp_path / "win"), "--merge", "--from", "2024-10-22T00:25:00.5Z",
                        "--until", "10m"] + base, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    frm, until = po.parse_line(b"2024-10-22T00:25:00.5Z x")[0], (now - 600, 0)
    wflags = [ref.emitted(ref.cut(frm, until), 20, GZ) for ref in refs]
    assert 0 < sum(map(sum, wflags)) and wflags != flags
    assert (tmp_path / "win" / "merged.log").read_bytes() == merged(refs, wflags, tags)[1]
    # --merge-timestamps alone is a usage error
    r = subprocess.run([str(H.CLI), "-p", str(tmp_path / "none"), "--merge-timestamps"] + base, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and "usage:" in r.stderr
    assert not (tmp_path / "none").exists()
