"""klf_window on the GPU (SPEC.md S4b): a time window [from, until) over a finished run,
against the reference of tests/test_window_ref.py (the Python oracle's pieces).  Each case is
one engine run and then many windows; every window is compared in full and exactly."""
import os
import subprocess

import pytest

import c_oracle as co
import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import host as H
from klogs_amd import synth
from test_gpu_regroup import CARRY_HITS, CARRY_N, PATTERN_SETS, _tiny_streams
from test_window_ref import OPEN_HI, OPEN_LO, WindowRef

pytestmark = pytest.mark.gpu

GZ = po.GO_ZERO_TIME
COUNT_KEYS = ("lines", "parsed", "since_ok")
NS = 10**9


def shift(t, d_ns):
    """The instant t (sec, nsec) moved by d_ns nanoseconds."""
    total = t[0] * NS + t[1] + d_ns
    return (total // NS, total % NS)


def opt(t):
    """A reference bound as Result.window takes it (None = open)."""
    return None if t in (OPEN_LO, OPEN_HI) else t


class Session:
    """One engine run over `streams`; every window is checked in full against the reference."""

    def __init__(self, streams, grep=(), match=(), since=None, tail=-1):
        self.streams = streams
        self.since = since
        self.patterned = bool(list(grep) or list(match))
        self.refs = [WindowRef(s, grep, match) for s in streams]
        self.mbits = [r.m_bits() for r in self.refs]
        self.eng = E.Engine(0, grep=grep, match=match)
        self.eng.set_streams(len(streams))
        for i, s in enumerate(streams):
            if s:
                self.eng.stage(i, s)
        self.r = self.eng.run(since=since, tail=tail, n_streams=len(streams))
        self.base = [self.r.stream_counts(i) for i in range(len(streams))]
        self.memo = {}

    def sizes(self, frm, until, before=0, after=0, invert=False):
        """(|G''|, |G'|) over all streams, by the reference."""
        g2 = sum(sum(r.cut(frm, until, before, after, invert)) for r in self.refs)
        g1 = sum(sum(r.gprime(before, after, invert)) for r in self.refs)
        return g2, g1

    def assert_cuts(self, frm, until, before=0, after=0, invert=False):
        g2, g1 = self.sizes(frm, until, before, after, invert)
        assert 0 < g2 < g1, (g2, g1)
        return g2, g1

    def want(self, i, frm, until, before, after, invert, tail):
        g = self.refs[i].cut(frm, until, before, after, invert)
        key = (i, WindowRef.pack(g), tail)  # (many windows select the same lines)
        if key not in self.memo:
            self.memo[key] = self.refs[i].emit(g, tail, self.since or GZ)
        return self.memo[key]

    def check(self, r, frm, until, before=0, after=0, invert=False, tail=-1, what=""):
        for i in range(len(self.streams)):
            out, n, gbits, nsel = self.want(i, frm, until, before, after, invert, tail)
            tag = (what, i, frm, until, before, after, invert, tail)
            so = r.stream(i)
            assert so.out == out, tag
            c = so.counts
            assert (c["matched"], c["selected"], c["out_bytes"]) == (n, nsel, len(out)), (tag, c)
            for k in COUNT_KEYS:
                assert c[k] == self.base[i][k], (tag, k, c, self.base[i])
            assert r.group_bits(i) == gbits, tag
            if self.patterned:
                assert r.match_bits(i) == self.mbits[i], tag
            else:
                with pytest.raises(E.KlfError) as ei:
                    r.match_bits(i)
                assert ei.value.code == E.KLF_EINVAL

    def window(self, frm=OPEN_LO, until=OPEN_HI, before=0, after=0, invert=False, tail=-1):
        old, self.r = self.r, self.r.window(opt(frm), opt(until), before, after, invert, tail)
        old.free()
        self.check(self.r, frm, until, before, after, invert, tail)
        return self.r

    def close(self):
        self.r.free()
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ------------------------------------------------------------------ 1. small, adversarial ---

SMALL = [
    b"2024-10-22T00:00:05.000000000Z canonical a HIT\n",
    b"2024-10-22T7:00:00Z one-digit hour\n",
    b"not a timestamp HIT\n",
    b"2024-10-22T01:30:00+01:00 instant 00:30 HIT\n",
    b"2024-10-22T00:10:00-00:30 instant 00:40\n",
    b"2024-10-22T00:20:00,5Z comma fraction HIT\n",
    b"2024-10-22T00:25:00Z no fraction\n",
    b"2100-01-01T00:00:00.000000000Z canonical shape, year 2100 HIT\n",
    b"2024-10-22T00:00:07.123Z three digits\n",
    b"2024-10-22T00:00:06.123456789012Z twelve digits HIT\n",
    b"\n",
    b"0000-01-01T00:00:00Z year 0 HIT\n",
    b"1969-12-31T23:59:59.999999999Z canonical shape, year 1969\n",
    b"2024-10-22T00:00:05.000000001Z canonical b\n",
    b"2024-10-22T00:00:04.999999999Z canonical c HIT\n",
    b"2024-13-01T00:00:00.000000000Z bad month HIT\n",
    b"2024-10-22T00:00:05.000000000Z canonical a again\n",
    b"2099-12-31T23:59:59.999999999Z canonical, the fast path's last year HIT\n",
    b"1970-01-01T00:00:00.000000000Z canonical, the epoch\n",
    b"2024-10-22T00:00:09.000000000Z fragment HIT",
]
SMALL_MID = po.parse_line(b"2024-10-22T00:00:06Z x")[0]


@pytest.mark.parametrize("since", [None, SMALL_MID])
@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_small_adversarial(gpu, grep, since):
    data = b"".join(SMALL)
    with Session([data], grep=grep, since=since, tail=-1) as s:
        ref = s.refs[0]
        assert ref.n_lines == 20 and ref.n_parsed == 17
        instants = sorted({t for t in ref.ts if t is not None})
        assert len(instants) == 16  # (two lines share one)
        edges = sorted({shift(t, d) for t in instants for d in (-1, 0, 1)})
        mid = instants[len(instants) // 2]
        s.assert_cuts(mid, OPEN_HI)
        s.assert_cuts(OPEN_LO, mid)
        for tail in (-1, 0, 1, 3, 100):
            for x in edges:
                s.window(x, OPEN_HI, tail=tail)
                s.window(OPEN_LO, x, tail=tail)
            for x in instants:
                s.window(x, x, tail=tail)               # from == until: empty
                s.window(x, shift(x, 1), tail=tail)     # exactly the lines at x
                s.window(shift(x, 1), x, tail=tail)     # from > until: empty
            s.window(instants[3], instants[-3], tail=tail)
            s.window(tail=tail)                         # both sides open
        assert s.sizes(mid, mid)[0] == 0 and s.sizes(shift(mid, 1), mid)[0] == 0
        if not grep:
            assert s.sizes(mid, shift(mid, 1))[0] >= 1  # one nanosecond wide: the lines at `mid`
        if grep:  # with context and inverted, in the one call
            for x in edges[::3]:
                s.window(x, OPEN_HI, 1, 2, False, 3)
                s.window(OPEN_LO, x, 2, 0, True, -1)


# ------------------------------------------------- 2. stream boundaries inside a bitmap word ---

def _based_streams():
    """_tiny_streams with each stream on a time base of its own: stream i starts i ms after
    T0 and its lines are 20 minutes apart, so one window cuts through most streams."""
    out = []
    for i, s in enumerate(_tiny_streams()):
        lines = s.split(b"\n")
        for j, ln in enumerate(lines):
            if ln.startswith(b"2024-10-22T00:"):  # (the 31-byte prefix of test_gpu_regroup.ts)
                m = 20 * j
                lines[j] = b"2024-10-22T%02d:%02d:00.%03d000000Z " % (m // 60, m % 60, i) + ln[31:]
        out.append(b"\n".join(lines))
    return out


@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_stream_boundaries_in_a_word(gpu, grep):
    streams = _based_streams()
    with Session(streams, grep=grep, tail=-1) as s:
        assert sum(r.n_lines for r in s.refs) < 1200  # ~3 lines a stream: several streams per word
        frm, until = (synth.T0 + 30 * 60, 0), (synth.T0 + 70 * 60, 0)  # lines 2 and 3 of every stream
        g2, _ = s.assert_cuts(frm, until)
        cut_streams = sum(1 for r in s.refs if 0 < sum(r.cut(frm, until)) < sum(r.gprime()))
        assert g2 > (20 if grep else 150) and cut_streams >= (5 if grep else 100)
        s.window(frm, until)
        s.window(frm, until, tail=2)
        s.window(OPEN_LO, until, tail=1)
        if grep:
            s.assert_cuts(frm, until, 1, 2)
            s.window(frm, until, 1, 2)
            s.window(frm, until, 1, 2, True, 2)


# ------------------------------------------------------------------ 3. word and chunk edges ---

def _carry_ts(i):
    return b"2024-10-22T%02d:%02d:%02d.000000000Z " % (i // 3600, i // 60 % 60, i % 60)


@pytest.fixture(scope="module", params=["no patterns", "four hits"])
def carry_session(gpu, request):
    hits = CARRY_HITS if request.param == "four hits" else ()
    big = b"".join(_carry_ts(i) + (b"HIT %05d padding .....\n" if i in hits else b"line %05d padding ....\n") % i
                   for i in range(CARRY_N))
    second = b"".join(_carry_ts(i) + (b"HIT second\n" if i == 0 else b"second %d\n" % i) for i in range(40))
    assert len(big) > 1_000_000
    s = Session([big, second], grep=[b"HIT"] if hits else (), tail=-1)
    yield s
    s.close()


@pytest.mark.parametrize("edge", [31, 32, 33, 8191, 8192, 8193])
def test_word_and_chunk_edges(carry_session, edge):
    s = carry_session
    t = lambda i: (synth.T0 + i, 0)
    assert s.refs[0].ts[edge] == t(edge)
    hi = CARRY_N - 1 - edge
    if s.patterned:  # the hits sit at 5, 8191, 8192 and 24001: context makes G' dense around them
        s.window(t(edge), OPEN_HI, 40, 40)
        s.window(OPEN_LO, t(edge), 40, 40, tail=7)
        s.window(t(edge), t(hi))
        s.window(t(edge), t(hi), 0, 0, True, 9)  # inverted: nearly every line, cut at both edges
        s.assert_cuts(t(edge), t(hi), 0, 0, True)
    else:
        s.assert_cuts(t(edge), OPEN_HI)
        s.window(t(edge), OPEN_HI)
        s.window(OPEN_LO, t(edge))
        s.window(t(edge), t(hi))
        s.window(t(hi), OPEN_HI, tail=7)
        s.window(OPEN_LO, t(hi), tail=7)


# ------------------------------------------------------------------ 4. pattern-less engine ---

@pytest.fixture(params=["sparse", "dense", None])
def compact(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("KLF_COMPACT", raising=False)
    else:
        monkeypatch.setenv("KLF_COMPACT", request.param)
    return request.param


@pytest.mark.parametrize("run_tail", [-1, 5])
def test_patternless_engine(gpu, compact, run_tail):
    streams = [synth.generate(synth.TEXT, 71, 0, 400_000),
               synth.generate(synth.ADVERSARIAL, 72, 1, 4000, drop_final_nl=True),
               synth.generate(synth.JSON, 73, 2, 150_000, drop_final_nl=True)]
    since = (synth.T0 + 300, 0)
    with Session(streams, since=since, tail=run_tail) as s:
        assert s.refs[1].n_parsed < s.refs[1].n_lines  # unparseable lines
        if compact is None and run_tail == -1:
            assert s.r.compaction() == "one_pass"
        tenth = ((synth.T0 + 1800, 0), (synth.T0 + 2160, 0))
        most = ((synth.T0 + 180, 0), (synth.T0 + 3420, 0))
        n10, n = s.assert_cuts(*tenth)
        n90, _ = s.assert_cuts(*most)
        assert n // 20 < n10 < n // 5 and n90 > (3 * n) // 4
        for frm, until in (tenth, most):
            s.window(frm, until)
            s.window(frm, until, tail=3)
            s.window(frm, until)
            for t in (0, 1, 4, -1):
                old, s.r = s.r, s.r.retail(t)  # re-tails over G''
                s.check(s.r, frm, until, tail=t, what="retail")
                old.free()
        s.window()  # both sides open: the parsed lines, not the plain run (stream 1)
        assert s.r.stream(1).counts["matched"] == s.refs[1].n_parsed
        for tail in (run_tail, 2):  # a fresh run: the bitmap mode did not leak into it
            old, s.r = s.r, s.eng.run(since=since, tail=tail, n_streams=len(streams))
            old.free()
            for i, d in enumerate(streams):
                out, lo, bits, c = co.filter_stream(d, since, tail, [])
                so = s.r.stream(i)
                assert so.out == out, (i, tail)
                for k in ("lines", "parsed", "since_ok", "matched", "selected"):
                    assert so.counts[k] == c[k], (i, tail, k)
                with pytest.raises(E.KlfError) as ei:
                    s.r.group_bits(i)  # a run's result of a pattern-less engine: as before
                assert ei.value.code == E.KLF_EINVAL


# -------------------------------------- 5. every pattern mode, from a run with a partial index ---

@pytest.mark.parametrize("name", list(PATTERN_SETS))
def test_pattern_modes_from_a_partial_index(gpu, name):
    pats = PATTERN_SETS[name]
    streams = [synth.generate(synth.TEXT, 21, 0, 150_000, permille=20),
               synth.generate(synth.JSON, 22, 1, 120_000, permille=20, drop_final_nl=True),
               synth.generate(synth.ADVERSARIAL, 23, 2, 6000, permille=40, drop_final_nl=True)]
    frm, until = (synth.T0 + 1200, 0), (synth.T0 + 2700, 0)
    with Session(streams, since=(synth.T0 + 900, 0), tail=5, **pats) as s:
        if name != "never":
            s.assert_cuts(frm, until)
            s.assert_cuts(frm, until, 2, 2)
        if name != "all":
            s.assert_cuts(frm, until, 0, 0, True)
        for tail in (-1, 5):
            s.window(frm, until, tail=tail)
            s.window(frm, until, 2, 2, tail=tail)
            s.window(frm, until, 0, 0, True, tail=tail)


# --------------------------------------------------------------------------- 6. output growth ---

@pytest.mark.parametrize("grep", [(), (b"",)])
def test_output_growth(gpu, monkeypatch, grep):
    monkeypatch.setenv("KLF_DEBUG_OUT_INIT", "4096")
    data = synth.generate(synth.JSON, 31, 0, 1_500_000, permille=10)
    since = (synth.T0 + 300, 0)
    with Session([data], grep=grep, since=since, tail=1) as s:
        assert len(s.r.stream(0).out) < 4096
        r = s.window(tail=-1)
        every = po.filter_stream(data, since, -1, ())
        assert s.refs[0].n_parsed == s.refs[0].n_lines
        so = r.stream(0)
        assert so.out == every.out and so.counts["selected"] == every.n_since > 1000
        assert len(so.out) > 1_000_000


# ---------------------------------------------------------------------- 7. chaining and state ---

def test_chaining_and_state(gpu):
    streams = [synth.generate(synth.JSON, 41, 0, 300_000, permille=30),
               synth.generate(synth.ADVERSARIAL, 42, 1, 5000, permille=40, drop_final_nl=True)]
    since = (synth.T0 + 600, 0)
    a, b, c = (synth.T0 + 900, 0), (synth.T0 + 2000, 0), (synth.T0 + 3000, 0)
    with Session(streams, grep=[synth.NEEDLE], since=since, tail=3) as s:
        s.assert_cuts(a, b)
        s.assert_cuts(b, c)
        s.window(a, b)
        s.window(b, c)  # window -> window: the second alone decides (disjoint from the first)
        s.window(a, c, 1, 1, tail=4)
        stale = s.r
        s.r = s.r.regroup(1, 1, False, -1)  # window -> regroup: from M, with no window
        s.check(s.r, OPEN_LO, OPEN_HI, 1, 1, False, -1, "regroup")
        with pytest.raises(E.KlfError) as ei:
            stale.window(a, b)
        assert ei.value.code == E.KLF_ESTATE
        with pytest.raises(E.KlfError) as ei:
            stale.stream(0)
        assert ei.value.code == E.KLF_ESTATE
        stale.free()
        s.window(a, b, tail=2)
        old, s.r = s.r, s.r.retail(-1)  # re-tails over G''
        old.free()
        s.check(s.r, a, b, tail=-1, what="retail")
        s.window(tail=3)  # open, no context: klf_retail(prev, 3) over M byte for byte
        for i, d in enumerate(streams):
            want = po.filter_stream(d, since, 3, po.compile_patterns([synth.NEEDLE]))
            assert s.r.stream(i).out == want.out and s.r.group_bits(i) == want.match_bits
        old, s.r = s.r, s.eng.run(since=since, tail=3, n_streams=len(streams))  # a fresh run
        old.free()
        for i, d in enumerate(streams):
            out, lo, bits, cn = co.filter_stream(d, since, 3, [synth.NEEDLE])
            so = s.r.stream(i)
            assert so.out == out and so.counts["matched"] == cn["matched"]
            assert s.r.match_bits(i) == bits == s.r.group_bits(i)


def _raw_window(eng, r, opts, tail=-1):
    out = E.C.c_void_p()
    rc = E.lib().klf_window(eng._h, r._p, E.C.byref(opts) if opts is not None else None, tail, E.C.byref(out))
    assert not out.value or rc == E.KLF_OK
    return rc


def _opts(frm=OPEN_LO, until=OPEN_HI, before=0, after=0, flags=0, reserved=0, from_res=0, until_res=0):
    o = E._WindowOpts()
    o.from_.sec, o.from_.nsec, o.from_._reserved = frm[0], frm[1], from_res
    o.until.sec, o.until.nsec, o.until._reserved = until[0], until[1], until_res
    o.before, o.after, o.flags, o._reserved = before, after, flags, reserved
    return o


def test_errors(gpu):
    data = synth.generate(synth.JSON, 51, 0, 60_000, permille=50)
    t = (synth.T0 + 1500, 0)  # (the stream's three matches lie at 1372 s, 1502 s and 1657 s)
    bad = [_opts(flags=2), _opts(flags=1 | 0x80000000), _opts(reserved=7), _opts(from_res=1), _opts(until_res=1),
           _opts(frm=(t[0], -1)), _opts(frm=(t[0], NS)), _opts(until=(t[0], -1)), _opts(until=(t[0], NS))]
    for grep in ((), (synth.NEEDLE,)):
        with E.Engine(0, grep=grep) as eng:
            eng.set_streams(1)
            eng.stage(0, data)
            r = eng.run(tail=-1, n_streams=1)
            for o in bad:
                assert _raw_window(eng, r, o) == E.KLF_EINVAL
            assert _raw_window(eng, r, None) == E.KLF_EINVAL
            assert _raw_window(eng, r, _opts(), tail=-2) == E.KLF_EINVAL
            assert E.lib().klf_window(eng._h, r._p, E.C.byref(_opts()), -1, None) == E.KLF_EINVAL
            assert E.lib().klf_window(eng._h, None, E.C.byref(_opts()), -1, E.C.byref(E.C.c_void_p())) == E.KLF_EINVAL
            if not grep:  # context needs a pattern
                for o in (_opts(before=1), _opts(after=1), _opts(flags=1)):
                    assert _raw_window(eng, r, o) == E.KLF_EINVAL
                with pytest.raises(E.KlfError) as ei:
                    r.window(t, None, after=2)
                assert ei.value.code == E.KLF_EINVAL
            # prev is still the latest and untouched
            assert r.stream(0).out == po.filter_stream(data, GZ, -1, po.compile_patterns(grep)).out
            ref = WindowRef(data, grep=grep)
            r2 = r.window(t, None)
            with pytest.raises(E.KlfError) as ei:  # r is not the latest any more
                r.window(t, None)
            assert ei.value.code == E.KLF_ESTATE
            want = ref.window(t, OPEN_HI)
            assert r2.stream(0).out == want[0] != b"" and r2.group_bits(0) == want[2]
            r.free()
            r2.free()


# ------------------------------------------------------------------------------------- 8. CLI ---

@pytest.mark.parametrize("patterned", [False, True])
def test_cli_window_flags(gpu, tmp_path, patterned):
    bodies, rows = {}, []
    for p in range(2):
        for cname in ("app", "sidecar"):
            data = synth.generate(synth.JSON, 61 + p, p * 2 + len(cname), 150_000 + 3000 * p, permille=100,
                                  drop_final_nl=(cname == "sidecar"))
            f = tmp_path / f"body_{p}_{cname}.log"
            f.write_bytes(data)
            bodies[(f"pod-{p}", cname)] = data
            rows.append((f"pod-{p}", "container", cname, str(f)))
    m = tmp_path / "manifest.tsv"
    m.write_text("".join("\t".join(r) + "\n" for r in rows))
    now = synth.T0 + synth.SPAN + 1
    out = tmp_path / "logs"
    frm = po.parse_line(b"2024-10-22T00:25:00.5Z x")[0]
    until = (now - 10 * 60, 0)
    cmd = [str(H.CLI), "-p", str(out), "-s", "40m", "-t", "50", "--from", "2024-10-22T00:25:00.5Z", "--until", "10m"]
    pats = dict(grep=[synth.NEEDLE]) if patterned else {}
    ctx = 2 if patterned else 0
    cmd += ["--grep", synth.NEEDLE.decode(), "-C", "2"] if patterned else []
    r = subprocess.run(cmd + ["--now", str(now), "--no-color", str(m)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    since, tail, rej = H.lop_opts("40m", 50, (now, 0))
    assert not rej and tail == 50
    assert sorted(os.listdir(out)) == sorted(H.log_file_name(p, c) for p, c in bodies)
    for (p, c), data in bodies.items():
        ref = WindowRef(data, **pats)
        assert 0 < sum(ref.cut(frm, until, ctx, ctx)) < sum(ref.gprime(ctx, ctx))
        want = ref.window(frm, until, ctx, ctx, False, tail, since)[0]
        assert want
        assert (out / H.log_file_name(p, c)).read_bytes() == want, (p, c)
    # a value that is neither an instant nor a duration
    for flag in ("--until", "--from"):
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / "none"), flag, "yesterday", str(m)], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 1 and "usage:" in r.stderr
