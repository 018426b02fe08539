"""klf_result_histogram on the GPU (SPEC.md S4c): the lines of a finished run's selection
counted over time, against the reference of tests/test_hist_ref.py.  Each case is one engine
run and then many histograms; every histogram is compared in full and exactly, per stream, and
its sum is held against the result's own counts."""
import datetime
import os
import random
import subprocess

import numpy as np
import pytest

import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import host as H
from klogs_amd import synth
from test_gpu_regroup import CARRY_N, PATTERN_SETS
from test_gpu_window import SMALL, _based_streams, _carry_ts
from test_hist_ref import BAD_OPTS, NS, HistRef, hist_opts, shift

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


class Session:
    """One engine run over `streams`; every histogram is checked in full against the reference."""

    def __init__(self, streams, grep=(), match=(), since=None, tail=-1):
        self.streams = streams
        self.patterned = bool(list(grep) or list(match))
        self.refs = [HistRef(s, grep, match) for s in streams]
        self.eng = E.Engine(0, grep=grep, match=match)
        self.eng.set_streams(len(streams))
        for i, s in enumerate(streams):
            if s:
                self.eng.stage(i, s)
        self.r = self.eng.run(since=since, tail=tail, n_streams=len(streams))
        self.g = [r.gprime() for r in self.refs]  # the set self.r was selected from
        self.size_key = "matched" if self.patterned else "parsed"  # |H| among the result's counts

    def want(self, origin, w, n):
        return [ref.hist(g, origin, w, n) for ref, g in zip(self.refs, self.g)]

    def hist(self, origin, w, n, r=None, g=None, size_key=None):
        """One histogram of r (default: the session's result) over the flags g, checked; returns
        the reference's [(buckets, below, above)] per stream."""
        r = r or self.r
        g = g or self.g
        counts, outside = r.histogram(origin, w, n)
        assert counts.shape == (len(self.streams), n) and outside.shape == (len(self.streams), 2)
        assert counts.dtype == np.uint64 and outside.dtype == np.uint64
        want = []
        for i, ref in enumerate(self.refs):
            b, lo, hi = ref.hist(g[i], origin, w, n)
            tag = (i, origin, w, n)
            got = counts[i].tolist()
            assert got == b, (tag, [(k, x, y) for k, (x, y) in enumerate(zip(got, b)) if x != y][:8])
            assert (int(outside[i, 0]), int(outside[i, 1])) == (lo, hi), tag
            size = r.stream_counts(i)[size_key or self.size_key]
            assert lo + sum(got) + hi == size == sum(g[i]), (tag, size)
            want.append((b, lo, hi))
        return want

    def close(self):
        self.r.free()
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ------------------------------------------------------------------ 1. small, adversarial ---

# The guard's origin: the first instant of the cluster around 00:00:05 (the 4th of the 16
# instants).  From the median instant (00:00:09) one-second buckets hold one line only; from
# here, by the reference, both variants have lines below, above and in three buckets or more.
SMALL_ORG = po.parse_line(b"2024-10-22T00:00:04.999999999Z x")[0]


@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_small_adversarial(gpu, grep):
    data = b"".join(SMALL)
    with Session([data], grep=grep) as s:
        ref = s.refs[0]
        assert ref.n_lines == 20 and ref.n_parsed == 17
        instants = sorted({t for t in ref.ts if t is not None})
        assert len(instants) == 16 and SMALL_ORG in instants
        (b, lo, hi), = s.hist(SMALL_ORG, NS, 64)
        assert lo > 0 and hi > 0 and sum(1 for x in b if x) >= 3
        origins = sorted({shift(t, d) for t in instants for d in (-1, 0, 1)})
        for n in (1, 2, 64, 65536):
            for w in (1, 7, NS, 3600 * NS, ((1 << 63) - 1) // n):
                for org in origins:
                    s.hist(org, w, n)
        for n, w in ((1, 1), (65536, ((1 << 63) - 1) // 65536), (64, 3600 * NS)):
            (b, lo, hi), = s.hist((I64_MIN, 0), w, n)
            assert (sum(b), lo, hi) == (0, 0, sum(s.g[0]))       # every line above
            (b, lo, hi), = s.hist((I64_MAX, 999999999), w, n)
            assert (sum(b), lo, hi) == (0, sum(s.g[0]), 0)       # every line below
            s.hist((I64_MAX - 5, 0), w, n)                       # the end leaves int64: nothing is above
            s.hist((I64_MIN, 999999999), w, n)


# ------------------------------------------------- 2. stream boundaries inside a bitmap word ---

@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_stream_boundaries_in_a_word(gpu, grep):
    streams = _based_streams()
    with Session(streams, grep=grep) as s:
        assert sum(r.n_lines for r in s.refs) < 1200  # ~3 lines a stream: several streams per word
        want = s.hist((synth.T0, 0), 20 * 60 * NS, 8)
        spread = sum(1 for b, lo, hi in want if sum(1 for x in b if x) >= 2)
        assert spread > (10 if grep else 100), spread  # (HIT: about one line in eight)
        s.hist((synth.T0, 1), 20 * 60 * NS, 8)          # every line one bucket down, line 0 below
        s.hist((synth.T0 + 20 * 60, 0), 20 * 60 * NS + 1, 2)


# ------------------------------------------------------------------ 3. word and chunk edges ---

@pytest.fixture(scope="module")
def carry_session(gpu):
    big = b"".join(_carry_ts(i) + b"line %05d padding ....\n" % i for i in range(CARRY_N))
    second = b"".join(_carry_ts(i) + b"second %d\n" % i for i in range(40))
    assert len(big) > 1_000_000
    s = Session([big, second])
    yield s
    s.close()


def test_one_line_a_bucket(carry_session):
    s = carry_session
    (b0, lo0, hi0), (b1, lo1, hi1) = s.hist((synth.T0, 0), NS, CARRY_N)
    assert b0 == [1] * CARRY_N and (lo0, hi0) == (0, 0)
    assert b1 == [1] * 40 + [0] * (CARRY_N - 40)


@pytest.mark.parametrize("edge", [31, 32, 33, 8191, 8192, 8193])
def test_word_and_chunk_edges(carry_session, edge):
    s = carry_session
    org = (synth.T0 + edge, 0)
    assert s.refs[0].ts[edge] == org
    (b0, lo0, hi0), _ = s.hist(org, NS, CARRY_N)
    assert lo0 == edge and hi0 == 0 and b0[:CARRY_N - edge] == [1] * (CARRY_N - edge)
    for w in (64, 8192):
        n = (CARRY_N - edge + w - 1) // w
        (b0, lo0, hi0), _ = s.hist(org, w * NS, n)
        assert lo0 == edge and hi0 == 0 and b0[0] == w
        (b0, lo0, hi0), _ = s.hist(org, w * NS, n - 1)
        assert hi0 == (CARRY_N - edge) - (n - 1) * w
    s.hist(shift(org, 1), NS, 100)   # a nanosecond past the line: it is below
    s.hist(shift(org, -1), NS, 100)


# ------------------------------------------------------------------ 4. shuffled timestamps ---

SHUF_N = 20_000


def _shuffled_streams():
    """Three streams of SHUF_N canonical lines: seconds in a fixed-seed permutation (runs of one
    line, many keys per wave round); alternating between [0, 10000) and [10000, 20000); round
    robin over 64 ranges of 320 s."""
    perm = list(range(SHUF_N))
    random.Random(11).shuffle(perm)
    secs = [perm, [(i % 2) * 10000 + i // 2 for i in range(SHUF_N)], [(i % 64) * 320 + i // 64 for i in range(SHUF_N)]]
    return [b"".join(_carry_ts(x) + b"shuffled %d\n" % i for i, x in enumerate(col)) for col in secs]


def test_shuffled_timestamps(gpu):
    with Session(_shuffled_streams()) as s:
        t0 = (synth.T0, 0)
        one = s.hist(t0, 20480 * NS, 1)               # every line in one bucket
        assert [b for b, lo, hi in one] == [[SHUF_N]] * 3
        two = s.hist(t0, 10000 * NS, 2)               # stream 1 alternates between two buckets
        assert two[1][0] == [SHUF_N // 2] * 2
        rr = s.hist(t0, 320 * NS, 64)                 # stream 2: 64 buckets, round robin
        assert min(rr[2][0]) >= SHUF_N // 64 and rr[2][1:] == (0, 0)
        assert sum(1 for x in rr[0][0] if x) >= 62    # the permutation: every bucket, in any order
        s.hist(t0, 320 * NS + 1, 64)                  # the same through the 64-bit division
        s.hist((synth.T0 - 1, 999999999), 10**10 + 7, 2)
        s.hist((synth.T0 + 7, 0), 1_000_000_007, 9973)


# -------------------------------------- 5. every pattern mode, from a run with a partial index ---

@pytest.mark.parametrize("name", list(PATTERN_SETS))
def test_pattern_modes_from_a_partial_index(gpu, name):
    streams = [synth.generate(synth.TEXT, 21, 0, 150_000, permille=20),
               synth.generate(synth.JSON, 22, 1, 120_000, permille=20, drop_final_nl=True),
               synth.generate(synth.ADVERSARIAL, 23, 2, 6000, permille=40, drop_final_nl=True)]
    with Session(streams, since=(synth.T0 + 900, 0), tail=5, **PATTERN_SETS[name]) as s:
        want = s.hist((synth.T0, 0), 5 * 60 * NS, 12)
        total = sum(lo + sum(b) + hi for b, lo, hi in want)
        emitted = sum(s.r.stream_counts(i)["selected"] for i in range(3))
        assert emitted <= 15
        if name != "never":  # all of M, not the five emitted lines of each stream
            assert total > emitted
            assert sum(1 for k in range(12) if any(b[k] for b, lo, hi in want)) >= 6
        else:
            assert total == 0
        s.hist((synth.T0 + 900, 500), 7 * NS + 3, 300)


# ------------------------------------------------------------- 6. which set, and read-only ---

def test_which_set_and_read_only(gpu):
    streams = [synth.generate(synth.JSON, 41, 0, 300_000, permille=30),
               synth.generate(synth.ADVERSARIAL, 42, 1, 5000, permille=40, drop_final_nl=True)]
    since = (synth.T0 + 600, 0)
    a, b = (synth.T0 + 900, 0), (synth.T0 + 2000, 0)
    org, w, n = (synth.T0 + 300, 0), 4 * 60 * NS, 10
    with Session(streams, grep=[synth.NEEDLE], since=since, tail=3) as s:
        r = s.r
        before = [(r.stream(i).out, r.match_bits(i), r.group_bits(i), r.stream(i).counts) for i in range(2)]
        m_hist = s.hist(org, w, n)
        assert r.hist_ms > 0
        s.hist(org, 7, 3)  # repeated with other options
        assert before == [(r.stream(i).out, r.match_bits(i), r.group_bits(i), r.stream(i).counts) for i in range(2)]
        r2 = r.window(a, b, 1, 1)  # r was still the latest: no KLF_ESTATE
        g2 = [ref.cut(a, b, 1, 1) for ref in s.refs]
        assert 0 < sum(map(sum, g2)) and g2 != s.g
        assert s.hist(org, w, n, r=r2, g=g2) != m_hist  # G'', not M
        with pytest.raises(E.KlfError) as ei:  # r is not the latest any more
            r.histogram(org, w, n)
        assert ei.value.code == E.KLF_ESTATE
        r.free()
        r3 = r2.regroup(2, 1)
        g3 = [ref.group(2, 1) for ref in s.refs]
        assert g3 != g2 and g3 != s.g
        w3 = s.hist(org, w, n, r=r3, g=g3)
        r4 = r3.retail(1)
        assert s.hist(org, w, n, r=r4, g=g3) == w3
        r5 = r4.retail(-1)
        want = [ref.regroup(2, 1, False, -1, since)[0] for ref in s.refs]
        assert [r5.stream(i).out for i in range(2)] == want  # a histogram in between changed nothing
        for x in (r2, r3, r4):
            x.free()
        s.r = r5


@pytest.fixture(params=["sparse", "dense", None])
def compact(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("KLF_COMPACT", raising=False)
    else:
        monkeypatch.setenv("KLF_COMPACT", request.param)
    return request.param


def test_patternless_engine(gpu, compact):
    streams = [synth.generate(synth.TEXT, 71, 0, 200_000),
               synth.generate(synth.ADVERSARIAL, 72, 1, 4000, drop_final_nl=True)]
    org, w, n = (synth.T0 + 300, 0), 5 * 60 * NS, 9
    with Session(streams, since=(synth.T0 + 300, 0)) as s:
        if compact is None:
            assert s.r.compaction() == "one_pass"
        c = s.r.stream_counts(1)
        assert c["parsed"] < c["lines"] == c["matched"]  # G holds unparseable lines; H does not
        want = s.hist(org, w, n)                          # the sum is counts.parsed
        assert all(lo > 0 and hi > 0 for b, lo, hi in want)
        frm, until = (synth.T0 + 1000, 0), (synth.T0 + 2500, 0)
        r2 = s.r.window(frm, until)
        g2 = [ref.cut(frm, until) for ref in s.refs]
        assert 0 < sum(map(sum, g2)) < sum(map(sum, s.g))
        s.hist(org, w, n, r=r2, g=g2, size_key="matched")
        s.r.free()
        s.r = r2


# --------------------------------------------------------------- 7. errors on a live result ---

def _raw_hist(r, o, rows, n, counts=True, outside=True):
    c = np.full((rows, max(1, n)), 7, dtype=np.uint64)
    x = np.full((rows, 2), 7, dtype=np.uint64)
    rc = E.lib().klf_result_histogram(r._p, E.C.byref(o) if o is not None else None,
                                      E.C.c_void_p(c.ctypes.data) if counts else None,
                                      E.C.c_void_p(x.ctypes.data) if outside else None, None)
    return rc, c, x


def test_errors(gpu):
    # The streams of case 2, twice: a quarter of the 300 are empty and have no segment, and the
    # bound counts segments (227 * 65538 < 2^24 < 454 * 65538).
    streams = _based_streams() + _based_streams()
    segments = sum(1 for s in streams if s)
    assert segments * (65536 + 2) > 1 << 24 > segments * (4096 + 2)
    with Session(streams, grep=(b"HIT",)) as s:
        rows = len(streams)
        t0 = (synth.T0, 0)

        def intact():
            s.hist(t0, 20 * 60 * NS, 8)  # the next valid call is exact, the result as it was
            for i in (0, 5, rows - 1):
                assert s.r.group_bits(i) == HistRef.pack(s.g[i])

        for name, kw in BAD_OPTS.items():
            rc, c, x = _raw_hist(s.r, hist_opts(**kw), rows, 4)
            assert rc == E.KLF_EINVAL, name
            assert (c == 7).all() and (x == 7).all(), name  # nothing written
            intact()
        assert _raw_hist(s.r, None, rows, 4)[0] == E.KLF_EINVAL
        assert _raw_hist(s.r, hist_opts(), rows, 4, counts=False)[0] == E.KLF_EINVAL
        rc, c, x = _raw_hist(s.r, hist_opts(origin=t0, width_ns=20 * 60 * NS, n=8), rows, 8, outside=False)
        assert rc == E.KLF_OK and (x == 7).all()  # outside is optional
        assert [c[i].tolist() for i in range(rows)] == [b for b, lo, hi in s.want(t0, 20 * 60 * NS, 8)]
        with pytest.raises(E.KlfError) as ei:
            s.r.histogram(t0, NS, 65536)
        assert ei.value.code == E.KLF_ETOOBIG
        intact()
        s.hist(t0, NS, 4096)
        for wrong in (0, rows - 1, rows + 1):  # the binding sizes the arrays by the stream count it was given
            s.r.n_streams = wrong
            with pytest.raises(ValueError):
                s.r.histogram(t0, NS, 4)
        s.r.n_streams = rows
        intact()


# ------------------------------------------------------------------------------------- 8. CLI ---

def _rfc3339nano(t):
    d = datetime.datetime.fromtimestamp(t[0], datetime.timezone.utc)
    return d.strftime("%Y-%m-%dT%H:%M:%S") + ".%09dZ" % t[1]


def test_cli_histogram(gpu, tmp_path):
    bodies, rows = [], []
    for p in range(2):
        for cname in ("app", "sidecar"):
            data = synth.generate(synth.JSON, 61 + p, p * 2 + len(cname), 150_000 + 3000 * p, permille=100,
                                  drop_final_nl=(cname == "sidecar"))
            f = tmp_path / f"body_{p}_{cname}.log"
            f.write_bytes(data)
            bodies.append((f"pod-{p}", cname, data))
            rows.append((f"pod-{p}", "container", cname, str(f)))
    m = tmp_path / "manifest.tsv"
    m.write_text("".join("\t".join(r) + "\n" for r in rows))
    now = synth.T0 + synth.SPAN + 1
    frm = po.parse_line(b"2024-10-22T00:25:00.5Z x")[0]
    until = (now - 10 * 60, 0)
    base = ["--grep", synth.NEEDLE.decode(), "--from", "2024-10-22T00:25:00.5Z", "--until", "10m", "-t", "50",
            "--now", str(now), "--no-color", str(m)]
    plain, hist = tmp_path / "plain", tmp_path / "hist"
    for out, extra in ((plain, []), (hist, ["--histogram", "5m"])):
        r = subprocess.run([str(H.CLI), "-p", str(out)] + extra + base, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    names = sorted(H.log_file_name(p, c) for p, c, _ in bodies)
    assert sorted(os.listdir(plain)) == names and sorted(os.listdir(hist)) == sorted(names + ["histogram.tsv"])
    for nm in names:
        assert (hist / nm).read_bytes() == (plain / nm).read_bytes() != b"", nm
    w = 5 * 60 * NS
    span = (until[0] - frm[0]) * NS + until[1] - frm[1]
    n = (span + w - 1) // w
    want = ["Pod\tContainer\tBucket\tLines"]
    for pod, cname, data in bodies:
        ref = HistRef(data, grep=[synth.NEEDLE])
        b, lo, hi = ref.hist(ref.cut(frm, until), frm, w, n)
        assert (lo, hi) == (0, 0) and sum(b) >= 5 and sum(1 for x in b if x) >= 3
        want += [f"{pod}\t{cname}\t{_rfc3339nano(shift(frm, k * w))}\t{x}" for k, x in enumerate(b) if x]
    assert (hist / "histogram.tsv").read_text().splitlines() == want
    # without a window the rows `below` and `above` appear (lower edge: the --since instant)
    out = tmp_path / "since"
    r = subprocess.run([str(H.CLI), "-p", str(out), "-s", "40m", "--until", "30m", "--histogram", "150s", "--grep",
                        synth.NEEDLE.decode(), "--now", str(now), "--no-color", str(m)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    since, tail, rej = H.lop_opts("40m", -1, (now, 0))
    until2 = (now - 30 * 60, 0)
    want = ["Pod\tContainer\tBucket\tLines"]
    for pod, cname, data in bodies:
        ref = HistRef(data, grep=[synth.NEEDLE])
        b, lo, hi = ref.hist(ref.cut((E.TIME_MIN_SEC, 0), until2), since, 150 * NS, 4)
        assert lo > 0 and hi == 0
        want.append(f"{pod}\t{cname}\tbelow\t{lo}")
        want += [f"{pod}\t{cname}\t{_rfc3339nano(shift(since, k * 150 * NS))}\t{x}" for k, x in enumerate(b) if x]
    assert (out / "histogram.tsv").read_text().splitlines() == want
    # usage errors: no lower edge; a width of zero; more than 65536 buckets; an empty span
    for extra in (["--histogram", "5m"], ["--histogram", "0s", "--from", "30m"], ["--histogram", "1ms", "--from", "30m"],
                  ["--histogram", "5m", "--from", "10m", "--until", "20m"], ["--histogram", "soon", "--from", "30m"]):
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / "none")] + extra + ["--now", str(now), str(m)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "usage:" in r.stderr, extra
    assert not (tmp_path / "none").exists()
