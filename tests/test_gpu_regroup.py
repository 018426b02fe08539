"""klf_regroup on the GPU (SPEC.md S4a): context lines and inverted match over a finished
run, against the reference of tests/test_regroup_ref.py (the Python oracle's pieces).  Each
case is one engine run and then many regroups."""
import os
import random
import subprocess

import pytest

import c_oracle as co
import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import host as H
from klogs_amd import synth
from test_regroup_ref import RegroupRef

pytestmark = pytest.mark.gpu

GZ = po.GO_ZERO_TIME
TS = b"2024-10-22T00:%02d:%02d.%09dZ "
COUNT_KEYS = ("lines", "parsed", "since_ok")


def ts(i):
    return TS % (i // 60 % 60, i % 60, i // 3600)


class Session:
    """One engine run over `streams`; every regroup is checked in full against the reference."""

    def __init__(self, streams, grep=(), match=(), since=None, tail=-1):
        self.streams = streams
        self.since = since
        self.refs = [RegroupRef(s, grep, match) for s in streams]
        self.mbits = [r.m_bits() for r in self.refs]
        self.eng = E.Engine(0, grep=grep, match=match)
        self.eng.set_streams(len(streams))
        for i, s in enumerate(streams):
            if s:
                self.eng.stage(i, s)
        self.r = self.eng.run(since=since, tail=tail, n_streams=len(streams))
        self.base = [self.r.stream_counts(i) for i in range(len(streams))]
        self.memo = {}

    def want(self, i, before, after, invert, tail):
        g = self.refs[i].group(before, after, invert)
        key = (i, RegroupRef.pack(g), tail)  # (many contexts select the same lines)
        if key not in self.memo:
            self.memo[key] = self.refs[i].emit(g, tail, self.since or GZ)
        return self.memo[key]

    def check(self, r, before, after, invert, tail, what=""):
        for i in range(len(self.streams)):
            out, n, gbits, nsel = self.want(i, before, after, invert, tail)
            tag = (what, i, before, after, invert, tail)
            so = r.stream(i)
            assert so.out == out, tag
            c = so.counts
            assert (c["matched"], c["selected"], c["out_bytes"]) == (n, nsel, len(out)), (tag, c)
            for k in COUNT_KEYS:
                assert c[k] == self.base[i][k], (tag, k, c, self.base[i])
            assert r.group_bits(i) == gbits, tag
            assert r.match_bits(i) == self.mbits[i], tag

    def regroup(self, before=0, after=0, invert=False, tail=-1):
        old, self.r = self.r, self.r.regroup(before, after, invert, tail)
        old.free()
        self.check(self.r, before, after, invert, tail)
        return self.r

    def close(self):
        self.r.free()
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ------------------------------------------------------------------ 1. small, adversarial ---

def _small(frag_matches):
    body = [b"not a timestamp HIT\n", b"\n"]                                     # 0, 1 unparseable
    body += [ts(2) + b"a HIT\n", ts(3) + b"b\n", ts(4) + b"c\n", ts(5) + b"d\n"]   # 2..5
    body += [b"junk in the middle HIT\n"]                                         # 6 unparseable
    body += [ts(7) + b"e\n", ts(8) + b"f HIT\n", ts(9) + b"g\n", ts(10) + b"h\n", ts(11) + b"i\n"]  # 7..11
    body += [b"2024-13-45T00:00:00Z bad month HIT\n"]                             # 12 unparseable, just before the end
    body += [ts(13) + (b"frag HIT" if frag_matches else b"frag")]                 # 13 trailing fragment
    return b"".join(body)


@pytest.mark.parametrize("frag_matches", [False, True])
def test_small_adversarial(gpu, frag_matches):
    data = _small(frag_matches)
    since = po.parse_line(ts(5) + b"x")[0]  # drops the first third
    with Session([data], grep=[b"HIT"], since=since, tail=-1) as s:
        assert s.refs[0].n_lines == 14 and s.refs[0].n_parsed == 10
        for invert in (False, True):
            for before in (0, 1, 2, 3, 50):
                for after in (0, 1, 2, 3, 50):
                    for tail in (-1, 0, 1, 3, 100):
                        s.regroup(before, after, invert, tail)


# ------------------------------------------------- 2. stream boundaries inside a bitmap word ---

def _tiny_streams(n=300, seed=4):
    rng = random.Random(seed)
    streams, k = [], 0
    for i in range(n):
        nl = rng.choice([0, 0, 1, 2, 3, 4, 5])
        lines = []
        for j in range(nl):
            k += 1
            hit = rng.random() < 0.12
            if i % 7 == 3 and j == nl - 1:
                hit = True   # the last line of one stream ...
            if i % 7 == 4 and j == 0:
                hit = True   # ... and the first line of the next
            head = ts(k) if rng.random() < 0.9 else b"noise "
            lines.append(head + (b"HIT %d\n" % k if hit else b"quiet %d\n" % k))
        body = b"".join(lines)
        if nl and rng.random() < 0.2:
            body = body[:-1]  # a trailing fragment
        streams.append(body)
    return streams


def test_stream_boundaries_in_a_word(gpu):
    streams = _tiny_streams()
    assert any(not s for s in streams) and sum(1 for s in streams if s) > 200
    with Session(streams, grep=[b"HIT"], tail=-1) as s:
        assert sum(r.n_lines for r in s.refs) < 1200  # ~3 lines a stream: several streams per word
        for before in (1, 2, 40):
            for after in (1, 2, 40):
                s.regroup(before, after, False, -1)
        s.regroup(40, 40, False, 2)
        s.regroup(1, 2, True, -1)
        s.regroup(0, 0, True, 1)


# ---------------------------------------------------------------- 3. word and chunk carries ---

CARRY_N = 3 * 8192 + 500
CARRY_HITS = (5, 8191, 8192, 24001)
CARRY_STEPS = (31, 32, 33, 8191, 8192, 8193, 20000, 2**32 - 1)


@pytest.fixture(scope="module")
def carry_session(gpu):
    big = b"".join(ts(i) + (b"HIT %05d padding .....\n" if i in CARRY_HITS else b"line %05d padding ....\n") % i
                   for i in range(CARRY_N))
    second = b"".join(ts(i) + (b"HIT second\n" if i == 0 else b"second %d\n" % i) for i in range(40))
    assert len(big) > 1_000_000
    s = Session([big, second], grep=[b"HIT"], tail=-1)
    assert [i for i, m in enumerate(s.refs[0].m) if m] == list(CARRY_HITS) and s.refs[1].m[0]
    yield s
    s.close()


@pytest.mark.parametrize("before", CARRY_STEPS)
def test_word_and_chunk_carries(carry_session, before):
    for after in CARRY_STEPS:
        carry_session.regroup(before, after, False, -1)
    carry_session.regroup(before, 0, False, 7)
    carry_session.regroup(0, before, False, 7)


def test_word_and_chunk_carries_inverted(carry_session):
    carry_session.regroup(0, 0, True, -1)
    carry_session.regroup(1, 1, True, -1)
    carry_session.regroup(1, 1, True, 9)


# ------------------------------------- 4. every pattern mode, from a run with a partial index ---

PATTERN_SETS = {
    "literal": dict(grep=[synth.NEEDLE]),
    "literal set": dict(grep=[synth.NEEDLE, b"backoff", b"cache miss"]),
    "regex set": dict(match=[b"(?i)err_conn_[a-z]+", b"(?i)TIMEOUT [a-z]+="]),
    "mixed": dict(grep=[b"backoff"], match=[b"(?i)err_conn", b"sen[dt]=[a-z]"]),
    "all": dict(grep=[b""]),
    "never": dict(grep=[b"a\nb"]),
}
# klf_result_index_mode of the --tail 5 run as the engine chooses it today: the sets it indexes
# by windows only must stay so (the regroup builds the rest on demand, it does not force it)
NOT_FULL = {"literal", "literal set", "regex set", "mixed"}


@pytest.mark.parametrize("name", list(PATTERN_SETS))
def test_pattern_modes_from_a_partial_index(gpu, name):
    pats = PATTERN_SETS[name]
    streams = [synth.generate(synth.TEXT, 21, 0, 150_000, permille=20),
               synth.generate(synth.JSON, 22, 1, 120_000, permille=20, drop_final_nl=True),
               synth.generate(synth.ADVERSARIAL, 23, 2, 6000, permille=40, drop_final_nl=True)]
    with Session(streams, since=(synth.T0 + 900, 0), tail=5, **pats) as s:
        mode = s.r.index_mode()
        nm = sum(sum(r.m) for r in s.refs)
        n_parsed = sum(r.n_parsed for r in s.refs)
        assert {"all": nm == n_parsed, "never": nm == 0}.get(name, 0 < nm < n_parsed), (nm, n_parsed)
        if name in NOT_FULL:
            assert mode != "full", mode
        s.regroup(2, 2, False, -1)
        s.regroup(0, 0, True, 5)
        s.regroup(2, 2, True, -1)
        s.regroup(2, 2, False, 5)


# --------------------------------------------------------------------------- 5. output growth ---

def test_output_growth(gpu):
    data = synth.generate(synth.JSON, 31, 0, 1_500_000, permille=10)
    since = (synth.T0 + 300, 0)
    with Session([data], grep=[synth.NEEDLE], since=since, tail=1) as s:
        assert 0 < sum(s.refs[0].m) < s.refs[0].n_lines // 20  # sparse
        assert len(s.r.stream(0).out) < 5000
        r = s.regroup(10**6, 10**6, False, -1)
        every = po.filter_stream(data, since, -1, ())
        assert s.refs[0].n_parsed == s.refs[0].n_lines
        so = r.stream(0)
        assert so.out == every.out and so.counts["selected"] == every.n_since > 1000


# ---------------------------------------------------------------------- 6. chaining and state ---

def test_chaining_and_state(gpu):
    streams = [synth.generate(synth.JSON, 41, 0, 300_000, permille=30),
               synth.generate(synth.ADVERSARIAL, 42, 1, 5000, permille=40, drop_final_nl=True)]
    since = (synth.T0 + 600, 0)
    with Session(streams, grep=[synth.NEEDLE], since=since, tail=3) as s:
        r1 = s.regroup(1, 1, False, -1)
        for t in (0, 1, 4, 100, -1):
            old, s.r = s.r, s.r.retail(t)  # re-tails over G'
            s.check(s.r, 1, 1, False, t, "retail")
            with pytest.raises(E.KlfError) as ei:
                old.stream(0)
            assert ei.value.code == E.KLF_ESTATE
            old.free()
        assert r1 is not s.r
        s.regroup(1, 1, False, -1)  # again on the regrouped result: from M, no compounding
        s.regroup(1, 1, False, 4)
        s.regroup(0, 0, False, 3)   # the identity: klf_retail(prev, 3) byte for byte
        for i, d in enumerate(streams):
            want = po.filter_stream(d, since, 3, po.compile_patterns([synth.NEEDLE]))
            assert s.r.stream(i).out == want.out and s.r.group_bits(i) == want.match_bits
        stale = s.r
        s.r = s.eng.run(since=since, tail=3, n_streams=len(streams))  # a fresh run: from its own matches
        with pytest.raises(E.KlfError) as ei:
            stale.regroup(1, 1)
        assert ei.value.code == E.KLF_ESTATE
        stale.free()
        for i, d in enumerate(streams):
            out, lo, bits, c = co.filter_stream(d, since, 3, [synth.NEEDLE])
            so = s.r.stream(i)
            assert so.out == out and so.counts["matched"] == c["matched"] and so.counts["selected"] == c["selected"]
            assert s.r.match_bits(i) == bits == s.mbits[i]
            assert s.r.group_bits(i) == bits  # never regrouped: M


# ---------------------------------------------------------------------------------- 7. errors ---

def test_errors(gpu):
    data = synth.generate(synth.JSON, 51, 0, 60_000, permille=50)
    with E.Engine(0) as eng:  # no patterns
        eng.set_streams(1)
        eng.stage(0, data)
        r = eng.run(tail=-1, n_streams=1)
        with pytest.raises(E.KlfError) as ei:
            r.regroup(1, 1)
        assert ei.value.code == E.KLF_EINVAL
        with pytest.raises(E.KlfError) as ei:
            r.group_bits(0)
        assert ei.value.code == E.KLF_EINVAL
        assert r.stream(0).out == po.filter_stream(data, GZ, -1, ()).out  # still the latest, untouched
        r.free()
    with E.Engine(0, grep=[synth.NEEDLE]) as eng:
        eng.set_streams(1)
        eng.stage(0, data)
        r = eng.run(tail=-1, n_streams=1)
        for kw in (dict(tail=-2), dict(flags=2), dict(flags=1 | 0x80000000)):
            with pytest.raises(E.KlfError) as ei:
                r.regroup(1, 1, **kw)
            assert ei.value.code == E.KLF_EINVAL, kw
        o = E._RegroupOpts(1, 1, 0, 7)  # _reserved != 0
        out = E.C.c_void_p()
        assert E.lib().klf_regroup(eng._h, r._p, E.C.byref(o), -1, E.C.byref(out)) == E.KLF_EINVAL
        assert E.lib().klf_regroup(eng._h, r._p, None, -1, E.C.byref(out)) == E.KLF_EINVAL
        r2 = r.regroup(1, 1)
        with pytest.raises(E.KlfError) as ei:  # r is not the latest any more
            r.regroup(1, 1)
        assert ei.value.code == E.KLF_ESTATE
        ref = RegroupRef(data, grep=[synth.NEEDLE])
        assert r2.stream(0).out == ref.regroup(1, 1)[0] != b""
        r.free()
        r2.free()


# ------------------------------------------------------------------------------------- 8. CLI ---

@pytest.mark.parametrize("invert", [False, True])
def test_cli_context_flags(gpu, tmp_path, invert):
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
    cmd = [str(H.CLI), "-p", str(out), "-s", "40m", "-t", "5", "--grep", synth.NEEDLE.decode(), "-C", "2"]
    cmd += ["--invert-match"] if invert else []
    r = subprocess.run(cmd + ["--now", str(now), "--no-color", str(m)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    since, tail, rej = H.lop_opts("40m", 5, (now, 0))
    assert not rej and tail == 5
    assert sorted(os.listdir(out)) == sorted(H.log_file_name(p, c) for p, c in bodies)
    for (p, c), data in bodies.items():
        want = RegroupRef(data, grep=[synth.NEEDLE]).regroup(2, 2, invert, tail, since)[0]
        assert want
        assert (out / H.log_file_name(p, c)).read_bytes() == want, (p, c)
    # the context flags need a pattern
    r = subprocess.run([str(H.CLI), "-p", str(tmp_path / "none"), "-C", "2", str(m)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "usage:" in r.stderr
