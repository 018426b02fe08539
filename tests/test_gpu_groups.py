"""klf_result_groups on the GPU (SPEC.md S4e): the most frequent messages of a finished run,
against the reference of tests/test_groups_ref.py.  Every call is compared in full and exactly:
all entry records, the key bytes, n_groups and n_lines; with a `top` that holds every group,
the counts also add up to n_lines and to the result's own counts."""
import os
import random
import subprocess

import pytest

from klogs_amd import engine as E
from klogs_amd import host as H
from klogs_amd import synth
from test_gpu_regroup import PATTERN_SETS
from test_gpu_window import SMALL, _based_streams
from test_groups_ref import (BAD_OPTS, BIG_N, BY_HAND, GroupsRef, big_streams, cli_bodies, grouped, groups_opts,
                             odd_streams, render_tsv, sixty_four_keys, _ts)

pytestmark = pytest.mark.gpu

ALL = 65536  # a `top` that holds every group of the inputs here


class Session:
    """One engine run over `streams`; every groups call is checked in full against the reference."""

    def __init__(self, streams, grep=(), match=(), since=None, tail=-1):
        self.streams = streams
        self.patterned = bool(list(grep) or list(match))
        self.refs = [GroupsRef(s, grep, match) for s in streams]
        self.eng = E.Engine(0, grep=grep, match=match)
        self.eng.set_streams(len(streams))
        for i, s in enumerate(streams):
            if s:
                self.eng.stage(i, s)
        self.r = self.eng.run(since=since, tail=tail, n_streams=len(streams))
        self.g = [r.gprime() for r in self.refs]  # the set self.r was selected from
        self.size_key = "matched" if self.patterned else "parsed"  # |H| among the result's counts
        self.memo = {}

    def want(self, g, top, mask, max_key):
        key = (id(g), mask, max_key)  # (the reference groups once per selection and option pair)
        if key not in self.memo:
            self.memo[key] = (g, grouped(self.refs, g, 10**9, mask, max_key))
        ent, n_groups, n_lines = self.memo[key][1]
        return ent[:top], n_groups, n_lines

    def check(self, top=ALL, mask=False, max_key=0, max_groups=0, r=None, g=None, size_key=None):
        """One groups call on r (default: the session's result, selected from the flags g),
        checked in full; returns (entries, n_groups, n_lines) as the reference has them."""
        r = r or self.r
        g = g or self.g
        want, n_groups, n_lines = self.want(g, top, mask, max_key)
        with r.groups(top, mask, max_key, max_groups) as gr:
            ent = gr.entries
            assert ent.dtype == E.GROUP_ENTRY
            keys = gr.keys()
            got = [(int(e["count"]), int(e["first_stream"]), int(e["first_line"]), int(e["last_stream"]),
                    int(e["last_line"]), k) for e, k in zip(ent, keys)]
            tag = (top, mask, max_key)
            assert len(got) == len(want) == len(gr) == min(top, n_groups), (tag, len(got), len(want))
            assert got == want, (tag, [(k, a, b) for k, (a, b) in enumerate(zip(got, want)) if a != b][:4])
            assert (gr.n_groups, gr.n_lines) == (n_groups, n_lines), tag
            assert gr.key_bytes == b"".join(k for *_, k in want), tag  # packed in result order, nothing between
            assert [int(e["key_off"]) for e in ent] == [sum(len(k) for *_, k in want[:i]) for i in range(len(want))]
            assert not ent["_pad"].any()
            if top >= n_groups:
                size = sum(r.stream_counts(i)[size_key or self.size_key] for i in range(len(self.streams)))
                assert sum(x[0] for x in got) == n_lines == size, (tag, size)
            assert gr.ms >= 0
        return want, n_groups, n_lines

    def close(self):
        self.r.free()
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


GRID = [(top, mask, max_key) for top in (1, 2, ALL) for mask in (False, True) for max_key in (0, 1, 5, 7, 40)]


# ------------------------------------------------------------------ 1. small, adversarial ---

@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_small_adversarial(gpu, grep):
    with Session([b"".join(SMALL), b"".join(BY_HAND)], grep=grep) as s:
        assert [r.n_lines for r in s.refs] == [20, 9] and s.refs[0].n_parsed == 17
        for top, mask, max_key in GRID:
            s.check(top, mask, max_key)
        ent, n_groups, n_lines = s.check(mask=True, max_key=5)
        if not grep:
            assert (3, 1, 0, 1, 7, b"ab#") in ent  # cut to 5 bytes, then masked
            assert (2, 0, 10, 1, 6, b"") not in ent and any(k == b"" for *_, k in ent)  # the empty key is a key
            ties = [x for x in s.check()[0] if x[0] == 2]
            assert len(ties) >= 2 and [x[1:3] for x in ties] == sorted(x[1:3] for x in ties)  # ties: by first
    with Session([b"".join(BY_HAND)]) as s:  # the by-hand case alone, as the reference test pins it
        assert s.check()[0][:2] == [(2, 0, 3, 0, 6, b""), (2, 0, 5, 0, 8, b"zz top")]
        assert s.check(2, True, 5)[0] == [(3, 0, 0, 0, 7, b"ab#"), (2, 0, 3, 0, 6, b"")]


# ------------------------------------------------- 2. stream boundaries inside a bitmap word ---

@pytest.mark.parametrize("grep", [(), (b"HIT",)])
def test_stream_boundaries_in_a_word(gpu, grep):
    streams = _based_streams()
    with Session(streams, grep=grep) as s:
        assert sum(r.n_lines for r in s.refs) < 1200  # ~3 lines a stream: several streams per word
        ent, n_groups, n_lines = s.check(mask=True)
        assert any(fs != ls for _, fs, _, ls, _, _ in ent)  # a group whose first and last line lie in two streams
        assert n_groups <= 3 and n_lines > (20 if grep else 500)
        s.check(mask=False)
        s.check(3, True, 4)


# ------------------------------------------- 3. more than one chunk, and a wave's rounds ---

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
    ent, n_groups, n_lines = s.check(mask=True)
    assert n_lines > 6000 and (n_groups > 340 if s.name == "no patterns" else 90 <= n_groups <= 110)
    ent, n_plain, _ = s.check(mask=False)
    assert n_plain > 4 * n_groups
    s.check(10, True)
    s.check(ALL, True, 12)
    s.check(1, False, 30)


# ------------------------------------------- 3a. the sort at its block boundaries ---

def _sort_size_streams(n_groups):
    """n_groups distinct keys whose counts cycle over 2, 1, 3, 1, 1, so that the order is decided
    partly by count and partly by first line: every group once in a shuffled order, then the
    further lines of the groups with more than one, shuffled again; cut into two streams."""
    rng = random.Random(n_groups)
    first = list(range(n_groups))
    rng.shuffle(first)
    more = [g for g in range(n_groups) for _ in range((2, 1, 3, 1, 1)[g % 5] - 1)]
    rng.shuffle(more)
    lines = [_ts(i) + b"grp %05d seen\n" % g for i, g in enumerate(first + more)]
    cut = max(1, len(lines) * 2 // 5)
    return [b"".join(lines[:cut]), b"".join(lines[cut:])]


@pytest.mark.parametrize("n_groups", [1, 2047, 2048, 2049, 4097])  # one item; T - 1, T, T + 1, 2 T + 1 for kTlSortBlock
def test_sort_sizes(gpu, n_groups):
    with Session(_sort_size_streams(n_groups)) as s:
        ent, n, n_lines = s.check(top=ALL, mask=False)
        assert n == len(ent) == n_groups <= ALL and n_lines == sum(x[0] for x in ent)
        assert {x[0] for x in ent} == ({2} if n_groups == 1 else {1, 2, 3})
        assert any(x[1] != x[3] for x in ent)  # a group with lines in both streams


# ------------------------------------------------------------------------- 4. collisions ---

@pytest.mark.parametrize("bits", ["1", "4", "12"])
def test_hash_collisions_change_nothing(big_session, bits, monkeypatch):
    s = big_session
    monkeypatch.delenv("KLF_GROUPS_HASH_BITS", raising=False)
    full = [s.check(mask=True), s.check(mask=False), s.check(7, True, 9)]
    old = os.environ.get("KLF_GROUPS_HASH_BITS")
    os.environ["KLF_GROUPS_HASH_BITS"] = bits
    try:
        assert s.check(mask=True)[1] <= 2000 and s.check(mask=False)[1] <= 2000
        got = [s.check(mask=True), s.check(mask=False), s.check(7, True, 9)]
    finally:
        if old is None:
            del os.environ["KLF_GROUPS_HASH_BITS"]
        else:
            os.environ["KLF_GROUPS_HASH_BITS"] = old
    assert got == full


# ----------------------------------------------------------------------- 5. table bounds ---

def test_table_bounds(gpu):
    with Session(sixty_four_keys()) as s:
        for _ in range(2):  # the same on repeated calls
            assert s.check(mask=True, max_groups=64)[1] == 64
            with pytest.raises(E.KlfError) as ei:
                s.r.groups(ALL, True, 0, 63)
            assert ei.value.code == E.KLF_ETOOBIG and "max_groups" in str(ei.value)
        with pytest.raises(E.KlfError) as ei:  # without the mask there are more keys than 64
            s.r.groups(ALL, False, 0, 64)
        assert ei.value.code == E.KLF_ETOOBIG
        with pytest.raises(E.KlfError) as ei:  # far more keys than slots: the table runs full
            s.r.groups(ALL, False, 0, 2)
        assert ei.value.code == E.KLF_ETOOBIG
        assert s.check(mask=True, max_key=3, max_groups=1)[1] == 1  # one key, a table for one
        s.check(5, True, 0, 64)  # after KLF_ETOOBIG the result is valid and the next call exact
        s.check(mask=False)


# ------------------------------------------------------------------ 6. long and odd lines ---

@pytest.mark.parametrize("max_key", [0, 100])
def test_long_and_odd_lines(gpu, max_key):
    streams = odd_streams()
    with Session(streams) as s:
        assert len(streams[0]) % 256 == 0 and not streams[1].endswith(b"\n")
        lens = {e - b for r in s.refs for b, e in r.lines}
        assert max(lens) > 70_000
        for mask in (False, True):
            ent, n_groups, n_lines = s.check(mask=mask, max_key=max_key)
            keys = [k for *_, k in ent]
            if mask:
                assert b"tail #" in keys  # the unterminated last line, its digit run at the very end
                assert b"# begins with digits" in keys
            if mask and not max_key:  # the seam: the fragment's digit run ends where the stream ends
                assert [x[:5] for x in ent if x[5].endswith(b"end #")] == [(2, 0, s.refs[0].n_lines - 1, 1, 1)]
            if not max_key:
                assert any(len(k) == 70_000 for k in keys) and b"" in keys
                assert sum(1 for k in keys if len(k) == 4096) == 2  # they differ in the last byte only
            s.check(3, mask, max_key)


# ------------------------------------------------------------- 7. composition, read-only ---

def test_composition_and_read_only(gpu):
    streams = [synth.generate(synth.TEXT, 31, 0, 200_000, permille=60),
               synth.generate(synth.ADVERSARIAL, 32, 1, 5000, permille=60, drop_final_nl=True)]
    a, b = (synth.T0 + 900, 0), (synth.T0 + 2000, 0)
    with Session(streams, grep=[synth.NEEDLE, b"cache miss"], since=(synth.T0 + 600, 0), tail=3) as s:
        r = s.r

        def state(x):
            return [(x.stream(i).out, x.match_bits(i), x.group_bits(i), x.stream(i).counts) for i in range(2)]

        before = state(r)
        first = s.check(mask=True)
        r.histogram((synth.T0, 0), 60 * 10**9, 30)
        assert s.check(mask=True) == first and first[1] > 1  # groups, histogram, groups again
        s.check(5, False, 20)
        assert state(r) == before
        lib, out = E.lib(), E.C.c_void_p()
        for name, kw in BAD_OPTS.items():
            o = groups_opts(**kw)
            assert lib.klf_result_groups(r._p, E.C.byref(o), E.C.byref(out)) == E.KLF_EINVAL, name
            assert out.value is None
        assert lib.klf_result_groups(r._p, None, E.C.byref(out)) == E.KLF_EINVAL
        o = groups_opts()
        assert lib.klf_result_groups(r._p, E.C.byref(o), None) == E.KLF_EINVAL
        r1 = r.retail(-1)  # a re-tail: H is unchanged
        assert s.check(mask=True, r=r1) == first
        r2 = r1.window(a, b)  # groups over G''
        g2 = [ref.cut(a, b) for ref in s.refs]
        cut = s.check(mask=True, r=r2, g=g2)
        assert 0 < cut[2] < first[2]
        with pytest.raises(E.KlfError) as ei:  # r1 is not the latest any more
            r1.groups(5)
        assert ei.value.code == E.KLF_ESTATE
        r3 = r2.regroup(0, 0, True)  # groups over G': what else is in there
        g3 = [ref.group(0, 0, True) for ref in s.refs]
        inv = s.check(mask=True, r=r3, g=g3)
        assert inv[2] + first[2] == sum(ref.n_parsed for ref in s.refs)
        keep = r3.groups(4, True)
        kept = (keep.entries.tolist(), keep.keys(), keep.n_groups, keep.n_lines)
        assert len(kept[0]) == 4
        for x in (r, r1, r2, r3):
            x.free()
        # a Groups object outlives the next run and a reset
        s.r = s.eng.run(since=None, tail=1, n_streams=2)
        assert (keep.entries.tolist(), keep.keys(), keep.n_groups, keep.n_lines) == kept
        assert s.check(mask=True) == first
        s.r.free()
        s.eng.reset()
        for i, d in enumerate(streams):
            s.eng.stage(i, d)
        assert (keep.entries.tolist(), keep.keys(), keep.n_groups, keep.n_lines) == kept
        keep.free()
        s.r = s.eng.run(since=None, tail=-1, n_streams=2)
        assert s.check(mask=True) == first


# ---------------------------------------------------------------------------- 8. empty ---

def test_empty_and_streams_without_bytes(gpu):
    with Session([b"".join(SMALL), b"".join(BY_HAND)], grep=[b"matches nothing at all"]) as s:
        assert s.check() == ([], 0, 0)
        with s.r.groups(1, True) as gr:
            assert len(gr) == 0 and gr.keys() == [] and gr.key_bytes == b"" and (gr.n_groups, gr.n_lines) == (0, 0)
    # streams without bytes among streams with bytes: the entries name streams, not segments
    streams = [b"", b"".join(BY_HAND[:2]), b"", b"", b"".join(BY_HAND[3:]), b""]
    with Session(streams) as s:
        ent, n_groups, n_lines = s.check()
        assert {x[1] for x in ent} | {x[3] for x in ent} == {1, 4}
        s.check(2, True, 5)
    with Session([b"", b"junk\n", b""]) as s:  # no parsed line
        assert s.check(mask=True) == ([], 0, 0)
    eng = E.Engine(0)
    eng.set_streams(2)
    r = eng.run(n_streams=2)  # no stream has bytes
    with r.groups(3) as gr:
        assert len(gr) == 0 and (gr.n_groups, gr.n_lines) == (0, 0) and gr.keys() == []
    r.free()
    eng.close()


# ------------------------------------------------------------------------------- 9. CLI ---

def test_cli_top(gpu, tmp_path):
    bodies, rows = cli_bodies(), []
    for pod, cname, data in bodies:
        f = tmp_path / f"body_{pod}_{cname}.log"
        f.write_bytes(data)
        rows.append((pod, "container", cname, str(f)))
    m = tmp_path / "manifest.tsv"
    m.write_text("".join("\t".join(r) + "\n" for r in rows))
    now = synth.T0 + synth.SPAN + 1
    base = ["--grep", "e", "-t", "20", "--now", str(now), "--no-color", str(m)]
    for name, extra in (("plain", []), ("top", ["--top", "5", "--top-mask-digits"]),
                        ("cut", ["--top", "3", "--top-key-bytes", "12"])):
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / name)] + extra + base, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
    names = sorted(H.log_file_name(p, c) for p, c, _ in bodies)
    assert sorted(os.listdir(tmp_path / "plain")) == names  # without --top: no top.tsv
    refs = [GroupsRef(data, grep=[b"e"]) for _, _, data in bodies]
    flags = [ref.gprime() for ref in refs]
    pc = [(p, c) for p, c, _ in bodies]
    for name, top, mask, max_key in (("top", 5, True, 0), ("cut", 3, False, 12)):
        assert sorted(os.listdir(tmp_path / name)) == sorted(names + ["top.tsv"])
        for nm in names:
            assert (tmp_path / name / nm).read_bytes() == (tmp_path / "plain" / nm).read_bytes() != b"", nm
        ent, n_groups, n_lines = grouped(refs, flags, top, mask, max_key)
        assert len(ent) == top and n_lines > 100  # taken before --tail 20
        assert (tmp_path / name / "top.tsv").read_bytes() == render_tsv(ent, pc)
    # usage errors: K outside 1..65536, the other two flags without --top
    for extra in (["--top", "0"], ["--top", "65537"], ["--top", "-3"], ["--top", "many"], ["--top-mask-digits"],
                  ["--top-key-bytes", "8"], ["--top", "5", "--top-key-bytes", "x"]):
        r = subprocess.run([str(H.CLI), "-p", str(tmp_path / "none")] + extra + base, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 1 and "usage:" in r.stderr, extra
    assert not (tmp_path / "none").exists()
