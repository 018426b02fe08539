"""Every reachable k_scan variant, run once each (tests/scan_variants.py: the table of pattern
sets and knobs, and the input).  An entry reads the layout its run used from the KLF_DIAG
lines -- the prefilter layout line for general sets, the attempt line's grep_mode / fuse for
the plain, one-pass and literal scans -- asserts that it is the variant the entry names, and
compares every stream's selected bytes and counts with the C oracle, without and with
--since / --tail.  The input: three streams (a partial last tile; a tile group of 8 crossed and
no final newline; empty), needles across tile seams and in the last lines, one dense tile."""
import functools
import re

import pytest

import c_oracle as co
import scan_variants as sv
from klogs_amd import engine as E

pytestmark = pytest.mark.gpu

LAYOUT = re.compile(r"^\[klf\] prefilter layout from \d+ sampled bytes: (.*)$", re.M)
ATTEMPT = re.compile(r"^\[klf\] attempt (\d+) \S+ grep_mode=(\d+) .* fuse=(\d) .* -> (\w+)", re.M)
KNOBS = ("KLF_QF_TUNE", "KLF_QF_TWO", "KLF_QF_ANCHOR", "KLF_QF_QMAX", "KLF_FUSE")
FILTERS = [(co.GO_ZERO_TIME, -1), (sv.SINCE, 50)]
GREP_MODE = {"plain": 0, "one_pass": 0, "lit": 3, "gen": 4}  # GrepMode of klf_kernels.hpp


@functools.lru_cache(maxsize=None)
def case(name, dense=True):
    """(streams, {filter: [oracle result per stream]}) of an entry; computed once, never changed."""
    v = next(x for x in sv.TABLE if x.name == name)
    ss = sv.streams(v, dense)
    return ss, {f: [co.filter_stream(s, f[0], f[1], v.grep) for s in ss] for f in FILTERS}


def layout_of(text):
    """(stride, gram bytes, bits per gram, anchored) of the last layout line in text."""
    lay = LAYOUT.findall(text)[-1]
    m = re.search(r"S=(\d+) q=(\d+).* k=(\d+) ", lay)
    return int(m.group(1)), int(m.group(2)), int(m.group(3)), "anchored at" in lay


def run_and_check(eng, capfd, v, ss, want, f):
    r = eng.run(since=None if f[0] == co.GO_ZERO_TIME else f[0], tail=f[1], n_streams=len(ss))
    err = capfd.readouterr().err
    for i, (out, _, _, counts) in enumerate(want[f]):
        so = r.stream(i)
        assert so.out == out, (v.name, f, i)
        for k in ("lines", "parsed", "since_ok", "matched", "selected", "out_bytes"):
            assert so.counts[k] == counts[k], (v.name, f, i, k, so.counts, counts)
    mode = r.compaction()
    r.free()
    return err, mode


@pytest.mark.parametrize("v", sv.TABLE, ids=[v.name for v in sv.TABLE])
def test_variant(gpu, monkeypatch, capfd, v):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, val in v.env.items():
        monkeypatch.setenv(k, val)
    monkeypatch.setenv("KLF_DIAG", "1")
    ss, want = case(v.name)
    capfd.readouterr()
    with E.Engine(0, grep=v.grep) as eng:
        eng.set_streams(len(ss))
        for i, s in enumerate(ss):
            if s:
                eng.stage(i, s)
        seen = ""
        for f in FILTERS:
            err, mode = run_and_check(eng, capfd, v, ss, want, f)
            seen += err
            att = ATTEMPT.findall(err)
            assert att and att[-1][3] == "done", err
            assert all(int(a[1]) == GREP_MODE[v.mode] for a in att), (v.name, att)
            if v.mode == "plain":
                assert all(a[2] == "0" for a in att), att
            if v.mode == "one_pass" and f[1] == -1:  # (the dense tile voids the pass: the plain scan redoes it)
                assert att[0][2] == "1" and mode != "one_pass", (att, mode)
        if v.mode == "gen":
            assert layout_of(seen) == (v.S, v.q, v.k, v.anchored), (v.name, LAYOUT.findall(seen))
    if v.mode == "one_pass":  # without the dense tile the one-pass scan's own output stands
        ss, want = case(v.name, dense=False)
        with E.Engine(0) as eng:
            eng.set_streams(len(ss))
            for i, s in enumerate(ss):
                if s:
                    eng.stage(i, s)
            err, mode = run_and_check(eng, capfd, v, ss, want, FILTERS[0])
            assert mode == "one_pass" and ATTEMPT.findall(err)[-1][2:] == ("1", "done"), err
