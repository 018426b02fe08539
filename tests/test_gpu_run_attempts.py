"""The attempts of a run ("The run on the host"): each case forces one redo path
with the knob that exists for it and reads, from the KLF_DIAG line that every attempt prints
after its readback, which outcomes the run went through -- the forcing tests elsewhere pass
as well when the forced path is silently not taken -- and checks every stream's output
against the C or the Python oracle."""
import functools
import re

import pytest

import c_oracle as co
import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import synth

pytestmark = pytest.mark.gpu

GZ = po.GO_ZERO_TIME
ATTEMPT = re.compile(r"^\[klf\] attempt (\d+) (\S+) .* -> (\w+)((?: \+\w+)*)$", re.M)


@functools.lru_cache(maxsize=None)
def text(n=300_000, seed=8):
    return synth.generate(synth.TEXT, seed, 0, n)  # 300 000 B: 37 tiles


@functools.lru_cache(maxsize=None)
def beside():
    return [b"", synth.generate(synth.ADVERSARIAL, 9, 1, 3000, drop_final_nl=True)]


def attempts(capfd):
    """(shape, outcome) of each attempt line printed since the last call, in order."""
    got = ATTEMPT.findall(capfd.readouterr().err)
    assert [int(g[0]) for g in got] == list(range(len(got))), got
    print("attempts:", [(g[1], g[2] + g[3]) for g in got])
    return [g[1] for g in got], [g[2] + g[3] for g in got]


def stage(eng, streams):
    eng.set_streams(len(streams))
    for i, s in enumerate(streams):
        if s:
            eng.stage(i, s)


def check_outputs(r, streams, tail, grep=(), match=()):
    pats = po.compile_patterns(list(grep), list(match)) if match else None
    for i, s in enumerate(streams):
        want = po.filter_stream(s, GZ, tail, pats).out if match else co.filter_stream(s, GZ, tail, list(grep))[0]
        assert r.stream(i).out == want, f"stream {i}"


def run_once(capfd, streams, tail=-1, grep=(), match=(), **kw):
    """A fresh engine's first run: its attempts, outputs checked; the result's compaction."""
    with E.Engine(0, grep=grep, match=match) as eng:
        stage(eng, streams)
        capfd.readouterr()
        r = eng.run(tail=tail, n_streams=len(streams), **kw)
        shapes, outs = attempts(capfd)
        check_outputs(r, streams, tail, grep, match)
        mode = r.compaction()
        r.free()
    return shapes, outs, mode


def test_underestimated_lines_rerun_exactly(gpu, monkeypatch, capfd):
    monkeypatch.setenv("KLF_DIAG", "1")
    monkeypatch.setenv("KLF_DEBUG_NL_SCALE", "0.0001")
    _, outs, _ = run_once(capfd, [text()] + beside(), tail=50)
    assert outs == ["done"]  # (the estimate's margin of 65 536 lines covers a 300 000-byte batch)
    dense = b"".join(b"2024-10-22T00:00:%02d.000000000Z x\n" % (i % 60) for i in range(60_000)) + b"\n" * 40_000
    _, outs, _ = run_once(capfd, [dense] + beside(), tail=50)  # 100 000 lines: past the margin
    assert outs == ["lines", "done"]


def test_pool_overflow(gpu, monkeypatch, capfd):
    monkeypatch.setenv("KLF_DIAG", "1")
    monkeypatch.setenv("KLF_DEBUG_POOL_CAP", "64")
    _, outs, _ = run_once(capfd, [text()] + beside(), grep=[synth.NEEDLE])
    assert outs == ["done"]  # (short lines: the record regions hold the slots, the pool only dense tiles')
    monkeypatch.setenv("KLF_WAVE_POOL", "1")  # every tile with two or more line starts takes pool slots
    _, outs, _ = run_once(capfd, [text()] + beside(), grep=[synth.NEEDLE])
    assert outs == ["lines", "done"]


def test_two_phase_first_run(gpu, monkeypatch, capfd):
    monkeypatch.setenv("KLF_DIAG", "1")
    monkeypatch.setenv("KLF_TWO_PHASE", "1")
    streams = [text()] + beside()
    with E.Engine(0) as eng:
        stage(eng, streams)
        capfd.readouterr()
        for shape in ("two-phase", "plain"):  # (the second run sizes by the first one's line density)
            r = eng.run(tail=20, n_streams=len(streams))
            assert attempts(capfd) == ([shape], ["done"])
            check_outputs(r, streams, 20)
            r.free()


def test_clamped_capacity_fails_every_attempt(gpu, monkeypatch, capfd):
    monkeypatch.setenv("KLF_DIAG", "1")
    monkeypatch.setenv("KLF_DEBUG_CAP_CLAMP", "40")
    rx = [rb"pod=\d+", rb"(?i)TIMEOUT \w+", rb"took \d+ms"]
    with E.Engine(0, match=rx) as eng:
        eng.stage(0, text())
        capfd.readouterr()
        with pytest.raises(E.KlfError) as ei:
            eng.run(n_streams=1)
        assert ei.value.code == E.KLF_ENOMEM
        _, outs = attempts(capfd)
        assert outs == ["lines", "lines"]
        monkeypatch.delenv("KLF_DEBUG_CAP_CLAMP")
        r = eng.run(n_streams=1)
        assert attempts(capfd)[1] == ["done"]
        check_outputs(r, [text()], -1, match=rx)
        r.free()


def test_match_fallback_then_whole_index(gpu, monkeypatch, capfd):
    monkeypatch.setenv("KLF_DIAG", "1")
    monkeypatch.setenv("KLF_HITS_CAP", "16")
    lits = synth.c4_literals(1024)[:300] + [b"ms"]
    _, outs, _ = run_once(capfd, [text()] + beside(), tail=50, grep=lits)
    assert outs == ["done"]  # (beside b"ms" the prefilter is off: k_match runs from the start)
    _, outs, _ = run_once(capfd, [text()] + beside(), tail=50, grep=lits[:-1])  # prefiltered: k_match skipped
    assert outs == ["match", "index", "done"]  # (the windowed index was on: a literal set)


def test_one_pass_voided(gpu, monkeypatch, capfd):
    monkeypatch.setenv("KLF_DIAG", "1")
    dense = b"".join(b"\n" if i % 3 else b"2024-10-22T00:00:00Z x\n" for i in range(30000))
    _, outs, mode = run_once(capfd, [dense])
    assert outs in (["fuse", "done"], ["lines", "fuse", "done"])
    assert mode != "one_pass"


def test_pair_set_grows(gpu, monkeypatch, capfd):
    monkeypatch.setenv("KLF_DIAG", "1")
    monkeypatch.setenv("KLF_PAIRS_LOG2", "4")
    d = text(200_000, 9)
    grep, match = [b"pod", b"ready", b"took"], [rb"sync\w*"]
    with E.Engine(0, grep=grep, match=match) as eng:
        eng.stage(0, d)
        capfd.readouterr()
        r = eng.run(n_streams=1, pattern_counts=True)
        _, outs = attempts(capfd)
        assert outs in (["pairs", "done"], ["pairs", "pairs", "done"])
        assert r.pattern_counts(0) == po.pattern_counts(d, po.compile_patterns(grep, match))
        check_outputs(r, [d], -1, grep, match)
        r.free()


def test_output_grown(gpu, monkeypatch, capfd):
    monkeypatch.setenv("KLF_DIAG", "1")
    monkeypatch.setenv("KLF_DEBUG_OUT_INIT", "4096")
    streams = [text(), text(50_000, 3), b"", text(120_000, 4), beside()[1]]
    _, outs, _ = run_once(capfd, streams, tail=10**9)
    assert outs == ["done +tcopy +grown"]  # (every line selected: the dense path, its copy deferred)
