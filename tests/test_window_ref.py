"""klf_window (SPEC.md S4b: a time window [from, until) over a finished run): the reference
the GPU tests compare against, built from the Python oracle's own pieces on top of
RegroupRef, an independent check of that reference, and the library's new ABI entries.
No GPU here."""
import ctypes as C
from pathlib import Path

import pytest

import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import synth
from test_regroup_ref import RegroupRef

ROOT = Path(__file__).resolve().parent.parent
GZ = po.GO_ZERO_TIME
OPEN_LO = (E.TIME_MIN_SEC, 0)
OPEN_HI = (E.TIME_MAX_SEC, 0)


class WindowRef(RegroupRef):
    """RegroupRef plus every line's instant: G'' = G' cut to [frm, until) by the definition."""

    def __init__(self, data: bytes, grep=(), match=()):
        super().__init__(data, grep, match)
        self.patterned = bool(list(grep) or list(match))
        self.ts = []
        for s, e in self.lines:
            p = po.parse_line(data[s:e])
            self.ts.append(p[0] if p is not None else None)

    def gprime(self, before=0, after=0, invert=False):
        if not self.patterned:
            assert not (before or after or invert)
            return list(self.parsed)
        return self.group(before, after, invert)

    def cut(self, frm, until, before=0, after=0, invert=False):
        g = self.gprime(before, after, invert)
        return [bool(g[i]) and self.ts[i] is not None and tuple(frm) <= tuple(self.ts[i]) < tuple(until)
                for i in range(self.n_lines)]

    def window(self, frm, until, before=0, after=0, invert=False, tail=-1, since=GZ):
        return self.emit(self.cut(frm, until, before, after, invert), tail, since)


def _golden():
    return sorted((ROOT / "tests" / "golden").glob("*.log"))


def _text_stream():
    return synth.generate(synth.TEXT, 3, 0, 40_000)


def _monotonic_stream():
    data = _text_stream()
    ref = WindowRef(data)
    assert ref.n_parsed == ref.n_lines > 100
    assert all(ref.ts[i] <= ref.ts[i + 1] for i in range(ref.n_lines - 1))
    return data, ref


def _cut_before(data, ref, until):
    """The stream cut before its first line with ts >= until."""
    for i, t in enumerate(ref.ts):
        if t >= until:
            return data[: ref.lines[i][0]]
    return data


def test_window_equals_filter_stream_of_the_cut_stream():
    data, ref = _monotonic_stream()
    n = ref.n_lines
    instants = [ref.ts[n // 10], ref.ts[n // 2], ref.ts[(9 * n) // 10], (ref.ts[n // 2][0], ref.ts[n // 2][1] + 1)]
    for since in (GZ, ref.ts[n // 3]):
        for until in instants:
            cut = _cut_before(data, ref, until)
            assert 0 < len(cut) < len(data)
            for frm in [OPEN_LO] + instants:
                lo = max(since, frm)
                want = po.filter_stream(cut, lo, -1, ())
                out, m, bits, nsel = ref.window(frm, until, tail=-1, since=since)
                assert out == want.out, (since, frm, until)
                assert nsel == want.n_selected
            for tail in (0, 1, 7, 100, 10**6):
                want = po.filter_stream(cut, since, tail, ())
                out, m, bits, nsel = ref.window(OPEN_LO, until, tail=tail, since=since)
                assert out == want.out and nsel == want.n_selected, (since, until, tail)
                assert m == want.n_lines  # |G''| = the lines before `until`


@pytest.mark.parametrize("tail", [-1, 0, 1, 7, 100])
def test_open_bounds_are_the_regroup(tail):
    assert _golden(), "tests/golden/*.log is missing"
    inputs = [(p.name, p.read_bytes()) for p in _golden()] + [("synthetic text", _text_stream())]
    for name, data in inputs:
        for grep in ([synth.NEEDLE], [b"e"]):
            ref = WindowRef(data, grep=grep)
            since = (synth.T0 + 600, 0) if name == "synthetic text" else GZ
            for before, after, invert in ((0, 0, False), (2, 1, False), (0, 0, True)):
                assert ref.window(OPEN_LO, OPEN_HI, before, after, invert, tail, since) == \
                    ref.regroup(before, after, invert, tail, since), (name, grep, before, after, invert)


def test_window_cuts_context_after_it_is_taken():
    ts = b"2024-10-22T00:00:%02dZ "
    lines = [ts % 0 + b"a\n", b"junk\n", ts % 2 + b"HIT\n", ts % 3 + b"b\n", ts % 4 + b"c\n", ts % 1 + b"late\n"]
    ref = WindowRef(b"".join(lines), grep=[b"HIT"])
    t = [po.parse_line(ts % i + b"x")[0] for i in range(6)]
    # the match (second 2) lies outside [3, 5) and still lends its context; line 5 is out of order
    assert ref.cut(t[3], t[5], 0, 3) == [False, False, False, True, True, False]
    assert ref.cut(t[1], t[3], 2, 3) == [False, False, True, False, False, True]
    assert ref.cut(t[3], t[3], 2, 3) == [False] * 6 and ref.cut(t[4], t[3], 2, 3) == [False] * 6
    nop = WindowRef(b"".join(lines))  # no patterns: the parsed lines
    assert nop.cut(OPEN_LO, OPEN_HI) == [True, False, True, True, True, True]
    assert nop.window(t[1], t[3], tail=1)[0] == b"late\n"


# ---------------------------------------------------------------- the library (no device) ---

def test_library_exports_window():
    lib = E.lib()
    assert hasattr(lib, "klf_window")
    assert "klf_window" in E.SIGNATURES
    hdr = (ROOT / "include" / "klf.h").read_text()
    for name in ("klf_window_opts", "KLF_TIME_MIN_SEC", "KLF_TIME_MAX_SEC"):
        assert name in hdr, name
    assert C.sizeof(E._WindowOpts) == 48
    assert (E.TIME_MIN_SEC, E.TIME_MAX_SEC) == (-(1 << 63), (1 << 63) - 1)


def test_window_null_arguments_are_einval():
    lib = E.lib()
    o = E._WindowOpts()
    r = C.c_void_p()
    assert lib.klf_window(None, None, C.byref(o), -1, C.byref(r)) == E.KLF_EINVAL
    assert lib.klf_window(None, None, None, -1, None) == E.KLF_EINVAL
