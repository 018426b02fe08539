"""klf_regroup (SPEC.md S4a: context lines and inverted match over a finished run): the
reference the GPU tests compare against, built from the Python oracle's own pieces, and the
library's new ABI entries.  No GPU here."""
import ctypes as C
from pathlib import Path

import pytest

import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import synth

ROOT = Path(__file__).resolve().parent.parent
GZ = po.GO_ZERO_TIME


class RegroupRef:
    """One stream's line table and match set M (computed once), then any number of regroups."""

    def __init__(self, data: bytes, grep=(), match=()):
        pats = po.compile_patterns(grep, match)
        self.data = data
        self.lines = po.split_lines(data)
        self.parsed = []
        self.m = []
        for s, e in self.lines:
            p = po.parse_line(data[s:e])
            self.parsed.append(p is not None)
            self.m.append(p is not None and any(pt.matches(po.content_for_match(p[1])) for pt in pats))
        self.n_lines = len(self.lines)
        self.n_parsed = sum(self.parsed)

    @staticmethod
    def pack(flags) -> bytes:
        bits = bytearray((len(flags) + 7) // 8)
        for i, f in enumerate(flags):
            if f:
                bits[i >> 3] |= 1 << (i & 7)
        return bytes(bits)

    def m_bits(self) -> bytes:
        return self.pack(self.m)

    def group(self, before=0, after=0, invert=False):
        """G' by the definition: the parsed lines l with some m in S, l - after <= m <= l + before."""
        n = self.n_lines
        s = [self.parsed[i] and not self.m[i] for i in range(n)] if invert else self.m
        g = [False] * n
        for mi in range(n):  # plain loop over S, marking each line's context (clipped to the stream)
            if s[mi]:
                for l in range(max(0, mi - before), min(n, mi + after + 1)):
                    g[l] = True
        return [g[i] and self.parsed[i] for i in range(n)]

    def emit(self, g, tail=-1, since=GZ):
        """(out bytes, |G'|, packed G' bits, selected lines) of the selection flags g"""
        gfile = b"".join(self.data[s:e] for (s, e), f in zip(self.lines, g) if f)
        out = po.read_logs(gfile, tail, since)
        if self.data.endswith(b"\n"):  # every emitted content ends its line: count them
            nsel = out.count(b"\n")
        else:  # (a selected fragment may have no content at all)
            nsel = po._count_selected(gfile, tail, since)
        return out, sum(g), self.pack(g), nsel

    def regroup(self, before=0, after=0, invert=False, tail=-1, since=GZ):
        return self.emit(self.group(before, after, invert), tail, since)


def _text_stream():
    return synth.generate(synth.TEXT, 3, 0, 40_000)


def _golden():
    return sorted((ROOT / "tests" / "golden").glob("*.log"))


def _inputs():
    return [(p.name, p.read_bytes()) for p in _golden()] + [("synthetic text", _text_stream())]


@pytest.mark.parametrize("tail", [-1, 0, 1, 7, 100])
def test_identity_equals_filter_stream(tail):
    assert _golden(), "tests/golden/*.log is missing"
    for name, data in _inputs():
        for grep in ([synth.NEEDLE], [b"timeout"], [b"e"], [b" "]):
            ref = RegroupRef(data, grep=grep)
            since = (synth.T0 + 600, 0) if name == "synthetic text" else GZ
            want = po.filter_stream(data, since, tail, po.compile_patterns(grep))
            out, n, bits, nsel = ref.regroup(0, 0, False, tail, since)
            assert out == want.out, (name, grep)
            assert n == want.n_matched, (name, grep)
            assert bits == want.match_bits, (name, grep)
            assert nsel == want.n_selected, (name, grep)
            assert (ref.n_lines, ref.n_parsed) == (want.n_lines, want.n_parsed)


def test_invert_of_all_is_nothing():
    for name, data in _inputs():
        ref = RegroupRef(data, grep=[b""])
        assert sum(ref.m) == ref.n_parsed
        for b, a in ((0, 0), (3, 2)):
            out, n, bits, nsel = ref.regroup(b, a, True, -1)
            assert (out, n, nsel) == (b"", 0, 0), name
            assert bits == bytes(len(bits))


def test_invert_of_never_is_the_patternless_run():
    data = _text_stream()
    ref = RegroupRef(data, grep=[b"a\nb"])
    assert ref.n_parsed == ref.n_lines and not any(ref.m)  # no unparseable line
    for tail in (-1, 0, 1, 7, 100):
        since = (synth.T0 + 600, 0)
        want = po.filter_stream(data, since, tail, ())
        out, n, _, nsel = ref.regroup(0, 0, True, tail, since)
        assert out == want.out and n == want.n_matched and nsel == want.n_selected


def test_context_is_clipped_and_skips_unparseable_lines():
    ts = b"2024-10-22T00:00:%02dZ "
    lines = [ts % 0 + b"a\n", b"junk\n", ts % 2 + b"HIT\n", ts % 3 + b"b\n", b"junk2\n", ts % 5 + b"c\n", ts % 6 + b"d"]
    ref = RegroupRef(b"".join(lines), grep=[b"HIT"])
    assert ref.group(0, 0) == [False, False, True, False, False, False, False]
    assert ref.group(1, 0) == [False, False, True, False, False, False, False]  # the line before is unparseable
    assert ref.group(2, 0) == [True, False, True, False, False, False, False]   # distances count it all the same
    assert ref.group(0, 3) == [False, False, True, True, False, True, False]
    assert ref.group(50, 50) == [True, False, True, True, False, True, True]
    assert ref.group(0, 0, True) == [True, False, False, True, False, True, True]
    out, n, bits, nsel = ref.regroup(0, 3, False, 2)
    assert out == b"b\nc\n" and n == 3 and nsel == 2 and bits == bytes([0b0101100])


# ---------------------------------------------------------------- the library (no device) ---

def test_library_exports_regroup():
    lib = E.lib()
    for name in ("klf_regroup", "klf_result_group_bits"):
        assert hasattr(lib, name), name
        assert name in E.SIGNATURES, name
    hdr = (ROOT / "include" / "klf.h").read_text()
    assert "KLF_REGROUP_INVERT" in hdr and "klf_regroup_opts" in hdr
    assert E.KLF_REGROUP_INVERT == 1
    assert C.sizeof(E._RegroupOpts) == 16


def test_regroup_null_arguments_are_einval():
    lib = E.lib()
    o = E._RegroupOpts()
    r = C.c_void_p()
    assert lib.klf_regroup(None, None, C.byref(o), -1, C.byref(r)) == E.KLF_EINVAL
    assert lib.klf_regroup(None, None, None, -1, None) == E.KLF_EINVAL
    assert lib.klf_result_group_bits(None, 0, None, None) == E.KLF_EINVAL
