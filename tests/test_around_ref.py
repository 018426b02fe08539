"""klf_around (SPEC.md S4g: time context across streams over a finished run): the reference the
GPU tests compare against, built over a list of streams from WindowRef, an independent brute
force of the definition that checks it, the set's basic facts, and the library's new ABI
entries.  No GPU here."""
import bisect
import ctypes as C
from pathlib import Path

import pytest

import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import synth
from test_window_ref import OPEN_HI, OPEN_LO, WindowRef

ROOT = Path(__file__).resolve().parent.parent
GZ = po.GO_ZERO_TIME
NS = 10**9
MAX_NS = E.AROUND_MAX_NS  # KLF_AROUND_MAX_NS: the largest duration


def ns_of(t):
    """The instant (sec, nsec) as one Python integer of nanoseconds (unbounded: no overflow)."""
    return t[0] * NS + t[1]


class AroundRef:
    """The streams of one run, each a WindowRef (line table, M, every line's instant), and over
    them the anchors A and the selections G' / G'' of any number of `around` calls."""

    def __init__(self, streams, grep=(), match=(), refs=None):
        self.refs = list(refs) if refs is not None else [WindowRef(s, grep, match) for s in streams]
        self._anchors = None

    def anchors(self):
        """The instants of M of all streams, ascending, in nanoseconds (every line of M is parsed)."""
        if self._anchors is None:
            self._anchors = sorted(ns_of(r.ts[i]) for r in self.refs for i in range(r.n_lines) if r.m[i])
        return self._anchors

    def group(self, before_ns=0, after_ns=0):
        """G' as flags per line, per stream: ts(a) - before <= ts(l) <= ts(a) + after for some a,
        that is, the first anchor at or above ts(l) - after lies at or below ts(l) + before."""
        a = self.anchors()
        out = []
        for r in self.refs:
            g = []
            for i in range(r.n_lines):
                if r.ts[i] is None:
                    g.append(False)
                    continue
                t = ns_of(r.ts[i])
                k = bisect.bisect_left(a, t - after_ns)
                g.append(k < len(a) and a[k] <= t + before_ns)
            out.append(g)
        return out

    def cut(self, before_ns=0, after_ns=0, frm=OPEN_LO, until=OPEN_HI):
        """G'' = G' cut to [frm, until), S4b's rule."""
        return [[f and tuple(frm) <= tuple(r.ts[i]) < tuple(until) for i, f in enumerate(g)]
                for r, g in zip(self.refs, self.group(before_ns, after_ns))]

    def around(self, before_ns=0, after_ns=0, frm=OPEN_LO, until=OPEN_HI, tail=-1, since=GZ):
        """Per stream (out bytes, |G''|, packed G'' bits, selected lines), as WindowRef.window."""
        return [r.emit(g, tail, since) for r, g in zip(self.refs, self.cut(before_ns, after_ns, frm, until))]


def brute_group(refs, before_ns, after_ns):
    """The definition, O(lines x anchors), on (sec, nsec) pairs with a carry and a borrow written
    out (nothing shared with AroundRef.group but the line tables)."""
    def add(t, d):
        s, n = t[0] + d // NS, t[1] + d % NS
        return (s + 1, n - NS) if n >= NS else (s, n)

    def sub(t, d):
        s, n = t[0] - d // NS, t[1] - d % NS
        return (s - 1, n + NS) if n < 0 else (s, n)

    anchors = [tuple(r.ts[i]) for r in refs for i in range(r.n_lines) if r.m[i]]
    return [[r.ts[i] is not None and any(sub(a, before_ns) <= tuple(r.ts[i]) <= add(a, after_ns) for a in anchors)
             for i in range(r.n_lines)] for r in refs]


def _golden():
    return sorted((ROOT / "tests" / "golden").glob("*.log"))


def three_streams():
    """api logs ERR_CONN_RESET 40 ms after the restart line of sidecar; db is quiet, unordered and
    has an unparseable line; instants on both sides of a second and equal across streams."""
    api = (b"2024-10-22T00:00:00.900000000Z GET /a 200\n"
           b"2024-10-22T00:00:01.040000000Z ERR_CONN_RESET upstream\n"
           b"2024-10-22T00:00:03.000000000Z GET /b 200\n"
           b"2024-10-22T00:10:00.000000000Z ERR_CONN_RESET again\n"
           b"2024-10-22T00:10:00.000000001Z GET /c 200\n")
    sidecar = (b"2024-10-22T00:00:01.000000000Z restarting\n"
               b"2024-10-22T01:00:01+01:00 ready, written with a zone\n"
               b"2024-10-22T00:00:01.540000000Z at +500 ms\n"
               b"2024-10-22T00:00:01.540000001Z at +500 ms and 1 ns\n"
               b"2024-10-22T00:00:00.540000000Z at -500 ms\n"
               b"2024-10-22T00:00:00.539999999Z at -500 ms and 1 ns\n")
    db = (b"2024-10-22T00:10:00.000000000Z checkpoint at the second anchor's instant\n"
          b"no timestamp here ERR_CONN_RESET\n"
          b"2024-10-22T00:09:59.999999999Z one ns ahead of it\n"
          b"2024-10-22T00:00:01.040000000Z out of order, at the first anchor's instant\n"
          b"2024-10-22T00:05:00.000000000Z far from both")
    return [api, sidecar, db]


DURATIONS = (0, 1, 999_999_999, NS, NS + 1, 500_000_000, 40 * 60 * NS, MAX_NS)


def test_three_streams_by_hand():
    ar = AroundRef(three_streams(), grep=[b"ERR_CONN_RESET"])
    assert [sum(r.m) for r in ar.refs] == [2, 0, 0] and len(ar.anchors()) == 2
    g = ar.group(0, 0)  # equal instants only: also lines outside M, of other streams
    assert g == [[False, True, False, True, False], [False] * 6, [True, False, False, True, False]]
    g = ar.group(500_000_000, 500_000_000)
    assert g[0] == [True, True, False, True, True]
    assert g[1] == [True, True, True, False, True, False]   # both ends closed, 1 ns past them is out
    assert g[2] == [True, False, True, True, False]
    g = ar.group(0, 500_000_000)  # before reaches back ahead of an anchor: none here
    assert g[1] == [False, False, True, False, False, False] and g[2] == [True, False, False, True, False]
    t = po.parse_line(b"2024-10-22T00:05:00Z x")[0]
    cut = ar.cut(500_000_000, 500_000_000, t, OPEN_HI)  # the first anchor's context is cut away
    assert cut == [[False, False, False, True, True], [False] * 6, [True, False, True, False, False]]
    out = ar.around(500_000_000, 500_000_000, tail=1)
    assert out[1][0] == b"at -500 ms\n" and out[1][1] == 4 and out[1][3] == 1


@pytest.mark.parametrize("grep", [(synth.NEEDLE,), (b"timeout",), (b"e",)])
def test_reference_equals_the_brute_force(grep):
    assert _golden(), "tests/golden/*.log is missing"
    inputs = [[p.read_bytes()[:6000] for p in _golden()], three_streams()]
    for streams in inputs:
        ar = AroundRef(streams, grep=grep)
        for b in DURATIONS:
            for a in DURATIONS:
                assert ar.group(b, a) == brute_group(ar.refs, b, a), (grep, b, a)


def test_basic_facts():
    inputs = [[p.read_bytes() for p in _golden()], [synth.generate(synth.TEXT, 3, 0, 40_000), synth.generate(synth.JSON, 4, 1, 30_000, permille=50)],
              three_streams()]
    spanning = 0
    for streams in inputs:
        for grep in ((synth.NEEDLE,), (b"e",)):
            ar = AroundRef(streams, grep=grep)
            n_anchors = len(ar.anchors())
            assert n_anchors == sum(sum(r.m) for r in ar.refs) > 0
            prev = None
            for d in (0, 1, NS, 40 * 60 * NS, MAX_NS):
                g = ar.group(d, d)
                for r, f in zip(ar.refs, g):
                    assert all(f[i] for i in range(r.n_lines) if r.m[i])            # M is a subset of G'
                    assert not any(f[i] for i in range(r.n_lines) if not r.parsed[i])  # unparseable: never
                for one_sided in (ar.group(d, 0), ar.group(0, d)):                  # monotone in each duration
                    assert all(not x or y for fa, fb in zip(one_sided, g) for x, y in zip(fa, fb))
                if prev is not None:
                    assert all(not x or y for fa, fb in zip(prev, g) for x, y in zip(fa, fb))
                prev = g
            stamps = [ns_of(t) for r in ar.refs for t in r.ts if t is not None]
            span = max(stamps) - min(stamps)
            if span <= MAX_NS:  # both durations span everything: the parsed lines
                spanning += 1
                assert ar.group(span, span) == [list(r.parsed) for r in ar.refs] == prev
                assert ar.cut(span, span, OPEN_LO, OPEN_HI) == prev
    assert spanning >= 4
    none = AroundRef(three_streams(), grep=[b"a\nb"])  # no anchor: a valid empty selection
    assert not none.anchors() and not any(any(f) for f in none.group(MAX_NS, MAX_NS))


def test_cut_takes_context_from_all_anchors_first():
    ar = AroundRef(three_streams(), grep=[b"ERR_CONN_RESET"])
    t = lambda s: po.parse_line(s + b" x")[0]
    frm, until = t(b"2024-10-22T00:00:01.5Z"), t(b"2024-10-22T00:00:02Z")  # holds no anchor
    assert ar.cut(NS, NS, frm, until) == [[False] * 5, [False, False, True, True, False, False], [False] * 5]
    assert not any(any(f) for f in ar.cut(NS, NS, until, frm))  # from > until: empty


# ---------------------------------------------------------------- the library (no device) ---

def test_library_exports_around():
    lib = E.lib()
    assert hasattr(lib, "klf_around") and hasattr(lib, "klf_result_around_info")
    assert "klf_around" in E.SIGNATURES and "klf_result_around_info" in E.SIGNATURES
    hdr = (ROOT / "include" / "klf.h").read_text()
    for name in ("klf_around_opts", "KLF_AROUND_MAX_NS", "klf_around(", "before_ns", "after_ns"):
        assert name in hdr, name
    assert C.sizeof(E._AroundOpts) == 56
    assert E.AROUND_MAX_NS == MAX_NS == (1 << 62) - 1 and "((1ull << 62) - 1)" in hdr
    assert callable(E.Result.around)


def test_around_null_arguments_are_einval():
    lib = E.lib()
    o = E._AroundOpts()
    r = C.c_void_p()
    assert lib.klf_around(None, None, C.byref(o), -1, C.byref(r)) == E.KLF_EINVAL
    assert lib.klf_around(None, None, None, -1, None) == E.KLF_EINVAL
    assert lib.klf_result_around_info(None, None, None, None) == E.KLF_EINVAL


def test_docs_describe_around():
    for doc, words in (("SPEC.md", ("S4g", "klf_around")), ("README.md", ("--around",)), ("DESIGN.md", ("k_ar_build",)),
                       ("INTEGRATION.md", ("klf_around",))):
        text = (ROOT / doc).read_text()
        for w in words:
            assert w in text, (doc, w)
