"""klf_result_histogram (SPEC.md S4c: the lines of a finished run's selection counted over
time): the reference the GPU tests compare against, an independent check of that reference
through WindowRef.cut, and the library's new ABI entries.  No GPU here."""
import ctypes as C
from pathlib import Path

import pytest

from klogs_amd import engine as E
from klogs_amd import synth
from test_window_ref import OPEN_HI, OPEN_LO, WindowRef

ROOT = Path(__file__).resolve().parent.parent
NS = 10**9


def shift(t, d_ns):
    """The instant t (sec, nsec) moved by d_ns nanoseconds."""
    total = t[0] * NS + t[1] + d_ns
    return (total // NS, total % NS)


class HistRef(WindowRef):
    """WindowRef plus the histogram of a selection g (flags per line), by the definition."""

    def hist(self, g, origin, width_ns, n):
        """(buckets, below, above) in plain integers."""
        assert width_ns >= 1 and n >= 1
        buckets, below, above = [0] * n, 0, 0
        for i in range(self.n_lines):
            if not g[i] or self.ts[i] is None:
                continue
            ts = tuple(self.ts[i])
            if ts < tuple(origin):
                below += 1
                continue
            d = (ts[0] - origin[0]) * NS + ts[1] - origin[1]
            if d >= n * width_ns:
                above += 1
            else:
                buckets[d // width_ns] += 1
        return buckets, below, above


def _golden():
    return sorted((ROOT / "tests" / "golden").glob("*.log"))


def _text_stream():
    return synth.generate(synth.TEXT, 3, 0, 40_000)


def _check_against_cut(ref, origin, w, n):
    g = ref.gprime()
    buckets, below, above = ref.hist(g, origin, w, n)
    end = shift(origin, n * w)
    for k in range(n):
        assert buckets[k] == sum(ref.cut(shift(origin, k * w), shift(origin, (k + 1) * w))), (origin, w, k)
    assert below == sum(ref.cut(OPEN_LO, origin))
    assert above == sum(ref.cut(end, OPEN_HI))
    assert below + sum(buckets) + above == sum(g)
    return buckets, below, above


@pytest.mark.parametrize("grep", [(), (synth.NEEDLE,), (b"e",)])
def test_hist_equals_the_windows_of_its_buckets(grep):
    assert _golden(), "tests/golden/*.log is missing"
    inputs = [(p.name, p.read_bytes()) for p in _golden()] + [("synthetic text", _text_stream())]
    counted = 0
    for name, data in inputs:
        ref = HistRef(data, grep=grep)
        instants = sorted({t for t in ref.ts if t is not None})
        if not instants:
            continue
        origin = instants[len(instants) // 4]
        for w, n in ((NS, 48), (60 * NS, 64), (7, 40)):
            for org in (origin, shift(origin, -3), shift(origin, 1)):
                b, lo, hi = _check_against_cut(ref, org, w, n)
                counted += sum(b)
        if name == "synthetic text":  # the stream spans 3600 s
            b, lo, hi = ref.hist(ref.gprime(), (synth.T0, 0), 60 * NS, 64)
            if not grep or grep == (b"e",):
                assert sum(1 for x in b if x) >= 10
            assert lo == 0 and hi == 0
    assert counted > 0


def test_hist_edges_by_hand():
    ts = b"2024-10-22T00:00:%02d.%09dZ "
    lines = [ts % (0, 0) + b"a\n", b"junk\n", ts % (2, 999999999) + b"HIT\n", ts % (3, 0) + b"HIT\n",
             ts % (1, 5) + b"late HIT\n", ts % (9, 0) + b"b"]
    data = b"".join(lines)
    t0 = HistRef(data).ts[0]
    nop = HistRef(data)
    assert nop.hist(nop.gprime(), t0, NS, 4) == ([1, 1, 1, 1], 0, 1)
    assert nop.hist(nop.gprime(), shift(t0, 1), NS, 3) == ([0, 1, 2], 1, 1)  # 3.0 falls back into bucket 2
    hit = HistRef(data, grep=[b"HIT"])
    assert hit.hist(hit.gprime(), t0, 3 * NS, 1) == ([2], 0, 1)       # [0, 3): 2.999999999 and 1.000000005
    assert hit.hist(hit.gprime(), shift(t0, 5), NS, 3) == ([0, 1, 2], 0, 0)  # 1.000000005 is bucket 1's lower edge
    assert hit.hist(hit.gprime(), shift(t0, 6), NS, 3) == ([1, 0, 2], 0, 0)  # one ns later it is bucket 0's last instant


# ---------------------------------------------------------------- the library (no device) ---

def test_library_exports_histogram():
    lib = E.lib()
    assert hasattr(lib, "klf_result_histogram")
    assert "klf_result_histogram" in E.SIGNATURES
    hdr = (ROOT / "include" / "klf.h").read_text()
    for name in ("klf_result_histogram", "klf_hist_opts", "KLF_HIST_MAX_BUCKETS"):
        assert name in hdr, name
    assert C.sizeof(E._HistOpts) == 32
    assert E.HIST_MAX_BUCKETS == 65536


def hist_opts(origin=(0, 0), width_ns=NS, n=4, flags=0, reserved=0):
    o = E._HistOpts()
    o.origin.sec, o.origin.nsec, o.origin._reserved = origin[0], origin[1], reserved
    o.width_ns, o.n_buckets, o.flags = width_ns, n, flags
    return o


# every option the call refuses with KLF_EINVAL (also used on a live result by the GPU tests)
BAD_OPTS = {
    "width 0": dict(width_ns=0),
    "no bucket": dict(n=0),
    "too many buckets": dict(n=65537),
    "span 2^63": dict(width_ns=1 << 62, n=2),
    "span past 2^64": dict(width_ns=(1 << 64) - 1, n=65536),
    "span 2^63 exactly": dict(width_ns=1 << 47, n=65536),
    "nsec -1": dict(origin=(5, -1)),
    "nsec 1e9": dict(origin=(5, NS)),
    "flags": dict(flags=1),
    "reserved": dict(reserved=1),
}


def test_histogram_bad_arguments_are_einval_without_a_device():
    lib = E.lib()
    counts = (C.c_uint64 * 8)()
    o = hist_opts()
    assert lib.klf_result_histogram(None, C.byref(o), counts, None, None) == E.KLF_EINVAL
    assert lib.klf_result_histogram(None, None, counts, None, None) == E.KLF_EINVAL
    assert lib.klf_result_histogram(None, C.byref(o), None, None, None) == E.KLF_EINVAL
    for name, kw in BAD_OPTS.items():
        assert lib.klf_result_histogram(None, C.byref(hist_opts(**kw)), counts, None, None) == E.KLF_EINVAL, name
    assert (1 << 47) * 65536 == 1 << 63 and ((1 << 63) - 1) // 65536 * 65536 < 1 << 63
