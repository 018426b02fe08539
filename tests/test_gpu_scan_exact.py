"""The exact gram-table scan (k_scan<gen, 4, kQfExact, 3 | 4>) against the Bloom scan and the
Python oracle.  Each set runs on fresh engines with KLF_QF_EXACT=force and =0: output bytes,
counts, match bits and per-pattern counts of both equal the oracle's, and the KLF_DIAG layout
line shows that the first run took the exact kind (k = 6) and the second did not.

The input: the three streams of tests/scan_variants.py (2 tiles + 1,000 B; 9 tiles + 17 B, no
final newline, one dense tile; empty) with the set's needles across tile seams and in the last
lines, and hand-built streams where a needle's sampled gram is the last dword of a tile, the
first dword of the next, and where the stream ends 1 to 3 bytes into a dword (clipped samples)
behind a whole needle or a cut one."""
import functools
import re

import pytest

import klf_oracle as po
import scan_variants as sv
from klogs_amd import engine as E
from klogs_amd import synth

pytestmark = pytest.mark.gpu

EXACT = 6  # kQfExact
LAYOUT = re.compile(r"^\[klf\] prefilter layout from \d+ sampled bytes: (.*)$", re.M)
KNOBS = ("KLF_QF_EXACT", "KLF_QF_TUNE", "KLF_QF_TWO", "KLF_QF_ANCHOR", "KLF_QF_QMAX")
FILTERS = [(po.GO_ZERO_TIME, -1), (sv.SINCE, 50)]
FAMILIES = [8 * f + (3 * f + 1) % 8 for f in range(8)]  # one regex per C5 family, variants mixed

# name -> (grep, match, strings to plant (they match), near misses, gram bytes or None)
SETS = {
    "six": ([b"ab_cd1", b"Xy.z9w", b"qr=stu"], [], [b"ab_cd1", b"Xy.z9w", b"qr=stu"], [b"ab_cd", b"y.z9w", b"qr=stv"], 3),
    "seven": ([b"ab_cd1e", b"Xy.z9wv", b"qr=stuw"], [], [b"ab_cd1e", b"Xy.z9wv", b"qr=stuw"],
              [b"ab_cd1", b"y.z9wv", b"qr=stux"], 4),
    "c5_families": ([], [synth.c5_pattern(r, 0) for r in FAMILIES], [synth.c5_pattern(r, 1) for r in FAMILIES],
                    [synth.c5_pattern(r, 2) for r in FAMILIES], None),
}


def seam_stream(plant, miss, rem, cut):
    """About six tiles of kubelet lines.  plant[0] starts at tile offsets 8,188 (its first gram
    is the tile's last dword), 0 (the next tile's first), 8,190, 8,189 and 8,191 of successive
    seams; a near miss lies across one more seam.  The last line has no newline and ends with
    plant[1] (cut: without its last two bytes) at a stream length of rem mod 4."""
    out, sec = bytearray(), 0
    fill = b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor "

    def head():
        nonlocal sec
        sec += 1
        return b"2024-10-22T00:%02d:%02d.%09dZ " % (sec // 60, sec % 60, sec * 1001)

    def body(n):
        return (fill * (n // len(fill) + 1))[:n]

    def put_at(off, what):  # a line whose content holds `what` at stream offset off
        while off - len(out) > 400:
            out.extend(head() + body(120 + (len(out) * 7) % 90) + b"\n")
        assert off - len(out) >= 31, (off, len(out))
        out.extend(head())
        out.extend(body(off - len(out)) + what + b" tail\n")

    starts = [sv.TILE - 4, 2 * sv.TILE, 3 * sv.TILE - 2, 4 * sv.TILE - 3, 5 * sv.TILE - 1]
    for o in starts:
        put_at(o, plant[0])
    put_at(6 * sv.TILE - 3, miss[0])
    last = plant[1][:-2] if cut else plant[1]
    out.extend(head())
    out.extend(body(40 + (rem - (len(out) + 40 + len(last))) % 4) + last)
    assert len(out) % 4 == rem and not out.endswith(b"\n")
    for o in starts:
        assert out[o:o + len(plant[0])] == plant[0]
    return bytes(out)


@functools.lru_cache(maxsize=None)
def case(name):
    """(streams, patterns, {filter: [oracle result per stream]}, [oracle pattern counts per stream]); computed once."""
    grep, match, plant, miss, _ = SETS[name]
    ss = sv.streams(sv.Variant(name, plant + miss[:1], {}, "gen", 4, 0, 0, False))
    ss += [seam_stream(plant, miss, rem, cut) for rem, cut in ((1, False), (2, False), (3, False), (2, True))]
    pats = po.compile_patterns(grep, match)
    want = {f: [po.filter_stream(s, f[0], f[1], pats) for s in ss] for f in FILTERS}
    assert sum(r.n_matched for r in want[FILTERS[0]]) >= 20  # (the planted needles are found)
    return ss, want, [po.pattern_counts(s, pats) for s in ss]


def run_mode(name, mode, monkeypatch, capfd):
    grep, match, *_ = SETS[name]
    ss, want, pcounts = case(name)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KLF_QF_EXACT", mode)
    monkeypatch.setenv("KLF_DIAG", "1")
    capfd.readouterr()
    seen = ""
    with E.Engine(0, grep=grep, match=match) as eng:
        eng.set_streams(len(ss))
        for i, s in enumerate(ss):
            if s:
                eng.stage(i, s)
        for f in FILTERS:
            r = eng.run(since=None if f[0] == po.GO_ZERO_TIME else f[0], tail=f[1], n_streams=len(ss), pattern_counts=True)
            seen += capfd.readouterr().err
            for i, ref in enumerate(want[f]):
                so = r.stream(i)
                assert so.out == ref.out, (name, mode, f, i, len(so.out), len(ref.out))
                got = [so.counts[k] for k in ("lines", "parsed", "since_ok", "matched", "selected", "out_bytes")]
                assert got == [ref.n_lines, ref.n_parsed, ref.n_since, ref.n_matched, ref.n_selected, len(ref.out)], (name, mode, f, i)
                assert r.match_bits(i) == (ref.match_bits or b""), (name, mode, f, i)
                assert r.pattern_counts(i) == pcounts[i], (name, mode, f, i)
            r.free()
    return LAYOUT.findall(seen)


@pytest.mark.parametrize("name", list(SETS))
def test_exact_and_bloom_scans_equal_the_oracle(gpu, monkeypatch, capfd, name):
    lay = run_mode(name, "force", monkeypatch, capfd)
    assert lay and all(f"S=4 " in x and f" k={EXACT} " in x for x in lay), lay
    q = SETS[name][4]
    if q:
        assert all(f" q={q} " in x for x in lay), lay
    lay = run_mode(name, "0", monkeypatch, capfd)
    assert lay and not any(f" k={EXACT} " in x for x in lay), lay
