"""Generated regex sets (tests/rxfuzz.py) through the C ABI on the GPU against the Python
oracle: output bytes, line offsets, match bits and counts.  Every input is a valid pattern
set over valid logs; the shapes are the smallest at which k_verify / k_nfa_win / k_nfa /
k_match take their different paths."""
import functools
import random

import pytest

import klf_oracle as po
import rxfuzz
from klogs_amd import engine as E
from klogs_amd import synth

pytestmark = pytest.mark.gpu

GZ = po.GO_ZERO_TIME
SEEDS = range(8)
SETS_PER_SEED = 6


def _ts(k):
    return b"2024-10-22T00:%02d:%02d.%09dZ " % (k // 60 % 60, k % 60, k * 7919 % 1_000_000_000)


def _stream(rng, pats, n_lines, k0=0):
    out = []
    for k in range(n_lines):
        c = rxfuzz.content(rng, pats, max_noise=60)
        r = rng.random()
        if r < 0.02:
            pre = b"2024-10-22T01:%02d:%02d+01:00 " % (k // 60 % 60, k % 60)  # non-canonical: a deferred line
        elif r < 0.03:
            pre = b"not-a-time "  # unparseable
        else:
            pre = _ts(k0 + k)
        out.append(pre + c + b"\n")
    return b"".join(out)


def _compilable(lits, pats):
    return E.debug_compile(lits, [p.pattern for p in pats])[0] == 0


@functools.lru_cache(maxsize=None)
def _sets(seed):
    """The seed's sets: (literals, [Pat], streams); refused ones counted."""
    rng = random.Random(11000 + seed)
    out, refused = [], 0
    while len(out) < SETS_PER_SEED:
        lits, pats = rxfuzz.pattern_set(rng, max_rx=4, max_lit=2)
        if not _compilable(lits, pats):
            refused += 1
            continue
        streams = [_stream(rng, pats, 1800), b"", _stream(rng, pats, 1200, 1800)[:-1]]
        out.append((lits, pats, streams))
    return out, refused


def _run_and_check(lits, match, streams, runs, counts=False):
    pats = po.compile_patterns(lits, match)
    with E.Engine(0, grep=lits, match=match) as eng:
        eng.set_streams(len(streams))
        for i, s in enumerate(streams):
            if s:
                eng.stage(i, s)
        for since, tail in runs:
            r = eng.run(since=since, tail=tail, n_streams=len(streams), pattern_counts=counts)
            for i, s in enumerate(streams):
                ref = po.filter_stream(s, since or GZ, tail, pats)
                so = r.stream(i)
                key = (match, lits, since, tail, i)
                assert so.out == ref.out, key
                assert r.lines(i).tolist() == ref.line_off, key
                assert r.match_bits(i) == ref.match_bits, key
                assert [so.counts[k] for k in ("lines", "parsed", "since_ok", "matched", "selected")] == \
                    [ref.n_lines, ref.n_parsed, ref.n_since, ref.n_matched, ref.n_selected], key
                if counts:
                    assert r.pattern_counts(i) == po.pattern_counts(s, pats), key
            r.free()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_regex_sets(gpu, seed):
    """1-4 regexes and 0-2 literals per set, one engine per set, about 3,000 lines in three
    streams (one empty, one without a final newline; a few deferred and unparseable lines):
    every line, a small tail, and a since cutoff."""
    sets, _ = _sets(seed)
    for lits, pats, streams in sets:
        _run_and_check(lits, [p.pattern for p in pats], streams,
                       [(None, -1), (None, 7), ((synth.T0 + 900, 0), -1)])


def test_generated_sets_are_not_trivial():
    """The shares of the sets test_random_regex_sets runs (from the compile's report and the
    reference alone)."""
    n = on = refused = b = u = nf = parsed = matched = 0
    for seed in SEEDS:
        sets, ref = _sets(seed)
        refused += ref
        for lits, pats, streams in sets:
            n += 1
            match = [p.pattern for p in pats]
            on += E.debug_prefilter(b"", grep=lits, match=match)[1]["on"]
            for p in pats:
                f = E.debug_factors(p.pattern, 0)
                nf += f is None
                b += f is not None and f[1] is not None
                u += f is not None and f[1] is None
            r = po.filter_stream(streams[2], GZ, -1, po.compile_patterns(lits, match))
            parsed += r.n_parsed
            matched += r.n_matched
    print(f"sets {n} refused {refused} on {on}; bounded {b} unbounded {u} no factor {nf}; lines {parsed} matched {matched}")
    assert refused <= 0.10 * (n + refused)
    assert on >= 0.50 * n
    assert b >= 0.40 * (b + u + nf) and u >= 0.10 * (b + u + nf)
    assert 0.25 * parsed <= matched <= 0.75 * parsed


def _pick(rng, want_bounded):
    """A compilable, unanchored pattern whose longest factor set has / has not a bounded
    match-start window, its factor strings and the bound."""
    for _ in range(2000):
        p = rxfuzz.pattern(rng)
        f = E.debug_factors(p.pattern, 0)
        if p.bol or p.eol or f is None or (f[1] is not None) != want_bounded or not _compilable([], [p]):
            continue
        if not want_bounded and not 2 <= len(p.example(rng, "min")) <= 16:
            continue  # (the 17-byte content must be able to hold one across its one boundary)
        if want_bounded and f[1] < 2:
            continue  # (offsets pre - 1, pre, pre + 1 apart from 0 and 1)
        return p, f
    raise AssertionError("the generator no longer yields such a pattern")


def _line(k, content):
    return _ts(k) + content + b"\n"


def _seam_stream(rng, pu, pb, fb):
    """Lines for one unbounded pattern pu (k_nfa: 64 lane chunks per line) and one bounded
    pattern pb with factors fb (k_nfa_win).  Returns the stream and the placements made per
    category."""
    lines = []
    made = {}

    def put(cat, n, at, ex):  # a content of n bytes holding ex at offset `at` (when it fits)
        if at < 0 or at + len(ex) > n:
            return
        made[cat] = made.get(cat, 0) + 1
        s = rxfuzz.noise(rng, n)
        lines.append(_line(len(lines), s[:at] + ex + s[at + len(ex):]))
        if ex:  # and a look-alike at the same place: one byte of the example changed
            k = rng.randrange(len(ex))
            bad = ex[:k] + bytes([rng.choice(rxfuzz.NOISE)]) + ex[k + 1:]
            lines.append(_line(len(lines), s[:at] + bad + s[at + len(ex):]))

    for n in (17, 33, 100, 1000, 3000):
        chunk = (-(-n // 64) + 15) // 16 * 16  # ceil(n / 64) rounded up to 16 B
        bounds = [chunk * k for k in (1, 2, 3) if chunk * k < n] + [(n - 1) // chunk * chunk]
        for bnd in bounds:
            for _ in range(3):
                # an example that starts d = 1..15 bytes before the boundary, crosses it (it is
                # longer than d) and fits the content
                for _ in range(20):
                    ex = pu.example(rng, "min" if n < 100 else "rand")
                    ds = [d for d in range(1, 16) if d <= bnd and d < len(ex) <= n - (bnd - d)]
                    if ds:
                        d = rng.choice(ds)
                        put("chunk%d" % n, n, bnd - d, ex)
                        break
    alts, pre, loose = fb
    for k in range(12):
        ex = pb.example(rng, "min" if k < 6 else "rand")
        t = bytes(c | 0x20 for c in ex) if loose else ex
        fo = min((t.find(a) for a in alts if a in t), default=None)
        if fo is None:
            continue
        for target in (0, 1, pre - 1, pre, pre + 1):  # the factor's content offset
            put("pre%+d" % (target - pre) if abs(target - pre) <= 1 else "at%d" % target, 200, target - fo, ex)
        put("whole", len(ex), 0, ex)
        made["end"] = made.get("end", 0) + 1
        lines.append(_line(len(lines), rxfuzz.noise(rng, 90) + ex))  # right at the content's end
    # examples across 8 KiB tile seams of the stream
    off = sum(map(len, lines))
    for _ in range(6):
        seam = (off // 8192 + 1) * 8192
        ex = (pu if rng.random() < 0.5 else pb).example(rng, "rand")
        before = seam - rng.randint(1, max(1, len(ex) - 1)) - (off + 31) if len(ex) > 1 else -1
        if 0 <= before <= 8000:
            made["tile"] = made.get("tile", 0) + 1
            lines.append(_line(len(lines), rxfuzz.noise(rng, before) + ex + rxfuzz.noise(rng, 20)))
        else:
            lines.append(_line(len(lines), rxfuzz.noise(rng, 500)))
        off += len(lines[-1])
    return b"".join(lines), made


@pytest.mark.parametrize("seed", range(4))
def test_matches_across_chunk_and_tile_seams(gpu, seed):
    """k_nfa splits a line's content over 64 lanes in chunks of ceil(n / 64) bytes rounded up
    to 16: examples of an unbounded pattern start 1..15 bytes before the first three chunk
    boundaries and the last, in contents of 17 B to 3 KiB.  k_nfa_win starts at most `pre`
    bytes before a factor: the factor at content offsets 0, 1, pre - 1, pre, pre + 1 and at the
    content's end.  Further examples straddle 8 KiB tile seams."""
    rng = random.Random(12000 + seed)
    pu, _ = _pick(rng, False)
    pb, fb = _pick(rng, True)
    assert len(_ts(0)) == 31
    s, made = _seam_stream(rng, pu, pb, fb)
    # every category was really placed.  (The factor at an offset below `pre` needs an example
    # whose factor comes that early; where the pattern's prefix has a fixed length there is
    # none, so offsets 0, 1 and pre - 1 are placed where they exist and not counted.)
    for cat in ("chunk17", "chunk33", "chunk100", "chunk1000", "chunk3000", "pre+0", "pre+1", "whole", "end",
                "tile"):
        assert made.get(cat, 0) >= 1, (cat, made, pu.pattern, pb.pattern)
    _run_and_check([], [pu.pattern, pb.pattern], [s, b""], [(None, -1)])
    _run_and_check([], [pu.pattern], [s], [(None, -1)])


@pytest.mark.parametrize("knob", ["KLF_CAND_CAP=16", "KLF_HITS_CAP=16", "KLF_WIN_INDEX_RX=0", "no_factor"])
def test_fallback_matchers_random(gpu, monkeypatch, knob):
    """The same few sets with the candidate queue or the hit list forced to overflow (k_match
    decides every line), without the windowed index, and with a factor-less regex added (the
    prefilter off); per-pattern counts against the oracle's."""
    extra = []
    if knob == "no_factor":
        extra = [rb"\d+[a-c]"]
        assert not E.debug_prefilter(b"", match=extra)[1]["on"]
    else:
        name, val = knob.split("=")
        monkeypatch.setenv(name, val)
    for lits, pats, streams in _sets(0)[0][:2]:
        _run_and_check(lits, [p.pattern for p in pats] + extra, streams, [(None, -1), (None, 5)], counts=True)
