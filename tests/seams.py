"""Input stream seams: a seeded builder of one contiguous text T whose streams end where it
hurts (no GPU here; tests/test_seams_ref.py proves the seams hostile on the host,
tests/test_gpu_seams.py runs them on the device).

Every kernel reads past a stream's end (the scan stages whole tiles plus a halo, the
timestamp paths load 16-byte chunks, the copies move whole chunks), and what lies there is
not defined: the next stream's first byte when the length is a multiple of 256, up to 255
pad bytes otherwise, then the allocation's slack.  Results must not depend on those bytes.
T puts a feature at the end of each stream and its completion right behind it:

* layout A, abutting: every cut is a multiple of 256, stream i is T[c_i:c_i+1], the streams
  touch, and the buffer goes on with more of T over the whole slack;
* layout B, stale pad: bases are multiples of 256, stream i stops g_i = 1..255 bytes short of
  the next base, and the buffer is still contiguous T, so each pad holds exactly the bytes
  that were cut off (what a long-lived engine's buffer holds after an earlier batch).

Both placements are what klf_layout computes from the lengths (checked in the tests), so
the staged path lays the streams out the same way.  A seam is the end of one stream; its
class says which feature was cut and `k` where.  Tiles are counted from each stream's
base, so `tile_aligned` is about the stream's length (layout A) or its span to the next base
(layout B, whose lengths are never a multiple of 256), and `group` marks a stream that ends a
64-tile scatter group of the batch.
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

from klogs_amd import synth

TILE = 8192
ALIGN = 256                      # kSegAlign
SLACK = TILE + 64 + 1024         # kAllocSlack (test_seams_ref checks it against klf_layout)
GROUP_TILES = 64
OVER = 64                        # test_seams_ref: the oracle reads this far past a seam
NEEDLE = synth.NEEDLE
TINY = (0, 1, 2, 30, 31, 32, 33)

_WORDS = (b"pod sync loop ready volume mount probe status node lease renew cache entry watch event "
          b"queue worker retry backoff image pull layer digest sandbox network route endpoint slice "
          b"container started stopped healthy latency bucket shard replica leader follower commit").split()


def _c4_by_len(lo, hi, n):
    return [l for l in synth.c4_literals(1024) if lo <= len(l) <= hi][:n]


def _short_set():
    """4- and 5-byte needles: the heads of the vocabulary's literals (it starts at 6 bytes), less
    the family prefixes that every other literal of the family would match."""
    out = []
    for i, l in enumerate(synth.c4_literals(1024)[:160]):
        p = l[:4 + (i & 1)]
        if p not in out and p not in (b"ERR_", b"ORA-", b"HTTP", b"HTTP_"):
            out.append(p)
    return out


@functools.lru_cache(maxsize=None)
def pattern_sets() -> Dict[str, Tuple[tuple, tuple]]:
    """name -> (grep, match): the pattern sets the seams are built for.  lit4 / lit6 / lit8 are
    the sets of synth.c4_literals the scan samples at stride 4, 6 and 8 (shortest needle 6-7,
    8-9 and >= 12 bytes: the stride follows the shortest needle, at most its length - 2); lit2
    holds needles of 4-5 bytes (stride 2); anch is a stride-8 set with one short needle,
    anchored under KLF_QF_ANCHOR=force."""
    lit4, lit6, lit8 = _c4_by_len(6, 7, 200), _c4_by_len(8, 9, 200), _c4_by_len(12, 24, 300)
    rx = tuple(synth.c5_regexes()) + (rb"took \d+ms", rb"ERR_\w+")
    return {
        "none": ((), ()),
        "needle": ((NEEDLE,), ()),
        "lit2": (tuple(_short_set()), ()),
        "lit4": (tuple(lit4), ()),
        "lit6": (tuple(lit6), ()),
        "lit8": (tuple(lit8), ()),
        "anch": (tuple(lit8[:100]) + (anchored_needle(),), ()),
        "rx": ((), rx),
        "mixed": ((NEEDLE, set_needles()["lit6"][0]), (rb"took \d+ms", synth.c5_pattern(27, 0), rb"(?i)err_\w+")),
        "off": ((b"ab",), (rb"\d+",)),  # no usable factor: the prefilter is off, k_match decides
    }


@functools.lru_cache(maxsize=None)
def set_needles() -> Dict[str, List[bytes]]:
    """The needles of each literal set that get cut at every interior byte."""
    pick = lambda lo, hi, n: [l for l in _c4_by_len(lo, hi, 10**6) if len(l) == n and not l.startswith(b"ERR_")][0]
    short = [p for p in _short_set() if not p.startswith(b"ERR_")]
    return {"lit2": [[p for p in short if len(p) == n][0] for n in (4, 5)],
            "lit4": [pick(6, 7, 6), pick(6, 7, 7)], "lit6": [pick(8, 9, 8), pick(8, 9, 9)],
            "lit8": [pick(12, 24, 12), pick(12, 24, 16)]}


def anchored_needle() -> bytes:
    return set_needles()["lit4"][1]


@dataclass
class Seam:
    cls: str                 # feature class
    k: int                   # where the feature was cut (bytes of it before the cut)
    stream: int              # the stream that ends here
    cut: int                 # offset of the stream's end in the layout's buffer
    expect: Optional[Tuple[str, str]]  # (pattern set, field) that differs when the bytes behind are read
    control: bool            # the clean cut: nothing has to differ
    tile_aligned: bool
    group: bool
    ts: Optional[Tuple[int, int]]      # the cut line's instant, where its prefix is the canonical one


@dataclass
class Layout:
    name: str
    buf: bytes               # klf_layout's total_alloc bytes of T
    bases: List[int]
    lens: List[int]
    seams: List[Seam] = field(default_factory=list)
    mid: Tuple[int, int] = (0, 0)     # instants of seam lines at 1/2, 1/4 and 3/4 of the layout
    frm: Tuple[int, int] = (0, 0)
    until: Tuple[int, int] = (0, 0)

    def stream(self, i: int, extra: int = 0) -> bytes:
        return self.buf[self.bases[i]:self.bases[i] + self.lens[i] + extra]

    def streams(self) -> List[bytes]:
        return [self.stream(i) for i in range(len(self.lens))]

    def filled(self, byte: bytes) -> bytes:
        """The buffer with everything outside the streams (pads and slack) set to `byte`."""
        out = bytearray(byte * len(self.buf))
        for b, n in zip(self.bases, self.lens):
            out[b:b + n] = self.buf[b:b + n]
        return bytes(out)

    def classes(self) -> Dict[str, int]:
        out: Dict[str, int] = {}
        for s in self.seams:
            out[s.cls] = out.get(s.cls, 0) + 1
        return out


@dataclass
class _Feature:
    cls: str
    k: int
    make: Callable[[bytes], Tuple[bytes, bytes]]  # 30-byte timestamp -> (bytes before the cut, bytes behind it)
    expect: Optional[Tuple[str, str]]
    control: bool = False
    canonical: bool = True


def _features() -> List[_Feature]:
    F: List[_Feature] = []

    def cut_line(cls, k, pre, feat, post, at, expect, **kw):
        """A canonical line `pre feat post` cut `at` bytes into feat."""
        def make(ts, pre=pre, feat=feat, post=post, at=at):
            line = ts + b" " + pre + feat + post + b"\n"
            c = 31 + len(pre) + at
            return line[:c], line[c:]
        F.append(_Feature(cls, k, make, expect, **kw))

    for k in range(2):  # the control: a cut right after '\n'
        F.append(_Feature("clean_after_nl", k, lambda ts: (ts + b" clean cut " + NEEDLE + b" here\n", b""), None, True))
    for k in range(2):  # right before '\n': the next stream starts with an empty line
        F.append(_Feature("cut_before_nl", k, lambda ts: (ts + b" cut before the newline " + NEEDLE, b"\n"),
                          ("none", "lines")))
    for k in range(1, 32):  # the canonical prefix: 30 = "...Z" without the space, 31 = parsed and empty
        def make(ts, k=k):
            line = ts + b" " + NEEDLE + b" right behind the prefix\n"
            return line[:k], line[k:]
        F.append(_Feature("prefix_cut", k, make, ("none", "parsed") if k < 31 else ("needle", "matched")))
    forms = {  # non-canonical prefixes: deferred lines at a stream's end
        "zone": lambda ts: ts[:29] + b"+01:30",
        "frac12": lambda ts: ts[:29] + b"012Z",
        "hour1": lambda ts: ts[:11] + ts[12:],
        "comma": lambda ts: ts[:19] + b"," + ts[20:],
    }
    for name, form in forms.items():
        n = len(form(b"2024-10-22T00:00:00.000000000Z"))
        for k in sorted({12, 20, n - 4, n - 1, n, n + 1}):  # n: no space yet; n + 1: parsed, empty content
            def make(ts, form=form, k=k):
                line = form(ts) + b" " + NEEDLE + b" behind an odd prefix\n"
                return line[:k], line[k:]
            F.append(_Feature("noncanon_" + name, k, make, ("none", "parsed") if k <= n else ("needle", "matched"),
                              canonical=False))
    for j in range(1, len(NEEDLE)):
        cut_line("needle_cut", j, b"upstream said ", NEEDLE, b" and closed", j, ("needle", "matched"))
    for name, needles in set_needles().items():
        for nd in needles:
            for j in range(1, len(nd)):
                cut_line(name + "_cut", j, b"code ", nd, b" seen", j, (name, "matched"))
    nd = anchored_needle()
    for j in range(1, len(nd)):
        cut_line("anch_cut", j, b"anchored ", nd, b" seen", j, ("anch", "matched"))
    snip = synth.c5_pattern(27, 1)  # tx-0a1b2c3d-commit3
    for j in range(1, len(snip)):
        cut_line("rx_c5_cut", j, b"worker ", snip, b" ok", j, ("rx", "matched"))
    fold = synth.c5_pattern(60, 1)  # Connection reset by peer4, for (?i)conn(ection)? reset by peer4
    for j in (3, 10, 17, len(fold) - 1):
        cut_line("rx_fold_cut", j, b"socket: ", fold, b" again", j, ("rx", "matched"))
    for j in (5, 7, 9, 10):  # took |1234ms, took 12|34ms, took 1234|ms, took 1234m|s
        cut_line("rx_took_cut", j, b"request ", b"took 1234ms", b" done", j, ("rx", "matched"))
    for j in (16, 18):  # the left half matches on its own: took 12ms took 3|4ms, ...34m|s
        cut_line("rx_left_half", j, b"", b"took 12ms took 34ms", b" twice", j, ("none", "out"))
    for j, exp in ((3, ("rx", "matched")), (4, ("rx", "matched")), (8, ("none", "out"))):
        # ERR|_, ERR_|TIMEOUT (\w+ needs the neighbour), ERR_TIME|OUT (\w+ would run on into it)
        cut_line("rx_unbounded", j, b"failed with ", b"ERR_TIMEOUT_X9", b" twice", j, exp)

    # the stream's last tile holds more line starts than the scan stages slots for (lines
    # under 32 bytes: the pool path), some of them deferred, and ends in a cut prefix / needle
    dense = (b"\n" + b"x\n" + b"2024-10-22T00:00:07Z ok\n" + b"\n") * 310
    for k in (17, 31, 38):
        def make(ts, k=k):
            line = ts + b" " + NEEDLE + b" behind short lines\n"
            return dense + line[:k], line[k:]
        F.append(_Feature("dense_tail", k, make, ("none", "parsed") if k < 31 else ("needle", "matched")))

    def long_make(ts):  # > 64 KiB, one needle before the cut and one behind it
        w = b" ".join(_WORDS)
        body = lambda n: (w * (n // len(w) + 1))[:n]
        return (ts + b" " + body(17000) + b" " + NEEDLE + b" " + body(17000),
                body(16500) + b" " + NEEDLE + b" " + body(16500) + b"\n")
    for k in range(2):
        F.append(_Feature("long_line", k, long_make, ("none", "out")))
    return F


class _Builder:
    def __init__(self, seed: int):
        self.rng = random.Random(seed)
        self.parts: List[bytes] = []
        self.pos = 0
        self.nline = 0

    def ts(self) -> Tuple[bytes, Tuple[int, int]]:
        n = self.nline
        self.nline += 1
        sec, nsec = n // 4, (n % 4) * 250_000_000 + n
        assert sec < 3600
        return (b"2024-10-22T00:%02d:%02d.%09dZ" % (sec // 60, sec % 60, nsec)), (synth.T0 + sec, nsec)

    def emit(self, b: bytes):
        self.parts.append(b)
        self.pos += len(b)

    def filler(self, n: int):
        """One filler line of exactly n bytes (lower-case words: no needle, no event)."""
        assert n >= 33, n
        words = []
        while sum(map(len, words)) + len(words) < n - 32:
            words.append(self.rng.choice(_WORDS) if self.rng.random() < 0.9 else b"n=%d" % self.rng.randrange(1000))
        c = b" ".join(words)[:n - 32]
        self.emit(self.ts()[0] + b" " + c + b"x" * (n - 32 - len(c)) + b"\n")

    def fill_to(self, target: int):
        """Filler lines up to `target`, the last one of tuned length."""
        gap = target - self.pos
        assert gap == 0 or gap >= 33, (self.pos, target)
        while target - self.pos > 420:
            self.filler(self.rng.randint(90, 260))
        if target > self.pos:
            self.filler(target - self.pos)


def _up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def _place(b: _Builder, origin: int, stale: bool) -> Tuple[List[int], List[int], List[Seam]]:
    """One pass over every feature from b.pos == origin (a line start): abutting streams
    (stale False) or streams that stop 1..255 bytes short of the next base (stale True).
    Offsets are relative to `origin`."""
    rng = b.rng
    bases, lens, seams = [], [], []
    base, tiles, grouped = origin, 0, False
    per_class: Dict[str, int] = {}
    gaps = [1, 255, 2, 254, 16, 240, 15, 17, 128]

    def close(feat, L, end, stamp):
        nonlocal base, tiles
        nt = -(-(end - base) // TILE)
        tiles += nt
        seams.append(Seam(feat.cls, feat.k, len(lens), end - origin, feat.expect, feat.control,
                          L % TILE == 0, tiles % GROUP_TILES == 0, stamp if feat.canonical else None))
        bases.append(base - origin)
        lens.append(end - base)
        base += L

    feats = _features()
    if stale:  # one more control, so that the tiny streams behind it start on a line
        feats.append(_Feature("clean_after_nl", 2, feats[0].make, None, True))
    for feat in feats:
        idx = per_class.get(feat.cls, 0)
        per_class[feat.cls] = idx + 1
        head_len = len(feat.make(b"2024-10-22T00:00:00.000000000Z")[0])
        if stale:
            i = len(lens)  # two of three gaps from the edge cases, the third at random
            g = gaps[(i - i // 3 - 1) % len(gaps)] if i % 3 else rng.randint(1, 255)
            if feat.control:
                g = rng.randint(64, 255)  # the pad is one whole filler line: the next base starts a line
        else:
            g = 0
        need = max(b.pos - base, 0) + 33 + head_len + g  # (a short remainder ends inside the pad before `base`)
        want_tile = idx % 7 == 0  # every class: its first seam on a tile boundary, its second one off it
        if not grouped and tiles % GROUP_TILES >= 52 and tiles % GROUP_TILES + -(-need // TILE) <= GROUP_TILES:
            L = (GROUP_TILES - tiles % GROUP_TILES) * TILE  # this stream ends the batch's 64-tile group
            grouped = True
        elif want_tile:
            L = _up(need, TILE)
        else:
            j = -(-need // ALIGN) + rng.randint(0, 7) + (32 if rng.random() < 0.05 else 0)
            L = ALIGN * (j + 1 if j % 32 == 0 else j)
        end = base + L - g
        b.fill_to(end - head_len)
        ts, stamp = b.ts()
        head, rest = feat.make(ts)
        b.emit(head)
        assert b.pos == end
        b.emit(rest)
        if stale and feat.control:
            b.fill_to(base + L)
        close(feat, L, end, stamp)
    if stale:  # tiny streams: each base starts a canonical line whose content starts with the needle
        assert b.pos == base
        for n in TINY:
            exp = ("none", "lines") if n == 0 else ("none", "parsed") if n < 31 else ("needle", "matched")
            f = _Feature("tiny", n, None, exp, canonical=n > 0)
            if n == 0:
                close(f, 0, base, None)  # no bytes, no room: the next stream has the same base
                continue
            ts, stamp = b.ts()
            b.emit(ts + b" " + NEEDLE + b" tiny\n")
            b.fill_to(base + ALIGN)
            close(f, ALIGN, base + n, stamp)
    assert grouped and any(s.group for s in seams) and min(lens) >= 0
    return bases, lens, seams


@dataclass
class Seams:
    T: bytes
    A: Layout
    B: Layout


@functools.lru_cache(maxsize=None)
def build(seed: int = 20241022) -> Seams:
    b = _Builder(seed)
    a_bases, a_lens, a_seams = _place(b, 0, False)
    a_end = a_bases[-1] + a_lens[-1]
    assert a_end % ALIGN == 0 and b.pos >= a_end
    origin = _up(b.pos + 33, ALIGN)
    b.fill_to(origin)
    b_bases, b_lens, b_seams = _place(b, origin, True)
    b_end = _up(b_bases[-1] + b_lens[-1], ALIGN)
    b.fill_to(max(b.pos + 33, origin + b_end + SLACK + 512))
    T = b"".join(b.parts)
    assert len(T) == b.pos

    def layout(name, off, end, bases, lens, seams):
        lay = Layout(name, T[off:off + end + SLACK], bases, lens, seams)
        stamps = [s.ts for s in seams if s.ts is not None]
        lay.frm, lay.mid, lay.until = stamps[len(stamps) // 4], stamps[len(stamps) // 2], stamps[3 * len(stamps) // 4]
        return lay
    return Seams(T, layout("A", 0, a_end, a_bases, a_lens, a_seams),
                 layout("B", origin, b_end, b_bases, b_lens, b_seams))


# ---- the expectations: the oracles over each stream's own bytes, computed once ---------------

COUNT_KEYS = ("lines", "parsed", "since_ok", "matched", "selected", "out_bytes")


def oracle(data: bytes, name: str, since=None, tail: int = -1) -> dict:
    """{out, lines, bits, counts} of one stream under pattern set `name`: the C oracle for
    literal sets and no patterns, the Python oracle for sets with a regex."""
    import c_oracle as co
    import klf_oracle as po
    grep, match = pattern_sets()[name]
    since = since or po.GO_ZERO_TIME
    if not match:
        out, lo, bits, c = co.filter_stream(data, since, tail, list(grep))
        return dict(out=out, lines=[int(x) for x in lo], bits=bits, counts={k: c[k] for k in COUNT_KEYS})
    ref = po.filter_stream(data, since, tail, _compiled(name))
    return dict(out=ref.out, lines=ref.line_off, bits=ref.match_bits,
                counts=dict(lines=ref.n_lines, parsed=ref.n_parsed, since_ok=ref.n_since, matched=ref.n_matched,
                            selected=ref.n_selected, out_bytes=len(ref.out)))


@functools.lru_cache(maxsize=None)
def _compiled(name: str):
    import klf_oracle as po
    return po.compile_patterns(*pattern_sets()[name])


@functools.lru_cache(maxsize=None)
def expected(layout: str, name: str, since=None, tail: int = -1) -> List[dict]:
    """oracle() of every stream of layout "A" / "B" (shared by the tests; never changed)."""
    lay = getattr(build(), layout)
    return [oracle(s, name, since, tail) for s in lay.streams()]


# ---- the staged legs: what an engine's batch buffer holds when the pieces arrive ---------------

def staged_first() -> bytes:
    """The stream a long-lived engine runs first: layout B's buffer up to its last base's end,
    then layout A's with its slack.  klf_run puts it at offset 0 of the batch buffer, so that a
    second batch of B's pieces and then A's (placed by klf_layout from 0 again) finds behind
    every piece exactly the bytes that were cut off."""
    s = build()
    return s.B.buf[:len(s.B.buf) - SLACK] + s.A.buf + b"\n"


def staged_pieces() -> List[bytes]:
    s = build()
    return s.B.streams() + s.A.streams()


def staged_buffer() -> Tuple[bytes, List[int], List[int]]:
    """(buffer, bases, lens) of that second batch, simulated: the first batch's bytes (what the
    allocation holds behind them is unknown: 0xff here), the pieces copied to their bases and
    nothing else touched, as klf_run does.  The buffer is not reallocated: it only grows."""
    first = staged_first()
    buf = bytearray(first + b"\xff" * (_up(len(first), ALIGN) + SLACK - len(first)))
    bases, lens, off = [], [], 0
    for p in staged_pieces():
        bases.append(off)
        lens.append(len(p))
        buf[off:off + len(p)] = p
        off = _up(off + len(p), ALIGN)
    assert off + SLACK <= len(buf)
    return bytes(buf), bases, lens
