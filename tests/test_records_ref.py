"""klf_records (SPEC.md S4h: multi-line records over a finished run): the reference the GPU tests
compare against, a literal restatement of the semantics line by line on top of TimelineRef /
WindowRef, cases worked out by hand, the host classifier (klf_record_class) against the Python
one, and the library's new ABI entries.  No GPU here."""
import ctypes as C
import random
import shutil
import subprocess
from pathlib import Path

import pytest

import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import synth
from test_regroup_ref import RegroupRef
from test_timeline_ref import TimelineRef
from test_window_ref import OPEN_HI, OPEN_LO

ROOT = Path(__file__).resolve().parent.parent
GZ = po.GO_ZERO_TIME
TS = b"2024-10-22T00:00:%02d.000000000Z "


def opts(indent=False, blank=False, cont=(), head=(), invert=False, head_mode=None):
    """One option set; head mode when `head` is given, or on request (it is legal without prefixes)."""
    return dict(indent=indent, blank=blank, cont=tuple(cont), head=tuple(head), invert=invert,
                head_mode=bool(head) if head_mode is None else head_mode)


def classify(c: bytes, indent=False, blank=False, cont=(), head=(), invert=False, head_mode=None) -> bool:
    """S4h: the content c (without its '\\n') is a continuation."""
    if bool(head) if head_mode is None else head_mode:
        assert not (indent or blank or cont)
        return not any(c.startswith(p) for p in head)
    return bool((indent and c[:1] in (b" ", b"\t")) or (blank and c == b"") or any(c.startswith(p) for p in cont))


class RecordsRef(TimelineRef):
    """TimelineRef (WindowRef plus E) plus every parsed line's content C; records and G' / G'' by
    the definition."""

    def __init__(self, data: bytes, grep=(), match=()):
        super().__init__(data, grep, match)
        self.c = []
        for s, e in self.lines:
            p = po.parse_line(data[s:e])
            self.c.append(po.content_for_match(p[1]) if p is not None else None)

    def is_cont(self, o):
        """Per line: None (unparseable), True (continuation by content) or False (head)."""
        return [None if c is None else classify(c, **o) for c in self.c]

    def record_list(self, o):
        """The records: lists of parsed line numbers.  The first parsed line opens one whatever it is."""
        recs = []
        for i, k in enumerate(self.is_cont(o)):
            if k is None:
                continue  # belongs to no record, interrupts none
            if not recs or not k:
                recs.append([])
            recs[-1].append(i)
        return recs

    def group(self, o=0, *a, **kw):
        """G' of the option set o (a dict of `opts`); with anything else, RegroupRef's group."""
        if not isinstance(o, dict):
            return super().group(o, *a, **kw)
        g = [False] * self.n_lines
        for rec in self.record_list(o):
            if any(self.m[i] for i in rec) != bool(o["invert"]):
                for i in rec:
                    g[i] = True
        return g

    def cut(self, o, *a, **kw):
        """cut(opts, frm, until): G'' = G' of the option set cut to [frm, until), S4b's rule; with
        anything else in front, WindowRef's cut."""
        return self.records_cut(o, *a, **kw) if isinstance(o, dict) else super().cut(o, *a, **kw)

    def records_cut(self, o, frm=OPEN_LO, until=OPEN_HI):
        g = self.group(o)
        return [g[i] and self.ts[i] is not None and tuple(frm) <= tuple(self.ts[i]) < tuple(until)
                for i in range(self.n_lines)]

    def records(self, o, frm=OPEN_LO, until=OPEN_HI, tail=-1, since=GZ):
        """Per stream (out bytes, |G''|, packed G'' bits, selected lines), as WindowRef.window."""
        return self.emit(self.cut(o, frm, until), tail, since)

    def class_counts(self, o):
        k = [x for x in self.is_cont(o) if x is not None]
        return len(k) - sum(k), sum(k)  # heads, continuations: by content alone


def stream(*contents, last_nl=True):
    """Parsed lines with ascending seconds; None = an unparseable line."""
    out = b""
    for i, c in enumerate(contents):
        out += (b"no timestamp here\n" if c is None else TS % (i % 60) + c + b"\n")
    return out if last_nl else out[:-1]


JAVA = stream(b"INFO  starting",
              b"ERROR request failed: java.lang.NullPointerException",
              b"\tat com.example.Handler.run(Handler.java:41)",
              b"\tat com.example.Server.loop(Server.java:7)",
              b"Caused by: java.io.IOException: closed",
              b"\tat com.example.Io.read(Io.java:3)",
              b"INFO  next request",
              b"\tat orphan.frame(Of.java:1)",
              b"WARN  slow")
JAVA_OPTS = opts(indent=True, cont=[b"Caused by:"])

PYTHON = stream(b"2024 INFO worker up",
                b"Traceback (most recent call last):",
                b'  File "a.py", line 3, in <module>',
                b"    main()",
                b"ValueError: boom",
                b"2024 INFO worker down",
                b"2024 ERROR ValueError again")
PY_HEAD = opts(head=[b"2024 "])

ORPHANS = stream(b"\tat first.line(A.java:1)", b"\tat second(A.java:2)", b"ERROR head", b"\tat x", b"INFO y")
JUNK = stream(b"ERROR head", b"\tat a", None, b"\tat b NEEDLE", None, b"INFO next", None)
FRAGMENT = stream(b"INFO a", b"ERROR b", b"\tat c", last_nl=False)
HAND_STREAMS = [JAVA, PYTHON, ORPHANS, JUNK, FRAGMENT]
HAND_OPTS = [opts(), JAVA_OPTS, PY_HEAD, opts(blank=True), opts(indent=True, blank=True), opts(cont=[b"\tat ", b"Caused by:"]),
             opts(head=[b"INFO", b"ERROR", b"WARN"]), opts(head=[b"E", b"I", b"W", b"2024"])]


def flags(ref, o):
    return "".join("x" if f else "." for f in ref.group(o))


def test_java_trace_with_caused_by():
    ref = RecordsRef(JAVA, grep=[b"NullPointerException"])
    assert ref.m == [False, True] + [False] * 7
    assert flags(ref, JAVA_OPTS) == ".xxxxx..."
    assert flags(ref, opts(indent=True)) == ".xxx....."          # 'Caused by:' is a head of its own
    assert flags(ref, dict(JAVA_OPTS, invert=True)) == "x.....xxx"
    ref = RecordsRef(JAVA, grep=[b"Io.read"])                    # the match in the last line of the record
    assert flags(ref, JAVA_OPTS) == ".xxxxx..."
    ref = RecordsRef(JAVA, grep=[b"orphan"])                     # a trace behind an INFO line joins it
    assert flags(ref, JAVA_OPTS) == "......xx."
    out, n, bits, nsel = RecordsRef(JAVA, grep=[b"IOException"]).records(JAVA_OPTS, tail=2)
    assert n == 5 and nsel == 2 and out == b"Caused by: java.io.IOException: closed\n\tat com.example.Io.read(Io.java:3)\n"


def test_python_traceback_in_head_mode():
    ref = RecordsRef(PYTHON, grep=[b"ValueError"])
    assert ref.m == [False, False, False, False, True, False, True]
    assert flags(ref, PY_HEAD) == "xxxxx.x"
    assert flags(ref, opts(head=[b"2024 "], invert=True)) == ".....x."
    assert ref.class_counts(PY_HEAD) == (3, 4)


def test_orphan_continuations_open_a_record_of_their_own():
    ref = RecordsRef(ORPHANS, grep=[b"second"])
    assert flags(ref, opts(indent=True)) == "xx..."
    assert flags(ref, opts(indent=True, invert=True)) == "..xxx"
    assert ref.class_counts(opts(indent=True)) == (2, 3)  # by content alone: the first-line rule is not applied
    assert flags(RecordsRef(ORPHANS, grep=[b"head"]), opts(indent=True)) == "..xx."


def test_unparseable_line_inside_a_record():
    ref = RecordsRef(JUNK, grep=[b"NEEDLE"])
    assert ref.parsed == [True, True, False, True, False, True, False]
    assert flags(ref, opts(indent=True)) == "xx.x..."
    assert flags(ref, opts(indent=True, invert=True)) == ".....x."
    ref = RecordsRef(JUNK, grep=[b"head"])
    assert flags(ref, opts(indent=True)) == "xx.x..."  # the record goes on behind the junk
    only_junk_first = stream(None, b"\tat a", b"\tat b NEEDLE", b"INFO c")
    assert flags(RecordsRef(only_junk_first, grep=[b"NEEDLE"]), opts(indent=True)) == ".xx."


def test_unterminated_trailing_fragment_is_a_continuation():
    ref = RecordsRef(FRAGMENT, grep=[b"ERROR"])
    assert ref.c[-1] == b"\tat c" and not FRAGMENT.endswith(b"\n")
    assert flags(ref, opts(indent=True)) == ".xx"
    out, n, bits, nsel = ref.records(opts(indent=True))
    assert out == b"ERROR b\n\tat c" and n == 2 and nsel == 2
    frag_match = RecordsRef(FRAGMENT, grep=[b"at c"])
    assert flags(frag_match, opts(indent=True)) == ".xx"


def test_classifier_by_hand():
    assert classify(b"", blank=True) and not classify(b"") and not classify(b"", indent=True)
    assert classify(b"", head=[b"x"])  # head mode: empty starts with no prefix
    assert not classify(b"\r", blank=True) and not classify(b"\r", indent=True)  # a '\r' stays: not empty, not indented
    assert classify(b"\r", cont=[b"\r"])
    assert classify(b"\tx", indent=True) and classify(b" x", indent=True) and not classify(b"x ", indent=True)
    assert classify(b"\tx", cont=[b"\t"]) and not classify(b" x", cont=[b"\t"])  # tab against space
    assert classify(b"Caused by:", cont=[b"Caused by:"])        # equal to the prefix
    assert not classify(b"Caused by", cont=[b"Caused by:"])     # one byte shorter
    assert not classify(b"Caused by:", head=[b"Caused by:"]) and classify(b"Caused by", head=[b"Caused by:"])
    p32 = bytes(range(65, 97))
    assert len(p32) == 32 and classify(p32, cont=[p32]) and classify(p32 + b"z", cont=[p32])
    assert not classify(p32[:31] + b"!", cont=[p32]) and not classify(p32[:31], cont=[p32])
    for c, kw in ((b"", dict(blank=True)), (b"", {}), (b"\r", dict(blank=True, indent=True)), (b"\tx", dict(indent=True)),
                  (b" x", dict(cont=[b"\t"])), (b"Caused by:", dict(cont=[b"Caused by:"])),
                  (b"Caused by", dict(cont=[b"Caused by:"])), (b"Caused by", dict(head=[b"Caused by:"])),
                  (p32, dict(cont=[p32])), (p32[:31] + b"!", dict(cont=[p32])), (p32[:31], dict(cont=[p32])),
                  (p32 + b"z", dict(head=[p32])), (b"", dict(head=[b"x"]))):
        assert E.record_class(c, **kw) == int(classify(c, **kw)), (c, kw)  # the kernels' classifier agrees


def test_empty_content_and_blank():
    s = stream(b"ERROR a", b"", b"\tat b", b"", b"INFO c")
    ref = RecordsRef(s, grep=[b"ERROR"])
    assert ref.c[1] == b""
    assert flags(ref, opts(indent=True)) == "x...."               # the empty line is a head: it ends the record
    assert flags(ref, opts(indent=True, blank=True)) == "xxxx."
    assert flags(ref, opts(blank=True)) == "xx..."
    crlf = stream(b"ERROR a\r", b"\r", b" b\r")
    assert flags(RecordsRef(crlf, grep=[b"ERROR"]), opts(indent=True, blank=True)) == "x.."   # "\r" is neither
    assert flags(RecordsRef(crlf, grep=[b" b"]), opts(indent=True, blank=True)) == ".xx"


def test_invert_is_record_level():
    ref = RecordsRef(JAVA, grep=[b"Handler.run"])
    g, gi = ref.group(JAVA_OPTS), ref.group(dict(JAVA_OPTS, invert=True))
    assert [a or b for a, b in zip(g, gi)] == ref.parsed and not any(a and b for a, b in zip(g, gi))
    assert not any(gi[i] for i in range(ref.n_lines) if ref.m[i])   # M is disjoint from the inverted G'
    assert all(g[i] for i in range(ref.n_lines) if ref.m[i])        # and a subset of the plain one
    line_level = RegroupRef(JAVA, grep=[b"Handler.run"]).group(0, 0, True)
    assert line_level != gi  # KLF_REGROUP_INVERT keeps the rest of the matching record


def test_cut_comes_after_the_records():
    ref = RecordsRef(JAVA, grep=[b"NullPointerException"])
    frm, until = ref.ts[3], ref.ts[5]  # holds no match
    assert "".join("x" if f else "." for f in ref.cut(JAVA_OPTS, frm, until)) == "...xx...."
    assert not any(ref.cut(JAVA_OPTS, until, frm))


def _golden():
    return sorted((ROOT / "tests" / "golden").glob("*.log"))


@pytest.mark.parametrize("tail", [-1, 0, 1, 7])
def test_no_flags_and_no_prefixes_is_retail_over_m(tail):
    assert _golden(), "tests/golden/*.log is missing"
    for p in _golden():
        data = p.read_bytes()
        for grep in ([synth.NEEDLE], [b"timeout"], [b"e"]):
            ref = RecordsRef(data, grep=grep)
            assert ref.group(opts()) == ref.m
            assert ref.records(opts(), tail=tail) == RegroupRef(data, grep=grep).emit(ref.m, tail), (p.name, grep)


def test_head_mode_without_prefixes_selects_whole_streams():
    for data in [p.read_bytes()[:20000] for p in _golden()] + HAND_STREAMS:
        for grep in ([b"e"], [b"no such bytes anywhere"]):
            ref = RecordsRef(data, grep=grep)
            g = ref.group(opts(head_mode=True))
            assert g == (list(ref.parsed) if any(ref.m) else [False] * ref.n_lines)
            gi = ref.group(opts(invert=True, head_mode=True))
            assert gi == ([False] * ref.n_lines if any(ref.m) else list(ref.parsed))


def test_basic_facts_on_the_hand_streams():
    for data in HAND_STREAMS:
        for grep in ([b"ERROR"], [b"at"], [b"2024"], [b"NEEDLE"]):
            ref = RecordsRef(data, grep=grep)
            for o in HAND_OPTS:
                g = ref.group(o)
                assert all(g[i] for i in range(ref.n_lines) if ref.m[i])
                assert not any(g[i] for i in range(ref.n_lines) if not ref.parsed[i])
                recs = ref.record_list(o)
                assert sorted(i for r in recs for i in r) == [i for i in range(ref.n_lines) if ref.parsed[i]]
                assert sum(ref.class_counts(o)) == ref.n_parsed


# ------------------------------------------------ the host classifier against the Python one ---

def generated_cases(seed=20241022, n_sets=40, n_contents=100):
    """Option sets with prefixes drawn from the contents' own starts, and contents of 0..40 bytes
    over a small alphabet, so that matches, near misses and every length up to the cap occur."""
    rng = random.Random(seed)
    alphabet = b" \t\rab:C{\"\x00\xff"
    for _ in range(n_sets):
        contents = [bytes(rng.choice(alphabet) for _ in range(rng.choice((0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32,
                                                                          33, 40, rng.randrange(41)))))
                    for _ in range(n_contents)]
        pre = []
        for _ in range(rng.randrange(0, E.RECORDS_MAX_PREFIXES + 1)):
            c = rng.choice(contents)
            if not c:
                continue
            k = rng.choice((1, len(c), min(len(c), 32), rng.randrange(1, min(len(c), 32) + 1)))
            p = bytearray(c[:min(k, 32)])
            if rng.random() < 0.2:
                p[-1] ^= 1  # a near miss in the last byte
            pre.append(bytes(p))
        if rng.random() < 0.4:  # (head mode also with no prefix left)
            yield opts(head=pre, head_mode=True), contents
        else:
            yield opts(indent=rng.random() < 0.5, blank=rng.random() < 0.5, cont=pre), contents


def lib_flags(o):
    return ((E.RECORDS_INDENT if o["indent"] else 0) | (E.RECORDS_BLANK if o["blank"] else 0) |
            (E.RECORDS_PREFIX_HEAD if o["head_mode"] else 0) | (E.RECORDS_INVERT if o["invert"] else 0))


def lib_opts(o, from_=None, until=None):
    """klf_records_opts of a reference option set (head mode spelled out as its flag bit)."""
    return E.records_opts(cont=o["head"] if o["head_mode"] else o["cont"], flags=lib_flags(o), from_=from_, until=until)


def test_klf_record_class_equals_the_python_classifier():
    n = conts = 0
    lib = E.lib()
    for kw, contents in generated_cases():
        o, keep = lib_opts(kw)
        for c in contents:
            want = classify(c, **kw)
            buf = C.create_string_buffer(c, len(c) or 1)
            got = lib.klf_record_class(C.addressof(buf), len(c), C.byref(o))
            assert got == int(want), (c, kw)
            n += 1
            conts += got
    assert n >= 4000 and n // 10 < conts < n - n // 10  # both classes are common


# ------------------------------------------ the classifier header in a stand-alone program ---

HOST_CHECK = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "klf_recordcls.hpp"
static std::vector<uint8_t> unhex(const char* s) {
  std::vector<uint8_t> v;
  if (s[0] == '-') return v;
  for (; s[0] && s[1]; s += 2) { char b[3] = {s[0], s[1], 0}; v.push_back((uint8_t)strtoul(b, nullptr, 16)); }
  return v;
}
int main(int argc, char** argv) {  // lines: "P flags n" then n prefix-hex lines, or "C content-hex class"
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char kind[4], a[256];
  unsigned x, flags = 0;
  int bad = 0, n = 0;
  klf::RecordPrefixes pre{};
  while (fscanf(f, "%3s %255s %u", kind, a, &x) == 3) {
    if (kind[0] == 'P') {
      flags = (unsigned)strtoul(a, nullptr, 10);
      pre = klf::RecordPrefixes{};
      for (unsigned k = 0; k < x; ++k) {
        if (fscanf(f, "%255s", a) != 1) return 2;
        const std::vector<uint8_t> pv = unhex(a);
        klf::record_prefix_add(pre, pv.data(), (uint32_t)pv.size());
      }
      continue;
    }
    const std::vector<uint8_t> cv = unhex(a);
    uint8_t* heap = (uint8_t*)malloc(cv.size() ? cv.size() : 1);  // exactly the content: a read past it is caught
    if (!cv.empty()) memcpy(heap, cv.data(), cv.size());
    const int got = klf::record_class(klf::RecordHostLoad{}, heap, cv.size(), flags, pre);
    if (got != (int)x) { printf("case %d: class %d\n", n, got); ++bad; }
    free(heap);
    ++n;
  }
  printf("%d cases, %d wrong\n", n, bad);
  return bad ? 1 : 0;
}
"""


def test_classifier_header_stands_alone_under_sanitizers(tmp_path):
    """klf_recordcls.hpp in a program of its own (no HIP, no library), built with the address and
    undefined-behaviour sanitizers where the compiler has them: the generated contents, each in a
    heap block of exactly its length, against the Python classifier."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    text, n = [], 0
    for kw, contents in generated_cases(seed=7):
        pre = kw["head"] if kw["head_mode"] else kw["cont"]
        text.append("P %d %d\n" % (lib_flags(kw), len(pre)) + "".join(p.hex() + "\n" for p in pre))
        for c in contents:
            text.append("C %s %d\n" % (c.hex() or "-", int(classify(c, **kw))))
            n += 1
    (tmp_path / "cases.txt").write_text("".join(text))
    (tmp_path / "check.cpp").write_text(HOST_CHECK)
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'klogs_amd' / 'csrc'}",
            str(tmp_path / "check.cpp"), "-o", str(tmp_path / "check")]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program still checks the cases
        subprocess.run(base, check=True)
    r = subprocess.run([str(tmp_path / "check"), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 wrong" % n in r.stdout and n >= 4000


# ---------------------------------------------------------------- the library (no device) ---

def test_library_exports_records():
    lib = E.lib()
    for name in ("klf_records", "klf_result_records_info", "klf_record_class"):
        assert hasattr(lib, name) and name in E.SIGNATURES, name
    hdr = (ROOT / "include" / "klf.h").read_text()
    for name in ("klf_records_opts", "KLF_RECORDS_INDENT 1u", "KLF_RECORDS_BLANK 2u", "KLF_RECORDS_PREFIX_HEAD 4u",
                 "KLF_RECORDS_INVERT 8u", "KLF_RECORDS_MAX_PREFIXES 8u", "KLF_RECORDS_MAX_PREFIX 32u", "klf_records(",
                 "klf_result_records_info(", "klf_record_class("):
        assert name in hdr, name
    assert C.sizeof(E._RecordsOpts) == 56
    assert (E.RECORDS_INDENT, E.RECORDS_BLANK, E.RECORDS_PREFIX_HEAD, E.RECORDS_INVERT) == (1, 2, 4, 8)
    assert callable(E.Result.records) and callable(E.Result.records_info) and callable(E.record_class)


def raw_opts(flags=0, prefixes=(b"ab",), offsets=None, n=None, frm=OPEN_LO, until=OPEN_HI, reserved=(0, 0),
             null_bytes=False, null_off=False):
    o = E._RecordsOpts()
    o.from_.sec, o.from_.nsec, o.from_._reserved = frm[0], frm[1], reserved[0]
    o.until.sec, o.until.nsec, o.until._reserved = until[0], until[1], reserved[1]
    blob = b"".join(prefixes)
    buf = C.create_string_buffer(blob, len(blob) or 1)
    if offsets is None:
        offsets = [0]
        for p in prefixes:
            offsets.append(offsets[-1] + len(p))
    off = (C.c_uint32 * len(offsets))(*offsets)
    o.prefixes = None if null_bytes else C.addressof(buf)
    o.prefix_off = None if null_off else C.addressof(off)
    o.n_prefixes = len(prefixes) if n is None else n
    o.flags = flags
    return o, (buf, off)


BAD_OPTS = {
    "unknown flag bits": dict(flags=16),
    "a high flag bit": dict(flags=1 << 31),
    "indent with head": dict(flags=E.RECORDS_INDENT | E.RECORDS_PREFIX_HEAD),
    "blank with head": dict(flags=E.RECORDS_BLANK | E.RECORDS_PREFIX_HEAD),
    "from._reserved": dict(reserved=(1, 0)),
    "until._reserved": dict(reserved=(0, 1)),
    "from.nsec negative": dict(frm=(0, -1)),
    "until.nsec 1e9": dict(until=(0, 10**9)),
    "nine prefixes": dict(prefixes=[b"a"] * 9),
    "null prefixes": dict(null_bytes=True),
    "null prefix_off": dict(null_off=True),
    "offsets descend": dict(prefixes=(b"ab", b"cd"), offsets=[0, 3, 2]),
    "an empty prefix": dict(prefixes=(b"ab", b""), offsets=[0, 2, 2]),
    "a prefix of 33 bytes": dict(prefixes=(b"x" * 33,)),
}
GOOD_OPTS = {
    "defaults": dict(),
    "no prefixes, null arrays": dict(prefixes=(), null_bytes=True, null_off=True),
    "every flag of default mode": dict(flags=E.RECORDS_INDENT | E.RECORDS_BLANK | E.RECORDS_INVERT),
    "head mode, inverted": dict(flags=E.RECORDS_PREFIX_HEAD | E.RECORDS_INVERT),
    "eight prefixes of 32 bytes": dict(prefixes=[bytes([65 + k]) * 32 for k in range(8)]),
    "closed bounds": dict(frm=(5, 999_999_999), until=(6, 0)),
}


def test_records_bad_arguments_are_einval_without_a_device():
    lib = E.lib()
    out = C.c_void_p()
    o, keep = raw_opts()
    assert lib.klf_records(None, None, None, -1, C.byref(out)) == E.KLF_EINVAL
    assert lib.klf_records(None, None, C.byref(o), -1, None) == E.KLF_EINVAL
    assert lib.klf_records(None, None, C.byref(o), -1, C.byref(out)) == E.KLF_EINVAL   # null engine and result
    assert lib.klf_records(None, None, C.byref(o), -2, C.byref(out)) == E.KLF_EINVAL   # tail < -1
    assert lib.klf_result_records_info(None, None, None, None) == E.KLF_EINVAL
    buf = C.create_string_buffer(b"abc")
    assert lib.klf_record_class(None, 3, C.byref(o)) == E.KLF_EINVAL
    assert lib.klf_record_class(C.addressof(buf), 3, None) == E.KLF_EINVAL
    assert lib.klf_record_class(None, 0, C.byref(o)) == 0  # an empty content needs no bytes
    for name, kw in GOOD_OPTS.items():  # the helper takes what klf_records takes ...
        o, keep = raw_opts(**kw)
        assert lib.klf_record_class(C.addressof(buf), 3, C.byref(o)) in (0, 1), name
    for name, kw in BAD_OPTS.items():   # ... and refuses what it refuses: the same check, no engine, no device
        o, keep = raw_opts(**kw)
        assert lib.klf_record_class(C.addressof(buf), 3, C.byref(o)) == E.KLF_EINVAL, name
        assert lib.klf_records(None, None, C.byref(o), -1, C.byref(out)) == E.KLF_EINVAL, name
    assert out.value is None


def test_python_wrapper_refuses_head_with_default_mode_arguments():
    for kw in (dict(cont=[b"x"]), dict(indent=True), dict(blank=True)):
        with pytest.raises(ValueError):
            E.records_opts(head=[b"20"], **kw)
        with pytest.raises(ValueError):
            E.Result.records(None, head=[b"20"], **kw)  # before any call: no engine is touched
    with pytest.raises(E.KlfError):
        E.record_class(b"abc", cont=[b"x" * 33])


def test_docs_describe_records():
    for doc, words in (("SPEC.md", ("S4h", "klf_records")), ("README.md", ("--record-indent",)),
                       ("DESIGN.md", ("k_rc_heads", "k_rc_build")), ("INTEGRATION.md", ("klf_records",))):
        text = (ROOT / doc).read_text()
        for w in words:
            assert w in text, (doc, w)
