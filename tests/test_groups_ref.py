"""klf_result_groups (SPEC.md S4e: the most frequent messages of a finished run): the reference
the GPU tests compare against, an independent check of it, the host helper klf_group_key against
the Python normaliser, and the library's new ABI entries.  No GPU here."""
import collections
import ctypes as C
import functools
import random
import re
from pathlib import Path

import pytest

import klf_oracle as po
from klogs_amd import engine as E
from klogs_amd import synth
from test_window_ref import WindowRef

ROOT = Path(__file__).resolve().parent.parent
MASK = E.GROUPS_MASK_DIGITS


def normalise(content: bytes, mask: bool, max_key: int) -> bytes:
    """The S4e key of a content without its '\\n', byte by byte: cut first, mask second."""
    if max_key:
        content = content[:max_key]
    if not mask:
        return content
    out = bytearray()
    in_run = False
    for c in content:
        if 0x30 <= c <= 0x39:
            if not in_run:
                out.append(0x23)
            in_run = True
        else:
            out.append(c)
            in_run = False
    return bytes(out)


class GroupsRef(WindowRef):
    """WindowRef plus the S4e key of every line: the groups of a selection by the definition."""

    def content(self, i):
        """S1's content of line i without its terminating '\\n' (a parsed line: it has a space)."""
        s, e = self.lines[i]
        c = self.data[s:e].split(b" ", 1)[1]
        return c[:-1] if c.endswith(b"\n") else c

    def groups(self, g, top, mask=False, max_key=0):
        return grouped([self], [g], top, mask, max_key)


def grouped(refs, flags, top, mask=False, max_key=0):
    """(entries, n_groups, n_lines) over the streams `refs` with H flags `flags`: entries are
    (count, first_stream, first_line, last_stream, last_line, key) tuples in result order."""
    table = {}  # key -> [count, first, last], first / last = (stream, line)
    n_lines = 0
    for s, (ref, g) in enumerate(zip(refs, flags)):
        for i in range(ref.n_lines):
            if not (g[i] and ref.parsed[i]):
                continue
            n_lines += 1
            k = normalise(ref.content(i), mask, max_key)
            if k not in table:
                table[k] = [0, (s, i), (s, i)]
            t = table[k]
            t[0] += 1
            t[1] = min(t[1], (s, i))
            t[2] = max(t[2], (s, i))
    order = sorted(table.items(), key=lambda kv: (-kv[1][0], kv[1][1]))
    entries = [(c, f[0], f[1], l[0], l[1], k) for k, (c, f, l) in order[:top]]
    return entries, len(table), n_lines


def render_tsv(entries, names):
    """top.tsv of klogs-filter --top: names[i] = (pod, container) of stream i."""
    rows = [b"Lines\tFirstPod\tFirstContainer\tFirstLine\tLastPod\tLastContainer\tLastLine\tKey\n"]
    for c, fs, fl, ls, ll, key in entries:
        esc = b"".join(b"\\x%02X" % b if b < 0x20 or b >= 0x7F or b == 0x5C else bytes([b]) for b in key)
        rows.append(b"%d\t%s\t%s\t%d\t%s\t%s\t%d\t" % (c, names[fs][0].encode(), names[fs][1].encode(), fl + 1,
                                                     names[ls][0].encode(), names[ls][1].encode(), ll + 1) + esc + b"\n")
    return b"".join(rows)


# ------------------------------------------------------------- the inputs of the GPU tests ---

def _ts(i):
    return b"2024-10-22T%02d:%02d:%02d.%09dZ " % (i // 3600 % 24, i // 60 % 60, i % 60, i % 1000)


BY_HAND = [
    _ts(0) + b"ab123456 tail\n",
    _ts(1) + b"ab1\r\n",
    b"no-space-so-unparseable\n",
    _ts(3) + b"\n",
    _ts(4) + b"ab999999 other\n",
    _ts(5) + b"zz top\n",
    _ts(6) + b"\n",
    _ts(7) + b"ab1\n",
    _ts(8) + b"zz top",
]

TEMPLATES = 300
BIG_N = 20_000


def _template(t, a, b):
    name = bytes([97 + t // 26, 97 + t % 26])
    if t % 3 == 0:
        return b"%s handler HIT after %d ms code %d" % (name, a, b)
    if t % 3 == 1:
        return b"%s peer %d ERR_CONN_RESET retry %d" % (name, a, b)
    return b"%s ok in %d us, %d rows" % (name, a, b)


@functools.lru_cache(maxsize=None)
def big_streams():
    """A stream of BIG_N lines (> 2 chunks of 8192): 300 templates whose two numbers take six
    value pairs, so about 350 keys with the digits masked and about 1,850 without, plus 50 lines
    of their own; and a second stream of the same templates, ending in a fragment."""
    rng = random.Random(11)
    pairs = [(7, 200), (31, 404), (120, 500), (5, 200), (9999, 0), (10, 10)]
    lines = []
    for i in range(BIG_N):
        t = min(rng.randrange(TEMPLATES), rng.randrange(TEMPLATES))  # uneven counts
        a, b = pairs[rng.randrange(6)]
        lines.append(_ts(i) + _template(t, a, b) + b"\n")
    for u in range(50):
        lines[(u * 397 + 13) % BIG_N] = _ts(u) + b"one of a kind %s\n" % bytes([65 + u % 26, 65 + u // 26])
    second = [_ts(i) + _template((i * 7) % TEMPLATES, *pairs[i % 6]) + b"\n" for i in range(1500)]
    second[-1] = second[-1][:-1]
    return (b"".join(lines), b"".join(second))


def sixty_four_keys():
    """Exactly 64 distinct keys (also with the digits masked) over 700 lines in two streams."""
    keys = [b"key %s" % bytes([65 + k % 26, 97 + k // 26]) for k in range(64)]
    a = b"".join(_ts(i) + keys[(i * i) % 64] + b" %d\n" % (i % 3) for i in range(500))
    b = b"".join(_ts(i) + keys[i % 64] + b" 7\n" for i in range(200))
    return [a, b]


def odd_streams():
    """Lines of 0, 1, 15, 16, 17, 4,095 and 70,000 content bytes; digit runs across the 16-byte
    loads and the 64-byte steps; keys that differ in their last byte only or are a prefix of another; a stream whose
    length is a multiple of 256, ending unterminated in digits and directly followed by a stream
    that begins with digits; the last line of the last stream unterminated and ending in a digit run."""
    body = []
    for n in (0, 1, 15, 16, 17, 4095, 70_000):
        body.append(bytes(97 + (k * 7) % 26 for k in range(n)))
        body.append(bytes(97 + (k * 7) % 26 for k in range(n)))  # each twice: a count of 2
    for n in (14, 15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129):  # a digit run over the walks' steps of 16 / 64 bytes
        body.append(b"x" * (n - 2) + b"12345" + b"y")
        body.append(b"x" * (n - 2) + b"987" + b"y")  # the same key with the digits masked
    long = bytes(65 + (k * 11) % 26 for k in range(4095))
    body += [long + b"a", long + b"b", long, long[:100], long[:99], long[:100] + b"1", long[:100] + b"22"]
    body += [b"p" * 16, b"p" * 17, b"p" * 15 + b"q", b"p" * 16 + b"q"]
    first = b"".join(_ts(i) + c + b"\n" for i, c in enumerate(body))
    pad = -(len(first) + len(_ts(0)) + 8) % 256
    first += _ts(0) + b"e" * pad + b"end 4242"  # (8 bytes) a fragment: the next stream's digits follow its digits
    assert len(first) % 256 == 0
    second = _ts(1) + b"4242 begins with digits\n" + _ts(2) + b"e" * pad + b"end 4242\n" + _ts(3) + b"tail 123456789"
    return [first, second]


def cli_bodies():
    """(pod, container, body) of the CLI test: two containers of one pod."""
    return [("pod-0", "app", synth.generate(synth.TEXT, 81, 0, 60_000, permille=100)),
            ("pod-0", "sidecar", synth.generate(synth.TEXT, 82, 1, 40_000, permille=100, drop_final_nl=True))]


# ------------------------------------------------------------- the reference, checked ---

def _golden():
    return sorted((ROOT / "tests" / "golden").glob("*.log"))


def _independent(data, grep, mask, max_key):
    """sort | uniq -c | sort -rn over the oracle's own line split and parse, with re.sub."""
    counts, first, last = collections.Counter(), {}, {}
    for i, (s, e) in enumerate(po.split_lines(data)):
        p = po.parse_line(data[s:e])
        if p is None:
            continue
        c = po.content_for_match(p[1])
        if grep and not any(x in c for x in grep):
            continue
        k = c[:max_key] if max_key else c
        if mask:
            k = re.sub(rb"[0-9]+", b"#", k)
        counts[k] += 1
        first.setdefault(k, i)
        last[k] = i
    order = sorted(counts, key=lambda k: (-counts[k], first[k]))
    return [(counts[k], 0, first[k], 0, last[k], k) for k in order], sum(counts.values())


@pytest.mark.parametrize("grep", [(), (synth.NEEDLE,), (b"e",)], ids=["none", "needle", "e"])
def test_reference_equals_counter(grep):
    assert _golden(), "tests/golden/*.log is missing"
    inputs = [(p.name, p.read_bytes()) for p in _golden()] + [("synthetic text", synth.generate(synth.TEXT, 3, 0, 40_000))]
    seen = 0
    for name, data in inputs:
        ref = GroupsRef(data, grep=grep)
        g = ref.gprime()
        for mask in (False, True):
            for max_key in (0, 1, 7, 40):
                want, n_lines = _independent(data, grep, mask, max_key)
                got, n_groups, got_lines = ref.groups(g, 10**9, mask, max_key)
                assert got == want, (name, grep, mask, max_key)
                assert (n_groups, got_lines) == (len(want), n_lines) and sum(x[0] for x in got) == n_lines
                assert ref.groups(g, 3, mask, max_key)[0] == want[:3]
                seen += n_lines
    assert seen > 0


def test_groups_by_hand():
    ref = GroupsRef(b"".join(BY_HAND))
    assert ref.n_lines == 9 and ref.n_parsed == 8
    g = ref.gprime()
    ent, n_groups, n_lines = ref.groups(g, 100)
    assert (n_groups, n_lines) == (6, 8)  # the unparseable line is not counted
    assert ent == [(2, 0, 3, 0, 6, b""),            # the empty key; the tie with "zz top" goes to the earlier first
                   (2, 0, 5, 0, 8, b"zz top"),      # the fragment shares the terminated line's key
                   (1, 0, 0, 0, 0, b"ab123456 tail"),
                   (1, 0, 1, 0, 1, b"ab1\r"),       # '\r' stays: not the key of line 7
                   (1, 0, 4, 0, 4, b"ab999999 other"),
                   (1, 0, 7, 0, 7, b"ab1")]
    ent, n_groups, n_lines = ref.groups(g, 100, True, 5)
    assert ent == [(3, 0, 0, 0, 7, b"ab#"),         # "ab123" / "ab999" / "ab1": cut to 5 bytes, then masked
                   (2, 0, 3, 0, 6, b""),
                   (2, 0, 5, 0, 8, b"zz to"),
                   (1, 0, 1, 0, 1, b"ab#\r")]
    assert (n_groups, n_lines) == (4, 8)
    assert ref.groups(g, 2, True, 5) == (ent[:2], 4, 8)
    assert normalise(b"ab123456", True, 5) == b"ab#" and normalise(b"ab123456", True, 0) == b"ab#"
    hit = GroupsRef(b"".join(BY_HAND), grep=[b"ab"])
    assert hit.groups(hit.gprime(), 100, True, 2) == ([(4, 0, 0, 0, 7, b"ab")], 1, 4)
    # over two streams: first / last in (stream, line) order
    two = [GroupsRef(b"".join(BY_HAND[5:])), GroupsRef(b"".join(BY_HAND[:6]))]
    ent, n_groups, n_lines = grouped(two, [r.gprime() for r in two], 2)
    assert ent == [(3, 0, 0, 1, 5, b"zz top"), (2, 0, 1, 1, 3, b"")] and (n_groups, n_lines) == (6, 9)


def test_big_streams_shape():
    refs = [GroupsRef(s) for s in big_streams()]
    assert refs[0].n_lines == BIG_N > 2 * 8192 and refs[0].n_parsed == BIG_N
    flags = [r.gprime() for r in refs]
    masked = grouped(refs, flags, 10**9, True)
    plain = grouped(refs, flags, 10**9, False)
    assert 340 <= masked[1] <= 360 and 1500 <= plain[1] <= 2000
    assert any(e[1] != e[3] for e in masked[0])  # groups that span both streams
    assert len({e[0] for e in masked[0]}) < len(masked[0])  # count ties: `first` decides
    assert grouped([GroupsRef(s) for s in sixty_four_keys()], [[True] * 500, [True] * 200], 100, True)[1] == 64
    assert grouped([GroupsRef(s) for s in sixty_four_keys()], [[True] * 500, [True] * 200], 100, False)[1] > 64


# ------------------------------------------------------ klf_group_key (the host helper) ---

def _key(content, max_key, flags, cap=None):
    """(rc, key or None, n) of one klf_group_key call."""
    lib = E.lib()
    src = C.create_string_buffer(content, len(content) or 1)
    cap = len(content) if cap is None else cap
    out = C.create_string_buffer(b"\xEE" * (cap + 1), cap + 1)
    n = C.c_size_t(12345)
    rc = lib.klf_group_key(C.addressof(src), len(content), max_key, flags, C.addressof(out), cap, C.byref(n))
    assert out.raw[cap] == 0xEE  # never past cap
    return rc, (out.raw[: n.value] if rc == E.KLF_OK else out.raw[:cap]), n.value


def test_group_key_equals_the_python_normaliser():
    rng = random.Random(2024)
    lengths = list(range(0, 40)) + [rng.randrange(0, 301) for _ in range(3000)]
    assert {15, 16, 17, 31, 32, 33} <= set(lengths)
    for n in lengths:
        alphabet = rng.choice([b"0123456789", b"0123456789abc \r", bytes(range(256))])
        content = bytes(rng.choice(alphabet) for _ in range(n))
        for flags in (0, MASK):
            for max_key in (0, 1, 16, rng.randrange(1, 320)):
                rc, key, m = _key(content, max_key, flags)
                assert rc == E.KLF_OK and key == normalise(content, bool(flags), max_key), (content, flags, max_key)
                assert m == len(key)
                assert E.group_key(content, max_key, flags) == key
    assert _key(b"0123456789" * 30, 0, MASK)[1] == b"#"  # all digits
    assert _key(b"0123456789" * 30, 0, 0)[1] == b"0123456789" * 30
    assert _key(b"ab123456", 5, MASK)[1] == b"ab#"       # a digit run cut by max_key
    assert _key(b"ab123456", 2, MASK)[1] == b"ab" and _key(b"ab123456", 3, MASK)[1] == b"ab#"
    assert _key(b"12ab", 1, MASK)[1] == b"#" and _key(b"a\r\n1", 0, MASK)[1] == b"a\r\n#"
    assert _key(b"", 0, MASK) == (E.KLF_OK, b"", 0)


def test_group_key_cap_too_small_is_einval_with_the_needed_size():
    """The documented choice (klf.h): a cap below the key's length is KLF_EINVAL, *n is the needed
    size and nothing is written; cap = 0 with a null `out` sizes the buffer."""
    rc, buf, n = _key(b"abc123def", 0, MASK, cap=4)
    assert (rc, n) == (E.KLF_EINVAL, 7) and buf == b"\xEE" * 4
    assert _key(b"abc123def", 0, MASK, cap=7) == (E.KLF_OK, b"abc#def", 7)
    lib = E.lib()
    n = C.c_size_t()
    src = C.create_string_buffer(b"abc123def")
    assert lib.klf_group_key(C.addressof(src), 9, 0, MASK, None, 0, C.byref(n)) == E.KLF_EINVAL and n.value == 7
    assert lib.klf_group_key(C.addressof(src), 0, 0, MASK, None, 0, C.byref(n)) == E.KLF_OK and n.value == 0
    assert lib.klf_group_key(None, 3, 0, 0, None, 0, C.byref(n)) == E.KLF_EINVAL
    assert lib.klf_group_key(C.addressof(src), 9, 0, 2, None, 0, C.byref(n)) == E.KLF_EINVAL  # unknown flag
    assert lib.klf_group_key(C.addressof(src), 9, 0, MASK, None, 4, None) == E.KLF_EINVAL  # cap without out


# ---------------------------------------------------------------- the library (no device) ---

SYMBOLS = ("klf_result_groups", "klf_groups_entries", "klf_groups_keys", "klf_groups_totals", "klf_groups_ms",
           "klf_groups_free", "klf_group_key")


def test_library_exports_groups():
    lib = E.lib()
    hdr = (ROOT / "include" / "klf.h").read_text()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in E.SIGNATURES, name
        assert name in hdr, name
    for name in ("klf_groups_opts", "klf_group_entry", "KLF_GROUPS_MASK_DIGITS", "KLF_GROUPS_MAX_TOP",
                 "KLF_GROUPS_MAX_GROUPS"):
        assert name in hdr, name
    assert C.sizeof(E._GroupsOpts) == 16 and C.sizeof(E._GroupEntry) == 48 and E.GROUP_ENTRY.itemsize == 48
    assert [E.GROUP_ENTRY.fields[f][1] for f, _ in E._GroupEntry._fields_] == \
        [getattr(E._GroupEntry, f).offset for f, _ in E._GroupEntry._fields_]
    assert re.search(r"#define KLF_GROUPS_MASK_DIGITS 1u\b", hdr) and E.GROUPS_MASK_DIGITS == 1
    assert re.search(r"#define KLF_GROUPS_MAX_TOP 65536u\b", hdr) and E.GROUPS_MAX_TOP == 65536
    assert re.search(r"#define KLF_GROUPS_MAX_GROUPS \(1u << 26\)", hdr) and E.GROUPS_MAX_GROUPS == 1 << 26


def groups_opts(top=10, max_groups=0, max_key=0, flags=0):
    return E._GroupsOpts(top, max_groups, max_key, flags)


# every option the call refuses with KLF_EINVAL (also used on a live result by the GPU tests)
BAD_OPTS = {
    "top 0": dict(top=0),
    "top above the maximum": dict(top=65537),
    "top 2^32 - 1": dict(top=0xFFFFFFFF),
    "max_groups above the maximum": dict(max_groups=(1 << 26) + 1),
    "unknown flag": dict(flags=2),
    "unknown flags": dict(flags=0x80000001),
}


def test_groups_bad_arguments_are_einval_without_a_device():
    lib = E.lib()
    out = C.c_void_p()
    o = groups_opts()
    assert lib.klf_result_groups(None, C.byref(o), C.byref(out)) == E.KLF_EINVAL
    assert lib.klf_result_groups(None, None, C.byref(out)) == E.KLF_EINVAL
    assert lib.klf_result_groups(None, C.byref(o), None) == E.KLF_EINVAL
    for name, kw in BAD_OPTS.items():
        o = groups_opts(**kw)
        assert lib.klf_result_groups(None, C.byref(o), C.byref(out)) == E.KLF_EINVAL, name
    assert out.value is None
    n, p, ms = C.c_uint64(), C.c_void_p(), C.c_double()
    assert lib.klf_groups_entries(None, C.byref(p), C.byref(n)) == E.KLF_EINVAL
    assert lib.klf_groups_keys(None, C.byref(p), C.byref(n)) == E.KLF_EINVAL
    assert lib.klf_groups_totals(None, C.byref(n), C.byref(n)) == E.KLF_EINVAL
    assert lib.klf_groups_ms(None, C.byref(ms)) == E.KLF_EINVAL
    lib.klf_groups_free(None)  # like free(NULL)
