"""ctypes binding of the C ABI in ``include/klf.h`` (``klogs_amd/_lib/libklf.so``).

This is the same surface the Go host binds through cgo; Python uses it
for the tests and ``bench.py``.  There is deliberately no fallback: if the native
library is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

_LIB_DIR = Path(os.environ.get("KLF_LIB_DIR", Path(__file__).resolve().parent / "_lib"))
_LIB_PATH = _LIB_DIR / "libklf.so"

KLF_OK = 0
KLF_EINVAL = -1
KLF_ENOMEM = -2
KLF_EHIP = -3
KLF_EPATTERN = -4
KLF_ETOOBIG = -5
KLF_ESTATE = -6
KLF_EIO = -7
KLF_PAT_LITERAL = 0
KLF_PAT_REGEX = 1
GO_ZERO_TIME = (-62135596800, 0)
TIME_MIN_SEC = -(1 << 63)     # KLF_TIME_MIN_SEC: klf_window_opts.from.sec, open below
TIME_MAX_SEC = (1 << 63) - 1  # KLF_TIME_MAX_SEC: klf_window_opts.until.sec, open above
AROUND_MAX_NS = (1 << 62) - 1  # KLF_AROUND_MAX_NS: klf_around_opts.before_ns / after_ns at most
RECORDS_INDENT, RECORDS_BLANK, RECORDS_PREFIX_HEAD, RECORDS_INVERT = 1, 2, 4, 8  # KLF_RECORDS_* flag bits
RECORDS_MAX_PREFIXES = 8      # KLF_RECORDS_MAX_PREFIXES: klf_records_opts.n_prefixes at most
RECORDS_MAX_PREFIX = 32       # KLF_RECORDS_MAX_PREFIX: bytes of one prefix at most
HIST_MAX_BUCKETS = 65536      # KLF_HIST_MAX_BUCKETS: klf_hist_opts.n_buckets at most
TIMELINE_TIMESTAMPS = 1       # KLF_TIMELINE_TIMESTAMPS: render each line's prefix too
TIMELINE_MAX_TAG = 1024       # KLF_TIMELINE_MAX_TAG: bytes of one stream's tag at most
GROUPS_MASK_DIGITS = 1        # KLF_GROUPS_MASK_DIGITS: each run of ASCII digits in a key becomes one '#'
GROUPS_MAX_TOP = 65536        # KLF_GROUPS_MAX_TOP: klf_groups_opts.top at most
GROUPS_MAX_GROUPS = 1 << 26   # KLF_GROUPS_MAX_GROUPS: klf_groups_opts.max_groups at most
FIELD_DURATION = 1            # KLF_FIELD_DURATION: the value is a Go duration, in nanoseconds
FIELD_MAX_KEY = 64            # KLF_FIELD_MAX_KEY: klf_field_opts.key_len at most
FIELD_MAX_QUANTILES = 16      # KLF_FIELD_MAX_QUANTILES: klf_field_opts.n_quantiles at most
FIELD_HIT, FIELD_MISS, FIELD_BAD = 0, 1, 2  # KLF_FIELD_HIT / _MISS / _BAD: klf_field_value's classes

MODE_NAMES = {0: "none", 1: "never", 2: "all", 3: "literal1", 4: "general"}


class KlfError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        self.code = code
        super().__init__(f"klf error {code}: {msg}")


class _Time(C.Structure):
    _fields_ = [("sec", C.c_int64), ("nsec", C.c_int32), ("_reserved", C.c_int32)]


class _Pattern(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("len", C.c_uint32), ("kind", C.c_uint32)]


class _Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("n_patterns", C.c_uint32), ("patterns", C.POINTER(_Pattern)),
                ("hip_stream", C.c_void_p), ("staging_hint", C.c_uint64)]


class _Filter(C.Structure):
    _fields_ = [("since", _Time), ("tail", C.c_int64), ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class _RegroupOpts(C.Structure):
    _fields_ = [("before", C.c_uint32), ("after", C.c_uint32), ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class _WindowOpts(C.Structure):
    _fields_ = [("from_", _Time), ("until", _Time), ("before", C.c_uint32), ("after", C.c_uint32),
                ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class _AroundOpts(C.Structure):  # klf_around_opts (56 bytes)
    _fields_ = [("from_", _Time), ("until", _Time), ("before_ns", C.c_uint64), ("after_ns", C.c_uint64),
                ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


class _RecordsOpts(C.Structure):  # klf_records_opts (56 bytes)
    _fields_ = [("from_", _Time), ("until", _Time), ("prefixes", C.c_void_p), ("prefix_off", C.c_void_p),
                ("n_prefixes", C.c_uint32), ("flags", C.c_uint32)]


class _HistOpts(C.Structure):
    _fields_ = [("origin", _Time), ("width_ns", C.c_uint64), ("n_buckets", C.c_uint32), ("flags", C.c_uint32)]


class _TimelineOpts(C.Structure):
    _fields_ = [("tags", C.c_void_p), ("tag_off", C.c_void_p), ("flags", C.c_uint32), ("_reserved", C.c_uint32)]


# klf_timeline_entry (32 bytes)
TIMELINE_ENTRY = np.dtype([("sec", "<i8"), ("nsec", "<i4"), ("stream", "<u4"), ("line", "<u8"), ("off", "<u8")])


class _GroupsOpts(C.Structure):
    _fields_ = [("top", C.c_uint32), ("max_groups", C.c_uint32), ("max_key", C.c_uint32), ("flags", C.c_uint32)]


class _GroupEntry(C.Structure):
    _fields_ = [("count", C.c_uint64), ("first_line", C.c_uint64), ("last_line", C.c_uint64), ("key_off", C.c_uint64),
                ("first_stream", C.c_uint32), ("last_stream", C.c_uint32), ("key_len", C.c_uint32), ("_pad", C.c_uint32)]


# klf_group_entry (48 bytes)
GROUP_ENTRY = np.dtype([("count", "<u8"), ("first_line", "<u8"), ("last_line", "<u8"), ("key_off", "<u8"),
                        ("first_stream", "<u4"), ("last_stream", "<u4"), ("key_len", "<u4"), ("_pad", "<u4")])


class _FieldOpts(C.Structure):
    _fields_ = [("key", C.c_void_p), ("quantiles", C.c_void_p), ("key_len", C.c_uint32), ("decimals", C.c_uint32),
                ("n_quantiles", C.c_uint32), ("flags", C.c_uint32)]


class _FieldRow(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("hits", C.c_uint64), ("bad", C.c_uint64), ("min", C.c_int64),
                ("max", C.c_int64), ("sum_lo", C.c_uint64), ("sum_hi", C.c_int64), ("min_line", C.c_uint64),
                ("max_line", C.c_uint64), ("min_stream", C.c_uint32), ("max_stream", C.c_uint32)]


# klf_field_row (80 bytes)
FIELD_ROW = np.dtype([("lines", "<u8"), ("hits", "<u8"), ("bad", "<u8"), ("min", "<i8"), ("max", "<i8"),
                      ("sum_lo", "<u8"), ("sum_hi", "<i8"), ("min_line", "<u8"), ("max_line", "<u8"),
                      ("min_stream", "<u4"), ("max_stream", "<u4")])


class _Counts(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("parsed", C.c_uint64), ("since_ok", C.c_uint64),
                ("matched", C.c_uint64), ("selected", C.c_uint64), ("out_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# Every symbol include/klf.h and include/klf_debug.h declare, with its ctypes signature
# (checked by the CPU tests).
SIGNATURES = {
    "klf_open": (C.c_int, [C.POINTER(_Config), C.POINTER(C.c_void_p)]),
    "klf_close": (None, [C.c_void_p]),
    "klf_last_error": (C.c_char_p, [C.c_void_p]),
    "klf_strerror": (C.c_char_p, [C.c_int]),
    "klf_stage": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "klf_set_streams": (C.c_int, [C.c_void_p, C.c_uint32]),
    "klf_reset": (C.c_int, [C.c_void_p]),
    "klf_run": (C.c_int, [C.c_void_p, C.POINTER(_Filter), C.POINTER(C.c_void_p)]),
    "klf_layout": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "klf_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_uint64), C.POINTER(_Filter), C.POINTER(C.c_void_p)]),
    "klf_retail": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "klf_regroup": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_RegroupOpts), C.c_int64, C.POINTER(C.c_void_p)]),
    "klf_window": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_WindowOpts), C.c_int64, C.POINTER(C.c_void_p)]),
    "klf_around": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_AroundOpts), C.c_int64, C.POINTER(C.c_void_p)]),
    "klf_result_around_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_double)]),
    "klf_records": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_RecordsOpts), C.c_int64, C.POINTER(C.c_void_p)]),
    "klf_result_records_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_double)]),
    "klf_record_class": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_RecordsOpts)]),
    "klf_result_stream": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                    C.POINTER(_Counts)]),
    "klf_result_lines": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "klf_result_match_bits": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "klf_result_group_bits": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "klf_result_pattern_counts": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32,
                                            C.POINTER(C.c_uint32)]),
    "klf_result_histogram": (C.c_int, [C.c_void_p, C.POINTER(_HistOpts), C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_double)]),
    "klf_result_last_unparsed": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "klf_result_device_out": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64)]),
    "klf_result_write": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_uint32, C.POINTER(C.c_uint64)]),
    "klf_result_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint32)]),
    "klf_result_totals": (C.c_int, [C.c_void_p, C.POINTER(_Counts)]),
    "klf_result_index_mode": (C.c_int, [C.c_void_p]),
    "klf_result_compaction": (C.c_int, [C.c_void_p]),
    "klf_result_free": (None, [C.c_void_p]),
    "klf_result_timeline": (C.c_int, [C.c_void_p, C.POINTER(_TimelineOpts), C.POINTER(C.c_void_p)]),
    "klf_timeline_entries": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "klf_timeline_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "klf_timeline_write": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "klf_timeline_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "klf_timeline_free": (None, [C.c_void_p]),
    "klf_result_groups": (C.c_int, [C.c_void_p, C.POINTER(_GroupsOpts), C.POINTER(C.c_void_p)]),
    "klf_groups_entries": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "klf_groups_keys": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "klf_groups_totals": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "klf_groups_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "klf_groups_free": (None, [C.c_void_p]),
    "klf_group_key": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                C.POINTER(C.c_size_t)]),
    "klf_result_field_stats": (C.c_int, [C.c_void_p, C.POINTER(_FieldOpts), C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_double)]),
    "klf_field_value": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.POINTER(C.c_int64)]),
    "klf_follow_open": (C.c_int, [C.c_void_p, C.POINTER(_Filter), C.POINTER(C.c_void_p)]),
    "klf_follow_feed": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "klf_follow_flush": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "klf_follow_open_bytes": (C.c_uint64, [C.c_void_p, C.c_uint32]),
    "klf_follow_close": (None, [C.c_void_p]),
    "klf_parse_rfc3339nano": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_Time)]),
    "klf_debug_compile": (C.c_int, [C.POINTER(_Pattern), C.c_uint32, C.POINTER(C.c_uint32), C.c_char_p,
                                    C.c_size_t]),
    "klf_debug_match": (C.c_int, [C.POINTER(_Pattern), C.c_uint32, C.c_void_p, C.c_size_t,
                                  C.POINTER(C.c_int)]),
    "klf_debug_since_digits": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p]),
    "klf_debug_clock": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]),
    "klf_debug_factors": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_char_p, C.c_size_t,
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "klf_debug_prefilter": (C.c_int, [C.POINTER(_Pattern), C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32,
                                      C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "klf_debug_prefilter_hits": (C.c_int, [C.POINTER(_Pattern), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_size_t, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]),
}


def _load():
    # One HIP runtime per process: when PyTorch is present its bundled libamdhip64.so.7
    # must be the one libklf.so binds to (same SONAME), so device pointers and streams
    # from torch are valid here.  Loading libklf first would pull /opt/rocm's runtime
    # in beside torch's, and whichever initialises second sees no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not _LIB_PATH.exists():
        raise ImportError(f"{_LIB_PATH} is missing: build it with `python -m klogs_amd._build` "
                          "(the filter has no CPU fallback)")
    lib = C.CDLL(str(_LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = _load()


def lib():
    return _lib


def _check(rc: int, eng=None):
    if rc != KLF_OK:
        msg = _lib.klf_strerror(rc).decode()
        if eng is not None:
            detail = _lib.klf_last_error(eng).decode()
            if detail:
                msg += ": " + detail
        raise KlfError(rc, msg)


def _patterns(grep: Sequence[bytes], match: Sequence[bytes]):
    """The klf_pattern array (16 B each: bytes pointer, len, kind) over ONE buffer holding
    every pattern's bytes, filled with numpy (a 1,024-literal set costs microseconds, not the
    milliseconds of a ctypes object per pattern)."""
    items = [bytes(g) for g in grep] + [bytes(m) for m in match]
    n = len(items)
    lens = np.fromiter((len(b) for b in items), dtype=np.uint64, count=n)
    blob = np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8).copy()  # +1: never a zero-size buffer
    offs = np.zeros(n, dtype=np.uint64)
    if n > 1:
        np.cumsum(lens[:-1], out=offs[1:])
    rec = np.zeros(max(1, n), dtype=np.dtype([("p", "<u8"), ("len", "<u4"), ("kind", "<u4")]))
    rec["p"][:n] = np.uint64(blob.ctypes.data) + offs
    rec["len"][:n] = lens.astype(np.uint32)
    rec["kind"][:len(grep)] = KLF_PAT_LITERAL
    rec["kind"][len(grep):n] = KLF_PAT_REGEX
    arr = (_Pattern * max(1, n)).from_buffer(rec)
    return arr, n, (blob, rec)


KLF_FILTER_STAGE_TIMES = 1
KLF_FILTER_PATTERN_COUNTS = 2
KLF_FILTER_FULL_INDEX = 4
KLF_FILTER_NO_TIMING = 8
KLF_REGROUP_INVERT = 1
INDEX_MODES = {0: "full", 1: "windowed", 2: "on_demand"}  # klf_result_index_mode
COMPACTIONS = {0: "gather", 1: "tiles", 2: "one_pass"}  # klf_result_compaction


def _filter(since: Optional[Tuple[int, int]], tail: int, stage_times: bool = False,
            pattern_counts: bool = False, full_index: bool = False, timing: bool = True) -> _Filter:
    f = _Filter()
    s = GO_ZERO_TIME if since is None else since
    f.since.sec, f.since.nsec = int(s[0]), int(s[1])
    f.tail = int(tail)
    f.flags = ((KLF_FILTER_STAGE_TIMES if stage_times else 0) | (KLF_FILTER_PATTERN_COUNTS if pattern_counts else 0)
               | (KLF_FILTER_FULL_INDEX if full_index else 0) | (0 if timing else KLF_FILTER_NO_TIMING))
    return f


def layout(lens: Sequence[int]) -> Tuple[np.ndarray, int]:
    n = len(lens)
    L = (C.c_uint64 * max(1, n))(*[int(x) for x in lens])
    B = (C.c_uint64 * max(1, n))()
    tot = C.c_uint64()
    _check(_lib.klf_layout(n, L, B, C.byref(tot)))
    return np.array(B[:n], dtype=np.uint64), int(tot.value)


def parse_rfc3339nano(b: bytes) -> Optional[Tuple[int, int]]:
    t = _Time()
    buf = C.create_string_buffer(b, len(b) or 1)
    rc = _lib.klf_parse_rfc3339nano(buf, len(b), C.byref(t))
    return (t.sec, t.nsec) if rc == KLF_OK else None


def debug_compile(grep=(), match=()) -> Tuple[int, str, str]:
    arr, n, keep = _patterns(grep, match)
    mode = C.c_uint32()
    err = C.create_string_buffer(512)
    rc = _lib.klf_debug_compile(arr, n, C.byref(mode), err, 512)
    return rc, MODE_NAMES.get(mode.value, "?"), err.value.decode()


def debug_match(content: bytes, grep=(), match=()) -> bool:
    arr, n, keep = _patterns(grep, match)
    m = C.c_int()
    buf = C.create_string_buffer(content, len(content) or 1)
    _check(_lib.klf_debug_match(arr, n, buf, len(content), C.byref(m)))
    return bool(m.value)


def debug_prefilter(content: bytes, grep=(), match=(), phase: int = 0):
    """(match, {on, q, stride, needles, anchor, k, mul}) of the prefiltered general matcher on the
    host (anchor: the short needles' anchor byte, None when every needle is probed; k: bits per
    gram, 5 two-level, 6 exact; mul: the exact probe's multiplier)."""
    arr, n, keep = _patterns(grep, match)
    m = C.c_int()
    info = (C.c_uint32 * 7)()
    buf = C.create_string_buffer(content, len(content) or 1)
    _check(_lib.klf_debug_prefilter(arr, n, buf, len(content), phase, C.byref(m), info))
    return bool(m.value), dict(on=bool(info[0]), q=info[1], stride=info[2], needles=info[3],
                               anchor=(info[4] & 0xFF) if info[4] else None, k=info[5], mul=info[6])


def debug_prefilter_hits(sample: bytes, data: bytes, grep=(), match=()):
    """The prefilter layout chosen on `sample`'s statistics and its work over `data` (host):
    {stride, q, k, anchor, probes, bitmap_hits, anchor_hits, verified, pair_pass, grams, mul, layout}
    (grams: distinct probed grams; mul: the exact probe's multiplier, 0 for another kind)."""
    arr, n, keep = _patterns(grep, match)
    out = (C.c_uint64 * 11)()
    lay = C.create_string_buffer(256)
    sb = C.create_string_buffer(sample, len(sample) or 1)
    db = C.create_string_buffer(data, len(data) or 1)
    _check(_lib.klf_debug_prefilter_hits(arr, n, sb, len(sample), db, len(data), out, lay, 256))
    return dict(stride=out[0], q=out[1], k=out[2], anchor=(out[3] & 0xFF) if out[3] else None, probes=out[4],
                bitmap_hits=out[5], anchor_hits=out[6], verified=out[7], pair_pass=out[8], grams=out[9], mul=out[10],
                layout=lay.value.decode())


def debug_factors(pattern: bytes, want: int = 0):
    """(factor strings, pre bound or None, loose) of one regex, or None without a factor."""
    buf = C.create_string_buffer(4096)
    n, pre, loose = C.c_uint32(), C.c_uint32(), C.c_uint32()
    p = C.create_string_buffer(pattern, len(pattern) or 1)
    rc = _lib.klf_debug_factors(p, len(pattern), want, buf, 4096, C.byref(n), C.byref(pre), C.byref(loose))
    if rc == KLF_EINVAL:
        return None
    _check(rc)
    alts = buf.raw.split(b"\0")[: n.value]
    return alts, (None if pre.value == 0xFFFFFFFF else pre.value), bool(loose.value)


def debug_since_digits(sec: int, nsec: int = 0):
    """The since cutoff's packed digits as the scan's fast timestamp path compares them
    (six u32, klf_debug_since_digits)."""
    out = (C.c_uint32 * 6)()
    _check(_lib.klf_debug_since_digits(sec, nsec, out))
    return list(out)


def debug_clock(device: int = 0, iters: int = 200_000, reps: int = 20):
    """{median, min, max} MHz that a VALU loop holds on the device (needs a GPU)."""
    out = (C.c_double * 3)()
    _check(_lib.klf_debug_clock(device, iters, reps, out))
    return {"median_mhz": round(out[0], 1), "min_mhz": round(out[1], 1), "max_mhz": round(out[2], 1)}


class Timeline:
    """A merged timeline (klf_timeline): `entries` is a numpy structured array (TIMELINE_ENTRY:
    sec, nsec, stream, line, off), `bytes` the rendered entries in timeline order."""

    def __init__(self, ptr: int, eng):
        self._p = C.c_void_p(ptr)
        self._eng = eng

    @property
    def entries(self) -> np.ndarray:
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.klf_timeline_entries(self._p, C.byref(p), C.byref(n)), self._eng._h)
        if not n.value:
            return np.zeros(0, dtype=TIMELINE_ENTRY)
        return np.frombuffer(C.string_at(p.value, n.value * TIMELINE_ENTRY.itemsize), dtype=TIMELINE_ENTRY).copy()

    def __len__(self) -> int:
        n = C.c_uint64()
        p = C.c_void_p()
        _check(_lib.klf_timeline_entries(self._p, C.byref(p), C.byref(n)), self._eng._h)
        return int(n.value)

    @property
    def size(self) -> int:
        """Length of the merged bytes (no copy)."""
        n = C.c_uint64()
        _check(_lib.klf_timeline_bytes(self._p, None, C.byref(n)), self._eng._h)
        return int(n.value)

    @property
    def bytes(self) -> bytes:
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.klf_timeline_bytes(self._p, C.byref(p), C.byref(n)), self._eng._h)
        return C.string_at(p.value, n.value) if n.value else b""

    def write(self, fd: int) -> int:
        w = C.c_uint64()
        _check(_lib.klf_timeline_write(self._p, int(fd), C.byref(w)), self._eng._h)
        return int(w.value)

    @property
    def ms(self) -> float:
        v = C.c_double()
        _check(_lib.klf_timeline_ms(self._p, C.byref(v)), self._eng._h)
        return float(v.value)

    def free(self):
        if self._p:
            _lib.klf_timeline_free(self._p)
            self._p = C.c_void_p()


def group_key(content: bytes, max_key: int = 0, flags: int = 0) -> bytes:
    """klf_group_key: the SPEC.md S4e key of one content (without its '\\n'), by the normaliser
    the kernels run.  No GPU."""
    content = bytes(content)
    src = C.create_string_buffer(content, len(content) or 1)
    n = C.c_size_t()
    out = C.create_string_buffer(len(content) or 1)
    _check(_lib.klf_group_key(C.addressof(src), len(content), int(max_key), int(flags), C.addressof(out),
                              len(content), C.byref(n)))
    return out.raw[: n.value]


def field_value(content: bytes, key: bytes, decimals: int = 0, duration: bool = False) -> Tuple[int, int]:
    """klf_field_value: (class, value) of one content (without its '\\n') by SPEC.md S4f, from the
    extractor the kernels run; class is FIELD_HIT, FIELD_MISS or FIELD_BAD (value 0 unless a hit).
    No GPU."""
    content, key = bytes(content), bytes(key)
    src = C.create_string_buffer(content, len(content) or 1)
    kb = C.create_string_buffer(key, len(key) or 1)
    v = C.c_int64()
    rc = _lib.klf_field_value(C.addressof(src), len(content), C.addressof(kb), len(key), int(decimals),
                              FIELD_DURATION if duration else 0, C.byref(v))
    if rc < 0:
        _check(rc)
    return rc, int(v.value)


def records_opts(indent: bool = False, blank: bool = False, cont: Sequence[bytes] = (), head: Sequence[bytes] = (),
                 invert: bool = False, from_: Optional[Tuple[int, int]] = None,
                 until: Optional[Tuple[int, int]] = None, flags: Optional[int] = None):
    """(klf_records_opts, the buffers it points into) of `Result.records`' arguments.  `head`
    non-empty selects head mode; with `cont`, `indent` or `blank` beside it: ValueError.  flags:
    the raw KLF_RECORDS_* bits instead, with `cont` (or `head`) as the prefixes."""
    cont, head = [bytes(p) for p in cont], [bytes(p) for p in head]
    if head and (cont or indent or blank):
        raise ValueError("records: head prefixes exclude cont, indent and blank")
    pre = head or cont
    o = _RecordsOpts()
    lo = (TIME_MIN_SEC, 0) if from_ is None else from_
    hi = (TIME_MAX_SEC, 0) if until is None else until
    o.from_.sec, o.from_.nsec = int(lo[0]), int(lo[1])
    o.until.sec, o.until.nsec = int(hi[0]), int(hi[1])
    if flags is None:
        flags = ((RECORDS_INDENT if indent else 0) | (RECORDS_BLANK if blank else 0) |
                 (RECORDS_PREFIX_HEAD if head else 0) | (RECORDS_INVERT if invert else 0))
    o.flags = int(flags)
    o.n_prefixes = len(pre)
    blob = b"".join(pre)
    buf = C.create_string_buffer(blob, len(blob) or 1)
    off = (C.c_uint32 * (len(pre) + 1))()
    for k, p in enumerate(pre):
        off[k + 1] = off[k] + len(p)
    if pre:
        o.prefixes, o.prefix_off = C.addressof(buf), C.addressof(off)
    return o, (buf, off)


def record_class(content: bytes, indent: bool = False, blank: bool = False, cont: Sequence[bytes] = (),
                 head: Sequence[bytes] = ()) -> int:
    """klf_record_class: 1 when the content (without its '\\n') is a continuation by SPEC.md S4h, 0
    when it is a head, from the classifier the kernels run.  No GPU."""
    content = bytes(content)
    o, keep = records_opts(indent, blank, cont, head)
    src = C.create_string_buffer(content, len(content) or 1)
    rc = _lib.klf_record_class(C.addressof(src), len(content), C.byref(o))
    if rc < 0:
        _check(rc)
    return rc


class Groups:
    """Grouped counts (klf_groups): `entries` is a numpy structured array (GROUP_ENTRY: count,
    first_line, last_line, key_off, first_stream, last_stream, key_len) in result order,
    `keys()` the entries' key bytes."""

    def __init__(self, ptr: int, eng):
        self._p = C.c_void_p(ptr)
        self._eng = eng

    @property
    def entries(self) -> np.ndarray:
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.klf_groups_entries(self._p, C.byref(p), C.byref(n)), self._eng._h)
        if not n.value:
            return np.zeros(0, dtype=GROUP_ENTRY)
        return np.frombuffer(C.string_at(p.value, n.value * GROUP_ENTRY.itemsize), dtype=GROUP_ENTRY).copy()

    def __len__(self) -> int:
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.klf_groups_entries(self._p, C.byref(p), C.byref(n)), self._eng._h)
        return int(n.value)

    @property
    def key_bytes(self) -> bytes:
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.klf_groups_keys(self._p, C.byref(p), C.byref(n)), self._eng._h)
        return C.string_at(p.value, n.value) if n.value else b""

    def keys(self) -> List[bytes]:
        blob = self.key_bytes
        return [blob[int(e["key_off"]): int(e["key_off"]) + int(e["key_len"])] for e in self.entries]

    def _totals(self) -> Tuple[int, int]:
        a, b = C.c_uint64(), C.c_uint64()
        _check(_lib.klf_groups_totals(self._p, C.byref(a), C.byref(b)), self._eng._h)
        return int(a.value), int(b.value)

    @property
    def n_groups(self) -> int:
        return self._totals()[0]

    @property
    def n_lines(self) -> int:
        return self._totals()[1]

    @property
    def ms(self) -> float:
        v = C.c_double()
        _check(_lib.klf_groups_ms(self._p, C.byref(v)), self._eng._h)
        return float(v.value)

    def free(self):
        if self._p:
            _lib.klf_groups_free(self._p)
            self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


@dataclass
class StreamOut:
    out: bytes
    counts: dict


class Result:
    def __init__(self, ptr: int, n_streams: int, eng):
        self._p = C.c_void_p(ptr)
        self.n_streams = n_streams
        self._eng = eng
        self.hist_ms = 0.0  # device time of the last histogram() call

    def stream(self, i: int) -> StreamOut:
        p = C.c_void_p()
        n = C.c_uint64()
        c = _Counts()
        _check(_lib.klf_result_stream(self._p, i, C.byref(p), C.byref(n), C.byref(c)))
        data = C.string_at(p.value, n.value) if n.value else b""
        return StreamOut(data, c.as_dict())

    def lines(self, i: int) -> np.ndarray:
        p = C.c_void_p()
        n = C.c_uint64()
        _check(_lib.klf_result_lines(self._p, i, C.byref(p), C.byref(n)))
        cnt = n.value + 1
        if n.value == 0:
            return np.zeros(1, dtype=np.uint64) if p.value is None else np.frombuffer(
                C.string_at(p.value, 8), dtype=np.uint64).copy()
        return np.frombuffer(C.string_at(p.value, 8 * cnt), dtype=np.uint64).copy()

    def match_bits(self, i: int) -> bytes:
        p = C.c_void_p()
        n = C.c_uint64()
        _check(_lib.klf_result_match_bits(self._p, i, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def group_bits(self, i: int) -> bytes:
        """klf_result_group_bits: the bitmap the result was selected from, packed like
        match_bits: G' after regroup (SPEC.md S4a), the match bitmap otherwise."""
        p = C.c_void_p()
        n = C.c_uint64()
        _check(_lib.klf_result_group_bits(self._p, i, C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def pattern_counts(self, i: int) -> List[int]:
        """klf_result_pattern_counts: matching lines of stream i per pattern (the run needs
        pattern_counts=True)."""
        n = C.c_uint32()
        _check(_lib.klf_result_pattern_counts(self._p, i, None, 0, C.byref(n)), self._eng._h)
        buf = (C.c_uint64 * max(1, n.value))()
        _check(_lib.klf_result_pattern_counts(self._p, i, buf, n.value, C.byref(n)), self._eng._h)
        return [int(x) for x in buf[: n.value]]

    def histogram(self, origin: Tuple[int, int], width_ns: int, n_buckets: int) -> Tuple[np.ndarray, np.ndarray]:
        """klf_result_histogram (SPEC.md S4c): the lines of the set this result was selected from
        (M, G' or G''; the parsed lines without patterns), before --since and --tail, counted per
        stream by instant.  Returns (counts, outside): counts[i, k] = stream i's lines in
        [origin + k width_ns, origin + (k + 1) width_ns), outside[i] = (below origin, at or above
        the end), both np.uint64.  Read-only: this result stays the latest and valid.  The device
        time of the call (ms) is left in `self.hist_ms`.  Needs the stream count the result was
        made with (run(..., n_streams=)): ValueError when it is not the result's."""
        n = self.n_streams  # the library fills one row per stream of the result: the arrays must match
        if (_lib.klf_result_stream(self._p, n, None, None, None) != KLF_EINVAL
                or (n and _lib.klf_result_stream(self._p, n - 1, None, None, None) == KLF_EINVAL)):
            raise ValueError(f"histogram: the result does not have n_streams = {n} streams")
        o = _HistOpts()
        o.origin.sec, o.origin.nsec = int(origin[0]), int(origin[1])
        o.width_ns, o.n_buckets = int(width_ns), int(n_buckets)
        rows = max(1, self.n_streams)
        counts = np.zeros((rows, max(1, min(int(n_buckets), HIST_MAX_BUCKETS))), dtype=np.uint64)
        outside = np.zeros((rows, 2), dtype=np.uint64)
        ms = C.c_double()
        _check(_lib.klf_result_histogram(self._p, C.byref(o), C.c_void_p(counts.ctypes.data),
                                         C.c_void_p(outside.ctypes.data), C.byref(ms)), self._eng._h)
        self.hist_ms = float(ms.value)
        return counts[: self.n_streams], outside[: self.n_streams]

    def timeline(self, tags: Optional[Sequence[bytes]] = None, timestamps: bool = False) -> "Timeline":
        """klf_result_timeline (SPEC.md S4d): the emitted lines of all streams in one sequence
        ordered by (instant, stream, line).  tags: one byte string per stream, put in front of
        each of its entries (None: no tags); timestamps: keep each line's timestamp prefix.
        Read-only: this result stays the latest and valid.  The Timeline owns its buffers: it
        outlives later runs and must be freed before the engine is closed."""
        o = _TimelineOpts()
        keep = None
        if tags is not None:
            tags = [bytes(x) for x in tags]
            if len(tags) != self.n_streams:
                raise ValueError(f"timeline: {len(tags)} tags for {self.n_streams} streams")
            blob = np.frombuffer(b"".join(tags) + b"\0", dtype=np.uint8).copy()
            off = np.zeros(self.n_streams + 1, dtype=np.uint32)
            np.cumsum([len(x) for x in tags], out=off[1:])
            o.tags, o.tag_off = blob.ctypes.data, off.ctypes.data
            keep = (blob, off)
        o.flags = TIMELINE_TIMESTAMPS if timestamps else 0
        p = C.c_void_p()
        _check(_lib.klf_result_timeline(self._p, C.byref(o), C.byref(p)), self._eng._h)
        del keep
        return Timeline(p.value, self._eng)

    def groups(self, top: int, mask_digits: bool = False, max_key: int = 0, max_groups: int = 0) -> "Groups":
        """klf_result_groups (SPEC.md S4e): the lines of the set this result was selected from
        (M, G' or G''; the parsed lines without patterns), before --since and --tail, grouped by
        key: the content without its '\\n', cut to max_key bytes (0: all), with each run of digits
        as one '#' when mask_digits.  The first `top` groups by (count descending, first line
        ascending).  Read-only: this result stays the latest and valid.  The Groups object owns
        its buffers: it outlives later runs and must be freed before the engine is closed."""
        o = _GroupsOpts(int(top), int(max_groups), int(max_key), GROUPS_MASK_DIGITS if mask_digits else 0)
        p = C.c_void_p()
        _check(_lib.klf_result_groups(self._p, C.byref(o), C.byref(p)), self._eng._h)
        return Groups(p.value, self._eng)

    def field_stats(self, key: bytes, decimals: int = 0, duration: bool = False,
                    quantiles: Sequence[int] = ()) -> Tuple[np.ndarray, np.ndarray]:
        """klf_result_field_stats (SPEC.md S4f): over the lines of the set this result was
        selected from (M, G' or G''; the parsed lines without patterns), before --since and
        --tail, the statistics of the number behind the first `key` of each line: in units of
        10^-decimals, or with `duration` a Go duration in nanoseconds.  quantiles: permyriad
        values (0..10000), nearest rank.  Returns (rows, qvals): rows is a FIELD_ROW array of
        n_streams + 1 rows (the last one over all streams), qvals an int64 array of shape
        (n_streams + 1, len(quantiles)).  Read-only: this result stays the latest and valid.
        The device time of the call (ms) is left in `self.field_ms`."""
        key = bytes(key)
        qs = np.array([int(q) for q in quantiles], dtype=np.int64)
        if ((qs < 0) | (qs > 0xFFFF)).any():
            raise ValueError("field_stats: quantiles are permyriad values")
        q16 = qs.astype(np.uint16)
        kb = C.create_string_buffer(key, len(key) or 1)
        o = _FieldOpts(C.addressof(kb), q16.ctypes.data if len(q16) else None, len(key), int(decimals), len(q16),
                       FIELD_DURATION if duration else 0)
        rows = np.zeros(self.n_streams + 1, dtype=FIELD_ROW)
        qvals = np.zeros((self.n_streams + 1, len(q16)), dtype=np.int64)
        ms = C.c_double()
        _check(_lib.klf_result_field_stats(self._p, C.byref(o), C.c_void_p(rows.ctypes.data),
                                           C.c_void_p(qvals.ctypes.data) if len(q16) else None, C.byref(ms)),
               self._eng._h)
        self.field_ms = float(ms.value)
        return rows, qvals

    def last_unparsed(self, i: int) -> int:
        """klf_result_last_unparsed: rank from the end (over newline-terminated lines) of the
        stream's last unparseable terminated line, 0 = none."""
        v = C.c_uint64()
        _check(_lib.klf_result_last_unparsed(self._p, i, C.byref(v)))
        return int(v.value)

    def device_out(self, i: int) -> Tuple[int, int, int]:
        p = C.c_void_p()
        off = C.c_uint64()
        n = C.c_uint64()
        _check(_lib.klf_result_device_out(self._p, i, C.byref(p), C.byref(off), C.byref(n)))
        return p.value or 0, off.value, n.value

    def write_fds(self, fds: Sequence[int]) -> int:
        """klf_result_write: append stream i's selected bytes to fds[i] (< 0 skips it);
        returns the bytes written.  writeLogToDisk (cmd/root.go:359-374)."""
        arr = (C.c_int * len(fds))(*[int(f) for f in fds])
        n = C.c_uint64()
        _check(_lib.klf_result_write(self._p, arr, len(fds), C.byref(n)), self._eng._h)
        return n.value

    def write_files(self, paths: Sequence[Optional[str]]) -> int:
        """Create (truncate) paths[i] and write stream i into it (None skips the stream)."""
        fds = []
        try:
            for pth in paths:
                fds.append(-1 if pth is None else os.open(pth, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644))
            return self.write_fds(fds)
        finally:
            for f in fds:
                if f >= 0:
                    os.close(f)

    def timing(self) -> List[float]:
        ms = (C.c_double * 8)()
        k = C.c_uint32()
        _check(_lib.klf_result_timing(self._p, ms, 8, C.byref(k)))
        return list(ms[: k.value])

    def stream_counts(self, i: int) -> dict:
        """The stream's counts alone (klf_result_stream with bytes NULL: no output D2H)."""
        n = C.c_uint64()
        c = _Counts()
        _check(_lib.klf_result_stream(self._p, i, None, C.byref(n), C.byref(c)))
        return c.as_dict()

    def index_mode(self) -> str:
        """klf_result_index_mode: "full" (the run wrote every line's u64 offset), "windowed"
        (the --tail windows' lines only) or "on_demand" (none; klf_result_lines builds it)."""
        m = _lib.klf_result_index_mode(self._p)
        if m < 0:
            _check(m)
        return INDEX_MODES[m]

    def compaction(self) -> str:
        """klf_result_compaction: "gather" (the selected lines gathered), "tiles" (tile copy
        after the scan) or "one_pass" (compacted in the scan, range by range)."""
        m = _lib.klf_result_compaction(self._p)
        if m < 0:
            _check(m)
        return COMPACTIONS[m]

    def totals(self) -> dict:
        c = _Counts()
        _check(_lib.klf_result_totals(self._p, C.byref(c)))
        return c.as_dict()

    def retail(self, tail: int) -> "Result":
        """The same run with --tail N re-applied (klf_retail): counts, tail window and
        compaction only.  This result is stale afterwards (its output buffer is reused)."""
        r = C.c_void_p()
        _check(_lib.klf_retail(self._eng._h, self._p, int(tail), C.byref(r)), self._eng._h)
        return Result(r.value or 0, self.n_streams, self._eng)

    def regroup(self, before: int = 0, after: int = 0, invert: bool = False, tail: int = -1,
                flags: Optional[int] = None) -> "Result":
        """The same run with context lines and / or the match inverted (klf_regroup, SPEC.md
        S4a: grep -B / -A / --invert-match), then --tail N: always from the run's own matches,
        never from an earlier regroup.  This result is stale afterwards.  flags: the raw
        KLF_REGROUP_* bits instead of `invert`."""
        o = _RegroupOpts()
        o.before, o.after = int(before), int(after)
        o.flags = (KLF_REGROUP_INVERT if invert else 0) if flags is None else int(flags)
        r = C.c_void_p()
        _check(_lib.klf_regroup(self._eng._h, self._p, C.byref(o), int(tail), C.byref(r)), self._eng._h)
        return Result(r.value or 0, self.n_streams, self._eng)

    def window(self, from_: Optional[Tuple[int, int]] = None, until: Optional[Tuple[int, int]] = None,
               before: int = 0, after: int = 0, invert: bool = False, tail: int = -1,
               flags: Optional[int] = None) -> "Result":
        """The same run cut to the instants [from_, until) (klf_window, SPEC.md S4b), after the
        context / inversion of `regroup` and before --since and --tail N.  Bounds are
        (sec, nsec) tuples, None = open.  Always from the run's own matches (without patterns:
        its parsed lines).  This result is stale afterwards."""
        o = _WindowOpts()
        lo = (TIME_MIN_SEC, 0) if from_ is None else from_
        hi = (TIME_MAX_SEC, 0) if until is None else until
        o.from_.sec, o.from_.nsec = int(lo[0]), int(lo[1])
        o.until.sec, o.until.nsec = int(hi[0]), int(hi[1])
        o.before, o.after = int(before), int(after)
        o.flags = (KLF_REGROUP_INVERT if invert else 0) if flags is None else int(flags)
        r = C.c_void_p()
        _check(_lib.klf_window(self._eng._h, self._p, C.byref(o), int(tail), C.byref(r)), self._eng._h)
        return Result(r.value or 0, self.n_streams, self._eng)

    def around(self, before_ns: int = 0, after_ns: int = 0, from_: Optional[Tuple[int, int]] = None,
               until: Optional[Tuple[int, int]] = None, tail: int = -1, flags: int = 0) -> "Result":
        """The same run with time context across streams (klf_around, SPEC.md S4g): every parsed
        line, of every stream, whose instant lies in [ts(a) - before_ns, ts(a) + after_ns] of a
        matching line a of any stream, then cut to [from_, until) as `window` cuts, then --since
        and --tail N.  Always from the run's own matches.  This result is stale afterwards."""
        o = _AroundOpts()
        lo = (TIME_MIN_SEC, 0) if from_ is None else from_
        hi = (TIME_MAX_SEC, 0) if until is None else until
        o.from_.sec, o.from_.nsec = int(lo[0]), int(lo[1])
        o.until.sec, o.until.nsec = int(hi[0]), int(hi[1])
        o.before_ns, o.after_ns = int(before_ns), int(after_ns)
        o.flags = int(flags)
        r = C.c_void_p()
        _check(_lib.klf_around(self._eng._h, self._p, C.byref(o), int(tail), C.byref(r)), self._eng._h)
        return Result(r.value or 0, self.n_streams, self._eng)

    def around_counts(self) -> Tuple[int, int]:
        """klf_result_around_info: (anchors, merged intervals) of an `around` result."""
        n, k = C.c_uint64(), C.c_uint64()
        _check(_lib.klf_result_around_info(self._p, C.byref(n), C.byref(k), None))
        return int(n.value), int(k.value)

    def around_build_ms(self) -> float:
        """klf_result_around_info: the device time of building the selection alone (part of timing()[4])."""
        ms = C.c_double()
        _check(_lib.klf_result_around_info(self._p, None, None, C.byref(ms)))
        return float(ms.value)

    def records(self, indent: bool = False, blank: bool = False, cont: Sequence[bytes] = (),
                head: Sequence[bytes] = (), invert: bool = False, from_: Optional[Tuple[int, int]] = None,
                until: Optional[Tuple[int, int]] = None, tail: int = -1, flags: Optional[int] = None) -> "Result":
        """The same run with whole multi-line records selected (klf_records, SPEC.md S4h): every
        parsed line of each record that holds a match (invert: that holds none), a record being a
        head line and the continuation lines behind it.  A line continues a record when it is
        indented (`indent`), empty (`blank`) or starts with one of `cont`; with `head` given, when
        it starts with none of `head`.  Then cut to [from_, until) as `window` cuts, then --since
        and --tail N.  Always from the run's own matches.  This result is stale afterwards.  flags:
        the raw KLF_RECORDS_* bits instead, with `cont` (or `head`) as the prefixes."""
        o, keep = records_opts(indent, blank, cont, head, invert, from_, until, flags)
        r = C.c_void_p()
        _check(_lib.klf_records(self._eng._h, self._p, C.byref(o), int(tail), C.byref(r)), self._eng._h)
        return Result(r.value or 0, self.n_streams, self._eng)

    def records_info(self) -> Tuple[int, int, float]:
        """klf_result_records_info: (heads, continuations, build ms) of a `records` result: the
        parsed lines by class (by content alone) and the device time of building the selection
        (part of timing()[4])."""
        h, c, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        _check(_lib.klf_result_records_info(self._p, C.byref(h), C.byref(c), C.byref(ms)))
        return int(h.value), int(c.value), float(ms.value)

    def free(self):
        if self._p:
            _lib.klf_result_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """One engine = one GPU (klf_open).  grep: literals (Go bytes.Contains); match: Go
    regexp subset (SPEC.md S5)."""

    def __init__(self, device: int = 0, grep: Iterable[bytes] = (), match: Iterable[bytes] = (),
                 hip_stream: Optional[int] = None):
        arr, n, self._keep = _patterns(list(grep), list(match))
        cfg = _Config()
        cfg.device = device
        cfg.n_patterns = n
        cfg.patterns = arr
        cfg.hip_stream = hip_stream
        h = C.c_void_p()
        rc = _lib.klf_open(C.byref(cfg), C.byref(h))
        self._h = h
        if rc != KLF_OK:
            msg = _lib.klf_strerror(rc).decode()
            if h.value:
                msg += ": " + _lib.klf_last_error(h).decode()
                _lib.klf_close(h)
                self._h = C.c_void_p()
            raise KlfError(rc, msg)

    def set_streams(self, n: int):
        _check(_lib.klf_set_streams(self._h, n), self._h)

    def stage_array(self, stream_id: int, arr: np.ndarray):
        """klf_stage straight from a contiguous uint8 numpy array (no intermediate copy)."""
        a = np.ascontiguousarray(arr, dtype=np.uint8)
        _check(_lib.klf_stage(self._h, stream_id, C.c_void_p(a.ctypes.data if a.size else 0), a.size), self._h)

    def stage(self, stream_id: int, data: bytes):
        buf = C.create_string_buffer(data, len(data) or 1)
        _check(_lib.klf_stage(self._h, stream_id, buf, len(data)), self._h)

    def reset(self):
        _check(_lib.klf_reset(self._h), self._h)

    def run(self, since=None, tail: int = -1, n_streams: Optional[int] = None, stage_times: bool = False,
            pattern_counts: bool = False, full_index: bool = False, timing: bool = True) -> Result:
        f = _filter(since, tail, stage_times, pattern_counts, full_index, timing)
        r = C.c_void_p()
        _check(_lib.klf_run(self._h, C.byref(f), C.byref(r)), self._h)
        return Result(r.value or 0, n_streams if n_streams is not None else 0, self)

    def run_device(self, d_ptr: int, seg_base: Sequence[int], lens: Sequence[int], since=None,
                   tail: int = -1, stage_times: bool = False, pattern_counts: bool = False,
                   full_index: bool = False, timing: bool = True) -> Result:
        n = len(lens)
        B = (C.c_uint64 * max(1, n))(*[int(x) for x in seg_base])
        L = (C.c_uint64 * max(1, n))(*[int(x) for x in lens])
        f = _filter(since, tail, stage_times, pattern_counts, full_index, timing)
        r = C.c_void_p()
        _check(_lib.klf_run_device(self._h, C.c_void_p(d_ptr), n, B, L, C.byref(f), C.byref(r)), self._h)
        return Result(r.value or 0, n, self)

    def close(self):
        if self._h:
            _lib.klf_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
