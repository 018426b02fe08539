/*
 * klf.h — C ABI of the MI355X log-filter engine (libklf.so).
 *
 * This is the seam klogs' Go host binds through cgo.  It replaces
 * the byte sink `writeLogToDisk(logs io.ReadCloser, logFile *os.File)`
 * (/root/reference/cmd/root.go:359-374, called from streamLog at :337) for streams the
 * host now fetches with Timestamps=true and without SinceSeconds/TailLines
 * (getLopOpts, cmd/root.go:201-221).  The filtering kubelet used to do server-side
 * (k8s v1.30.3 logs.go ReadLogs / tail.go FindTailLineStartIndex) runs here, on the GPU,
 * with the exact semantics of SPEC.md.
 *
 * Conventions: every function returns 0 (KLF_OK) or a negative KLF_E* code; no C++
 * types, no HIP types (streams are passed as void*).  Pointers handed in are not
 * retained after return unless stated (cgo pointer rules).  Views handed out stay valid
 * until the owning object is freed.
 *
 * Threading: klf_stage may be called concurrently for DIFFERENT stream ids (one
 * goroutine per container stream, cmd/root.go:249/:261), with no other precondition (the
 * stream table grows as needed); calls for one id are in order.  Everything else is
 * single-caller per engine, and klf_run starts after every klf_stage has returned
 * (wg.Wait(), cmd/root.go:470).
 */
#ifndef KLF_H
#define KLF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------- */
#define KLF_OK 0
#define KLF_EINVAL -1      /* bad argument (null pointer, bad id, tail < -1, ...)      */
#define KLF_ENOMEM -2      /* host or device allocation failed                          */
#define KLF_EHIP -3        /* a HIP runtime call failed (no device, launch error, ...)  */
#define KLF_EPATTERN -4    /* a --match pattern is outside the supported RE2 subset     */
#define KLF_ETOOBIG -5     /* pattern set exceeds engine limits                         */
#define KLF_ESTATE -6      /* call out of order (e.g. stage after run without reset)    */
#define KLF_EIO -7         /* write(2) to a stream's file failed (klf_result_write)       */

/* ---- instants ------------------------------------------------------------------- */
/* An absolute UTC instant: seconds since the Unix epoch + nanoseconds in [0, 1e9).
 * Comparisons are lexicographic (Go time.Time.Before). */
typedef struct klf_time {
  int64_t sec;
  int32_t nsec;
  int32_t _reserved;
} klf_time;

/* Go's zero time.Time, 0001-01-01T00:00:00Z: kubelet's `since` when SinceSeconds is
 * unset (logs.go NewLogOptions); pass it for "no --since". */
#define KLF_GO_ZERO_TIME_SEC (-62135596800LL)

/* ---- patterns ------------------------------------------------------------------- */
#define KLF_PAT_LITERAL 0 /* --grep: Go bytes.Contains(content, p)                      */
#define KLF_PAT_REGEX 1   /* --match: Go regexp.Match(p, content), SPEC.md S5 subset     */

typedef struct klf_pattern {
  const uint8_t* bytes;
  uint32_t len;
  uint32_t kind; /* KLF_PAT_* */
} klf_pattern;

/* ---- engine --------------------------------------------------------------------- */
typedef struct klf_config {
  int32_t device;          /* HIP device ordinal (one process per GPU)                 */
  uint32_t n_patterns;     /* OR'ed; 0 = no grep stage                                 */
  const klf_pattern* patterns;
  void* hip_stream;        /* hipStream_t to launch on; NULL = HIP's null stream        */
  uint64_t staging_hint;   /* expected total staged bytes (pre-reserve), 0 = none       */
} klf_config;

typedef struct klf_engine klf_engine;

/* Compiles the pattern set once (replaces nothing in the reference: --grep/--match are
 * new flags added at cmd/root.go:485-497).  Every pattern error is reported here.  A set
 * with several literals starts one host thread that builds and uploads their Aho-Corasick
 * automaton while the first klf_run samples the data; that run (or klf_close) joins it. */
int klf_open(const klf_config* cfg, klf_engine** out);
void klf_close(klf_engine* e);
/* Human-readable detail of the last error on this engine (e.g. the pattern error). */
const char* klf_last_error(const klf_engine* e);
const char* klf_strerror(int code);

/* ---- host staging path (what the cgo glue calls) -------------------------------- */
/* Appends n bytes of stream `stream_id`'s body (chunks arrive in order).  Replaces the
 * io.Copy in writeLogToDisk (cmd/root.go:366).  Ids are dense, 0-based, caller-chosen
 * (the stream-table order of getPodLogs, cmd/root.go:240-262).  The bytes are copied into
 * pinned host chunks (large pieces striped over a few copy threads; KLF_STAGE_THREADS)
 * and every chunk that fills (64 MiB) is DMA'd to HBM at once, overlapping the capture.
 * KLF_ESTATE after klf_run until klf_reset. */
int klf_stage(klf_engine* e, uint32_t stream_id, const uint8_t* p, size_t n);
/* Declares stream ids [0, n_streams) (streams never staged are empty). */
int klf_set_streams(klf_engine* e, uint32_t n_streams);
/* Drops all staged bytes (engine and compiled patterns stay). */
int klf_reset(klf_engine* e);

typedef struct klf_filter {
  klf_time since;   /* lines with ts.Before(since) are dropped (S3)                    */
  int64_t tail;     /* -1 = all, else >= 0 (S4)                                        */
  uint32_t flags;   /* KLF_FILTER_* bits, 0 = none                                     */
  uint32_t _reserved;
} klf_filter;

/* klf_filter.flags: record the inner stage boundaries (klf_result_timing [0]-[3]).
 * Each boundary costs a few microseconds of idle GPU; off, only [4]-[6] are measured. */
#define KLF_FILTER_STAGE_TIMES 1u
/* klf_filter.flags: count matching lines per pattern (klf_result_pattern_counts). */
#define KLF_FILTER_PATTERN_COUNTS 2u
/* klf_filter.flags: write every line's u64 offset inside the run (KLF_INDEX_FULL), also where
 * the run needs only part of the index (see klf_result_index_mode). */
#define KLF_FILTER_FULL_INDEX 4u
/* klf_filter.flags: record no timing events (klf_result_timing then reports zeros; it
 * overrides KLF_FILTER_STAGE_TIMES).  The k_scan dispatch's own events and the run's
 * bracket cost a few microseconds of device time per run (C1: ~5 of ~75 us), which a
 * caller that never reads the timing need not pay. */
#define KLF_FILTER_NO_TIMING 8u

/* klf_result_index_mode: how much of the u64 line index the run wrote itself. */
#define KLF_INDEX_FULL 0       /* every line of every stream                                  */
#define KLF_INDEX_WINDOWS 1    /* the lines of each stream's --tail window (prefiltered sets)  */
#define KLF_INDEX_ON_DEMAND 2  /* none (no patterns, --tail -1, the dense copy path)          */

typedef struct klf_counts {
  uint64_t lines;      /* all lines (a trailing fragment counts)                       */
  uint64_t parsed;     /* lines with a valid RFC3339Nano prefix                       */
  uint64_t since_ok;   /* parsed lines with ts >= since                               */
  uint64_t matched;    /* |G|: matching parsed lines (all lines without patterns)     */
  uint64_t selected;   /* emitted lines                                               */
  uint64_t out_bytes;  /* emitted bytes                                               */
} klf_counts;

typedef struct klf_result klf_result;

/* Runs the whole filter over the staged streams (H2D, kernels, counts D2H).  Called
 * once after wg.Wait() (cmd/root.go:470). */
int klf_run(klf_engine* e, const klf_filter* f, klf_result** out);

/* ---- device-resident path (bench / callers that already hold bytes in HBM) ------- */
/* Device layout helper: segment base offsets (256-B aligned, in stream order) and the
 * total device bytes to allocate (includes tail slack the kernels may over-read).  The pad
 * between a stream's end and the next base and the slack may hold any bytes (klf_run leaves
 * an earlier batch's there), and a stream whose length is a multiple of 256 is followed at
 * once by the next one.  Results do not depend on any byte outside [seg_base, seg_base + len). */
int klf_layout(uint32_t n_streams, const uint64_t* lens, uint64_t* seg_base,
               uint64_t* total_alloc);
/* Runs over streams already laid out in device memory at d_bytes + seg_base[i]
 * (d_bytes must be a 16-B aligned device allocation of >= total_alloc bytes from klf_layout;
 * KLF_EINVAL otherwise).  The bytes between and behind the streams are the caller's: they
 * are read, never written, and whatever they hold changes no result. */
int klf_run_device(klf_engine* e, const uint8_t* d_bytes, uint32_t n_streams,
                   const uint64_t* seg_base, const uint64_t* lens, const klf_filter* f,
                   klf_result** out);

/* Re-applies the tail rule with a different N to the latest run (prev must be the
 * engine's latest result): re-runs only matched counts, the tail window and the
 * compaction on the line index, parse/since bits and match bitmap the run left in HBM.
 * The byte-range shards of one stream need it: a rank's share of the
 * global --tail is known only after the count exchange.  prev becomes stale
 * (KLF_ESTATE on access) because the output buffer is rewritten.  Replaces nothing in
 * the reference (kubelet applies --tail once, server-side: logs.go / tail.go). */
int klf_retail(klf_engine* e, klf_result* prev, int64_t tail, klf_result** out);

/* Context lines and inverted match over the latest run (SPEC.md S4a; grep -A / -B / -C and
 * --invert-match): with S = the run's matching lines M (KLF_REGROUP_INVERT: the parsed lines
 * outside M), the selection becomes G' = the parsed lines at most `after` lines behind or
 * `before` lines ahead of a line of S in the same stream (distances count every line, also
 * unparseable ones; overlapping contexts merge, no separator line, input order), and --since
 * and the tail rule with `tail` run over G' as they ran over M.  counts.matched = |G'|;
 * lines / parsed / since_ok do not change.  before = after = 0 without flags is
 * klf_retail(prev, tail) byte for byte.  Every u32 value is legal (it saturates at the
 * stream's ends).
 * The contract is klf_retail's: prev must be the engine's latest result (KLF_ESTATE) and is
 * stale afterwards; only the match bitmap (L/8 bytes) and the line meta (2 L) are read
 * again, never the input.  G' always starts from M, so regroups do not compound; a
 * klf_retail of the new result re-tails over G'; the next klf_run / klf_run_device starts
 * from its own matches.  KLF_EINVAL: an engine without patterns, o == NULL, tail < -1,
 * unknown flag bits, _reserved != 0.  Replaces nothing in the reference (its client writes
 * every line the server sends; the --grep / --match flags are new, cmd/root.go:485-497).
 * Out of scope: follow sessions (context would have to span flushes; a flush's result
 * regroups within that flush only) and shard.run_split (context would have to span the
 * byte-range shards of a stream). */
#define KLF_REGROUP_INVERT 1u
typedef struct klf_regroup_opts {
  uint32_t before, after; /* context lines ahead of / behind a line of S */
  uint32_t flags;         /* KLF_REGROUP_* bits, 0 = none */
  uint32_t _reserved;     /* 0 */
} klf_regroup_opts;
int klf_regroup(klf_engine* e, klf_result* prev, const klf_regroup_opts* o, int64_t tail, klf_result** out);

/* A time window over the latest run (SPEC.md S4b; --from / --until): with G' as klf_regroup
 * builds it from before / after / flags (G' = M when all are 0; on an engine without patterns
 * G' = the parsed lines), the selection becomes G'' = the lines of G' whose instant ts lies in
 * [from, until): from <= ts < until, compared as klf_time is (sec, then nsec).  Context is
 * taken from all of M first and cut by the window afterwards: a context line outside the
 * window is dropped, a match outside it still lends context to lines inside.  --since and the
 * tail rule with `tail` then run over G'' as they ran over M, so `until` with tail = 100 is
 * the last 100 selected lines before `until`; `from` differs from since in that it applies
 * before the tail count.  An unparseable line has no instant and is never in G'': on an
 * engine without patterns a window open on both sides equals the plain run only where every
 * line parses.  counts.matched = |G''|; lines / parsed / since_ok do not change.
 * from.sec = KLF_TIME_MIN_SEC is open below, until.sec = KLF_TIME_MAX_SEC open above;
 * from >= until is an empty window (legal, empty output).  Timestamps need not ascend: every
 * line is decided on its own.  With both bounds open and no context the call is
 * klf_retail(prev, tail) over M byte for byte on an engine with patterns.
 * The contract is klf_retail's: prev must be the engine's latest result (KLF_ESTATE) and is
 * stale afterwards.  Beside the bitmap and the line meta, each line of G' costs its line-index
 * entry and one read of the first 32 bytes of the line in the batch, which must still be
 * resident (klf_run_device: the caller's buffer); the batch is never scanned again.  A window
 * always starts from M: it never compounds with an earlier window or regroup; a klf_retail of
 * the new result re-tails over G''; a klf_regroup of it starts from M with no window; the next
 * klf_run / klf_run_device is untouched.  klf_result_group_bits returns G'' on the new result
 * and on a klf_retail of it, also on an engine without patterns.  KLF_EINVAL: a null argument,
 * tail < -1, unknown flag bits, a non-zero _reserved (also a klf_time's), nsec outside
 * [0, 1e9), non-zero before / after / flags on an engine without patterns (context needs a
 * pattern).  Replaces nothing in the reference (kubelet knows sinceTime only, a lower bound:
 * getLopOpts, cmd/root.go:201-221).  Out of scope: follow sessions and shard.run_split, as
 * for klf_regroup. */
#define KLF_TIME_MIN_SEC INT64_MIN /* from.sec: open below  */
#define KLF_TIME_MAX_SEC INT64_MAX /* until.sec: open above */
typedef struct klf_window_opts {
  klf_time from, until;   /* [from, until) */
  uint32_t before, after; /* context, as klf_regroup_opts */
  uint32_t flags;         /* KLF_REGROUP_INVERT, 0 = none */
  uint32_t _reserved;     /* 0 */
} klf_window_opts;        /* 48 bytes */
int klf_window(klf_engine* e, klf_result* prev, const klf_window_opts* o, int64_t tail, klf_result** out);

/* Time context across streams over the latest run (SPEC.md S4g; --around): what every stream
 * logged around the moments something matched.  With A (the anchors) = the matching lines M of
 * all streams together, the selection becomes G' = the parsed lines l, of any stream, for which
 * some a in A has ts(a) - before_ns <= ts(l) <= ts(a) + after_ns: both ends closed, exact
 * integer arithmetic on (sec, nsec) pairs (a duration is split into d / 1e9 and d % 1e9 with a
 * carry or borrow; one 64-bit nanosecond count would overflow at the years 0000 and 9999).
 * before_ns reaches back ahead of an anchor, after_ns behind it; the anchor's own stream is
 * treated like any other.  M is a subset of G'.  With before_ns = after_ns = 0, G' is the parsed
 * lines whose instant equals some anchor's, which may include lines outside M, also of other
 * streams: no setting makes the call klf_retail.  Timestamps need not ascend: every line is
 * decided on its own; an unparseable line has no instant and is never in G'.  Then G'' = G' cut
 * by [from, until) exactly as klf_window cuts (open bounds: no cut): context is taken from all
 * of A first, so an anchor outside the window still lends context to lines inside it.  --since
 * and the tail rule with `tail` run per stream over G'' as they ran over M.  counts.matched =
 * |G''| per stream; lines / parsed / since_ok do not change; klf_result_match_bits stays M,
 * klf_result_group_bits is G'', and the histogram, timeline, grouped counts and field statistics
 * of the new result work on G''.
 * The contract is klf_regroup's: prev must be the engine's latest result (KLF_ESTATE) and is
 * stale afterwards.  The call always starts from M and never compounds: a klf_retail of the new
 * result re-tails over G''; a klf_regroup, klf_window or klf_around of it starts from M again;
 * the next klf_run / klf_run_device is untouched.  Read again: M (L/8 bytes), the line meta,
 * the line index (built now if the run left it out) and the first 32 bytes of every parsed line
 * in the batch, which must still be resident (klf_run_device: the caller's buffer); the batch
 * is never scanned again.  All scratch of the call (the anchors' sort buffers, 2 x 16 bytes per
 * anchor, and 32 bytes per merged interval) is freed before it returns.  A run without an
 * anchor gives a valid empty selection.
 * klf_result_timing [4] of the new result is the device time of building G' plus the tail
 * stage's: two event brackets, summed, because the sort's digit read-back puts a host sync
 * between them (the first bracket spans the build's three small read-backs: the anchor
 * count, the sort's digit histograms, the interval count).
 * KLF_EINVAL (checked first, without touching the device, with a klf_last_error text): a null
 * argument, tail < -1, non-zero flags or _reserved (also a klf_time's), nsec outside [0, 1e9),
 * a duration above KLF_AROUND_MAX_NS, an engine without patterns.  KLF_ETOOBIG: 2^32 or more
 * anchors.  KLF_ENOMEM: the scratch does not fit.  Replaces nothing in the reference.  Out of
 * scope: follow sessions and shard.run_split, as for klf_regroup; a same-stream-only mode;
 * inversion or line context combined with it. */
#define KLF_AROUND_MAX_NS ((1ull << 62) - 1)
typedef struct klf_around_opts {
  klf_time from, until;          /* [from, until), as klf_window_opts; open bounds = no cut */
  uint64_t before_ns, after_ns;  /* each <= KLF_AROUND_MAX_NS */
  uint32_t flags;                /* 0 */
  uint32_t _reserved;            /* 0 */
} klf_around_opts;               /* 56 bytes */
int klf_around(klf_engine* e, klf_result* prev, const klf_around_opts* o, int64_t tail, klf_result** out);
/* On a klf_around result: the anchors |A|, the disjoint intervals K they merged into, and the
 * device time in ms of building G' alone, the first of the two brackets of klf_result_timing [4]
 * (all 0 on every other result, also on a klf_retail of an around result).  Each pointer may be
 * NULL. */
int klf_result_around_info(const klf_result* r, uint64_t* anchors, uint64_t* intervals, double* build_ms);

/* Multi-line records over the latest run (SPEC.md S4h; --record-*): a stack trace, a panic dump
 * or a traceback reaches us as one parsed line per physical line; this call selects whole
 * records, not single lines.  Per stream, over its parsed lines in input order, with C(l) = the
 * S1 content of line l without its terminating '\n' (a '\r' stays; an unterminated trailing
 * fragment counts like a terminated line):
 * - a parsed line is a continuation by its content alone.  Default mode: KLF_RECORDS_INDENT is
 *   set, C is non-empty and C[0] is ' ' or '\t'; or KLF_RECORDS_BLANK is set and C is empty; or C
 *   starts with one of the prefixes (bytewise; a prefix longer than C does not match, one equal
 *   to C does).  Head mode (KLF_RECORDS_PREFIX_HEAD; INDENT and BLANK must be clear): C starts
 *   with none of the prefixes (typical ones: `{"level":`, `I0`, `E0`, `W0`, `20`).
 * - every other parsed line is a head, and so is the first parsed line of a stream whatever its
 *   content: orphan continuations at a stream's start form a record of their own and never join
 *   the previous stream.  A record is a head plus the parsed lines behind it up to the next head
 *   of the same stream.  Unparseable lines belong to no record, do not interrupt one (as
 *   klf_regroup's context runs across them) and are never selected.
 * - G' = the parsed lines of every record that holds at least one line of M; with
 *   KLF_RECORDS_INVERT, of every record that holds none (grep -v at record level, not
 *   KLF_REGROUP_INVERT's line-level S).  M is a subset of G' without invert, disjoint with it.
 * - G'' = G' cut by [from, until) exactly as klf_window cuts (open bounds: no cut), afterwards: a
 *   record whose match lies outside the window still contributes its lines inside it.  --since
 *   and the tail rule with `tail` then run over G'' as they ran over M.
 * counts.matched = |G''| per stream; lines / parsed / since_ok do not change;
 * klf_result_match_bits stays M, klf_result_group_bits is G'', and the histogram, timeline, grouped
 * counts and field statistics of the new result work on G''.  Degenerate settings are legal:
 * default mode without flags and prefixes makes every line a head, and the call is
 * klf_retail(prev, tail) over M byte for byte; head mode without prefixes makes each stream one
 * record, selected whole if anything in it matched.
 * The contract is klf_regroup's: prev must be the engine's latest result (KLF_ESTATE) and is
 * stale afterwards.  The call always starts from M and never compounds: a klf_retail of the new
 * result re-tails over G''; a klf_regroup, klf_window, klf_around or klf_records of it starts from
 * M again; the next klf_run / klf_run_device is untouched.  Read again: M, the line meta, the
 * line index (built now if the run left it out) and at most the first 32 content bytes of every
 * parsed line in the batch, which must still be resident; no result depends on a byte outside a
 * line's [start, end).  The scratch (a second bitmap of L/8 bytes and 64 bytes per 8192 lines) is
 * freed before the call returns.  klf_result_timing [4] of the new result is the device time of
 * building G' plus the tail stage's, as for klf_around.
 * KLF_EINVAL (checked first, without touching the device, with a klf_last_error text where an
 * engine is given): a null argument, tail < -1, unknown flag bits, INDENT or BLANK together with
 * PREFIX_HEAD, a non-zero _reserved of a klf_time, nsec outside [0, 1e9), n_prefixes above
 * KLF_RECORDS_MAX_PREFIXES, n_prefixes > 0 with null prefixes or prefix_off, offsets that do not
 * ascend, an empty prefix or one longer than KLF_RECORDS_MAX_PREFIX, an engine without patterns.
 * KLF_ENOMEM: the scratch does not fit.  Replaces nothing in the reference.  Out of scope: follow
 * sessions and shard.run_split, as for klf_regroup; a cap on a record's length; regex or
 * case-insensitive head rules; line context or --around combined with it in one call; a sparse
 * variant that walks outward from the matches only. */
#define KLF_RECORDS_INDENT 1u
#define KLF_RECORDS_BLANK 2u
#define KLF_RECORDS_PREFIX_HEAD 4u
#define KLF_RECORDS_INVERT 8u
#define KLF_RECORDS_MAX_PREFIXES 8u
#define KLF_RECORDS_MAX_PREFIX 32u
typedef struct klf_records_opts {
  klf_time from, until;        /* [from, until), as klf_window_opts; open bounds = no cut */
  const uint8_t* prefixes;     /* all prefixes concatenated; may be NULL iff n_prefixes == 0 */
  const uint32_t* prefix_off;  /* n_prefixes + 1 offsets into prefixes, ascending */
  uint32_t n_prefixes, flags;  /* KLF_RECORDS_* bits */
} klf_records_opts;            /* 56 bytes */
int klf_records(klf_engine* e, klf_result* prev, const klf_records_opts* o, int64_t tail, klf_result** out);
/* On a klf_records result: the parsed lines classified head / continuation by content alone (the
 * first-line rule not applied; heads + conts = the parsed lines of all streams) and the device
 * time in ms of building G' alone; zeros on every other result, also on a klf_retail of a records
 * result.  Each pointer may be NULL. */
int klf_result_records_info(const klf_result* r, uint64_t* heads, uint64_t* conts, double* build_ms);
/* Host helper, no GPU: the S4h class of one content (without its '\n'), by the classifier the
 * kernels run (klf_recordcls.hpp): 1 = continuation, 0 = head.  from / until / KLF_RECORDS_INVERT
 * of `o` are checked but do not bear on the class.  KLF_EINVAL: a null content with len > 0, a
 * null o, or options klf_records refuses. */
int klf_record_class(const uint8_t* content, size_t len, const klf_records_opts* o);

/* ---- results -------------------------------------------------------------------- */
/* Selected bytes of one stream (host view, D2H on first access; bytes == NULL: len and
 * counts only, no D2H). */
int klf_result_stream(klf_result* r, uint32_t stream_id, const uint8_t** bytes,
                      uint64_t* len, klf_counts* counts);
/* Line-start offsets of one stream: n_lines+1 u64 (last = stream length).  Runs that did
 * not need the whole line index (no patterns with --tail -1, or literal patterns: only the
 * tail windows' lines were indexed) build it here on first use, on the device. */
int klf_result_lines(klf_result* r, uint32_t stream_id, const uint64_t** off,
                     uint64_t* n_lines);
/* Match bitmap of one stream (bit l LSB-first in byte l>>3); *nbytes = ceil(lines/8).
 * Returns KLF_EINVAL when the engine has no patterns. */
int klf_result_match_bits(klf_result* r, uint32_t stream_id, const uint8_t** bits,
                          uint64_t* nbytes);
/* Selection bitmap of one stream, packed like klf_result_match_bits: G' on a result of
 * klf_regroup (and on a klf_retail of one), M on every other result (klf_result_match_bits
 * returns M on all of them); G'' on a result of klf_window that cut or regrouped (and on a
 * klf_retail of one), and on a result of klf_around or klf_records (and on a klf_retail of
 * one).  KLF_EINVAL when the engine has no patterns, except on a klf_window
 * result (and a klf_retail of one): there it is G'', a subset of the parsed lines. */
int klf_result_group_bits(klf_result* r, uint32_t stream_id, const uint8_t** bits,
                          uint64_t* nbytes);
/* Per-pattern match counts of one stream (SURVEY.md §8a K4/K5 `count[stream][pattern]`, the
 * per-stream record the ranks gather, §8e): counts[p] = parsed lines whose content matches
 * pattern p (klf_config order; a line matching several patterns counts for each), for
 * p < min(cap, n_patterns); *n = n_patterns.  Independent of --since / --tail, like
 * klf_counts.matched.  The run must set KLF_FILTER_PATTERN_COUNTS (KLF_ESTATE otherwise).
 * A pattern that matches every content (an empty --grep, a regex such as `x*`) counts every
 * parsed line, also beside other patterns, whose counts are then evaluated as usual (their
 * tables are compiled on the first run that asks for counts).  Extends the size report of printLogSize
 * (cmd/root.go:279-309) with the new --grep / --match flags (:485-497). */
int klf_result_pattern_counts(klf_result* r, uint32_t stream_id, uint64_t* counts, uint32_t cap, uint32_t* n);
/* Histogram over time of the set the result was selected from (SPEC.md S4c; --histogram): per
 * stream, the parsed lines of H = what klf_result_group_bits returns (M on a run's result or a
 * klf_retail of one, G' after klf_regroup, G'' after klf_window; on an engine without patterns
 * a run's result counts every parsed line) are counted by their instant ts: below `origin`
 * (outside[2 i]), in bucket floor((ts - origin) / width_ns) when that is below n_buckets
 * (counts[i * n_buckets + k]: bucket k is [origin + k w, origin + (k + 1) w), closed below and
 * open above like the window), else at or above the end (outside[2 i + 1]).  ts - origin is
 * taken in nanoseconds as an exact integer.  Per stream below + the buckets + above = |H| =
 * klf_counts.matched (klf_counts.parsed on a run's result of an engine without patterns): like
 * matched the histogram is taken before --since and --tail.  Timestamps need not ascend; every
 * origin with nsec in [0, 1e9) is legal, also sec = INT64_MIN / INT64_MAX.
 * Read-only: r stays the engine's latest result and stays valid, its output, bitmaps and counts
 * are untouched, it can be windowed, regrouped or re-tailed afterwards, and the call may be
 * repeated with other options.  Read again: the bitmap (L/8 bytes; the line meta, 2 L, without
 * patterns) and, per line of H, its line-index entry (built now if the run left it out) and the
 * first 32 bytes of the line in the batch, which must still be resident (klf_run_device: the
 * caller's buffer).  counts: n_streams x n_buckets u64, row-major; outside (nullable): n_streams
 * x 2 {below, above}; *ms (nullable): device time of the call's table memset and kernel.  A
 * stream without bytes gets zeros.
 * KLF_EINVAL (checked first, without touching the device): null r, o or counts; width_ns == 0;
 * n_buckets == 0 or above KLF_HIST_MAX_BUCKETS; n_buckets * width_ns >= 2^63 (spans up to about
 * 292 years); nsec outside [0, 1e9); non-zero flags or origin._reserved.  KLF_ESTATE: r is not
 * the engine's latest result.  KLF_ETOOBIG: non-empty streams * (n_buckets + 2) > 2^24 (the
 * device table stays within 128 MiB).  Replaces nothing in the reference; it extends the size
 * report of printLogSize (cmd/root.go:279-309), like klf_result_pattern_counts.  Not promised:
 * follow sessions and shard.run_split (their per-stream rows simply add). */
#define KLF_HIST_MAX_BUCKETS 65536u
typedef struct klf_hist_opts {
  klf_time origin;     /* lower edge of bucket 0, inclusive */
  uint64_t width_ns;   /* >= 1 */
  uint32_t n_buckets;  /* 1 .. KLF_HIST_MAX_BUCKETS; n_buckets * width_ns < 2^63 */
  uint32_t flags;      /* 0 */
} klf_hist_opts;       /* 32 bytes */
int klf_result_histogram(klf_result* r, const klf_hist_opts* o, uint64_t* counts, uint64_t* outside, double* ms);
/* Position of the stream's last unparseable newline-terminated line, counted from the end
 * over the newline-terminated lines (1 = the last one; 0 = every terminated line parses).
 * The byte-range shards of one stream need it: kubelet emits the trailing
 * fragment when the --tail window holds an unparseable line (SPEC.md S4), and that line
 * may sit in an earlier shard.  Reads the latest run's line meta (KLF_ESTATE otherwise). */
int klf_result_last_unparsed(klf_result* r, uint32_t stream_id, uint64_t* rank);
/* Device views: the concatenated output and the stream's [off, len) in it.  No copy, except
 * for a one-pass result (KLF_COMPACT_ONEPASS), whose per-range extents the first call joins
 * into a second engine-owned device buffer the size of the output; that buffer is freed when
 * the engine's next run starts (the view is stale by then anyway) or at klf_close. */
int klf_result_device_out(klf_result* r, uint32_t stream_id, const uint8_t** d_out,
                          uint64_t* off, uint64_t* len);
/* Output write path: appends every stream's selected bytes to its open
 * file, fds[i] for stream i (fds[i] < 0 skips the stream), at the descriptor's current
 * offset with write(2), as io.Copy(logFile, logs) does in writeLogToDisk
 * (cmd/root.go:359-374).  The device output is copied D2H through 64 MiB pinned chunks,
 * double-buffered (DMA of the next 32 MiB while the current one is written).  With 8 MiB
 * or more of output and distinct descriptors, up to 8 worker threads (KLF_WRITE_THREADS
 * overrides) each own whole streams, so files are written in parallel and each file still
 * sees one in-order write(2) sequence; a descriptor shared by several streams gets them in
 * stream order from one thread.  EINTR and short writes are retried.  n_fds must equal
 * the stream count.  *written (optional) = bytes written over all streams.  KLF_EIO
 * (klf_last_error names the stream and errno text) reports the first failing write. */
int klf_result_write(klf_result* r, const int* fds, uint32_t n_fds, uint64_t* written);
/* Per-stage device time of the run in ms, HIP events on the launch stream:
 * [0] scan stage (newline + line index + timestamp + since + fused grep prefilter),
 * [1] pattern verification / matchers, [2] counts + tail + window prefix, [3] compaction
 * (these four only with KLF_FILTER_STAGE_TIMES, else 0), [4] total device time,
 * [5] workspace memsets (KLF_FILTER_STAGE_TIMES, else 0), [6] the k_scan kernel alone
 * (part of [0]): the start / end timestamps of its own dispatch (hipExtLaunchKernel
 * events, no event record beside it), [7] the dense copy kernel k_tcopy alone, the same way
 * (part of [3]; it exits at once when the run takes the sparse gather path).  With
 * KLF_GRAPH=1 a batch of at most KLF_GRAPH_MAX_MB (default 256) MiB whose run repeats the
 * previous run's arguments replays its launch sequence as a HIP graph: such a run reports
 * [4] only, a graph's replays recording no per-kernel events.  n = entries written. */
int klf_result_timing(const klf_result* r, double* ms, uint32_t cap, uint32_t* n);
/* Totals across streams. */
int klf_result_totals(const klf_result* r, klf_counts* totals);
/* KLF_INDEX_* of the run (klf_result_lines builds the rest on demand, after the run). */
int klf_result_index_mode(const klf_result* r);
/* klf_result_compaction: how the run put the selected bytes together in HBM. */
#define KLF_COMPACT_GATHER 0   /* line gather of the selected lines (--tail windows, sparse)   */
#define KLF_COMPACT_TILES 1    /* tile copy after the scan (most lines selected)               */
#define KLF_COMPACT_ONEPASS 2  /* in the scan itself, each tile range in place (no patterns,   */
                               /* --tail -1): a stream's output is a few extents in HBM, the   */
                               /* host views / klf_result_write join them, klf_result_device_out */
                               /* makes one contiguous copy on demand                          */
int klf_result_compaction(const klf_result* r);
void klf_result_free(klf_result* r);

/* ---- merged timeline (SPEC.md S4d; --merge) ---------------------------------------- */
/* The emitted lines of all streams of a finished run in one chronological sequence.  For a
 * result r that is the engine's latest (a run's, or a klf_retail / klf_regroup / klf_window
 * result; with or without patterns, any compaction), E(i) = the lines of stream i whose
 * contents make up r's output for that stream (after since and the tail rule;
 * |E(i)| = klf_counts.selected).  The timeline is the union of the E(i) ordered by
 * (ts.sec, ts.nsec, stream id, line number): equal instants keep stream order, then input
 * order; timestamps need not ascend within a stream; offsets compare by instant.  Entry k
 * renders as tag[stream] + P + content + N: the caller's tag bytes of the stream (none with
 * tags == NULL), P = the line's prefix up to and including its first space with
 * KLF_TIMELINE_TIMESTAMPS (else nothing), the S1 content, and N = "\n" iff the line has no
 * terminating '\n' (an emitted trailing fragment never glues onto the next entry).  The merged
 * bytes are the rendered entries in timeline order.
 * Read-only like klf_result_histogram: r stays the latest result and stays valid, its output,
 * bitmaps and counts are untouched, and the call may be repeated with other options.  Read
 * again: the selection bitmap, the line meta, per emitted line its line-index entry (built now
 * if the run left it out) and its bytes in the batch, which must still be resident.
 * A timeline owns its device and host buffers: it stays valid through later runs and
 * klf_reset until klf_timeline_free, which must come before klf_close.  The sort's scratch
 * is freed before klf_result_timeline returns.  Host views copy D2H on first access.
 * klf_timeline_entries: entry k's rendered length is off[k + 1] - off[k], the last one's
 * len - off[n - 1].  klf_timeline_bytes with bytes == NULL gives the length only (no copy).
 * klf_timeline_write appends the merged bytes to fd through the pinned double-buffered D2H
 * path of klf_result_write (EINTR and short writes retried, KLF_EIO).  klf_timeline_ms: device
 * time of the call, first launch to last.
 * KLF_EINVAL (checked first, without touching the device): null r, o or out; unknown flag
 * bits; non-zero _reserved; tags with a null tag_off; tag_off not ascending; a tag longer than
 * KLF_TIMELINE_MAX_TAG.  KLF_ESTATE: r is not the engine's latest result.  KLF_ETOOBIG: more
 * than 2^32 - 1 entries.  KLF_ENOMEM: an allocation failed.  A result with no emitted line
 * gives a valid empty timeline (n = 0, len = 0).  Not promised: follow sessions (a flush's
 * timeline covers that flush) and shard.run_split.  Replaces nothing in the reference, whose
 * per-container files (cmd/root.go:341-374) stay as they are. */
#define KLF_TIMELINE_TIMESTAMPS 1u
#define KLF_TIMELINE_MAX_TAG 1024u
typedef struct klf_timeline klf_timeline;
typedef struct klf_timeline_opts {
  const uint8_t* tags;      /* all tags concatenated; NULL = no tags (tag_off ignored) */
  const uint32_t* tag_off;  /* n_streams + 1 offsets into tags */
  uint32_t flags, _reserved;
} klf_timeline_opts;
typedef struct klf_timeline_entry {  /* 32 bytes */
  int64_t sec;
  int32_t nsec;
  uint32_t stream;
  uint64_t line;  /* 0-based in its stream */
  uint64_t off;   /* start in the merged bytes */
} klf_timeline_entry;
int klf_result_timeline(klf_result* r, const klf_timeline_opts* o, klf_timeline** out);
int klf_timeline_entries(klf_timeline* t, const klf_timeline_entry** e, uint64_t* n);
int klf_timeline_bytes(klf_timeline* t, const uint8_t** bytes, uint64_t* len);
int klf_timeline_write(klf_timeline* t, int fd, uint64_t* written);
int klf_timeline_ms(const klf_timeline* t, double* ms);
void klf_timeline_free(klf_timeline* t);

/* ---- grouped counts (SPEC.md S4e; --top K) ------------------------------------------ */
/* The most frequent messages of a finished run: sort | uniq -c | sort -rn | head over the set r
 * was selected from, without copying a line to the host.  For a result r that is the engine's
 * latest, H is klf_result_histogram's H: the parsed lines of M (a run's result or a klf_retail
 * of one), G' (klf_regroup), G'' (klf_window), or every parsed line on a run's result of an
 * engine without patterns; taken before --since and --tail, like klf_counts.matched.  The key of
 * a line is its S1 content without the terminating '\n' (a '\r' stays), cut to its first max_key
 * bytes when max_key > 0, then, with KLF_GROUPS_MASK_DIGITS, with every maximal run of ASCII
 * '0'..'9' replaced by one '#' (truncation first, masking second).  The empty key is a key; a
 * terminated line and an unterminated fragment with the same content share one.  Each distinct
 * key is a group: count = its lines in H, first / last = its lowest / highest line in (stream
 * id, line number) order over all streams.  Groups are ordered by count descending, then first
 * ascending (a total order); the object holds the first min(top, n_groups) of them, and
 * klf_groups_totals gives n_groups (distinct keys) and n_lines = |H| = the sum of every group's
 * count = klf_counts.matched over the streams (klf_counts.parsed on a run's result of an engine
 * without patterns).  Two lines are in one group iff their keys are byte-equal: hashing only
 * chooses where the device table is probed.
 * Read-only like klf_result_histogram: r stays the latest result and stays valid, nothing of it
 * is written, and the call may be repeated with other options.  Read again: the selection
 * bitmap (L/8 bytes; the line meta, 2 L, without patterns) and, per line of H, its line-index
 * entry (built now if the run left it out), its meta and its content bytes in the batch, which
 * must still be resident (klf_run_device: the caller's buffer).  On an engine without patterns
 * that is a second full read of the batch.
 * A klf_groups owns its device and host buffers (the entry records and their key bytes): it
 * stays valid through later runs and klf_reset until klf_groups_free, which must come before
 * klf_close.  The hash table and the sort's scratch are freed before klf_result_groups returns.
 * Host views copy D2H on first access.  klf_groups_entries: entry k's key is key_len bytes at
 * key_off of klf_groups_keys' bytes.  klf_groups_ms: device time of the call, first launch to
 * last.
 * KLF_EINVAL (checked first, without touching the device): null r, o or out; top == 0 or above
 * KLF_GROUPS_MAX_TOP; max_groups above KLF_GROUPS_MAX_GROUPS (0 means 2^20); unknown flag bits.
 * KLF_ESTATE: r is not the engine's latest result.  KLF_ETOOBIG: more than max_groups distinct
 * keys (this depends on the number of distinct keys alone; klf_last_error suggests masking or a
 * larger max_groups), or 2^40 or more lines in the run.  KLF_ENOMEM: an allocation failed (the
 * table takes 32 bytes a slot, 2 to 4 slots per max_groups, fewer when the run has fewer lines).  An H with no
 * line gives a valid empty object (n_groups = 0, no entries).  Not promised: follow sessions (a
 * flush's groups cover that flush) and shard.run_split.  Replaces nothing in the reference,
 * whose per-container files (cmd/root.go:341-374) stay as they are. */
#define KLF_GROUPS_MASK_DIGITS 1u
#define KLF_GROUPS_MAX_TOP 65536u
#define KLF_GROUPS_MAX_GROUPS (1u << 26)
typedef struct klf_groups_opts {   /* 16 bytes */
  uint32_t top;         /* 1 .. KLF_GROUPS_MAX_TOP: entries returned at most */
  uint32_t max_groups;  /* distinct keys the call can hold; 0 = 2^20 */
  uint32_t max_key;     /* key = the first max_key content bytes; 0 = all */
  uint32_t flags;       /* KLF_GROUPS_* */
} klf_groups_opts;
typedef struct klf_group_entry {   /* 48 bytes */
  uint64_t count;
  uint64_t first_line, last_line;  /* 0-based in their streams */
  uint64_t key_off;                /* start in the key bytes */
  uint32_t first_stream, last_stream;
  uint32_t key_len, _pad;
} klf_group_entry;
typedef struct klf_groups klf_groups;
int klf_result_groups(klf_result* r, const klf_groups_opts* o, klf_groups** out);
int klf_groups_entries(klf_groups* g, const klf_group_entry** e, uint64_t* n);
int klf_groups_keys(klf_groups* g, const uint8_t** bytes, uint64_t* len);
int klf_groups_totals(const klf_groups* g, uint64_t* n_groups, uint64_t* n_lines);
int klf_groups_ms(const klf_groups* g, double* ms);
void klf_groups_free(klf_groups* g);
/* Host helper, no GPU: the S4e key of one content (without its '\n'), by the normaliser the
 * kernels run (klf_groupkey.hpp).  *n (nullable) = the key's length, whatever cap is; the key is
 * written only when it fits: a cap below the key's length is KLF_EINVAL with *n set and nothing
 * written, so a call with cap = 0 sizes the buffer.  out may be null when cap is 0.  KLF_EINVAL
 * also for a null content with len > 0 and for unknown flag bits. */
int klf_group_key(const uint8_t* content, size_t len, uint32_t max_key, uint32_t flags,
                  uint8_t* out, size_t cap, size_t* n);

/* ---- numeric field statistics (SPEC.md S4f; --stat KEY) ------------------------------ */
/* How slow: the statistics of a numeric field such as latency_ms= or took= over the set r was
 * selected from, without copying a line to the host.  For a result r that is the engine's latest,
 * H is klf_result_histogram's and klf_result_groups' H: the parsed lines of M (a run's result or a
 * klf_retail of one), G' (klf_regroup), G'' (klf_window), or every parsed line on a run's result
 * of an engine without patterns; taken before --since and --tail, like klf_counts.matched.
 * Each line of H is classified from its content C alone (its S1 content without the terminating
 * '\n'; a '\r' stays; an unterminated fragment like a terminated line).  A line in which `key`
 * (1..64 arbitrary bytes, compared bytewise) does not occur is a miss.  Otherwise only the key's
 * first occurrence counts: behind it at most 4 bytes of { ' ', '\t', '=', ':', '"' } are skipped,
 * then an optional single '-' or '+', then a run of ASCII digits of any length (at least one)
 * and, if a '.' and a digit follow, a run of fraction digits.  Where a digit is missing, or C
 * ends first, the line is bad: the key is there, a value is not.  Plain mode: the value is the
 * number in units of 10^-decimals, cut toward zero ("12.3456" with decimals = 2 is 1234);
 * whatever follows the number is ignored ("12ms" is 12, "1e5" is 1).  With KLF_FIELD_DURATION
 * (decimals = 0) the value is nanoseconds by the prefix grammar of Go's time.ParseDuration: one or
 * more components number-then-unit with nothing between them (ns, us, µs, μs, ms, s, m, h,
 * longest match first; another component follows iff the next byte is a digit; the sign stands
 * before the first only), each worth int * unit + floor(first 9 fraction digits * unit / 1e9);
 * a component without a unit (a bare number too) makes the line bad.  A magnitude (a duration's
 * total) of 2^62 or more makes the line bad.  Every other line is a hit with |value| < 2^62.
 * rows[i] is stream i's row (a zero row for a stream without bytes), rows[n_streams] the row over
 * all streams: lines = |H|, hits, bad (misses = lines - hits - bad), min / max over the hits,
 * their exact sum as a 128-bit two's-complement pair, and the lowest (stream id, line number)
 * whose value is min / max; lines are 0-based in their streams.  Without a hit min = max = sum =
 * 0, the *_line fields are UINT64_MAX and the *_stream fields UINT32_MAX.  qvals[i * n_quantiles +
 * k] is row i's quantile quantiles[k] (permyriad, any order, duplicates allowed) by nearest rank:
 * of the row's n hits in ascending order the one at index max(1, ceil(q n / 10000)) - 1, so
 * 0 is min and 10000 is max; 0 with n = 0.
 * Read-only like klf_result_histogram: r stays the latest result and stays valid, nothing of it
 * is written, and the call may be repeated with other options.  Read again: the selection
 * bitmap (L/8 bytes; the line meta, 2 L, without patterns) and, per line of H, its line-index
 * entry (built now if the run left it out), its meta and its content bytes in the batch, which
 * must still be resident (klf_run_device: the caller's buffer).  On an engine without patterns
 * that is a second full read of the batch.  The outputs are the caller's arrays; all device
 * scratch (12 bytes per line of H, 32 per hit) is freed before the call returns, and two calls
 * with the same options give the same bytes.  *ms (nullable): device time of the call, first
 * launch to last.
 * KLF_EINVAL (checked first, without touching the device): null r, o, rows or key; key_len
 * outside 1..KLF_FIELD_MAX_KEY; decimals above 9, or non-zero with KLF_FIELD_DURATION; unknown
 * flag bits; n_quantiles above KLF_FIELD_MAX_QUANTILES; a quantile above 10000; null qvals or
 * quantiles with n_quantiles > 0.  KLF_ESTATE: r is not the engine's latest result.
 * KLF_ETOOBIG: 2^32 or more lines in H.  KLF_ENOMEM: an allocation failed.  Not promised: follow
 * sessions (a flush's statistics cover that flush) and shard.run_split.  Replaces nothing in the
 * reference, whose per-container files (cmd/root.go:341-374) stay as they are. */
#define KLF_FIELD_DURATION 1u
#define KLF_FIELD_MAX_KEY 64u
#define KLF_FIELD_MAX_QUANTILES 16u
typedef struct klf_field_opts {      /* 32 bytes */
  const uint8_t* key;
  const uint16_t* quantiles;         /* n_quantiles permyriad values; may be NULL iff n_quantiles == 0 */
  uint32_t key_len;                  /* 1 .. KLF_FIELD_MAX_KEY */
  uint32_t decimals;                 /* 0 .. 9; 0 with KLF_FIELD_DURATION */
  uint32_t n_quantiles;              /* 0 .. KLF_FIELD_MAX_QUANTILES */
  uint32_t flags;                    /* KLF_FIELD_* */
} klf_field_opts;
typedef struct klf_field_row {       /* 80 bytes */
  uint64_t lines, hits, bad;
  int64_t min, max;
  uint64_t sum_lo; int64_t sum_hi;
  uint64_t min_line, max_line;
  uint32_t min_stream, max_stream;
} klf_field_row;
int klf_result_field_stats(klf_result* r, const klf_field_opts* o, klf_field_row* rows /* n_streams + 1 */,
                           int64_t* qvals /* (n_streams + 1) * n_quantiles; NULL iff n_quantiles == 0 */,
                           double* ms /* nullable: device time, first launch to last */);
/* Host helper, no GPU: the S4f class and value of one content (without its '\n'), by the extractor
 * the kernels run (klf_fieldval.hpp).  Returns KLF_FIELD_HIT with *value set, KLF_FIELD_MISS or
 * KLF_FIELD_BAD (*value = 0), or KLF_EINVAL: a null content with len > 0, a null key or value,
 * key_len outside 1..KLF_FIELD_MAX_KEY, decimals above 9 or non-zero with KLF_FIELD_DURATION,
 * unknown flag bits. */
#define KLF_FIELD_HIT 0
#define KLF_FIELD_MISS 1
#define KLF_FIELD_BAD 2
int klf_field_value(const uint8_t* content, size_t len, const uint8_t* key, uint32_t key_len,
                    uint32_t decimals, uint32_t flags, int64_t* value);

/* ---- follow mode (-f) -------------------------------------------- */
/* The reference streams each container until EOF with Follow set (cmd/root.go:217-218,
 * streamLog :312-339, the "ended prematurely" warning :314-318) while the main goroutine
 * waits for 'q' (pressKeyToExit :399-421).  In follow mode the server keeps applying
 * SinceSeconds / TailLines to the backlog, so the engine applies what is per line: since
 * and the grep set (tail is -1; the filter's tail is ignored).  A session carries every
 * stream's open (unterminated) line across the chunks fed to it; each flush runs ONE engine
 * batch over the complete lines all streams received since the previous flush. */
typedef struct klf_follow klf_follow;
int klf_follow_open(klf_engine* e, const klf_filter* f, klf_follow** out);
/* Appends bytes read from stream `stream_id` (any split; concurrent calls for different
 * ids are safe, as klf_stage).  Complete lines are staged on the engine at once. */
int klf_follow_feed(klf_follow* fw, uint32_t stream_id, const uint8_t* p, size_t n);
/* Filters what is complete; final != 0 also flushes every stream's open line (the streams'
 * EOF: kubelet emits the last unterminated line).  *out covers stream ids [0, max id fed];
 * a stream fed nothing since the last flush has 0 lines.  The previous flush's result
 * stays valid until this call (results of the session share the engine's workspace). */
int klf_follow_flush(klf_follow* fw, int final, klf_result** out);
/* Bytes of the stream's open line (received, not yet filtered). */
uint64_t klf_follow_open_bytes(const klf_follow* fw, uint32_t stream_id);
void klf_follow_close(klf_follow* fw);

/* ---- host-side helpers mirroring cmd/root.go (no GPU needed) ---------------------- */
/* Go time.Parse(time.RFC3339Nano, s) restated (SPEC.md S2); 0 = ok. */
int klf_parse_rfc3339nano(const uint8_t* s, size_t n, klf_time* out);

#ifdef __cplusplus
}
#endif
#endif /* KLF_H */
