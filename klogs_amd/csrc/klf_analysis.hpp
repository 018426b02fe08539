// klf_analysis.hpp — argument structs and host launchers of the calls on a finished run
// (SPEC.md S4a .. S4h).  Kernels live in klf_analysis.hip; the host halves are in klf_analysis.cpp
// and, for the calls that end in the run's tail stage (klf_regroup, klf_window, klf_around,
// klf_records), in klf_engine.cpp.
#pragma once
#include "klf_kernels.hpp"
#include "klf_recordcls.hpp"

namespace klf {

// What the kernels over a finished run's selected lines read of it (the regroup, time-window,
// histogram and timeline kernels; the host fills it in one place, sel_view in klf_engine.cpp).
struct SelView {
  const uint32_t* bits_in;  // the selection bitmap the kernel reads (M, G' or G''), [cap_lines / 32 + 1];
                            // null: the parsed lines (no patterns)
  const uint16_t* meta;     // [cap_lines]
  const uint64_t* line_off; // [cap_lines + nsegs] the run's line index
  const uint8_t* bytes;     // the batch
  const SegDesc* segs;      // [nsegs]
  const SegOut* segout;     // [nsegs] (line_lo / line_hi; the line count is the last line_hi)
  uint32_t nsegs;
  uint64_t cap_lines;
  uint64_t nchunks;         // kMatchChunk chunks holding lines
};

// Context lines / inverted match over a finished run (klf_regroup, SPEC.md S4a): the
// regroup kernels read the run's match bitmap M (v.bits_in) and its line meta and write the
// selection bitmap G' the tail stage then runs over.  Their own arguments: RunArgs, and with
// it every kernel of the run itself, stays as it is.
struct RegroupArgs {
  SelView v;                // (meta, segout, nsegs, cap_lines, nchunks; bits_in = M, never null)
  uint32_t* bits_out;       // G', same layout as M
  uint32_t invert;          // S = parsed lines not in M
  uint64_t before, after;   // context lines before / after a line of S
  // per kMatchChunk chunk c: [0] last line of S in the chunk + 1 (0 = none), [1] ~(its first
  // line) (0 = none); then the same over the chunks before c ([2]) / after c ([3]);
  // 4 * (cap_lines / kMatchChunk + 1) u64
  uint64_t* csum;
};

// Time window over a finished run (klf_window, SPEC.md S4b): k_tw_build reads a selection
// bitmap G' and, for each of its lines, the first 32 bytes of the line in the resident batch,
// and writes G'' = the lines of G' whose instant lies in [from, until).
struct WindowArgs {
  SelView v;                // bits_in = G'; may be bits_out (a thread reads its word before it writes it)
  uint32_t* bits_out;       // G'', same layout
  int64_t from_sec, until_sec;
  int32_t from_nsec, until_nsec;
  uint32_t from_dig[6], until_dig[6];  // the bounds packed like RunArgs::since_dig
};

// launch_retail's two steps on a selection bitmap (klf_kernels.hip calls them; nothing outside the
// library does, so they stay out of its dynamic symbol table).
// k_rg_sum / k_rg_carry / k_rg_build: the selection bitmap g.bits_out from g.v.bits_in.
__attribute__((visibility("hidden")))
hipError_t launch_regroup(const RegroupArgs& g, hipStream_t stream, int num_cus);
// k_tw_build: tw.bits_out = the lines of tw.v.bits_in inside the time window.  Nothing without lines.
__attribute__((visibility("hidden")))
hipError_t launch_window(const WindowArgs& tw, hipStream_t stream, int num_cus);

// Histogram over time of a finished run's selection (klf_result_histogram, SPEC.md S4c): k_hist
// walks a selection bitmap as k_tw_build does and counts each of its lines, by stream, below
// `org`, in bucket floor((ts - org) / width_ns), or at / above `end` = org + n_buckets * width_ns.
// It writes the table alone: the run's arrays are only read.
struct HistArgs {
  SelView v;
  uint32_t n_buckets;
  int64_t org_sec, end_sec;
  int32_t org_nsec, end_nsec;
  uint32_t end_open;        // org + the span leaves int64 seconds: no line is above
  uint32_t width_s;         // width_ns / 1e9 when that is exact and the span is below 2^32 s, else 0
  uint64_t width_ns;
  uint64_t* table;          // [nsegs * (n_buckets + 2)] per segment: the buckets, below, above (zeroed by launch_hist)
};

// Merged timeline of a finished run (klf_result_timeline, SPEC.md S4d): the emitted lines E of
// all streams, sorted by (sec, nsec, stream, line) and rendered into one buffer.
//   k_tl_count<true> / k_tl_scan   E lines per kMatchChunk chunk, their exclusive prefix -> n
//   k_tl_keys                 the selected-line walk over E: item[ord] = the line's instant, side[ord] =
//                             its (line, segment); ord = its rank in (stream, line) order
//   the sort (SortArgs)       by the 96-bit key, stable
//   k_tl_plan / k_tl_scan / k_tl_copy   rendered lengths per block of sorted positions, their
//                             prefix, then the entry records and the gather copy
// No kernel waits on another block: kernel boundaries are the only ordering.
struct alignas(16) TlItem {  // 16 B: the sort key and the line's rank before the sort
  uint64_t sec_key;   // ts.sec ^ 2^63 (unsigned order = signed order of sec)
  uint32_t nsec;
  uint32_t ord;
};
struct alignas(16) TlSide {  // 16 B, indexed by TlItem::ord
  uint64_t line;      // global line index
  uint32_t seg, _pad;
};
struct TlEntry {      // = klf_timeline_entry
  int64_t sec;
  int32_t nsec;
  uint32_t stream;
  uint64_t line, off;
};
static_assert(sizeof(TlItem) == 16 && sizeof(TlSide) == 16 && sizeof(TlEntry) == 32, "timeline records");
constexpr uint32_t kTlDigits = 12;          // 8-bit digits of the key: nsec bytes 0..3, then sec_key bytes 0..7
constexpr uint32_t kTlSortBlock = 2048;     // items per block of a radix pass (8 rounds of 256)
constexpr uint32_t kTlPlanBlock = 256;      // sorted positions per block of the plan / copy

// The sort of TlItems by their 96-bit key, stable (LSD radix, 8-bit digits), shared by the
// timeline, the grouped counts and the field statistics; each fills items[0] with a kernel of
// its own first.
//   k_tl_digits               the twelve 256-bin histograms of the key in one read
//   k_tl_bcount / k_tl_bscan / k_tl_scatter   one pass over a digit between the two item
//                             buffers; the host skips a pass whose digit is the same in all
struct SortArgs {
  TlItem* items[2];         // [n] each: the ping-pong buffers
  uint64_t n;
  uint64_t* dhist;          // [kTlDigits * 256] (zeroed by launch_sort_digits)
  uint32_t* bcnt;           // [256 * ceil(n / kTlSortBlock)] digit-major per-block counts, then offsets
};
// Zeroes s.dhist, then k_tl_digits over s.items[0].
hipError_t launch_sort_digits(const SortArgs& s, hipStream_t stream, int num_cus);
// One pass over digit `digit` from s.items[from] into s.items[from ^ 1].
hipError_t launch_sort_pass(const SortArgs& s, uint32_t digit, uint32_t from, hipStream_t stream);

// k_tl_count + k_tl_scan: per kMatchChunk chunk the lines of E (`emitted`) or of H (view_word)
// into cbase[0 .. v.nchunks), then their exclusive prefix; cbase[v.nchunks] = the total.
hipError_t launch_tl_count(const SelView& v, uint64_t* cbase, bool emitted, hipStream_t stream, int num_cus);

struct TlArgs {
  SelView v;                // bits_in null: every line (no patterns)
  uint32_t timestamps;      // render the line's prefix too
  const uint32_t* segtab;   // [3 * nsegs] per segment: stream id, tag offset, tag length
  const uint8_t* tags;      // the tag bytes (null: no tags, every length 0)
  uint64_t* cbase;          // [nchunks + 1] E lines per chunk, then their exclusive prefix and n
  uint64_t n;               // entries (known after launch_tl_count)
  TlItem* items[2];         // [n] each: the sort's buffers (k_tl_keys fills [0]; the plan and the copy read the sorted one)
  TlSide* side;             // [n]
  uint64_t* psum;           // [ceil(n / kTlPlanBlock) + 1] rendered bytes per block, then prefix and total
  TlEntry* entries;         // [n]
  uint8_t* out;             // the merged bytes
};
// k_tl_keys into g.items[0] / g.side over E; emitted false: over g.v's own bitmap, the items
// alone (g.side unread), for klf_around's anchors.
hipError_t launch_tl_keys(const TlArgs& g, bool emitted, hipStream_t stream, int num_cus);
// k_tl_plan + k_tl_scan over the sorted g.items[which]: g.psum[blocks] = the merged length.
hipError_t launch_tl_plan(const TlArgs& g, uint32_t which, hipStream_t stream);
// k_tl_copy: g.entries and g.out from the sorted g.items[which] and the scanned g.psum.
hipError_t launch_tl_copy(const TlArgs& g, uint32_t which, hipStream_t stream);

// Grouped counts of a finished run (klf_result_groups, SPEC.md S4e): the lines of H grouped by
// their key (klf_groupkey.hpp), the groups ordered by (count desc, first asc).
//   k_gr_insert               the selected-line walk over H: each line hashes its key and finds its
//                             group's slot in an open-addressing table (one u64 word per slot: a
//                             hash tag and the representative line that claimed it; equal tags
//                             are settled by comparing the two keys byte for byte), then adds to
//                             the slot's count / lowest line / highest line
//   k_gr_count / k_tl_scan    occupied slots per kGrCountBlock slots, their prefix -> n_groups
//   k_gr_fill                 one TlItem per group: key = (~count, first), 80 bits of the 96
//   the sort (SortArgs)       over those items
//   k_gr_plan / k_tl_scan / k_gr_render   key lengths of the first `top` groups, their prefix,
//                             then the entry records and the key bytes
// No kernel waits on another thread: inside k_gr_insert a thread relies on the slot words alone
// (atomicCAS / agent-scope atomic loads); everything else it reads is immutable during the call.
struct GrEntry {      // = klf_group_entry
  uint64_t count, first_line, last_line, key_off;
  uint32_t first_stream, last_stream, key_len, _pad;
};
static_assert(sizeof(GrEntry) == 48, "group records");
constexpr uint32_t kGrLineBits = 40;        // a slot word: tag << 40 | representative line + 1
constexpr uint32_t kGrCountBlock = 2048;    // slots per block of the count / fill (8 per thread)
struct GroupArgs {
  SelView v;                // bits_in null: the parsed lines (no patterns)
  uint32_t max_key, flags;  // klf_groups_opts
  uint32_t hash_bits;       // low bits of the hash that are used (64; KLF_GROUPS_HASH_BITS)
  uint32_t table_log2;      // P = 1 << table_log2 slots
  // [4 P + 2] u64, zeroed by launch_gr_insert: the slot words, then per slot the count, ~(its
  // lowest line) and its highest line (global line indices), then {|H|, table full}
  uint64_t* table;
  uint64_t* bsum;           // [P / kGrCountBlock + 1] occupied slots per block, then prefix and n_groups
  uint64_t n_groups;        // (known after launch_gr_count)
  TlItem* items;            // [n_groups] the sort's input
  uint32_t* gslot;          // [n_groups] TlItem::ord -> slot
  uint32_t top;             // groups rendered: min(opts.top, n_groups)
  uint64_t* klen;           // [top + 1] key lengths, then their prefix and the total
  const uint32_t* segstream;  // [nsegs] segment -> stream id
  GrEntry* entries;         // [top]
  uint8_t* keys;            // the key bytes
};
// Zeroes g.table, then k_gr_insert.
hipError_t launch_gr_insert(const GroupArgs& g, hipStream_t stream, int num_cus);
// k_gr_count + k_tl_scan: g.bsum[blocks] = n_groups afterwards.
hipError_t launch_gr_count(const GroupArgs& g, hipStream_t stream);
// k_gr_fill into g.items / g.gslot.
hipError_t launch_gr_fill(const GroupArgs& g, hipStream_t stream);
// k_gr_plan + k_tl_scan over the first g.top of `sorted`: g.klen[g.top] = the key bytes.
hipError_t launch_gr_plan(const GroupArgs& g, const TlItem* sorted, hipStream_t stream);
// k_gr_render: g.entries and g.keys from `sorted` and the scanned g.klen.
hipError_t launch_gr_render(const GroupArgs& g, const TlItem* sorted, hipStream_t stream);

// Numeric field statistics of a finished run (klf_result_field_stats, SPEC.md S4f): per stream and
// over all streams, how many lines of H carry `key` with a value behind it, and the minimum,
// maximum, sum and nearest-rank quantiles of those values.
//   k_tl_count<false> / k_tl_scan   H lines per kMatchChunk chunk, their exclusive prefix -> n = |H|
//   k_fs_extract              the selected-line walk over H, one lane per line: the extractor of
//                             klf_fieldval.hpp over the content, 16 bytes a load; val[rank] /
//                             cs[rank] = the line's value / segment and class, rank = its place in
//                             H in (stream, line) order; per segment lines / hits / bad and the two
//                             halves of the 128-bit sum (a wave adds once per run of lines of one
//                             segment); hits per chunk
//   k_tl_scan (twice)         the prefix of the chunks' hits -> n_hits; of the segments' hits
//   k_fs_compact              one TlItem per hit, in rank order: key = (segment, value ^ 2^63),
//                             ord = rank
//   the sort (SortArgs)       in two stages: digits 0..7 order by value (then k_fs_rows takes the
//                             all-streams row), digits 8..11 by segment (then k_fs_rows takes the
//                             segments' rows)
// Equal values keep their rank order, so the first item of a run of equal values is its lowest
// (stream, line).  No kernel waits on another block: kernel boundaries are the only ordering.
struct FsRow {        // what k_fs_rows leaves per row (the counts and sums are in FieldArgs::tab)
  int64_t min, max;
  uint64_t min_line, max_line;  // 0-based in their streams; ~0 without a hit
  uint32_t min_seg, max_seg;    // ~0 without a hit
};
static_assert(sizeof(FsRow) == 40, "field rows");
constexpr uint32_t kFsMaxQuantiles = 16;  // = KLF_FIELD_MAX_QUANTILES
constexpr uint32_t kFsMaxKey = 64;        // = KLF_FIELD_MAX_KEY
constexpr uint32_t kFsTabRows = 5;        // FieldArgs::tab: lines, hits, bad, sum_hi, sum_lo
struct FieldArgs {
  SelView v;                // bits_in null: the parsed lines (no patterns)
  uint8_t key[kFsMaxKey];
  uint32_t key_len, decimals, flags;  // klf_field_opts
  uint32_t n_q;
  uint16_t q[kFsMaxQuantiles];        // permyriad
  uint64_t* cbase;          // [nchunks + 1] H lines per chunk, then their exclusive prefix and n
  uint64_t n;               // |H| (known after launch_tl_count)
  uint64_t* hbase;          // [nchunks + 1] hits per chunk, then their exclusive prefix and n_hits
  uint64_t n_hits;          // (known after launch_fs_extract)
  int64_t* val;             // [n] a hit's value (0 otherwise)
  uint32_t* cs;             // [n] segment << 2 | class (klf_fieldval.hpp kField*)
  uint64_t* tab;            // [kFsTabRows * nsegs] per segment (zeroed by launch_fs_extract): lines, hits, bad,
                            // sum of v >> 32 (two's complement), sum of v & 0xFFFFFFFF
  uint64_t* hpre;           // [nsegs + 1] the segments' hits, then their exclusive prefix and n_hits
  TlItem* items;            // [n_hits] the sort's input
  FsRow* rows;              // [nsegs + 1]: the segments, then all streams
  int64_t* qv;              // [(nsegs + 1) * n_q]
};
// Zeroes g.tab, then k_fs_extract and the two scans: g.hbase[g.v.nchunks] = n_hits afterwards.
hipError_t launch_fs_extract(const FieldArgs& g, hipStream_t stream, int num_cus);
// k_fs_compact into g.items.
hipError_t launch_fs_compact(const FieldArgs& g, hipStream_t stream, int num_cus);
// k_fs_rows over `sorted` (null with n_hits = 0): all != 0 the all-streams row (items in value
// order), else the segments' rows (items in (segment, value) order).
hipError_t launch_fs_rows(const FieldArgs& g, const TlItem* sorted, uint32_t all, hipStream_t stream);

// Time context across streams over a finished run (klf_around, SPEC.md S4g): G' = the parsed
// lines of any stream whose instant lies in [ts(a) - before, ts(a) + after] for some anchor a, a
// line of M of any stream.
//   k_tl_count<false> / k_tl_scan   anchors per kMatchChunk chunk of M, their exclusive prefix -> n
//   k_tl_keys<false>          the selected-line walk over M: one TlItem per anchor, its instant
//   the sort (SortArgs)       by instant
//   k_ar_heads / k_tl_scan    interval heads per kArBlock sorted anchors, their prefix -> K
//   k_ar_emit                 the K disjoint closed intervals, ascending
//   k_ar_build                the selected-line walk over the parsed lines: a binary search per line
// No kernel waits on another block: kernel boundaries are the only ordering.
struct alignas(32) ArIval {  // [lo, hi], both ends closed; the search reads the first 16 bytes
  int64_t lo_sec;
  int32_t lo_nsec, hi_nsec;
  int64_t hi_sec;
  uint64_t _pad;
};
static_assert(sizeof(ArIval) == 32, "interval records");
constexpr uint32_t kArPer = 8;                  // consecutive sorted anchors per thread
constexpr uint32_t kArBlock = 256 * kArPer;     // per block of k_ar_heads / k_ar_emit
struct ArArgs {
  SelView v;                // bits_in null: k_ar_build walks the parsed lines
  const TlItem* sorted;     // [n] the anchors by instant
  uint64_t n;
  uint64_t before_sec, after_sec, span_sec;     // the durations and their sum as (sec, nsec)
  uint32_t before_nsec, after_nsec, span_nsec;
  uint64_t* bsum;           // [ceil(n / kArBlock) + 1] heads per block, then their prefix and K
  ArIval* iv;               // [k]
  uint64_t k;               // K (known after launch_ar_heads)
  uint32_t* bits_out;       // G', the layout of M
};
// k_ar_heads + k_tl_scan: g.bsum[blocks] = K afterwards.
hipError_t launch_ar_heads(const ArArgs& g, hipStream_t stream);
// k_ar_emit into g.iv, then k_ar_build into g.bits_out (every word of it).  Nothing with K = 0.
hipError_t launch_ar_build(const ArArgs& g, hipStream_t stream, int num_cus);

// Multi-line records over a finished run (klf_records, SPEC.md S4h): G' = the parsed lines of
// every record (a head and the parsed lines behind it up to the next head of its stream) that
// holds a line of M; inverted: that holds none.
//   k_rc_heads                the selected-line walk over the parsed lines, one lane per line: the
//                             classifier of klf_recordcls.hpp over at most the first 32 content
//                             bytes; the start bitmap = the heads and every segment's first line;
//                             heads / continuations counted, one atomic pair per block
//   k_rc_sum / k_rc_carry / k_rc_build   the segmented OR of M between start bits.  A start bit on
//                             every segment's first line keeps records inside their streams, so
//                             the three kernels see one sequence of L lines.  Carries are kept
//                             like k_rg_*'s, as max-scan keys of line positions: P + 1 (0 = none)
//                             of the last, ~N (0 = none) of the first line of M and of the start
//                             bitmap before / after a word.  The record open at a word's first
//                             line already holds a match iff P_M >= P_start; the one open at its
//                             last line gets one further on iff N_M < N_start.  A word or chunk
//                             without a start passes both through by construction.  Inside a
//                             word two occluded fills (five doubling steps each) spread M and the
//                             two carries up and down to the next start bit.
// The cost beside the walk's own reads is 4 x L/8 + 2L bytes read and 2 x L/8 written.  No
// kernel waits on another block: kernel boundaries are the only ordering.
struct RecordArgs {
  SelView v;                // bits_in = M, never null (k_rc_heads walks the parsed lines)
  RecordPrefixes pre;       // the caller's prefixes, by value
  uint32_t flags;           // klf_records_opts
  uint32_t* start;          // [cap_lines / 32 + 1] the start bitmap, the layout of M (zeroed by launch_records)
  uint32_t* bits_out;       // G', same layout
  // per kMatchChunk chunk c: [0] last line of M in the chunk + 1 (0 = none), [1] ~(its first
  // line) (0 = none), [2] / [3] the same of the start bitmap; then [4] / [5] = [0] over the
  // chunks before c / [1] over the chunks after c, and [6] / [7] = [2] / [3] likewise;
  // 8 * nchunks u64
  uint64_t* csum;
  uint64_t* counts;         // [2] heads, continuations (zeroed by launch_records)
};
// Zeroes g.start and g.counts, then k_rc_heads, k_rc_sum, k_rc_carry, k_rc_build into g.bits_out.
hipError_t launch_records(const RecordArgs& g, hipStream_t stream, int num_cus);

// Zeroes g.table and counts into it (k_hist).
hipError_t launch_hist(const HistArgs& g, hipStream_t stream, int num_cus);

}  // namespace klf
