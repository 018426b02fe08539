// klf_analysis.cpp — the host halves of the calls on a finished run that make an object or a
// table of their own: klf_result_histogram, klf_result_timeline, klf_result_groups,
// klf_result_field_stats (SPEC.md S4c .. S4f), and klf_around's and klf_records' selection bitmaps
// (S4g, S4h).  They read
// the latest run's workspace through sel_view and launch the kernels of klf_analysis.hip; the run
// itself, and the calls that end in its tail stage, are klf_engine.cpp's.
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <cerrno>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "klf_engine_impl.hpp"
#include "klf_fieldval.hpp"
#include "klf_groupkey.hpp"
#include "klf_recordcls.hpp"

using namespace klf_impl;

// ------------------------------------------ the scaffold of a call on a finished run ---

namespace {
// What a call (klf_result_histogram, _timeline, _groups, _field_stats) holds for its duration:
// device buffers and the two events around its device time, given back on every return path.
// `fn` is the calling function's name and `noun` what it makes, for the messages.
struct CallScratch {
  klf_engine* e;
  const char *fn, *noun;
  hipStream_t st;
  std::vector<DevBuf> bufs;
  hipEvent_t ev[2] = {nullptr, nullptr};
  CallScratch(klf_engine* e_, const char* fn_, const char* noun_) : e(e_), fn(fn_), noun(noun_), st(e_->stream) {}
  CallScratch(const CallScratch&) = delete;
  ~CallScratch() {
    for (DevBuf& b : bufs) b.release();
    for (auto& x : ev)
      if (x) (void)hipEventDestroy(x);
  }
  // any buffer: the call's own or one of the object it returns
  int alloc(DevBuf& b, size_t bytes, const char* what) {
    const hipError_t h = b.ensure(bytes);
    if (h == hipSuccess) return KLF_OK;
    (void)hipGetLastError();
    if (h == hipErrorOutOfMemory) return set_err(e, KLF_ENOMEM, std::string(fn) + ": alloc " + what);
    return hip_err(e, h, what);
  }
  // a buffer of the call
  template <class T>
  int alloc(T*& p, size_t bytes, const char* what) {
    DevBuf b;
    const int rc = alloc(b, bytes, what);
    p = b.as<T>();
    bufs.push_back(b);
    return rc;
  }
  std::string msg(const char* a, const char* b = "") const { return std::string(a) + noun + b; }
  // The device time: start() before the first launch, then finish() after the last one, or
  // stop() there and elapsed() behind a sync of the caller's own.
  int start() {
    for (auto& x : ev) HIPCHK(e, hipEventCreate(&x), msg("", " events").c_str());
    HIPCHK(e, hipEventRecord(ev[0], st), msg("record ", " start").c_str());
    return KLF_OK;
  }
  int stop() {
    HIPCHK(e, hipEventRecord(ev[1], st), msg("record ", " end").c_str());
    return KLF_OK;
  }
  int elapsed(double& ms) {
    float f = 0.f;
    HIPCHK(e, hipEventElapsedTime(&f, ev[0], ev[1]), msg("", " timing").c_str());
    ms = f;
    return KLF_OK;
  }
  int finish(double& ms) {
    if (int rc = stop()) return rc;
    HIPCHK(e, hipStreamSynchronize(st), msg("sync ").c_str());
    return elapsed(ms);
  }
};

// The sort of n TlItems by their key (klf_analysis.hpp, SortArgs) as the host drives it:
// prepare(n), the caller's kernel fills s.items[0], digits() makes the digit histograms and
// reads them back (one copy, one sync), passes(p0, p1) runs the passes over the digits p0 ..
// p1 - 1 that differ somewhere (one bin holding all n: nothing to move); sorted() is the buffer
// the last pass wrote.  With n = 0 nothing is allocated, launched or read back.
struct DeviceSort {
  CallScratch& sc;
  klf::SortArgs s{};
  uint32_t cur = 0;
  std::vector<uint64_t> dh;
  explicit DeviceSort(CallScratch& sc_) : sc(sc_) {}
  int prepare(uint64_t n) {
    s.n = n;
    if (!n) return KLF_OK;
    for (auto& it : s.items)
      if (int rc = sc.alloc(it, (size_t)n * sizeof(klf::TlItem), "sort items")) return rc;
    return sc.alloc(s.dhist, (size_t)klf::kTlDigits * 256 * 8, "digit histograms");
  }
  int digits() {
    if (!s.n) return KLF_OK;
    dh.resize((size_t)klf::kTlDigits * 256);
    HIPCHK(sc.e, klf::launch_sort_digits(s, sc.st, sc.e->num_cus), "launch k_tl_digits");
    HIPCHK(sc.e, hipMemcpyAsync(dh.data(), s.dhist, dh.size() * 8, hipMemcpyDeviceToHost, sc.st), "D2H digit histograms");
    HIPCHK(sc.e, hipStreamSynchronize(sc.st), "sync digit histograms");
    return KLF_OK;
  }
  int passes(uint32_t p0, uint32_t p1) {
    for (uint32_t p = p0; p < p1 && s.n; ++p) {
      bool one_bin = false;
      for (uint32_t d = 0; d < 256 && !one_bin; ++d) one_bin = dh[(size_t)p * 256 + d] == s.n;
      if (one_bin) continue;
      if (!s.bcnt) {
        const size_t nblocks = (size_t)((s.n + klf::kTlSortBlock - 1) / klf::kTlSortBlock);
        if (int rc = sc.alloc(s.bcnt, nblocks * 256 * 4, "block digit counts")) return rc;
      }
      HIPCHK(sc.e, klf::launch_sort_pass(s, p, cur, sc.st), "launch radix pass");
      cur ^= 1u;
    }
    return KLF_OK;
  }
  klf::TlItem* sorted() const { return s.items[cur]; }
};
}  // namespace

// klf_around's selection bitmap (SPEC.md S4g; the kernels: klf_analysis.hpp, ArArgs).
int klf_impl::around_build(klf_engine* e, const klf_result* prev, const klf_around_opts* o, double& ms, uint64_t& n,
                        uint64_t& k) {
  hipStream_t st = e->stream;
  CallScratch sc(e, "klf_around", "around");
  klf::TlArgs t{};
  t.v = sel_view(prev);
  t.v.bits_in = e->d_bits.as<uint32_t>();  // M: the anchors, whatever prev was selected from
  uint32_t* gbits = e->d_gbits.as<uint32_t>();
  if (int rc = sc.alloc(t.cbase, (t.v.nchunks + 1) * 8, "chunk bases")) return rc;
  if (int rc = sc.start()) return rc;
  // 1. anchors per chunk -> n
  HIPCHK(e, klf::launch_tl_count(t.v, t.cbase, false, st, e->num_cus), "launch k_tl_count");
  n = k = 0;
  HIPCHK(e, hipMemcpyAsync(&n, t.cbase + t.v.nchunks, 8, hipMemcpyDeviceToHost, st), "D2H anchor count");
  HIPCHK(e, hipStreamSynchronize(st), "sync anchor count");
  if (n > 0xFFFFFFFFull) return set_err(e, KLF_ETOOBIG, "klf_around: 2^32 or more anchors");
  if (!n) {  // no anchor: a valid empty selection
    HIPCHK(e, hipMemsetAsync(gbits, 0, (size_t)(t.v.cap_lines / 32 + 1) * 4, st), "zero selection bitmap");
    return sc.finish(ms);
  }
  // 2. one item per anchor, 3. sorted by instant
  t.n = n;
  DeviceSort sort(sc);
  if (int rc = sort.prepare(n)) return rc;
  for (int i = 0; i < 2; ++i) t.items[i] = sort.s.items[i];
  HIPCHK(e, klf::launch_tl_keys(t, false, st, e->num_cus), "launch k_tl_keys");
  if (int rc = sort.digits()) return rc;
  if (int rc = sort.passes(0, klf::kTlDigits)) return rc;
  // 4. the merged intervals, 5. the parsed lines inside one
  klf::ArArgs g{};
  g.v = t.v;
  g.v.bits_in = nullptr;
  g.sorted = sort.sorted();
  g.n = n;
  const uint64_t span = o->before_ns + o->after_ns;  // < 2^63
  g.before_sec = o->before_ns / 1000000000ull;
  g.before_nsec = (uint32_t)(o->before_ns % 1000000000ull);
  g.after_sec = o->after_ns / 1000000000ull;
  g.after_nsec = (uint32_t)(o->after_ns % 1000000000ull);
  g.span_sec = span / 1000000000ull;
  g.span_nsec = (uint32_t)(span % 1000000000ull);
  g.bits_out = gbits;
  const size_t nb = (size_t)((n + klf::kArBlock - 1) / klf::kArBlock);
  if (int rc = sc.alloc(g.bsum, (nb + 1) * 8, "head sums")) return rc;
  HIPCHK(e, klf::launch_ar_heads(g, st), "launch k_ar_heads");
  HIPCHK(e, hipMemcpyAsync(&k, g.bsum + nb, 8, hipMemcpyDeviceToHost, st), "D2H interval count");
  HIPCHK(e, hipStreamSynchronize(st), "sync interval count");
  if (!k || k > n) return set_err(e, KLF_EHIP, "klf_around: interval count out of range");  // (never: anchor 0 opens one)
  g.k = k;
  if (int rc = sc.alloc(g.iv, (size_t)k * sizeof(klf::ArIval), "intervals")) return rc;
  HIPCHK(e, klf::launch_ar_build(g, st, e->num_cus), "launch k_ar_build");
  return sc.finish(ms);
}

// klf_records' options (SPEC.md S4h): null when klf_records takes them, else what is wrong.
static_assert(sizeof(klf_records_opts) == 56, "klf_records_opts layout");
static_assert(KLF_RECORDS_INDENT == klf::kRecordsIndent && KLF_RECORDS_BLANK == klf::kRecordsBlank &&
                  KLF_RECORDS_PREFIX_HEAD == klf::kRecordsPrefixHead && KLF_RECORDS_INVERT == klf::kRecordsInvert &&
                  KLF_RECORDS_MAX_PREFIXES == klf::kRecordsMaxPrefixes && KLF_RECORDS_MAX_PREFIX == klf::kRecordsMaxPrefix,
              "one set of values for the host helper and the kernels");
const char* klf_impl::records_opts_error(const klf_records_opts* o) {
  if (o->flags & ~(KLF_RECORDS_INDENT | KLF_RECORDS_BLANK | KLF_RECORDS_PREFIX_HEAD | KLF_RECORDS_INVERT))
    return "unknown flag bits";
  if ((o->flags & KLF_RECORDS_PREFIX_HEAD) && (o->flags & (KLF_RECORDS_INDENT | KLF_RECORDS_BLANK)))
    return "KLF_RECORDS_INDENT / KLF_RECORDS_BLANK together with KLF_RECORDS_PREFIX_HEAD";
  if (o->from._reserved || o->until._reserved) return "a non-zero _reserved";
  if (o->from.nsec < 0 || o->from.nsec >= 1000000000 || o->until.nsec < 0 || o->until.nsec >= 1000000000)
    return "nsec outside [0, 1e9)";
  if (o->n_prefixes > KLF_RECORDS_MAX_PREFIXES) return "more than KLF_RECORDS_MAX_PREFIXES prefixes";
  if (o->n_prefixes && (!o->prefixes || !o->prefix_off)) return "prefixes without their bytes or offsets";
  for (uint32_t k = 0; k < o->n_prefixes; ++k) {
    if (o->prefix_off[k + 1] < o->prefix_off[k]) return "prefix_off must ascend";
    const uint32_t len = o->prefix_off[k + 1] - o->prefix_off[k];
    if (len == 0 || len > KLF_RECORDS_MAX_PREFIX) return "a prefix must have 1 .. KLF_RECORDS_MAX_PREFIX bytes";
  }
  return nullptr;
}

// The prefixes of checked options, packed for the classifier.
static klf::RecordPrefixes record_prefixes(const klf_records_opts* o) {
  klf::RecordPrefixes p{};
  for (uint32_t k = 0; k < o->n_prefixes; ++k)
    klf::record_prefix_add(p, o->prefixes + o->prefix_off[k], o->prefix_off[k + 1] - o->prefix_off[k]);
  return p;
}

// klf_records' selection bitmap (SPEC.md S4h; the kernels: klf_analysis.hpp, RecordArgs).  Four
// kernels back to back; the host waits once, for the two counts.
int klf_impl::records_build(klf_engine* e, const klf_result* prev, const klf_records_opts* o, double& ms,
                            uint64_t& heads, uint64_t& conts) {
  hipStream_t st = e->stream;
  CallScratch sc(e, "klf_records", "records");
  klf::RecordArgs g{};
  g.v = sel_view(prev);
  g.v.bits_in = e->d_bits.as<uint32_t>();  // M, whatever prev was selected from
  g.pre = record_prefixes(o);
  g.flags = o->flags;
  g.bits_out = e->d_gbits.as<uint32_t>();
  if (int rc = sc.alloc(g.start, (size_t)(g.v.cap_lines / 32 + 1) * 4, "start bitmap")) return rc;
  if (int rc = sc.alloc(g.csum, (size_t)(g.v.nchunks + 1) * 8 * 8, "chunk sums")) return rc;
  if (int rc = sc.alloc(g.counts, 16, "class counts")) return rc;
  if (int rc = sc.start()) return rc;
  HIPCHK(e, klf::launch_records(g, st, e->num_cus), "launch k_rc_heads .. k_rc_build");
  if (int rc = sc.stop()) return rc;
  uint64_t cnt[2] = {0, 0};
  HIPCHK(e, hipMemcpyAsync(cnt, g.counts, 16, hipMemcpyDeviceToHost, st), "D2H class counts");
  HIPCHK(e, hipStreamSynchronize(st), "sync records");
  heads = cnt[0];
  conts = cnt[1];
  return sc.elapsed(ms);
}

extern "C" int klf_record_class(const uint8_t* content, size_t len, const klf_records_opts* o) {
  if ((!content && len) || !o || klf_impl::records_opts_error(o)) return KLF_EINVAL;
  const klf::RecordPrefixes p = record_prefixes(o);
  return klf::record_class(klf::RecordHostLoad{}, content, (uint64_t)len, o->flags, p);
}

// Segment -> stream id.
static std::vector<uint32_t> seg_streams(const klf_result* r) {
  std::vector<uint32_t> v(r->so.size(), 0u);
  for (uint32_t id = 0; id < r->n_streams; ++id)
    if (r->seg_of[id] >= 0) v[(size_t)r->seg_of[id]] = id;
  return v;
}

// The host copy of the n elements at d that a view of a returned object hands out: made by the
// first call that asks, kept until the object is freed.
template <class T>
static int host_view(klf_engine* e, std::vector<T>& v, bool& have, const DevBuf& d, uint64_t n, const char* what) {
  if (!have && n) {
    try { v.resize((size_t)n); } catch (const std::bad_alloc&) { return KLF_ENOMEM; }
    HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
    HIPCHK(e, hipMemcpy(v.data(), d.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost), what);
  }
  have = true;
  return KLF_OK;
}

extern "C" int klf_result_histogram(klf_result* r, const klf_hist_opts* o, uint64_t* counts, uint64_t* outside,
                                    double* ms) {
  if (!r || !o || !counts) return KLF_EINVAL;
  klf_engine* e = r->e;
  if (o->width_ns == 0 || o->n_buckets == 0 || o->n_buckets > KLF_HIST_MAX_BUCKETS)
    return set_err(e, KLF_EINVAL, "klf_result_histogram: width_ns and n_buckets must be at least 1, n_buckets at most 65536");
  if (o->width_ns > (uint64_t)INT64_MAX / o->n_buckets)
    return set_err(e, KLF_EINVAL, "klf_result_histogram: n_buckets * width_ns must stay below 2^63");
  if (o->origin.nsec < 0 || o->origin.nsec >= 1000000000)
    return set_err(e, KLF_EINVAL, "klf_result_histogram: nsec outside [0, 1e9)");
  if (o->flags || o->origin._reserved)
    return set_err(e, KLF_EINVAL, "klf_result_histogram: unknown flag bits or a non-zero _reserved");
  if (int rc = check_latest(e, r, "klf_result_histogram")) return rc;
  const uint32_t nsegs = (uint32_t)r->so.size(), nb = o->n_buckets;
  const uint64_t row = (uint64_t)nb + 2;
  if ((uint64_t)nsegs * row > (1ull << 24))
    return set_err(e, KLF_ETOOBIG, "klf_result_histogram: non-empty streams * (n_buckets + 2) exceeds 2^24");
  if (ms) *ms = 0.0;
  memset(counts, 0, (size_t)r->n_streams * nb * 8);
  if (outside) memset(outside, 0, (size_t)r->n_streams * 2 * 8);
  if (!nsegs) return KLF_OK;
  if (int rc = ensure_index(e)) return rc;
  HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
  const uint64_t span = o->width_ns * nb;  // ns, < 2^63
  klf::HistArgs g{};
  g.v = sel_view(r);
  g.n_buckets = nb;
  g.org_sec = o->origin.sec;
  g.org_nsec = o->origin.nsec;
  int64_t end_nsec = o->origin.nsec + (int64_t)(span % 1000000000ull), carry = 0;
  if (end_nsec >= 1000000000) { end_nsec -= 1000000000; carry = 1; }
  g.end_nsec = (int32_t)end_nsec;
  g.end_open = __builtin_add_overflow(o->origin.sec, (int64_t)(span / 1000000000ull) + carry, &g.end_sec) ? 1u : 0u;
  g.width_ns = o->width_ns;
  g.width_s = o->width_ns % 1000000000ull == 0 && span / 1000000000ull < (1ull << 32)
                  ? (uint32_t)(o->width_ns / 1000000000ull) : 0u;
  const size_t tbytes = (size_t)nsegs * row * 8;
  HIPCHK(e, e->d_thist.ensure(tbytes), "alloc histogram table");
  HIPCHK(e, e->h_thist.ensure(tbytes), "alloc histogram readback");
  g.table = e->d_thist.as<uint64_t>();
  CallScratch sc(e, "klf_result_histogram", "histogram");  // (its events alone: the table is the engine's)
  if (int rc = sc.start()) return rc;
  HIPCHK(e, klf::launch_hist(g, e->stream, e->num_cus), "launch k_hist");
  if (int rc = sc.stop()) return rc;
  HIPCHK(e, hipMemcpyAsync(e->h_thist.p, e->d_thist.p, tbytes, hipMemcpyDeviceToHost, e->stream), "D2H histogram");
  HIPCHK(e, hipStreamSynchronize(e->stream), "sync histogram");
  if (ms)
    if (int rc = sc.elapsed(*ms)) return rc;
  const uint64_t* tab = e->h_thist.as<uint64_t>();
  for (uint32_t id = 0; id < r->n_streams; ++id) {
    const int64_t s = r->seg_of[id];
    if (s < 0) continue;
    memcpy(counts + (size_t)id * nb, tab + (size_t)s * row, (size_t)nb * 8);
    if (outside) memcpy(outside + (size_t)id * 2, tab + (size_t)s * row + nb, 16);
  }
  return KLF_OK;
}

// ------------------------------------------------------------- merged timeline ---

// A timeline owns what it returns: the entry records and the merged bytes on the device, and
// their host copies once a view asked for them.  Nothing of the engine's workspace is kept.
struct klf_timeline {
  klf_engine* e = nullptr;
  uint64_t n = 0, len = 0;
  double ms = 0.0;
  DevBuf d_entries, d_bytes;
  bool have_entries = false, have_bytes = false;
  std::vector<klf_timeline_entry> entries;
  std::vector<uint8_t> bytes;
  ~klf_timeline() {
    d_entries.release();
    d_bytes.release();
  }
};
static_assert(sizeof(klf_timeline_entry) == sizeof(klf::TlEntry) && sizeof(klf_timeline_entry) == 32,
              "klf_timeline_entry is the kernels' TlEntry");

extern "C" int klf_result_timeline(klf_result* r, const klf_timeline_opts* o, klf_timeline** out) {
  if (!r || !o || !out) return KLF_EINVAL;
  klf_engine* e = r->e;
  if ((o->flags & ~KLF_TIMELINE_TIMESTAMPS) || o->_reserved)
    return set_err(e, KLF_EINVAL, "klf_result_timeline: unknown flag bits or a non-zero _reserved");
  if (o->tags && !o->tag_off) return set_err(e, KLF_EINVAL, "klf_result_timeline: tags without tag_off");
  if (o->tags)
    for (uint32_t i = 0; i < r->n_streams; ++i) {
      if (o->tag_off[i + 1] < o->tag_off[i]) return set_err(e, KLF_EINVAL, "klf_result_timeline: tag_off must ascend");
      if (o->tag_off[i + 1] - o->tag_off[i] > KLF_TIMELINE_MAX_TAG)
        return set_err(e, KLF_EINVAL, "klf_result_timeline: a tag is longer than KLF_TIMELINE_MAX_TAG");
    }
  if (int rc = check_latest(e, r, "klf_result_timeline")) return rc;
  std::unique_ptr<klf_timeline> t(new (std::nothrow) klf_timeline());
  if (!t) return KLF_ENOMEM;
  t->e = e;
  const uint32_t nsegs = (uint32_t)r->so.size();
  if (!nsegs) {  // no stream has bytes
    *out = t.release();
    return KLF_OK;
  }
  if (int rc = ensure_index(e)) return rc;
  HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
  hipStream_t st = e->stream;
  CallScratch sc(e, "klf_result_timeline", "timeline");
  klf::TlArgs g{};
  g.v = sel_view(r);
  g.timestamps = (o->flags & KLF_TIMELINE_TIMESTAMPS) ? 1u : 0u;
  // per segment: its stream id and its tag
  const std::vector<uint32_t> streams = seg_streams(r);
  std::vector<uint32_t> segtab((size_t)nsegs * 3, 0u);
  for (uint32_t s = 0; s < nsegs; ++s) {
    const uint32_t id = segtab[3 * (size_t)s] = streams[s];
    if (o->tags) {
      segtab[3 * (size_t)s + 1] = o->tag_off[id];
      segtab[3 * (size_t)s + 2] = o->tag_off[id + 1] - o->tag_off[id];
    }
  }
  const uint32_t tag_bytes = o->tags ? o->tag_off[r->n_streams] : 0u;
  uint32_t* d_segtab = nullptr;
  if (int rc = sc.alloc(d_segtab, segtab.size() * 4, "segment table")) return rc;
  HIPCHK(e, hipMemcpyAsync(d_segtab, segtab.data(), segtab.size() * 4, hipMemcpyHostToDevice, st), "H2D segment table");
  g.segtab = d_segtab;
  if (tag_bytes) {
    uint8_t* d_tags = nullptr;
    if (int rc = sc.alloc(d_tags, tag_bytes, "tags")) return rc;
    HIPCHK(e, hipMemcpyAsync(d_tags, o->tags, tag_bytes, hipMemcpyHostToDevice, st), "H2D tags");
    g.tags = d_tags;
  }
  if (int rc = sc.alloc(g.cbase, (g.v.nchunks + 1) * 8, "chunk bases")) return rc;
  if (int rc = sc.start()) return rc;
  // 1. E lines per chunk -> n
  HIPCHK(e, klf::launch_tl_count(g.v, g.cbase, true, st, e->num_cus), "launch k_tl_count");
  uint64_t n = 0;
  HIPCHK(e, hipMemcpyAsync(&n, g.cbase + g.v.nchunks, 8, hipMemcpyDeviceToHost, st), "D2H timeline size");
  HIPCHK(e, hipStreamSynchronize(st), "sync timeline size");
  if (n > 0xFFFFFFFFull) return set_err(e, KLF_ETOOBIG, "klf_result_timeline: more than 2^32 - 1 entries");
  if (!n) {
    if (int rc = sc.finish(t->ms)) return rc;
    *out = t.release();
    return KLF_OK;
  }
  g.n = n;
  // 2. keys, 3. the sort
  DeviceSort sort(sc);
  if (int rc = sort.prepare(n)) return rc;
  for (int k = 0; k < 2; ++k) g.items[k] = sort.s.items[k];
  if (int rc = sc.alloc(g.side, n * sizeof(klf::TlSide), "side records")) return rc;
  HIPCHK(e, klf::launch_tl_keys(g, true, st, e->num_cus), "launch k_tl_keys");
  if (int rc = sort.digits()) return rc;
  if (int rc = sort.passes(0, klf::kTlDigits)) return rc;
  // 4. rendered lengths -> offsets, entries, bytes
  const size_t pblocks = (size_t)((n + klf::kTlPlanBlock - 1) / klf::kTlPlanBlock);
  if (int rc = sc.alloc(g.psum, (pblocks + 1) * 8, "block sums")) return rc;
  HIPCHK(e, klf::launch_tl_plan(g, sort.cur, st), "launch k_tl_plan");
  uint64_t total = 0;
  HIPCHK(e, hipMemcpyAsync(&total, g.psum + pblocks, 8, hipMemcpyDeviceToHost, st), "D2H merged length");
  HIPCHK(e, hipStreamSynchronize(st), "sync merged length");
  if (int rc = sc.alloc(t->d_entries, n * sizeof(klf::TlEntry), "entries")) return rc;
  if (int rc = sc.alloc(t->d_bytes, total + 16, "merged bytes")) return rc;
  g.entries = t->d_entries.as<klf::TlEntry>();
  g.out = t->d_bytes.as<uint8_t>();
  HIPCHK(e, klf::launch_tl_copy(g, sort.cur, st), "launch k_tl_copy");
  if (int rc = sc.finish(t->ms)) return rc;
  t->n = n;
  t->len = total;
  *out = t.release();
  return KLF_OK;
}

extern "C" int klf_timeline_entries(klf_timeline* t, const klf_timeline_entry** ent, uint64_t* n) {
  if (!t || !ent || !n) return KLF_EINVAL;
  if (int rc = host_view(t->e, t->entries, t->have_entries, t->d_entries, t->n, "D2H timeline entries")) return rc;
  *ent = t->entries.data();
  *n = t->n;
  return KLF_OK;
}

extern "C" int klf_timeline_bytes(klf_timeline* t, const uint8_t** bytes, uint64_t* len) {
  if (!t || !len) return KLF_EINVAL;
  *len = t->len;
  if (!bytes) return KLF_OK;
  if (int rc = host_view(t->e, t->bytes, t->have_bytes, t->d_bytes, t->len, "D2H merged bytes")) return rc;
  *bytes = t->bytes.data();
  return KLF_OK;
}

// klf_result_write's path for one descriptor: a pinned chunk from the staging pool, D2H in two
// halves of it with the next half in flight while the current one is written.
extern "C" int klf_timeline_write(klf_timeline* t, int fd, uint64_t* written) {
  if (written) *written = 0;
  if (!t || fd < 0) return KLF_EINVAL;
  klf_engine* e = t->e;
  if (!t->len) return KLF_OK;
  if (t->have_bytes) {  // already on the host
    if (!write_all(fd, t->bytes.data(), t->len))
      return set_err(e, KLF_EIO, std::string("write merged timeline: ") + strerror(errno));
    if (written) *written = t->len;
    return KLF_OK;
  }
  HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
  klf_engine::StageChunk c;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  const bool ok = take_chunk(e, &c) && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
                  hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess;
  WErr werr;
  uint64_t total = 0;
  const WPiece q{0, t->len, fd, 0, {}};
  if (ok) (void)copy_part(e, t->d_bytes.as<uint8_t>(), q, 0, t->len, c.p, kStageChunk / 2, st, ev, werr, total);
  if (st) (void)hipStreamSynchronize(st);  // no DMA into a chunk handed back below
  for (auto& x : ev)
    if (x) (void)hipEventDestroy(x);
  if (st) (void)hipStreamDestroy(st);
  if (c.p) {
    std::lock_guard<std::mutex> lk(e->mu);
    c.used = 0;
    e->chunk_pool.push_back(c);
  }
  if (written) *written = total;
  if (!ok) return set_err(e, KLF_ENOMEM, "klf_timeline_write: setup (pinned chunk / HIP stream)");
  if (werr.id.load() >= 0)
    return set_err(e, KLF_EIO, "write merged timeline: " + werr.what + (werr.err ? std::string(": ") + strerror(werr.err) : std::string()));
  return KLF_OK;
}

extern "C" int klf_timeline_ms(const klf_timeline* t, double* ms) {
  if (!t || !ms) return KLF_EINVAL;
  *ms = t->ms;
  return KLF_OK;
}

extern "C" void klf_timeline_free(klf_timeline* t) { delete t; }

// -------------------------------------------------------------- grouped counts ---

// A groups object owns what it returns, like a timeline: the entry records and the key bytes
// on the device, and their host copies once a view asked for them.
struct klf_groups {
  klf_engine* e = nullptr;
  uint64_t n = 0, key_bytes = 0, n_groups = 0, n_lines = 0;
  double ms = 0.0;
  DevBuf d_entries, d_keys;
  bool have_entries = false, have_keys = false;
  std::vector<klf_group_entry> entries;
  std::vector<uint8_t> keys;
  ~klf_groups() {
    d_entries.release();
    d_keys.release();
  }
};
static_assert(sizeof(klf_group_entry) == sizeof(klf::GrEntry) && sizeof(klf_group_entry) == 48 &&
                  sizeof(klf_groups_opts) == 16,
              "klf_group_entry is the kernels' GrEntry");
static_assert(KLF_GROUPS_MASK_DIGITS == klf::kGroupsMaskDigits, "one flag value for the host helper and the kernels");

// KLF_GROUPS_HASH_BITS (1..64, a test hook: DESIGN.md): the low bits of the hash that are used.
static uint32_t groups_hash_bits() {
  const char* s = getenv("KLF_GROUPS_HASH_BITS");
  if (!s || !*s) return 64;
  char* end = nullptr;
  const long v = strtol(s, &end, 10);
  return (*end || v < 1 || v > 64) ? 64u : (uint32_t)v;
}

extern "C" int klf_result_groups(klf_result* r, const klf_groups_opts* o, klf_groups** out) {
  if (!r || !o || !out) return KLF_EINVAL;
  klf_engine* e = r->e;
  if (o->top == 0 || o->top > KLF_GROUPS_MAX_TOP)
    return set_err(e, KLF_EINVAL, "klf_result_groups: top must be 1 .. 65536");
  if (o->max_groups > KLF_GROUPS_MAX_GROUPS)
    return set_err(e, KLF_EINVAL, "klf_result_groups: max_groups above 2^26");
  if (o->flags & ~KLF_GROUPS_MASK_DIGITS) return set_err(e, KLF_EINVAL, "klf_result_groups: unknown flag bits");
  if (int rc = check_latest(e, r, "klf_result_groups")) return rc;
  std::unique_ptr<klf_groups> t(new (std::nothrow) klf_groups());
  if (!t) return KLF_ENOMEM;
  t->e = e;
  const uint32_t nsegs = (uint32_t)r->so.size();
  if (!nsegs) {  // no stream has bytes
    *out = t.release();
    return KLF_OK;
  }
  if (r->total_lines >> klf::kGrLineBits)
    return set_err(e, KLF_ETOOBIG, "klf_result_groups: 2^40 or more lines in the run");
  if (int rc = ensure_index(e)) return rc;
  HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
  hipStream_t st = e->stream;
  CallScratch sc(e, "klf_result_groups", "groups");
  klf::GroupArgs g{};
  g.v = sel_view(r);
  g.max_key = o->max_key;
  g.flags = o->flags;
  g.hash_bits = groups_hash_bits();
  // P = pow2 >= 2 * the keys the table must hold: max_groups, or the run's lines when fewer
  const uint64_t max_groups = o->max_groups ? o->max_groups : (1ull << 20);
  const uint64_t hold = std::min<uint64_t>(max_groups, r->total_lines);
  g.table_log2 = 6;
  while ((1ull << g.table_log2) < 2 * hold) ++g.table_log2;  // (<= 27)
  const uint64_t P = 1ull << g.table_log2;
  const size_t cblocks = (size_t)((P + klf::kGrCountBlock - 1) / klf::kGrCountBlock);
  if (int rc = sc.alloc(g.table, (size_t)(4 * P + 2) * 8, "hash table")) return rc;
  if (int rc = sc.alloc(g.bsum, (cblocks + 1) * 8, "slot sums")) return rc;
  if (int rc = sc.start()) return rc;
  // 1. every line of H into the table; the occupied slots -> n_groups
  HIPCHK(e, klf::launch_gr_insert(g, st, e->num_cus), "launch k_gr_insert");
  HIPCHK(e, klf::launch_gr_count(g, st), "launch k_gr_count");
  uint64_t stats[2] = {0, 0}, n_groups = 0;
  HIPCHK(e, hipMemcpyAsync(stats, g.table + 4 * P, 16, hipMemcpyDeviceToHost, st), "D2H groups totals");
  HIPCHK(e, hipMemcpyAsync(&n_groups, g.bsum + cblocks, 8, hipMemcpyDeviceToHost, st), "D2H groups count");
  HIPCHK(e, hipStreamSynchronize(st), "sync groups count");
  if (stats[1] || n_groups > max_groups)  // (a full table holds P > max_groups keys: the same answer)
    return set_err(e, KLF_ETOOBIG, "klf_result_groups: more than max_groups = " + std::to_string(max_groups) +
                                       " distinct keys; mask digits (KLF_GROUPS_MASK_DIGITS), cut the key (max_key) or "
                                       "raise max_groups");
  t->n_lines = stats[0];
  t->n_groups = n_groups;
  if (!n_groups) {
    if (int rc = sc.finish(t->ms)) return rc;
    *out = t.release();
    return KLF_OK;
  }
  // 2. one item per group, sorted by (count desc, first asc)
  g.n_groups = n_groups;
  DeviceSort sort(sc);
  if (int rc = sort.prepare(n_groups)) return rc;
  g.items = sort.s.items[0];
  if (int rc = sc.alloc(g.gslot, n_groups * 4, "item slots")) return rc;
  HIPCHK(e, klf::launch_gr_fill(g, st), "launch k_gr_fill");
  if (int rc = sort.digits()) return rc;
  if (int rc = sort.passes(0, klf::kTlDigits)) return rc;
  // 3. the first `top` groups: key lengths -> offsets, then the records and the key bytes
  g.top = (uint32_t)std::min<uint64_t>(o->top, n_groups);
  const std::vector<uint32_t> segstream = seg_streams(r);
  uint32_t* d_segstream = nullptr;
  if (int rc = sc.alloc(d_segstream, (size_t)nsegs * 4, "segment table")) return rc;
  HIPCHK(e, hipMemcpyAsync(d_segstream, segstream.data(), (size_t)nsegs * 4, hipMemcpyHostToDevice, st), "H2D segment table");
  g.segstream = d_segstream;
  if (int rc = sc.alloc(g.klen, ((size_t)g.top + 1) * 8, "key lengths")) return rc;
  HIPCHK(e, klf::launch_gr_plan(g, sort.sorted(), st), "launch k_gr_plan");
  uint64_t total = 0;
  HIPCHK(e, hipMemcpyAsync(&total, g.klen + g.top, 8, hipMemcpyDeviceToHost, st), "D2H key bytes");
  HIPCHK(e, hipStreamSynchronize(st), "sync key bytes");
  if (int rc = sc.alloc(t->d_entries, (size_t)g.top * sizeof(klf::GrEntry), "entries")) return rc;
  if (int rc = sc.alloc(t->d_keys, total + 16, "key bytes")) return rc;
  g.entries = t->d_entries.as<klf::GrEntry>();
  g.keys = t->d_keys.as<uint8_t>();
  HIPCHK(e, klf::launch_gr_render(g, sort.sorted(), st), "launch k_gr_render");
  if (int rc = sc.finish(t->ms)) return rc;
  t->n = g.top;
  t->key_bytes = total;
  *out = t.release();
  return KLF_OK;
}

extern "C" int klf_groups_entries(klf_groups* t, const klf_group_entry** ent, uint64_t* n) {
  if (!t || !ent || !n) return KLF_EINVAL;
  if (int rc = host_view(t->e, t->entries, t->have_entries, t->d_entries, t->n, "D2H group entries")) return rc;
  *ent = t->entries.data();
  *n = t->n;
  return KLF_OK;
}

extern "C" int klf_groups_keys(klf_groups* t, const uint8_t** bytes, uint64_t* len) {
  if (!t || !bytes || !len) return KLF_EINVAL;
  if (int rc = host_view(t->e, t->keys, t->have_keys, t->d_keys, t->key_bytes, "D2H group keys")) return rc;
  *bytes = t->keys.data();
  *len = t->key_bytes;
  return KLF_OK;
}

extern "C" int klf_groups_totals(const klf_groups* t, uint64_t* n_groups, uint64_t* n_lines) {
  if (!t) return KLF_EINVAL;
  if (n_groups) *n_groups = t->n_groups;
  if (n_lines) *n_lines = t->n_lines;
  return KLF_OK;
}

extern "C" int klf_groups_ms(const klf_groups* t, double* ms) {
  if (!t || !ms) return KLF_EINVAL;
  *ms = t->ms;
  return KLF_OK;
}

extern "C" void klf_groups_free(klf_groups* t) { delete t; }

extern "C" int klf_group_key(const uint8_t* content, size_t len, uint32_t max_key, uint32_t flags, uint8_t* out,
                             size_t cap, size_t* n) {
  if (n) *n = 0;
  if ((!content && len) || (!out && cap) || (flags & ~KLF_GROUPS_MASK_DIGITS)) return KLF_EINVAL;
  const size_t span = (size_t)klf::group_key_span(len, max_key);
  size_t need = 0;
  {
    klf::GroupKeyNorm nm(flags);
    uint8_t c;
    for (size_t i = 0; i < span; ++i) need += nm.step(content[i], c) ? 1 : 0;
  }
  if (n) *n = need;
  if (need > cap) return KLF_EINVAL;
  klf::GroupKeyNorm nm(flags);
  size_t k = 0;
  for (size_t i = 0; i < span; ++i) {
    uint8_t c;
    if (nm.step(content[i], c)) out[k++] = c;
  }
  return KLF_OK;
}

// ------------------------------------------------------- numeric field statistics ---

static_assert(sizeof(klf_field_opts) == 32 && sizeof(klf_field_row) == 80, "klf_field_opts / klf_field_row layout");
static_assert(KLF_FIELD_DURATION == klf::kFieldDuration && KLF_FIELD_MAX_KEY == klf::kFieldMaxKey &&
                  KLF_FIELD_MAX_KEY == klf::kFsMaxKey && KLF_FIELD_MAX_QUANTILES == klf::kFsMaxQuantiles &&
                  KLF_FIELD_HIT == klf::kFieldHit && KLF_FIELD_MISS == klf::kFieldMiss && KLF_FIELD_BAD == klf::kFieldBad,
              "one set of values for the host helper and the kernels");

static bool field_opts_ok(const uint8_t* key, uint32_t key_len, uint32_t decimals, uint32_t flags) {
  return key && key_len >= 1 && key_len <= KLF_FIELD_MAX_KEY && !(flags & ~KLF_FIELD_DURATION) && decimals <= 9 &&
         !((flags & KLF_FIELD_DURATION) && decimals);
}

extern "C" int klf_result_field_stats(klf_result* r, const klf_field_opts* o, klf_field_row* rows, int64_t* qvals,
                                      double* ms) {
  if (!r || !o || !rows) return KLF_EINVAL;
  klf_engine* e = r->e;
  if (!field_opts_ok(o->key, o->key_len, o->decimals, o->flags))
    return set_err(e, KLF_EINVAL, "klf_result_field_stats: key of 1 .. 64 bytes, decimals 0 .. 9 (0 with "
                                  "KLF_FIELD_DURATION), no unknown flag bits");
  if (o->n_quantiles > KLF_FIELD_MAX_QUANTILES || (o->n_quantiles && (!o->quantiles || !qvals)))
    return set_err(e, KLF_EINVAL, "klf_result_field_stats: at most 16 quantiles, with their arrays");
  for (uint32_t k = 0; k < o->n_quantiles; ++k)
    if (o->quantiles[k] > 10000) return set_err(e, KLF_EINVAL, "klf_result_field_stats: a quantile above 10000");
  if (int rc = check_latest(e, r, "klf_result_field_stats")) return rc;
  const uint32_t nsegs = (uint32_t)r->so.size(), nq = o->n_quantiles, nrows = r->n_streams + 1;
  if (ms) *ms = 0.0;
  for (uint32_t i = 0; i < nrows; ++i) {
    rows[i] = klf_field_row{};
    rows[i].min_line = rows[i].max_line = UINT64_MAX;
    rows[i].min_stream = rows[i].max_stream = UINT32_MAX;
  }
  if (nq) memset(qvals, 0, (size_t)nrows * nq * 8);
  if (!nsegs) return KLF_OK;  // no stream has bytes
  if (nsegs >> 30) return set_err(e, KLF_ETOOBIG, "klf_result_field_stats: 2^30 or more streams with bytes");
  if (int rc = ensure_index(e)) return rc;
  HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
  hipStream_t st = e->stream;
  CallScratch sc(e, "klf_result_field_stats", "field statistics");
  klf::FieldArgs g{};
  g.v = sel_view(r);
  memcpy(g.key, o->key, o->key_len);
  g.key_len = o->key_len;
  g.decimals = o->decimals;
  g.flags = o->flags;
  g.n_q = nq;
  for (uint32_t k = 0; k < nq; ++k) g.q[k] = o->quantiles[k];
  if (int rc = sc.alloc(g.cbase, (g.v.nchunks + 1) * 8, "chunk bases")) return rc;
  if (int rc = sc.alloc(g.hbase, (g.v.nchunks + 1) * 8, "chunk hit bases")) return rc;
  // the result block: the table, the segments' hit prefix, the rows, the quantile values
  const size_t tab_w = (size_t)klf::kFsTabRows * nsegs, hpre_w = (size_t)nsegs + 1,
               rows_w = ((size_t)nsegs + 1) * (sizeof(klf::FsRow) / 8), qv_w = ((size_t)nsegs + 1) * nq;
  const size_t res_w = tab_w + hpre_w + rows_w + qv_w;
  if (int rc = sc.alloc(g.tab, res_w * 8, "result block")) return rc;
  g.hpre = g.tab + tab_w;
  g.rows = reinterpret_cast<klf::FsRow*>(g.hpre + hpre_w);
  g.qv = reinterpret_cast<int64_t*>(g.hpre + hpre_w + rows_w);
  if (int rc = sc.start()) return rc;
  // 1. H lines per chunk -> n
  HIPCHK(e, klf::launch_tl_count(g.v, g.cbase, false, st, e->num_cus), "launch k_tl_count");
  uint64_t n = 0;
  HIPCHK(e, hipMemcpyAsync(&n, g.cbase + g.v.nchunks, 8, hipMemcpyDeviceToHost, st), "D2H field statistics size");
  HIPCHK(e, hipStreamSynchronize(st), "sync field statistics size");
  if (n > 0xFFFFFFFFull) return set_err(e, KLF_ETOOBIG, "klf_result_field_stats: 2^32 or more lines in the selection");
  g.n = n;
  // 2. every line's class and value; per segment the counts and the sum; the hits per chunk -> n_hits
  if (int rc = sc.alloc(g.val, (size_t)n * 8, "values")) return rc;
  if (int rc = sc.alloc(g.cs, (size_t)n * 4, "classes")) return rc;
  HIPCHK(e, klf::launch_fs_extract(g, st, e->num_cus), "launch k_fs_extract");
  uint64_t n_hits = 0;
  HIPCHK(e, hipMemcpyAsync(&n_hits, g.hbase + g.v.nchunks, 8, hipMemcpyDeviceToHost, st), "D2H field statistics hits");
  HIPCHK(e, hipStreamSynchronize(st), "sync field statistics hits");
  g.n_hits = n_hits;
  // 3. the hits as sort items; value order -> the all-streams row; (segment, value) order -> the rest
  DeviceSort sort(sc);
  if (int rc = sort.prepare(n_hits)) return rc;
  g.items = sort.s.items[0];
  HIPCHK(e, klf::launch_fs_compact(g, st, e->num_cus), "launch k_fs_compact");  // (nothing with n_hits = 0)
  if (int rc = sort.digits()) return rc;
  if (int rc = sort.passes(0, 8)) return rc;
  HIPCHK(e, klf::launch_fs_rows(g, sort.sorted(), 1u, st), "launch k_fs_rows");
  if (int rc = sort.passes(8, klf::kTlDigits)) return rc;
  HIPCHK(e, klf::launch_fs_rows(g, sort.sorted(), 0u, st), "launch k_fs_rows");
  // 4. one copy of the result block; segments -> stream ids; the all-streams counts and sum
  std::vector<uint64_t> res(res_w);
  if (int rc = sc.stop()) return rc;
  HIPCHK(e, hipMemcpyAsync(res.data(), g.tab, res_w * 8, hipMemcpyDeviceToHost, st), "D2H field statistics");
  HIPCHK(e, hipStreamSynchronize(st), "sync field statistics");
  if (ms)
    if (int rc = sc.elapsed(*ms)) return rc;
  const std::vector<uint32_t> segstream = seg_streams(r);
  const uint64_t* tab = res.data();
  const klf::FsRow* drows = reinterpret_cast<const klf::FsRow*>(res.data() + tab_w + hpre_w);
  const int64_t* dqv = reinterpret_cast<const int64_t*>(res.data() + tab_w + hpre_w + rows_w);
  auto place = [&](klf_field_row& out, const klf::FsRow& d, __int128 sum) {
    out.sum_lo = (uint64_t)(unsigned __int128)sum;
    out.sum_hi = (int64_t)(sum >> 64);
    if (!out.hits) return;
    out.min = d.min;
    out.max = d.max;
    out.min_line = d.min_line;
    out.max_line = d.max_line;
    out.min_stream = d.min_seg < nsegs ? segstream[d.min_seg] : UINT32_MAX;
    out.max_stream = d.max_seg < nsegs ? segstream[d.max_seg] : UINT32_MAX;
  };
  klf_field_row& all = rows[r->n_streams];
  __int128 all_sum = 0;
  for (uint32_t s = 0; s < nsegs; ++s) {
    klf_field_row& out = rows[segstream[s]];
    out.lines = tab[s];
    out.hits = tab[(size_t)nsegs + s];
    out.bad = tab[2 * (size_t)nsegs + s];
    // the sum of v = (v >> 32) * 2^32 + (v & 0xFFFFFFFF) over the hits, from its two halves
    const __int128 sum = (__int128)(int64_t)tab[3 * (size_t)nsegs + s] * ((__int128)1 << 32) + (__int128)tab[4 * (size_t)nsegs + s];
    place(out, drows[s], sum);
    if (nq) memcpy(qvals + (size_t)segstream[s] * nq, dqv + (size_t)s * nq, (size_t)nq * 8);
    all.lines += out.lines;
    all.hits += out.hits;
    all.bad += out.bad;
    all_sum += sum;
  }
  place(all, drows[nsegs], all_sum);
  if (nq) memcpy(qvals + (size_t)r->n_streams * nq, dqv + (size_t)nsegs * nq, (size_t)nq * 8);
  return KLF_OK;
}

extern "C" int klf_field_value(const uint8_t* content, size_t len, const uint8_t* key, uint32_t key_len,
                               uint32_t decimals, uint32_t flags, int64_t* value) {
  if ((!content && len) || !value || !field_opts_ok(key, key_len, decimals, flags)) return KLF_EINVAL;
  *value = 0;
  klf::FieldHostBytes src{content};
  int64_t v = 0;
  const int cls = klf::field_classify(src, (uint64_t)len, key, key_len, decimals, flags, &v);
  if (cls == klf::kFieldHit) *value = v;
  return cls;
}
