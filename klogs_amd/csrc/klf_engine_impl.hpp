// klf_engine_impl.hpp — internal: what the two host files of the engine share.  klf_engine.cpp
// (staging, the run, the result views, the calls that end in the run's tail stage) defines
// everything declared here; klf_analysis.cpp (the other calls on a finished run) uses it.
// Nothing here is part of the C ABI: the helpers live in klf_impl, whose symbols stay out of the
// library's dynamic table.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/klf.h"
#include "klf_analysis.hpp"
#include "klf_copypool.hpp"
#include "klf_kernels.hpp"
#include "klf_patterns.hpp"

using klf::SegDesc;
using klf::SegOut;

// On what the two files share: no entry of the library's dynamic symbol table, nor one for a
// template instantiated over it (std::vector<DevBuf>).  The structs that hold a DevBuf -- the
// handle types of the C ABI among them -- keep the default visibility they always had, which is
// all that GCC's -Wattributes has to say about them in these two files.
#define KLF_LOCAL __attribute__((visibility("hidden")))
#pragma GCC diagnostic ignored "-Wattributes"

namespace klf_impl KLF_LOCAL {

// time spent growing device buffers (KLF_DIAG: the first run's allocation share)
extern std::atomic<uint64_t> g_alloc_ns;  // (klf_engine.cpp)
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool borrowed = false;  // p lies in an engine's workspace block (not freed here)
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    const auto t0 = std::chrono::steady_clock::now();
    if (p && !borrowed) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    borrowed = false;
    size_t want = std::max<size_t>(bytes, 256);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    const uint64_t ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    g_alloc_ns += ns;
    static const bool diag = getenv("KLF_DIAG_ALLOC") != nullptr;
    if (diag) fprintf(stderr, "[klf] alloc %zu B: %.1f us\n", want, ns / 1e3);
    return e;
  }
  void release() {
    if (p && !borrowed) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    borrowed = false;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// Pinned host buffer (hipHostMalloc): per-run readbacks land here with one async DMA each
// and a single stream sync (a pageable destination costs a staged copy and a wait per call).
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    release();
    const size_t want = std::max<size_t>(bytes, 4096);
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

}  // namespace klf_impl
using klf_impl::DevBuf;
using klf_impl::HostBuf;

struct klf_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  int num_cus = 256;
  klf::CompiledSet cs;
  std::string err;
  uint64_t gen = 0;
  // Staging (host path).  Each stream fills a pinned host chunk
  // (hipHostMalloc, pooled across runs); a chunk that fills is DMA'd at once on the copy
  // stream into a pooled 64 MiB device chunk, so the H2D overlaps the rest of the capture.
  // klf_run DMAs the partly filled last chunk of every stream straight into the batch and
  // one kernel (k_assemble) moves the device chunks into their places in the batch.
  // Per-stream records are heap objects that never move (klf_stage on different ids runs
  // concurrently while the table grows).
  std::mutex mu;
  struct StageChunk {
    uint8_t* p = nullptr;
    size_t used = 0;
    bool pinned = false;
  };
  struct StagedStream {
    std::vector<uint8_t*> dchunks;  // full chunks already DMA'd (device, kStageChunk each)
    StageChunk cur;                 // pinned chunk being filled (p = null: none)
    uint64_t len = 0;
  };
  std::vector<std::unique_ptr<StagedStream>> staged;
  std::vector<StageChunk> chunk_pool;  // free pinned chunks (used = 0)
  std::vector<uint8_t*> dchunk_pool;   // free device chunks
  struct Inflight {
    StageChunk c;
    hipEvent_t ev;
  };
  std::deque<Inflight> inflight;       // pinned chunks whose H2D may still be running
  std::vector<hipEvent_t> ev_pool;
  hipStream_t copy_stream = nullptr;   // early H2D of full chunks
  hipEvent_t copy_done = nullptr;
  bool ran = false;                    // klf_run since the last klf_reset (stage -> ESTATE)
  std::unique_ptr<klf::CopyPool> copier;  // started by the first klf_stage (device-resident runs never stage)
  std::once_flag copier_once;
  std::once_flag copy_stream_once;     // the copy stream: created by the first klf_stage / klf_run
  hipError_t copy_stream_err = hipSuccess;
  DevBuf d_asm;                        // k_assemble piece table
  DevBuf d_scratch;                    // small query results (klf_result_last_unparsed)
  DevBuf d_ac_out, d_ac_dict, d_pcount, d_pairs;  // per-pattern counts
  uint32_t pairs_log2 = 20;            // (line, pattern) pair set: 2^20 entries, grows on overflow
  uint32_t n_user = 0;                 // patterns as given to klf_open
  // a set with an always-pattern beside others (CompiledSet::also_all_pending): the patterns,
  // compiled in full on the first run that asks for per-pattern counts
  std::vector<std::vector<uint8_t>> pend_pats;
  std::vector<uint32_t> pend_kinds;
  bool tune_later = true;
  int counts_code = KLF_OK;            // that compile failed: counts unavailable (the filter is kAll's)
  std::string counts_err;
  // device pattern tables
  DevBuf d_lit, d_ac_class, d_ac_next, d_ac_accept, d_rx_class, d_rx_b, d_rx_follow, d_rx_vec, d_rx_flags, d_rx_pre;
  DevBuf d_qf_bitmap, d_qf_head, d_qf_ent, d_qf_nbytes, d_cand, d_rx_vec4, d_qhits, d_hslots, d_hist, d_hflat, d_qf_anc;
  HostBuf h_hist;  // gram / byte statistics of the first batch (pinned readback)
  uint32_t cand_cap = 1u << 22;  // NFA candidate queue (32 MiB); overflow -> k_match
  uint64_t hits_cap_max = 1u << 26;  // prefilter hit list (512 MiB at most); overflow -> k_match
  klf::DevPatterns dpats;
  // workspace
  std::vector<SegDesc> last_segs;  // tile_seg cache key
  DevBuf d_tile_seg;
  DevBuf d_cmap, d_cseg;
  DevBuf d_block;  // the first run's workspace buffers (ensure_all), freed last
  std::vector<DevBuf*> block_users;  // the buffers still mapped into d_block
  DevBuf d_block2;  // the first run's line arrays, slot pool / records and output (sized after its sample)
  std::vector<DevBuf*> block2_users;
  DevBuf d_batch, d_segs, d_tstat, d_slots, d_pool, d_tile_base, d_bsum, d_cstatus, d_counters, d_line_off,
      d_meta, d_bits, d_wpre, d_out, d_mpart, d_trec, d_truns, d_kbase;
  // one-pass compaction (RunArgs::fuse): range table, extents, range states; d_out2 the
  // contiguous device copy klf_result_device_out makes of a fused result on demand
  DevBuf d_fext0, d_fext, d_frinfo, d_out2;
  uint32_t fuse_range = 0, fuse_nranges = 0, fuse_next = 0;  // the layout d_fext0 was made for
  std::vector<uint32_t> fuse_ext0;
  // the segment table the extent table was built for: its own cache key (last_segs follows
  // every run, fused or not, and a failed run may leave it behind d_fext0)
  std::vector<SegDesc> fuse_segs;
  uint64_t pool_cap = 1 << 20;
  // lines per input byte of the last run (0: no run yet): sizes the line arrays of the next
  // runs (the first run sizes them from its own tile index, between two launch phases)
  double line_density = 0.0;
  bool dense_tail_seen = false;  // a --tail run took the dense compaction (keep its run table)
  HostBuf h_rb;  // run readback: the counters (kCtrBytes), the SegOut table, a one-pass run's extents
  HostBuf h_stage;  // pinned staging of the prefilter tables (upload_prefilter)
  HostBuf h_acblk;  // the automaton thread's tables (pinned), uploaded on the launch stream at the join
  size_t ac_total = 0, ac_off[5] = {0, 0, 0, 0, 0}, ac_cap[5] = {0, 0, 0, 0, 0};
  // The literals' Aho-Corasick automaton (deferred lines, the fallback matcher): klf_open
  // starts a host thread that builds it and uploads it as one block (d_acblk, one
  // synchronous copy); ensure_ac joins it before the first launch that may read it, so the
  // build overlaps the first run's sampling and needle placement
  std::thread ac_thread;
  bool ac_pending = false;  // the automaton is built (or being built) but not yet uploaded
  std::vector<std::vector<uint8_t>> ac_lits;
  klf::AcTables ac_tabs;
  hipError_t ac_err = hipSuccess;
  DevBuf d_acblk;
  hipEvent_t stage_ev = nullptr;  // the staged copies have drained
  bool stage_ev_pending = false;
  // KLF_GRAPH=1: small batches replay their launch sequence as a HIP graph (round 6): ~12
  // launches cost ~35-45 us of host time.  Opt-in: measured on C1 (64 MiB) the run went
  // 104 -> ~95 us, the device being the bound, while the first capture costs 5-7 ms (most
  // of it creating cap_stream), which a short-lived engine pays in full.  A sequence is
  // captured (on cap_stream: the engine's own stream may be the null stream) the second
  // time the same arguments run; graph_off after a capture that failed.
  hipStream_t cap_stream = nullptr;
  hipGraphExec_t gexec = nullptr;
  std::vector<uint8_t> gkey, gprev;  // the captured arguments; the previous eager run's
  bool graph_off = false;
  hipEvent_t ev[11] = {};  // [7], [8]: k_scan's dispatch (hipExtLaunchKernel start / stop); [9], [10]: k_tcopy's; [6] unused
  klf::RunArgs last_args{};  // arguments of the latest completed run (klf_retail)
  // klf_regroup: the selection bitmap G' (the layout of d_bits) and the regroup kernels'
  // chunk summaries; allocated by the first regroup, so a plain run pays nothing for them
  DevBuf d_gbits, d_gsum;
  // klf_result_histogram: the per-segment table and its pinned readback, the engine's own (no
  // result's buffer is touched); allocated by the first histogram
  DevBuf d_thist;
  HostBuf h_thist;
  // the latest run's global line index is still to be built (lazy index, dense path): the
  // k_scatter launch that builds it
  std::vector<klf::RunArgs> index_pending;
  uint64_t last_gen = 0;     // gen of that run's result
};

struct klf_result {
  klf_engine* e = nullptr;
  uint64_t gen = 0;
  uint32_t n_streams = 0;
  std::vector<int64_t> seg_of;       // stream id -> segment (-1 = empty stream)
  std::vector<SegOut> so;            // per segment
  std::vector<uint64_t> seg_base;    // per segment (device byte offset)
  bool has_bits = false;
  bool grouped = false;              // selected over klf_regroup's bitmap (the engine's d_gbits)
  uint64_t total_lines = 0, total_out = 0;
  double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t ar_anchors = 0, ar_intervals = 0;  // a klf_around result: |A| and the merged intervals K,
  double ar_build_ms = 0.0;                   // and the device time of building G' (part of ms[4])
  uint64_t rc_heads = 0, rc_conts = 0;        // a klf_records result: the parsed lines by class,
  double rc_build_ms = 0.0;                   // and the device time of building G' (part of ms[4])
  uint32_t ev_mask = 0;              // the timing events the run recorded
  int index_mode = KLF_INDEX_FULL;   // how much of the line index the run itself wrote
  // lazily filled host copies
  bool have_out = false, have_lines = false;
  std::vector<uint8_t> out;
  std::vector<uint64_t> line_off;
  // [0] the match bitmap M, [1] a regrouped result's selection bitmap G'
  struct HostBits {
    bool have = false;
    std::vector<uint32_t> bits;
    std::vector<std::vector<uint8_t>> stream_bits;
    std::vector<uint8_t> have_stream_bits;
  } hbits[2];
  // per-pattern counts (KLF_FILTER_PATTERN_COUNTS): [segment][compiled id]
  bool counted = false, pcount_ok = false;
  std::vector<uint32_t> pcount;
  // a one-pass compaction run: each segment's output is the extents fx[2 k], fx[2 k + 1]
  // (d_out offset, length) for k in [fx_first[s], fx_first[s + 1]); so[s].out_lo / out_hi
  // are then the segment's place in the concatenated (host) output
  bool fused = false, have_dev = false;
  int compaction = KLF_COMPACT_GATHER;
  std::vector<uint64_t> fx;
  std::vector<uint32_t> fx_first;
};

namespace klf_impl KLF_LOCAL {

int set_err(klf_engine* e, int code, const std::string& m);
int hip_err(klf_engine* e, hipError_t h, const char* where);
#define HIPCHK(e, x, where) do { hipError_t _h = (x); if (_h != hipSuccess) return klf_impl::hip_err(e, _h, where); } while (0)

// Transforms and accessors of a finished run read the engine's workspace: only the latest
// result still owns it.
int check_latest(klf_engine* e, const klf_result* r, const char* what);
int check_result(klf_result* r, uint32_t id);
// The bitmap r was selected from (klf_result_group_bits): G' / G'', M, or none (no patterns:
// the parsed lines).
const uint32_t* sel_bits(const klf_result* r);
// What the kernels over r's selected lines read of its run (e->last_args: r is the latest).
klf::SelView sel_view(const klf_result* r);
// The latest run's global line index, built now if that run left it out (lazy index).
int ensure_index(klf_engine* e);
// Builds klf_around's G' into e->d_gbits (sized by the caller) from the latest run's M; ms = the
// build's device time, n / k = the anchors and their merged intervals.  (klf_analysis.cpp)
int around_build(klf_engine* e, const klf_result* prev, const klf_around_opts* o, double& ms, uint64_t& n,
                 uint64_t& k);
// What is wrong with klf_records' options, or null (no engine, no device).  (klf_analysis.cpp)
const char* records_opts_error(const klf_records_opts* o);
// Builds klf_records' G' into e->d_gbits (sized by the caller) from the latest run's M; ms = the
// build's device time, heads / conts = the parsed lines by class.  (klf_analysis.cpp)
int records_build(klf_engine* e, const klf_result* prev, const klf_records_opts* o, double& ms, uint64_t& heads,
                  uint64_t& conts);

// Device bytes -> a file descriptor (klf_result_write, klf_timeline_write).
constexpr size_t kStageChunk = 64u << 20;  // pinned staging chunk = device chunk
// A free pinned chunk of the staging pool, or a new one (false: none to be had).
bool take_chunk(klf_engine* e, klf_engine::StageChunk* c);
bool write_all(int fd, const uint8_t* p, uint64_t n);  // io.Copy's write loop
// a stream's output: [lo, hi) of the concatenated output, in d_out as `parts` ({offset,
// length}: one part, or a fused run's extents)
struct WPiece {
  uint64_t lo, hi;
  int fd;
  uint32_t id;
  std::vector<std::pair<uint64_t, uint64_t>> parts;
};

struct WErr { std::atomic<int> id{-1}; int err = 0; std::string what; std::mutex mu; };

// D2H each part of the stream's output in two halves of `buf` (double-buffered on `st`) and
// write(2) each half to fd.  Returns false with `werr` set on the first failure.
bool copy_part(klf_engine* e, const uint8_t* d_out, const WPiece& q, uint64_t dlo, uint64_t n, uint8_t* buf,
               uint64_t half, hipStream_t st, hipEvent_t ev[2], WErr& werr, uint64_t& total);

}  // namespace klf_impl
