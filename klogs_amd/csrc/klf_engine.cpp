// klf_engine.cpp — the C ABI of include/klf.h: staging, device workspace, the run,
// result views.  One engine = one GPU = one HIP stream (one process per GPU; the
// multi-GPU split happens above, in the host, by stream sharding — DESIGN.md §5).
// The calls on a finished run that make an object or a table of their own (histogram,
// timeline, groups, field statistics) are in klf_analysis.cpp.
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/klf.h"
#include "../../include/klf_debug.h"
#include "klf_engine_impl.hpp"
#include "klf_ts.hpp"

using namespace klf_impl;

// time spent growing device buffers (KLF_DIAG: the first run's allocation share)
std::atomic<uint64_t> klf_impl::g_alloc_ns{0};

namespace {

// An engine's first run maps its workspace buffers as one allocation (each hipMalloc costs
// tens of us of host time, ~20 of them add up in a one-shot run): buffers not yet mapped
// get 256-B aligned pieces of one block; later growth maps a buffer of its own.
// Maps the missing buffers of `req` into one block (an engine's first run: one allocation);
// a buffer that later outgrows its slice gets its own allocation, and the block is freed
// once no buffer borrows from it any more (`users`: the buffers mapped into it).
static hipError_t ensure_all(DevBuf& block, std::vector<DevBuf*>& users,
                             const std::vector<std::pair<DevBuf*, size_t>>& req) {
  size_t total = 0;
  for (auto& r : req)
    if (!r.first->p) total += (std::max<size_t>(r.second, 256) + 255) & ~(size_t)255;
  if (total && !block.p) {
    hipError_t h = block.ensure(total);
    if (h != hipSuccess) return h;
    size_t off = 0;
    for (auto& r : req) {
      if (r.first->p) continue;
      const size_t n = (std::max<size_t>(r.second, 256) + 255) & ~(size_t)255;
      r.first->p = static_cast<uint8_t*>(block.p) + off;
      r.first->cap = n;
      r.first->borrowed = true;
      users.push_back(r.first);
      off += n;
    }
  }
  for (auto& r : req)
    if (hipError_t h = r.first->ensure(r.second); h != hipSuccess) return h;
  if (block.p) {
    const uint8_t* lo = static_cast<const uint8_t*>(block.p);
    users.erase(std::remove_if(users.begin(), users.end(),
                               [&](DevBuf* b) {
                                 const uint8_t* q = static_cast<const uint8_t*>(b->p);
                                 return !(b->borrowed && q >= lo && q < lo + block.cap);
                               }),
                users.end());
    if (users.empty()) block.release();  // (every buffer outgrew its slice)
  }
  return hipSuccess;
}

uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

}  // namespace

// The run's counters and its per-stream records share one allocation (d_counters: the
// counters, then the records from byte kCtrBytes on), so that one D2H copy reads both back.
constexpr size_t kCtrBytes = klf::kNumCounters * 4;
static SegOut* segout_of(klf_engine* e) {
  return reinterpret_cast<SegOut*>(e->d_counters.as<uint8_t>() + kCtrBytes);
}

int klf_impl::set_err(klf_engine* e, int code, const std::string& m) {
  if (e) e->err = m;
  return code;
}

// The since cutoff as the scan compares it (RunArgs::since_dig): the 23 digits of its
// canonical UTC prefix, packed like parse_fast's p0..p5.  The fast path only accepts years
// 1970..2099, so an earlier cutoff passes every such line (1970-01-01T00:00:00Z) and a
// later one none (all '9').
static void since_digits(int64_t sec, int64_t nsec, uint32_t out[6]) {
  sec += nsec / 1000000000;  // (nsec normalised into [0, 1e9))
  nsec %= 1000000000;
  if (nsec < 0) {
    nsec += 1000000000;
    --sec;
  }
  char d[48];
  if (sec < 0) {
    memcpy(d, "19700101000000000000000", 23);
  } else if (sec >= 4102444800LL) {  // 2100-01-01T00:00:00Z
    memset(d, '9', 23);
  } else {
    const int64_t z = sec / 86400 + 719468, era = z / 146097;  // civil from days (proleptic Gregorian)
    const int64_t doe = z - era * 146097, yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100), mp = (5 * doy + 2) / 153;
    const int64_t day = doy - (153 * mp + 2) / 5 + 1, month = mp < 10 ? mp + 3 : mp - 9;
    const int64_t year = yoe + era * 400 + (month <= 2 ? 1 : 0), sod = sec % 86400;
    snprintf(d, sizeof d, "%04d%02d%02d%02d%02d%02d%09d", (int)year, (int)month, (int)day, (int)(sod / 3600),
             (int)(sod / 60 % 60), (int)(sod % 60), (int)nsec);
  }
  auto be = [&](char a, char b, char c, char e) {
    return (uint32_t)(uint8_t)a << 24 | (uint32_t)(uint8_t)b << 16 | (uint32_t)(uint8_t)c << 8 | (uint8_t)e;
  };
  out[0] = be(d[0], d[1], d[2], d[3]);      // YYYY
  out[1] = be(d[4], d[5], d[6], d[7]);      // MMDD
  out[2] = be(d[8], d[9], d[10], d[11]);    // hhmm
  out[3] = be(d[12], d[13], d[14], d[15]);  // ss n0 n1
  out[4] = be(d[16], d[17], d[18], d[19]);  // n2..n5
  out[5] = be(d[20], d[21], '0', d[22]);    // n6 n7 pad n8
}
int klf_impl::hip_err(klf_engine* e, hipError_t h, const char* where) {
  return set_err(e, KLF_EHIP, std::string(where) + ": " + hipGetErrorString(h));
}

extern "C" const char* klf_strerror(int code) {
  switch (code) {
    case KLF_OK: return "ok";
    case KLF_EINVAL: return "invalid argument";
    case KLF_ENOMEM: return "out of memory";
    case KLF_EHIP: return "HIP runtime error";
    case KLF_EPATTERN: return "pattern outside the supported RE2 subset";
    case KLF_ETOOBIG: return "pattern set exceeds engine limits";
    case KLF_ESTATE: return "call out of order";
    case KLF_EIO: return "write to a stream's file failed";
    default: return "unknown error";
  }
}

extern "C" const char* klf_last_error(const klf_engine* e) { return e ? e->err.c_str() : ""; }

template <class T>
static hipError_t upload(DevBuf& b, const std::vector<T>& v, hipStream_t st) {
  hipError_t h = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16));
  if (h != hipSuccess || v.empty()) return h;
  h = hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
  if (h != hipSuccess) return h;
  return hipStreamSynchronize(st);
}
// Several tables through one pinned staging buffer: async copies in stream order, no sync
// (the staging buffer is rewritten only after the stream has drained it: the next
// staged upload waits for the previous one's event)
struct StagedUpload {
  HostBuf& stage;
  hipStream_t st;
  hipEvent_t done;
  size_t off = 0;
  std::vector<std::pair<DevBuf*, std::pair<size_t, size_t>>> items;  // (buffer, (offset, bytes))
  template <class T>
  hipError_t add(DevBuf& b, const std::vector<T>& v) {
    hipError_t h = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16));
    if (h != hipSuccess) return h;
    items.push_back({&b, {off, v.size() * sizeof(T)}});
    off += (v.size() * sizeof(T) + 255) & ~(size_t)255;
    return hipSuccess;
  }
  template <class T>
  void fill(size_t k, const std::vector<T>& v) {
    if (!v.empty()) memcpy(stage.as<uint8_t>() + items[k].second.first, v.data(), v.size() * sizeof(T));
  }
};

// The prefilter tables that the layout choice (place_needles) rewrites: bitmap, buckets,
// anchor pre-checks, and the scalar layout fields of the device pattern set.
static hipError_t upload_prefilter(klf_engine* e) {
  const auto& cs = e->cs;
  hipStream_t st = e->stream;
  hipError_t h;
  std::vector<uint32_t> anc = cs.qf_anc_pre;
  if (anc.empty()) anc.assign(2, 0u);
  std::vector<uint32_t> pre = cs.rx_pre;  // the chosen needle set's match-start bounds
  if (pre.empty()) pre.assign(std::max<uint32_t>(cs.rx_count, 1u), klf::kRxPreUnbounded);
  // one pinned staging buffer, six async copies, no host sync (first-run latency)
  if (e->stage_ev_pending && (h = hipEventSynchronize(e->stage_ev)) != hipSuccess) return h;
  StagedUpload u{e->h_stage, st, e->stage_ev};
  if ((h = u.add(e->d_qf_bitmap, cs.qf_bitmap)) != hipSuccess || (h = u.add(e->d_qf_head, cs.qf_head)) != hipSuccess ||
      (h = u.add(e->d_qf_ent, cs.qf_ent)) != hipSuccess || (h = u.add(e->d_qf_anc, anc)) != hipSuccess ||
      (h = u.add(e->d_qf_nbytes, cs.qf_nbytes)) != hipSuccess || (h = u.add(e->d_rx_pre, pre)) != hipSuccess)
    return h;
  if ((h = e->h_stage.ensure(u.off + 256)) != hipSuccess) return h;
  u.fill(0, cs.qf_bitmap);
  u.fill(1, cs.qf_head);
  u.fill(2, cs.qf_ent);
  u.fill(3, anc);
  u.fill(4, cs.qf_nbytes);
  u.fill(5, pre);
  for (auto& it : u.items)
    if (it.second.second &&
        (h = hipMemcpyAsync(it.first->p, e->h_stage.as<uint8_t>() + it.second.first, it.second.second,
                            hipMemcpyHostToDevice, st)) != hipSuccess)
      return h;
  if ((h = hipEventRecord(e->stage_ev, st)) != hipSuccess) return h;
  e->stage_ev_pending = true;
  klf::DevPatterns& P = e->dpats;
  if (cs.rx_count) {  // (k_nfa_win / k_nfa split)
    P.rx_pre = e->d_rx_pre.as<uint32_t>();
    P.rx_unbounded = (uint32_t)std::count(pre.begin(), pre.end(), klf::kRxPreUnbounded);
  }
  P.qf_stride = cs.qf_stride;
  P.qf_mask = cs.qf_mask;
  P.qf_w24 = cs.qf_q == 4 ? 24u : 0u;
  P.qf_k = cs.qf_k;
  P.qf_bitmap = e->d_qf_bitmap.as<uint32_t>();
  P.qf_head = e->d_qf_head.as<uint32_t>();
  P.qf_ent = e->d_qf_ent.as<uint4>();
  P.qf_nbytes = e->d_qf_nbytes.as<uint32_t>();
  P.qf_anc_on = cs.qf_anc_on ? 1u : 0u;
  P.qf_anc_byte = cs.qf_anc_byte * 0x01010101u;
  P.qf_anc_fold = cs.qf_anc_fold;
  P.qf_anc_n = (uint32_t)(cs.qf_anc_pre.size() / 2);
  P.qf_anc_pre = e->d_qf_anc.as<uint32_t>();
  return hipSuccess;
}

// Host tables -> device buffers through the pinned staging buffer: one memcpy each into it,
// async copies in stream order, no host sync (the next staged upload waits for this one's
// event before it rewrites the buffer).  klf_open's pattern tables go up this way.
struct TableItem {
  DevBuf* dst;
  const void* src;
  size_t bytes;
};
static hipError_t stage_tables(klf_engine* e, const std::vector<TableItem>& items) {
  hipError_t h;
  if (e->stage_ev_pending && (h = hipEventSynchronize(e->stage_ev)) != hipSuccess) return h;
  e->stage_ev_pending = false;
  size_t total = 0;
  for (auto& it : items) {
    if ((h = it.dst->ensure(std::max<size_t>(it.bytes, 16))) != hipSuccess) return h;
    total += (it.bytes + 255) & ~(size_t)255;
  }
  if ((h = e->h_stage.ensure(total + 256)) != hipSuccess) return h;
  size_t off = 0;
  for (auto& it : items) {
    if (it.bytes) {
      memcpy(e->h_stage.as<uint8_t>() + off, it.src, it.bytes);
      if ((h = hipMemcpyAsync(it.dst->p, e->h_stage.as<uint8_t>() + off, it.bytes, hipMemcpyHostToDevice, e->stream)) !=
          hipSuccess)
        return h;
    }
    off += (it.bytes + 255) & ~(size_t)255;
  }
  if ((h = hipEventRecord(e->stage_ev, e->stream)) != hipSuccess) return h;
  e->stage_ev_pending = true;
  return hipSuccess;
}
template <class T>
static TableItem item(DevBuf& b, const std::vector<T>& v) {
  return TableItem{&b, v.data(), v.size() * sizeof(T)};
}

// The compiled set's matcher tables to the device (the prefilter layout only when it is
// placed already: tune_later = the first batch's statistics will place it).
static hipError_t upload_pattern_tables(klf_engine* e, bool tune_later) {
  const auto& cs = e->cs;
  hipError_t h;
  std::vector<TableItem> items;
  std::vector<uint8_t> padded;
  std::vector<uint64_t> vec, vec4;
  std::vector<uint32_t> pre0;
  if (cs.mode == klf::CompiledSet::kLiteral1) {
    padded = cs.literal;
    padded.resize((cs.literal.size() + 3) / 4 * 4 + 4, 0);  // bytes, then dword view at +0
    items.push_back(item(e->d_lit, padded));
  } else if (cs.mode == klf::CompiledSet::kGeneral) {
    klf::DevPatterns& P = e->dpats;
    if (cs.ac_states) {
      for (auto x : {item(e->d_ac_class, cs.ac_class), item(e->d_ac_next, cs.ac_next), item(e->d_ac_accept, cs.ac_accept),
                     item(e->d_ac_out, cs.ac_out), item(e->d_ac_dict, cs.ac_dict)})
        items.push_back(x);
      P.ac_states = cs.ac_states;
      P.ac_classes = cs.ac_classes;
    }
    if (cs.rx_count) {
      // first | last | init0 | end, each [rx_count]; and [rx][4] interleaved for k_nfa
      for (const auto* v : {&cs.rx_first, &cs.rx_last, &cs.rx_init0, &cs.rx_end}) vec.insert(vec.end(), v->begin(), v->end());
      for (uint32_t r = 0; r < cs.rx_count; ++r)
        for (const auto* v : {&cs.rx_first, &cs.rx_last, &cs.rx_init0, &cs.rx_end}) vec4.push_back((*v)[r]);
      pre0 = cs.rx_pre.empty() ? std::vector<uint32_t>(cs.rx_count, klf::kRxPreUnbounded) : cs.rx_pre;
      for (auto x : {item(e->d_rx_class, cs.rx_class), item(e->d_rx_b, cs.rx_b), item(e->d_rx_follow, cs.rx_follow),
                     item(e->d_rx_vec, vec), item(e->d_rx_flags, cs.rx_flags), item(e->d_rx_pre, pre0),
                     item(e->d_rx_vec4, vec4)})
        items.push_back(x);
      P.rx_unbounded = (uint32_t)std::count(pre0.begin(), pre0.end(), klf::kRxPreUnbounded);
      P.rx_count = cs.rx_count;
      P.rx_classes = cs.rx_classes;
      P.rx_maxpos = std::max<uint32_t>(1, cs.rx_maxpos);
    }
  }
  if (!items.empty() && (h = stage_tables(e, items)) != hipSuccess) return h;
  if (cs.mode == klf::CompiledSet::kGeneral) {  // device pointers of the staged tables
    klf::DevPatterns& P = e->dpats;
    if (cs.ac_states) {
      P.ac_class = e->d_ac_class.as<uint8_t>();
      P.ac_next = e->d_ac_next.as<uint32_t>();
      P.ac_accept = e->d_ac_accept.as<uint8_t>();
      P.ac_out = e->d_ac_out.as<int32_t>();
      P.ac_dict = e->d_ac_dict.as<uint32_t>();
    }
    if (cs.rx_count) {
      const uint64_t* v = e->d_rx_vec.as<uint64_t>();
      P.rx_class = e->d_rx_class.as<uint8_t>();
      P.rx_b = e->d_rx_b.as<uint64_t>();
      P.rx_follow = e->d_rx_follow.as<uint64_t>();
      P.rx_first = v;
      P.rx_last = v + cs.rx_count;
      P.rx_init0 = v + 2 * cs.rx_count;
      P.rx_end = v + 3 * cs.rx_count;
      P.rx_flags = e->d_rx_flags.as<uint32_t>();
      P.rx_pre = e->d_rx_pre.as<uint32_t>();
      P.rx_vec = e->d_rx_vec4.as<uint64_t>();
    }
    if (cs.qf_on) {
      if (!tune_later && (h = upload_prefilter(e)) != hipSuccess) return h;
      P.qf_on = 1;
      P.qf_fold = cs.qf_fold;
    }
  }
  return hipSuccess;
}

// the automaton thread: build, then one block on the device and one copy
// The literal automaton's thread: builds the tables, lays them out as one pinned block and
// maps the device block.  The upload itself is left to the join (ensure_ac), on the launch
// stream: a copy from this thread would go to HIP's null stream, where it queues behind a
// scan already running on that stream (an engine opened without a stream) and the join
// then waits for the scan (advisor r04).
static void ac_build_upload(klf_engine* e) {
  klf::build_ac(e->ac_lits, e->ac_tabs);
  const klf::AcTables& t = e->ac_tabs;
  hipError_t h = hipSetDevice(e->device);
  const std::pair<const void*, size_t> parts[5] = {
      {t.cls.data(), t.cls.size()}, {t.next.data(), t.next.size() * 4}, {t.accept.data(), t.accept.size()},
      {t.out.data(), t.out.size() * 4}, {t.dict.data(), t.dict.size() * 4}};
  size_t total = 0;
  for (int k = 0; k < 5; ++k) {
    e->ac_off[k] = total;
    e->ac_cap[k] = (std::max<size_t>(parts[k].second, 256) + 255) & ~(size_t)255;
    total += e->ac_cap[k];
  }
  e->ac_total = total;
  if (h == hipSuccess) h = e->h_acblk.ensure(total);
  if (h == hipSuccess) {
    memset(e->h_acblk.p, 0, total);
    for (int k = 0; k < 5; ++k) memcpy(e->h_acblk.as<uint8_t>() + e->ac_off[k], parts[k].first, parts[k].second);
  }
  if (h == hipSuccess) h = e->d_acblk.ensure(total);
  e->ac_err = h;
}

// Joins the automaton thread (if any) and points the device patterns at its tables.
static int ensure_ac(klf_engine* e) {
  if (e->ac_thread.joinable()) e->ac_thread.join();
  if (!e->ac_pending) return KLF_OK;
  e->ac_pending = false;
  if (e->ac_err != hipSuccess) return hip_err(e, e->ac_err, "Aho-Corasick tables");
  // the upload, ordered on the launch stream before the first kernel that reads it (the
  // pinned block stays until klf_close)
  HIPCHK(e, hipMemcpyAsync(e->d_acblk.p, e->h_acblk.p, e->ac_total, hipMemcpyHostToDevice, e->stream),
         "upload Aho-Corasick tables");
  DevBuf* dst[5] = {&e->d_ac_class, &e->d_ac_next, &e->d_ac_accept, &e->d_ac_out, &e->d_ac_dict};
  for (int k = 0; k < 5; ++k) {
    dst[k]->release();
    dst[k]->p = e->d_acblk.as<uint8_t>() + e->ac_off[k];
    dst[k]->cap = e->ac_cap[k];
    dst[k]->borrowed = true;
  }
  klf::CompiledSet& cs = e->cs;
  klf::AcTables& t = e->ac_tabs;
  cs.ac_states = t.states;
  cs.ac_classes = t.classes;
  cs.ac_class = std::move(t.cls);
  cs.ac_next = std::move(t.next);
  cs.ac_accept = std::move(t.accept);
  cs.ac_out = std::move(t.out);
  cs.ac_dict = std::move(t.dict);
  klf::DevPatterns& P = e->dpats;
  P.ac_states = cs.ac_states;
  P.ac_classes = cs.ac_classes;
  P.ac_class = e->d_ac_class.as<uint8_t>();
  P.ac_next = e->d_ac_next.as<uint32_t>();
  P.ac_accept = e->d_ac_accept.as<uint8_t>();
  P.ac_out = e->d_ac_out.as<int32_t>();
  P.ac_dict = e->d_ac_dict.as<uint32_t>();
  return KLF_OK;
}

extern "C" int klf_open(const klf_config* cfg, klf_engine** out) {
  if (!cfg || !out || (cfg->n_patterns && !cfg->patterns)) return KLF_EINVAL;
  *out = nullptr;
  auto* e = new (std::nothrow) klf_engine();
  if (!e) return KLF_ENOMEM;
  // 1) patterns (host only; errors surface before any device work)
  std::vector<std::vector<uint8_t>> pats;
  std::vector<uint32_t> kinds;
  for (uint32_t i = 0; i < cfg->n_patterns; ++i) {
    const klf_pattern& p = cfg->patterns[i];
    if (p.len && !p.bytes) { delete e; return KLF_EINVAL; }
    pats.emplace_back(p.bytes, p.bytes + p.len);
    kinds.push_back(p.kind);
  }
  int code = KLF_OK;
  std::string err;
  const auto t_open0 = std::chrono::steady_clock::now();
  // the prefilter layout waits for the first batch's statistics (the first run places the
  // needles), unless tuning is off (KLF_QF_TUNE=0: placed here, from byte-class estimates)
  const char* tune_env = getenv("KLF_QF_TUNE");
  const bool tune_later = !(tune_env && strcmp(tune_env, "0") == 0);
  const bool compiled = klf::compile_set(pats, kinds, e->cs, err, code, !tune_later, true, true);
  e->tune_later = tune_later;
  e->ac_lits.swap(e->cs.ac_lits);  // (the automaton thread's input; built after the device setup)
  if (compiled && e->cs.also_all_pending) {
    e->pend_pats = pats;
    e->pend_kinds = kinds;
  }
  if (getenv("KLF_DIAG"))
    fprintf(stderr, "[klf] open: pattern compile %.1f us\n",
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_open0).count());
  if (getenv("KLF_DIAG") && compiled && e->cs.qf_on && !tune_later)  // (tuned: the first run prints it)
    fprintf(stderr, "[klf] prefilter layout from 0 sampled bytes: %s\n", e->cs.qf_layout.c_str());
  if (!compiled) {
    // keep the engine alive so the caller can read klf_last_error; report failure
    e->err = err;
    *out = e;
    return code;
  }
  // 2) device
  e->device = cfg->device;
  e->n_user = cfg->n_patterns;
  e->dpats.n_cids = e->cs.n_cids;
  e->dpats.n_lits = e->cs.n_lits;
  hipError_t h = hipSetDevice(cfg->device);
  if (h != hipSuccess) { e->err = std::string("hipSetDevice: ") + hipGetErrorString(h); *out = e; return KLF_EHIP; }
  const bool diag_open = getenv("KLF_DIAG") != nullptr;
  auto open_mark = [&](const char* what) {
    if (diag_open)
      fprintf(stderr, "[klf] open: %s at %.1f us\n", what,
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_open0).count());
  };
  open_mark("device set");
  int ncu = 0;  // (one attribute query: hipGetDeviceProperties fills the whole struct, ~ms)
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && ncu > 0)
    e->num_cus = ncu;
  open_mark("attribute");
  // the caller's stream, else HIP's null stream: it exists from device init, while a new
  // stream costs ~5 ms of host time when it brings up a hardware queue (MI355X), which a
  // one-shot klogs invocation would pay in full
  e->stream = static_cast<hipStream_t>(cfg->hip_stream);
  open_mark("stream");
  for (auto& x : e->ev) {
    h = hipEventCreate(&x);
    if (h != hipSuccess) { e->err = "hipEventCreate failed"; *out = e; return KLF_EHIP; }
  }
  if (getenv("KLF_DIAG"))
    fprintf(stderr, "[klf] open: events done at %.1f us\n",
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_open0).count());
  if ((h = hipEventCreateWithFlags(&e->stage_ev, hipEventDisableTiming)) != hipSuccess) {
    *out = e;
    return hip_err(e, h, "staging event");
  }
  if (getenv("KLF_DIAG"))
    fprintf(stderr, "[klf] open: device setup done at %.1f us\n",
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_open0).count());
  // 3) pattern tables to the device
  if ((h = upload_pattern_tables(e, tune_later)) != hipSuccess) {
    *out = e;
    return hip_err(e, h, "upload pattern tables");
  }
  if (const char* cc = getenv("KLF_CAND_CAP"))  // tests: force the queue-overflow fallback
    e->cand_cap = (uint32_t)std::max(1L, std::min(atol(cc), 1L << 28));
  if (const char* pl = getenv("KLF_PAIRS_LOG2"))  // tests: a small per-pattern pair set (grows on overflow)
    e->pairs_log2 = (uint32_t)std::max(4L, std::min(atol(pl), 28L));
  if (const char* hc = getenv("KLF_HITS_CAP"))  // tests: force the hit-list overflow fallback
    e->hits_cap_max = (uint64_t)std::max(1L, std::min(atol(hc), 1L << 28));
  if (!e->ac_lits.empty()) {
    e->ac_pending = true;
    try {
      e->ac_thread = std::thread(ac_build_upload, e);
    } catch (...) {  // no thread: build it here
      ac_build_upload(e);
    }
  }
  if (getenv("KLF_DIAG"))
    fprintf(stderr, "[klf] open: total %.1f us\n",
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_open0).count());
  *out = e;
  return KLF_OK;
}

static void release_staged(klf_engine* e);
static void free_chunk(klf_engine::StageChunk& c);

extern "C" void klf_close(klf_engine* e) {
  if (!e) return;
  if (e->ac_thread.joinable()) e->ac_thread.join();
  (void)hipStreamSynchronize(e->stream);
  if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
  for (DevBuf* b : {&e->d_lit, &e->d_ac_class, &e->d_ac_next, &e->d_ac_accept, &e->d_rx_class, &e->d_rx_b,
                    &e->d_rx_follow, &e->d_rx_vec, &e->d_rx_flags, &e->d_rx_pre, &e->d_qf_bitmap, &e->d_qf_head,
                    &e->d_qf_ent, &e->d_qf_nbytes, &e->d_qf_anc, &e->d_rx_vec4, &e->d_qhits, &e->d_hslots, &e->d_hist, &e->d_hflat, &e->d_cand, &e->d_batch, &e->d_segs, &e->d_tstat,
                    &e->d_slots, &e->d_pool, &e->d_tile_base, &e->d_bsum, &e->d_cstatus, &e->d_counters, &e->d_cmap, &e->d_cseg,
                    &e->d_line_off, &e->d_meta, &e->d_bits, &e->d_wpre, &e->d_out, &e->d_tile_seg, &e->d_mpart, &e->d_trec, &e->d_truns, &e->d_kbase,
                    &e->d_fext0, &e->d_fext, &e->d_frinfo, &e->d_out2, &e->d_gbits, &e->d_gsum})
    b->release();
  e->d_asm.release();
  e->d_scratch.release();
  e->h_rb.release();
  e->h_acblk.release();
  e->h_hist.release();
  e->d_thist.release();
  e->h_thist.release();
  e->h_stage.release();
  for (DevBuf* b : {&e->d_ac_out, &e->d_ac_dict, &e->d_pcount, &e->d_pairs}) b->release();
  e->d_block.release();
  e->d_block2.release();
  e->d_acblk.release();
  e->copier.reset();
  {
    std::lock_guard<std::mutex> g(e->mu);
    release_staged(e);
    for (auto& c : e->chunk_pool) free_chunk(c);
    e->chunk_pool.clear();
    for (uint8_t* d : e->dchunk_pool) (void)hipFree(d);
    e->dchunk_pool.clear();
    for (auto x : e->ev_pool) (void)hipEventDestroy(x);
    e->ev_pool.clear();
  }
  for (auto& x : e->ev)
    if (x) (void)hipEventDestroy(x);
  if (e->copy_done) (void)hipEventDestroy(e->copy_done);
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
  if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
  if (e->stage_ev) (void)hipEventDestroy(e->stage_ev);
  delete e;
  (void)hipGetLastError();  // nothing above reports: leave no sticky error for the next engine
}

// ------------------------------------------------------------------------ staging ---

static constexpr size_t kMaxInflight = 8;         // pinned chunks with an H2D in flight (512 MiB)

// The copy stream of the host staging path (and its event), made on first use: a
// device-resident caller (klf_run_device) never pays for it.
static hipError_t ensure_copy_stream(klf_engine* e) {
  std::call_once(e->copy_stream_once, [e] {
    hipError_t h = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking);
    if (h == hipSuccess) h = hipEventCreateWithFlags(&e->copy_done, hipEventDisableTiming);
    e->copy_stream_err = h;
  });
  return e->copy_stream_err;
}

static void grow_table(klf_engine* e, size_t n) {  // caller holds e->mu
  while (e->staged.size() < n) e->staged.emplace_back(new klf_engine::StagedStream());
}

extern "C" int klf_set_streams(klf_engine* e, uint32_t n) {
  if (!e) return KLF_EINVAL;
  std::lock_guard<std::mutex> g(e->mu);
  if (e->ran) return set_err(e, KLF_ESTATE, "klf_set_streams after klf_run: klf_reset first");
  if (n < e->staged.size()) return set_err(e, KLF_ESTATE, "cannot shrink the stream table; klf_reset first");
  try {
    grow_table(e, n);
  } catch (...) {
    return set_err(e, KLF_ENOMEM, "stream table");
  }
  return KLF_OK;
}

static void free_chunk(klf_engine::StageChunk& c) {
  if (!c.p) return;
  if (c.pinned) (void)hipHostFree(c.p);
  else free(c.p);
  c.p = nullptr;
}

// A free pinned chunk: the pool, else a chunk whose H2D has finished, else (with
// kMaxInflight chunks in flight) the oldest one once its DMA is done, else a new one.
bool klf_impl::take_chunk(klf_engine* e, klf_engine::StageChunk* c) {
  klf_engine::Inflight wait{};
  bool have_wait = false;
  {
    std::lock_guard<std::mutex> g(e->mu);
    while (!e->inflight.empty() && hipEventQuery(e->inflight.front().ev) == hipSuccess) {
      e->chunk_pool.push_back(e->inflight.front().c);
      e->ev_pool.push_back(e->inflight.front().ev);
      e->inflight.pop_front();
    }
    if (!e->chunk_pool.empty()) {
      *c = e->chunk_pool.back();
      e->chunk_pool.pop_back();
      c->used = 0;
      return true;
    }
    if (e->inflight.size() >= kMaxInflight) {
      wait = e->inflight.front();
      e->inflight.pop_front();
      have_wait = true;
    }
  }
  if (have_wait) {
    (void)hipEventSynchronize(wait.ev);
    {
      std::lock_guard<std::mutex> g(e->mu);
      e->ev_pool.push_back(wait.ev);
    }
    *c = wait.c;
    c->used = 0;
    return true;
  }
  void* p = nullptr;
  if (hipHostMalloc(&p, kStageChunk, hipHostMallocDefault) == hipSuccess && p) {
    c->p = static_cast<uint8_t*>(p);
    c->pinned = true;
  } else {
    (void)hipGetLastError();
    c->p = static_cast<uint8_t*>(malloc(kStageChunk));
    c->pinned = false;
    if (!c->p) return false;
  }
  c->used = 0;
  return true;
}

// The stream's full pinned chunk -> a device chunk, DMA'd now on the copy stream (the
// capture keeps running meanwhile); the pinned chunk returns to the pool when the DMA ends.
static int ship_chunk(klf_engine* e, klf_engine::StagedStream* s) {
  uint8_t* d = nullptr;
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->dchunk_pool.empty()) {
      d = e->dchunk_pool.back();
      e->dchunk_pool.pop_back();
    }
    if (!e->ev_pool.empty()) {
      ev = e->ev_pool.back();
      e->ev_pool.pop_back();
    }
  }
  hipError_t h = hipSuccess;
  if (!d) h = hipMalloc(reinterpret_cast<void**>(&d), kStageChunk);
  if (h != hipSuccess) {  // hand the event back; the error string is shared with other stagers
    std::lock_guard<std::mutex> g(e->mu);
    if (ev) e->ev_pool.push_back(ev);
    return hip_err(e, h, "device staging chunk");
  }
  if (!ev) h = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (h == hipSuccess) h = hipMemcpyAsync(d, s->cur.p, kStageChunk, hipMemcpyHostToDevice, e->copy_stream);
  if (h == hipSuccess) h = hipEventRecord(ev, e->copy_stream);
  std::lock_guard<std::mutex> g(e->mu);
  if (h != hipSuccess) {
    e->dchunk_pool.push_back(d);
    if (ev) e->ev_pool.push_back(ev);
    return hip_err(e, h, "early H2D");
  }
  s->dchunks.push_back(d);
  e->inflight.push_back({s->cur, ev});
  s->cur = klf_engine::StageChunk{};
  return KLF_OK;
}

extern "C" int klf_stage(klf_engine* e, uint32_t id, const uint8_t* p, size_t n) {
  if (!e || (n && !p)) return KLF_EINVAL;
  klf_engine::StagedStream* dst;
  {
    std::lock_guard<std::mutex> g(e->mu);
    if (e->ran) return set_err(e, KLF_ESTATE, "klf_stage after klf_run: klf_reset first");
    try {
      grow_table(e, (size_t)id + 1);
    } catch (...) {
      return set_err(e, KLF_ENOMEM, "stream table");
    }
    dst = e->staged[id].get();  // stable: the table holds pointers, only the table moves
  }
  if (hipError_t h = ensure_copy_stream(e); h != hipSuccess) return hip_err(e, h, "copy stream");
  std::call_once(e->copier_once, [e] {
    int nw = 3;  // staging copy workers (+ the calling thread)
    if (const char* v = getenv("KLF_STAGE_THREADS")) nw = std::max(0, std::min(atoi(v), 32));
    e->copier.reset(new klf::CopyPool(nw));
  });
  while (n) {
    if (!dst->cur.p && !take_chunk(e, &dst->cur)) {
      std::lock_guard<std::mutex> g(e->mu);
      return set_err(e, KLF_ENOMEM, "pinned staging chunk");
    }
    const size_t k = std::min(n, kStageChunk - dst->cur.used);
    e->copier->copy(dst->cur.p + dst->cur.used, p, k);
    dst->cur.used += k;
    dst->len += k;
    p += k;
    n -= k;
    if (dst->cur.used == kStageChunk) {
      const int rc = ship_chunk(e, dst);
      if (rc) return rc;
    }
  }
  return KLF_OK;
}

static void release_staged(klf_engine* e) {  // caller holds e->mu; no H2D may be in flight
  for (auto& s : e->staged) {
    for (uint8_t* d : s->dchunks) e->dchunk_pool.push_back(d);
    if (s->cur.p) {
      s->cur.used = 0;
      e->chunk_pool.push_back(s->cur);
    }
  }
  for (auto& f : e->inflight) {
    e->chunk_pool.push_back(f.c);
    e->ev_pool.push_back(f.ev);
  }
  e->inflight.clear();
  e->staged.clear();
  e->ran = false;
}

extern "C" int klf_reset(klf_engine* e) {
  if (!e) return KLF_EINVAL;
  std::lock_guard<std::mutex> g(e->mu);
  if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);  // early DMAs read the pinned chunks
  (void)hipStreamSynchronize(e->stream);       // k_assemble reads the device chunks
  release_staged(e);
  return KLF_OK;
}

extern "C" int klf_layout(uint32_t n, const uint64_t* lens, uint64_t* seg_base, uint64_t* total) {
  if ((n && (!lens || !seg_base)) || !total) return KLF_EINVAL;
  uint64_t off = 0;
  for (uint32_t i = 0; i < n; ++i) {
    seg_base[i] = off;
    off = align_up(off + lens[i], klf::kSegAlign);
  }
  *total = off + klf::kAllocSlack;
  return KLF_OK;
}

// -------------------------------------------------------------------------- run ---

// Waits for the run's readback by polling the stream: a blocking sync sleeps and wakes
// tens of microseconds after the last copy lands (measured ~50 us between batches of a
// capture loop), a poll returns within a microsecond or two.  The poll is bounded: past
// the expected run time (`spin_us`, the batch's bytes at ~2 TB/s plus a margin) the
// thread yields between polls for a while and then blocks, so one engine per GPU in one
// process does not keep a host core busy per GPU through a long run, and a hung kernel
// leaves the thread asleep in the runtime instead of spinning.
static hipError_t wait_stream(hipStream_t st, uint64_t spin_us) {
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 0;; ++i) {
    const hipError_t h = hipStreamQuery(st);
    if (h != hipErrorNotReady) return h;
    if ((i & 63) == 63) {
      const uint64_t us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                              std::chrono::steady_clock::now() - t0).count();
      if (us > spin_us + 20000) return hipStreamSynchronize(st);
      if (us > spin_us) std::this_thread::yield();
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
}

// An attempt's counters (the first 32) and stream records, and `ext` bytes of a one-pass run's extents
// behind them in h_rb, to the host: the copies on the engine stream, then the wait (`spin_us` of polling,
// 0: a blocking sync).  `*where`, if given, names the sync on entry and the call that failed on return.
static hipError_t read_back(klf_engine* e, uint32_t nsegs, size_t ext, uint64_t spin_us, uint32_t* counters, SegOut* so,
                            const char** where = nullptr) {
  uint8_t* rb = e->h_rb.as<uint8_t>();
  const size_t n = kCtrBytes + nsegs * sizeof(SegOut);
  const char* sync = where ? *where : "";
  if (where) *where = "D2H counters + records";
  hipError_t h = hipMemcpyAsync(rb, e->d_counters.p, n, hipMemcpyDeviceToHost, e->stream);
  if (h != hipSuccess) return h;
  if (where && ext) *where = "D2H extents";
  if (ext && (h = hipMemcpyAsync(rb + n, e->d_fext.p, ext, hipMemcpyDeviceToHost, e->stream)) != hipSuccess) return h;
  if (where) *where = sync;
  if ((h = spin_us ? wait_stream(e->stream, spin_us) : hipStreamSynchronize(e->stream)) != hipSuccess) return h;
  memcpy(counters, rb, 32 * sizeof(uint32_t));
  memcpy(so, rb + kCtrBytes, nsegs * sizeof(SegOut));
  return hipSuccess;
}

// Output bigger than the buffer (counters[kCtrOutShort], from k_cmove / k_tcopy, which
// skipped the copies that would not fit but still wrote every stream's output range): grow
// the buffer to the run's output and rerun the tail stage over the line index and bitmap
// still in HBM (k_mcount .. k_tcopy, tens of us), then read the stream records back.
static hipError_t grow_out_retail(klf_engine* e, klf::RunArgs& a, std::vector<SegOut>& so) {
  a.plan_runs = 0;  // the tile plans were consumed (k_cmove rewrote them): list the runs again
  a.skip_tcopy = 0;
  a.plan_mode = 0;  // (k_cplan / k_cmid / k_cmove, whichever path the window takes)
  for (int k = 0; k < 2; ++k) {
    uint64_t need = 0;
    for (auto& s : so) need = std::max(need, s.out_hi);
    hipError_t h = e->d_out.ensure(need + 64);
    if (h != hipSuccess) return h;
    a.out = e->d_out.as<uint8_t>();
    a.out_cap = e->d_out.cap;
    if ((h = klf::launch_retail(a, e->stream, e->ev, e->num_cus)) != hipSuccess) return h;
    uint32_t counters[32];
    if ((h = read_back(e, (uint32_t)so.size(), 0, 0, counters, so.data())) != hipSuccess) return h;
    if (!counters[klf::kCtrOutShort]) return hipSuccess;
  }
  return hipErrorOutOfMemory;  // the ranges did not settle (cannot happen: they do not depend on the buffer)
}

// One steady run's launch sequence (launch_pipeline, phase 0, no events inside: a graph's
// event nodes are not re-recorded by a replay) as a replayed graph, bracketed by ev[0] /
// ev[5] on the engine stream.  Returns false when the run should launch eagerly instead:
// a first sighting of these arguments, or a capture that failed (then never again).
static bool launch_graph(klf_engine* e, const klf::RunArgs& a, uint32_t& ev_mask, bool diag) {
  const uint8_t* k = reinterpret_cast<const uint8_t*>(&a);
  std::vector<uint8_t> key(k, k + sizeof(a));
  key.insert(key.end(), reinterpret_cast<const uint8_t*>(&e->num_cus),
             reinterpret_cast<const uint8_t*>(&e->num_cus) + sizeof(e->num_cus));
  if (!e->gexec || key != e->gkey) {
    if (key != e->gprev) {  // first sighting: eager, remembered
      e->gprev = std::move(key);
      return false;
    }
    if (e->gexec) {
      (void)hipGraphExecDestroy(e->gexec);
      e->gexec = nullptr;
      e->gkey.clear();
    }
    if (!e->cap_stream && hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();
      e->graph_off = true;
      return false;
    }
    hipGraph_t g = nullptr;
    bool ok = hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeRelaxed) == hipSuccess;
    if (ok) {
      const hipError_t h = klf::launch_pipeline(a, e->cap_stream, nullptr, e->num_cus, 0, nullptr);
      ok = hipStreamEndCapture(e->cap_stream, &g) == hipSuccess && h == hipSuccess && g;
    }
    if (ok) ok = hipGraphInstantiate(&e->gexec, g, nullptr, nullptr, 0) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    if (!ok) {
      (void)hipGetLastError();
      if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
      e->gexec = nullptr;
      e->graph_off = true;
      if (diag) fprintf(stderr, "[klf] graph capture failed: eager launches from here on\n");
      return false;
    }
    e->gkey = std::move(key);
  }
  if (hipEventRecord(e->ev[0], e->stream) != hipSuccess) return false;
  if (hipGraphLaunch(e->gexec, e->stream) != hipSuccess) {
    (void)hipGetLastError();
    e->graph_off = true;
    return false;
  }
  ev_mask = 1u;
  if (hipEventRecord(e->ev[5], e->stream) == hipSuccess) ev_mask |= 1u << 5;
  return true;
}

// ---- The run on the host: the knobs, the plan, what a redo changes, the steps ----
using Clock = std::chrono::steady_clock;
using BufList = std::vector<std::pair<DevBuf*, size_t>>;
// Every KLF_* variable of the run path (DESIGN.md 4a lists what each does), read once per run:
// tests flip them between the runs of one process.
struct RunKnobs {
  bool diag, two_phase, one_phase, tindex_wide, graph;
  bool qf_tune, fuse, lazy_index, plan_runs, win_index, win_index_rx, skip_idle;  // KLF_<NAME>=0 turns each off
  uint64_t graph_max, cap_clamp, out_init, pool_cap;
  uint32_t scatter_split;
  const char *fuse_range, *nl_scale, *compact, *wave_pool, *plan_mode, *timeline_out;  // parsed where they apply
};
static bool knob_off(const char* name) { const char* v = getenv(name); return v && !strcmp(v, "0"); }
static RunKnobs read_knobs() {
  auto num = [](const char* name, long lo, int64_t unset) {  // a number, at least `lo`
    const char* v = getenv(name);
    return (uint64_t)(v ? (int64_t)std::max(lo, atol(v)) : unset);
  };
  RunKnobs k;
  k.diag = getenv("KLF_DIAG"); k.two_phase = getenv("KLF_TWO_PHASE"); k.one_phase = getenv("KLF_ONE_PHASE");
  k.tindex_wide = getenv("KLF_DEBUG_TINDEX_WIDE");
  k.graph = getenv("KLF_GRAPH") && !knob_off("KLF_GRAPH");  // (opt-in)
  k.graph_max = num("KLF_GRAPH_MAX_MB", 0, 256) << 20;
  k.qf_tune = !knob_off("KLF_QF_TUNE"); k.fuse = !knob_off("KLF_FUSE"); k.lazy_index = !knob_off("KLF_LAZY_INDEX");
  k.plan_runs = !knob_off("KLF_PLAN_RUNS"); k.skip_idle = !knob_off("KLF_SKIP_IDLE");
  k.win_index = !knob_off("KLF_WIN_INDEX"); k.win_index_rx = !knob_off("KLF_WIN_INDEX_RX");
  k.cap_clamp = num("KLF_DEBUG_CAP_CLAMP", 1, -1); k.out_init = num("KLF_DEBUG_OUT_INIT", 1, 64ll << 20);  // (~0: none)
  k.pool_cap = num("KLF_DEBUG_POOL_CAP", 1, 0); k.scatter_split = (uint32_t)num("KLF_SCATTER_SPLIT", 0, 0);
  k.fuse_range = getenv("KLF_DEBUG_FUSE_RANGE"); k.nl_scale = getenv("KLF_DEBUG_NL_SCALE");
  k.compact = getenv("KLF_COMPACT"); k.wave_pool = getenv("KLF_WAVE_POOL"); k.plan_mode = getenv("KLF_PLAN_MODE");
  k.timeline_out = getenv("KLF_TIMELINE_OUT");
  return k;
}
struct RunPlan {  // what stays fixed through a run's attempts
  klf_engine* e; const klf_filter* f; const uint8_t* d_bytes; RunKnobs k;  // (aggregate-initialised: keep first)
  std::vector<SegDesc> segs;  // the non-empty streams
  uint32_t nsegs = 0, compact_mode = 0, qhits_cap = 0;
  uint64_t ntiles = 0, total_bytes = 0, hflat_cap = 0, out_need = 0, seg_end = 0;  // seg_end: past the last input byte
  klf::CompiledSet::Mode mode = klf::CompiledSet::kNone;
  bool count = false;        // per-pattern counts are evaluated
  bool same_layout = false;  // the last run's streams: d_segs / d_tile_seg stand
  bool small_first = false;  // a first batch that maps its 32-B-rule line arrays as they are
  bool want_truns = false, fuse_try = false, lazy_index = false, full_index = false, need_cand = false,
       need_hits = false;
  hipEvent_t* evs = nullptr;  // KLF_FILTER_NO_TIMING: none (launch_pipeline records none)
  bool gram = false;          // the first batch's sample (start_sample): the gram histogram is in flight,
  uint32_t nl_blocks = 0;     // or the newline count over this many tiles (0: neither)
  bool density_cap = false, wave_pool = false;  // (what the sample's density decides: plan_density)
  Clock::time_point t_run0 = Clock::now(), t_tune0;  // KLF_DIAG: wall-clock marks through the run
  uint64_t alloc0 = g_alloc_ns.load(), tune_ns = 0;
  std::vector<std::pair<const char*, Clock::time_point>> marks;
  void mark(const char* what) { if (k.diag) marks.emplace_back(what, Clock::now()); }
};
struct RunState {  // what a redo changes (apply_outcome), besides e->pool_cap and e->pairs_log2
  uint64_t cap = 0;           // line capacity of the next attempt
  uint32_t pool_chunk = 256;  // the wave pool's chunk size (pool_need)
  bool fuse_ok = false, win_ok = false;  // one-pass compaction; windowed line index
  bool force_match = false;              // an overflowed hit list / NFA queue: k_match decides
  int line_reruns = 0, pair_reruns = 0;
};
// What an attempt asks for.  kLines: more lines (or pool slots) than estimated; kMatch: an overflowed hit list or
// queue with k_match skipped; kFuse: the one pass was voided; kIndex: the whole line index is needed; kPairs: set full.
enum Outcome { kDone, kLines, kMatch, kFuse, kIndex, kPairs };
static const char* const kOutcomeName[] = {"done", "lines", "match", "fuse", "index", "pairs"};
enum Next { kStand, kRedo, kFail };  // what follows an attempt: its result stands, another attempt, the run fails
struct Attempt {
  klf::RunArgs a;
  uint32_t counters[32];
  uint32_t ev_mask;   // the events this attempt recorded (the timing queries read only those)
  const char* shape;  // plain / graph / two-phase / ac-split
  bool phase1;        // ended at phase 1's readback (kLines)
  bool tcopy, grown;  // in-place relaunches (the deferred k_tcopy, grow_out_retail); they clear the fields
  uint32_t skip_tcopy, plan_mode, plan_runs;  // kept here as launched, for the KLF_DIAG line
};
static void learn_density(klf_engine* e, const std::vector<SegOut>& so, uint64_t total_bytes) {
  e->line_density = (double)(so.back().line_hi + 1) / (double)total_bytes;
}
static void bump_pool(klf_engine* e, const uint32_t* counters) {  // what the scan reserved + every wave's last chunk
  e->pool_cap = std::max<uint64_t>(e->pool_cap, (uint64_t)counters[klf::kCtrPool] + (uint64_t)e->num_cus * 16 * 4096);
}
static uint64_t learned_cap(const RunPlan& p) {  // line capacity from the last run's line density (+25 %)
  return (uint64_t)(p.e->line_density * (double)p.total_bytes * 1.25) + 2ull * p.nsegs + 4096;
}
static uint32_t seg_of_tile(const std::vector<SegDesc>& segs, uint64_t t) {
  uint32_t lo = 0, hi = (uint32_t)segs.size();  // the last segment whose tile0 <= t
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (segs[mid].tile0 <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// The first run asking for per-pattern counts of a set with an always-pattern compiles the other
// patterns (klf_open kept the set as kAll); if that fails the counts are reported unavailable.
static int compile_pending(klf_engine* e) {
  if (const int rc = ensure_ac(e); rc != KLF_OK) return rc;
  klf::CompiledSet full;
  std::string cerr; int ccode = KLF_OK;
  if (klf::compile_set(e->pend_pats, e->pend_kinds, full, cerr, ccode, !e->tune_later, false)) {
    e->cs = std::move(full);
    e->dpats.n_cids = e->cs.n_cids; e->dpats.n_lits = e->cs.n_lits;
    HIPCHK(e, upload_pattern_tables(e, e->tune_later), "upload pattern tables");
  } else {
    e->cs.also_all_pending = false;
    e->counts_code = ccode; e->counts_err = "per-pattern counts unavailable: " + cerr;
  }
  return KLF_OK;
}
static int layout_segments(RunPlan& p, RunState& s, klf_result* r, uint32_t n_streams, const uint64_t* seg_base,
                           const uint64_t* lens) {
  for (uint32_t i = 0; i < n_streams; ++i) {
    if (!lens[i]) continue;
    if (seg_base[i] % klf::kSegAlign) return set_err(p.e, KLF_EINVAL, "seg_base must be 256-B aligned");
    SegDesc d;
    d.base = seg_base[i]; d.len = lens[i]; d.tile0 = (uint32_t)p.ntiles;
    d.ntiles = (uint32_t)((lens[i] + klf::kTile - 1) / klf::kTile);
    r->seg_of[i] = (int64_t)p.segs.size();
    p.segs.push_back(d); r->seg_base.push_back(d.base);
    p.ntiles += d.ntiles; p.total_bytes += lens[i];
    s.cap += lens[i] / 32 + 2;  // kubelet lines carry a >= 31-byte prefix; overflow -> exact rerun
  }
  if (p.ntiles >= (1ull << 32)) return set_err(p.e, KLF_EINVAL, "batch too large");
  p.nsegs = (uint32_t)p.segs.size();
  if (p.e->line_density > 0.0) s.cap = std::min<uint64_t>(s.cap, learned_cap(p));
  return KLF_OK;
}

static void plan_run(RunPlan& p, RunState& s) {
  klf_engine* e = p.e;
  const klf_filter* f = p.f;
  const bool general = p.mode == klf::CompiledSet::kGeneral, none = p.mode == klf::CompiledSet::kNone;
  s.cap = std::min(s.cap, p.k.cap_clamp);
  p.same_layout = p.segs.size() == e->last_segs.size() && e->d_tile_seg.cap >= p.ntiles * 4 &&
                  memcmp(p.segs.data(), e->last_segs.data(), p.segs.size() * sizeof(SegDesc)) == 0;
  // (32-B-rule line arrays of at most ~2 GB are mapped as they are: no sample, no sync before the scan)
  p.small_first = e->line_density == 0.0 && s.cap * 11 <= (2ull << 30) && !p.k.two_phase && !p.k.nl_scale;
  // the dense compaction's per-tile run table only without --tail or once a --tail run went dense (else k_tcopy lists)
  p.want_truns = f->tail < 0 || e->dense_tail_seen;
  if (const char* v = p.k.compact) p.compact_mode = !strcmp(v, "sparse") ? 1u : !strcmp(v, "dense") ? 2u : 0u;
  // a --tail run selects at most S (N + 1) lines: up to 2^20 the line gather is the path (no tile-copy tables)
  else if (f->tail >= 0 && (uint64_t)p.nsegs * ((uint64_t)f->tail + 1) <= (1ull << 20)) p.compact_mode = 1;
  // one-pass compaction (no patterns, --tail -1): the fused scan compacts each wave's tile range in place
  s.fuse_ok = p.fuse_try = none && f->tail < 0 && p.compact_mode == 0 && p.k.fuse;
  for (const auto& d : p.segs) p.seg_end = std::max<uint64_t>(p.seg_end, d.base + d.len);
  p.evs = (f->flags & KLF_FILTER_NO_TIMING) ? nullptr : e->ev;
  p.full_index = (f->flags & KLF_FILTER_FULL_INDEX) != 0; s.win_ok = !p.full_index;
  p.lazy_index = none && f->tail < 0 && !p.full_index && p.k.lazy_index;  // lazy line index (grep none, --tail -1)
  // the output buffer: the input's size without --tail, else grown on demand (a --tail run never maps as much)
  if (f->tail < 0) p.out_need = std::max<uint64_t>(p.total_bytes, p.fuse_try ? p.seg_end : 0) + 64;
  else if (!e->d_out.p)  // a first --tail run: room for a typical tail window (no rerun to grow)
    p.out_need = std::min<uint64_t>(p.total_bytes + 64, p.k.out_init);
  p.need_hits = general && e->cs.qf_on; p.need_cand = p.need_hits && e->cs.rx_count;
  // bitmap hits: kHitSlots per tile in place; spills beyond 1 per 8 KiB of input -> k_match decides
  p.qhits_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(p.total_bytes / 8192, 1u << 16), e->hits_cap_max);
  // flattened hit slots: up to 1 per 4 KiB of input (2 per tile); more -> k_match decides
  p.hflat_cap = std::min<uint64_t>(std::max<uint64_t>(p.total_bytes / 4096, 1u << 20),
                                   (uint64_t)p.ntiles * klf::kHitSlots);
  p.count = (f->flags & KLF_FILTER_PATTERN_COUNTS) && general && e->cs.n_cids;
}
static int upload_layout(RunPlan& p) {  // unless the last run's segment table and tile map stand
  klf_engine* e = p.e;
  p.mark("pre-segs");
  if (!p.same_layout) {
    HIPCHK(e, e->d_segs.ensure(p.nsegs * sizeof(SegDesc)), "alloc segs");
    p.mark("segs alloc");
    // (a pageable source: staged before the call returns, so no stream sync is needed)
    HIPCHK(e, hipMemcpyAsync(e->d_segs.p, p.segs.data(), p.nsegs * sizeof(SegDesc), hipMemcpyHostToDevice, e->stream),
           "H2D segs");
    p.mark("segs copy");
    HIPCHK(e, e->d_tile_seg.ensure(p.ntiles * 4 + 16), "alloc tile_seg");  // + whole 16-B loads past the end
  }
  p.mark("segs");
  return KLF_OK;
}

// The first batch's sample, read back while the host maps the workspace: a prefiltered set's gram statistics
// (they place the needles' sampling windows, their newline share sizes the line arrays), else, but for a small
// batch, a newline count over 64 tiles -- no readback between the scan and the rest of the pipeline.
static int start_sample(RunPlan& p) {
  klf_engine* e = p.e;
  hipStream_t st = e->stream;
  if (p.mode == klf::CompiledSet::kGeneral && e->cs.qf_on && !e->cs.qf_tuned) {
    e->cs.qf_tuned = true; p.t_tune0 = Clock::now(); p.gram = p.k.qf_tune;
  }
  if (!p.gram && (e->line_density != 0.0 || p.small_first || p.k.two_phase)) return KLF_OK;
  if (!p.gram) p.nl_blocks = (uint32_t)std::min<uint64_t>(p.ntiles, 64);
  const size_t nb = p.gram ? klf::kGramHistWords * 4 : (size_t)p.nl_blocks * 8;
  HIPCHK(e, e->d_hist.ensure(nb), p.gram ? "alloc hist" : "alloc line sample");
  HIPCHK(e, e->h_hist.ensure(nb), p.gram ? "alloc hist readback" : "alloc line sample readback");
  if (p.gram)
    HIPCHK(e, klf::launch_gramhist(p.d_bytes, e->d_segs.as<SegDesc>(), p.nsegs, klf::kGramHistSample, e->cs.qf_fold,
                                   e->d_hist.as<uint32_t>(), st), "gram histogram");
  else
    HIPCHK(e, klf::launch_nlsample(p.d_bytes, e->d_segs.as<SegDesc>(), p.nsegs, (uint32_t)p.ntiles, p.nl_blocks,
                                   e->d_hist.as<uint32_t>(), st), "line sample");
  HIPCHK(e, hipMemcpyAsync(e->h_hist.p, e->d_hist.p, nb, hipMemcpyDeviceToHost, st), p.gram ? "D2H hist" : "D2H line sample");
  return KLF_OK;
}
// Waits for the sample; `est`: its lines per byte.  The gram form also lays out and uploads the prefilter.
static int finish_sample(RunPlan& p, double& est) {
  klf_engine* e = p.e;
  if (!p.gram && !p.nl_blocks) return KLF_OK;
  HIPCHK(e, hipStreamSynchronize(e->stream), p.gram ? "sync hist" : "sync line sample");
  const uint32_t* hv = e->h_hist.as<uint32_t>();
  if (!p.gram) {
    uint64_t nl = 0, nb = 0;
    for (uint32_t b = 0; b < p.nl_blocks; ++b) { nl += hv[2 * b]; nb += hv[2 * b + 1]; }
    if (nb) est = (double)(nl + p.nl_blocks) / (double)nb;  // (+1 per tile: a margin, never 0)
    if (p.k.nl_scale) est *= atof(p.k.nl_scale);
    p.mark("line sample");
    return KLF_OK;
  }
  const auto t_hist = Clock::now();
  klf::DataStats ds;
  ds.bytes.assign(256, 0);
  for (int c = 0; c < 256; ++c) { ds.bytes[c] = hv[c]; ds.nbytes += hv[c]; }
  ds.pair.assign(hv + klf::kGramHistPairs, hv + klf::kGramHistPairs + 65536);
  for (auto& c : ds.pair) c *= 2;  // counted at every 2nd position
  klf::stats_finish(ds);
  if (ds.nbytes) est = (double)(ds.bytes['\n'] + 1) / (double)ds.nbytes;
  klf::place_needles(e->cs, &ds);
  const auto t_place = Clock::now();
  if (p.k.diag)
    fprintf(stderr, "[klf] prefilter layout from %llu sampled bytes: %s\n", (unsigned long long)ds.nbytes,
            e->cs.qf_layout.c_str());
  HIPCHK(e, upload_prefilter(e), "upload prefilter tables");
  if (p.k.diag)
    fprintf(stderr, "[klf] first-batch tuning: statistics %.1f us (with the workspace mapped meanwhile), layout %.1f us, uploads %.1f us\n",
            std::chrono::duration<double, std::micro>(t_hist - p.t_tune0).count(),
            std::chrono::duration<double, std::micro>(t_place - t_hist).count(),
            std::chrono::duration<double, std::micro>(Clock::now() - t_place).count());
  p.tune_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - p.t_tune0).count();
  p.mark("first-batch tuning");
  return KLF_OK;
}
// what the sample's line density decides: a first run's line capacity (x2 + a margin) and the slot storage
static void plan_density(RunPlan& p, RunState& s, double est) {
  klf_engine* e = p.e;
  p.density_cap = e->line_density == 0.0 && est > 0.0 && !p.k.two_phase;
  // slots of tiles with two or more line starts: lines over 1 KiB -> per-wave pool chunks, else per-tile records
  const double dens = e->line_density > 0.0 ? e->line_density : est;
  p.wave_pool = p.k.wave_pool ? strcmp(p.k.wave_pool, "0") != 0 : (dens > 0.0 && dens * 1024.0 < 1.0);
  if (p.density_cap) s.cap = std::min<uint64_t>(s.cap, (uint64_t)(est * (double)p.total_bytes * 2.0) + 2ull * p.nsegs + 65536);
}
// the one-pass ranges (n x kScanGroup tiles, one per wave of a full launch) and each one's first extent
static int fuse_ranges(RunPlan& p) {
  klf_engine* e = p.e;
  const uint64_t waves = (uint64_t)std::max(1, klf::fuse_waves(e->num_cus));
  uint64_t R = (p.ntiles + waves - 1) / waves;
  R = (R + klf::kScanGroup - 1) / klf::kScanGroup * klf::kScanGroup;
  if (p.k.fuse_range) R = std::max<uint64_t>(klf::kScanGroup, (uint64_t)atol(p.k.fuse_range) / klf::kScanGroup * klf::kScanGroup);
  const uint32_t nr = (uint32_t)((p.ntiles + R - 1) / R);
  const bool same_fuse_layout = p.segs.size() == e->fuse_segs.size() &&
                                memcmp(p.segs.data(), e->fuse_segs.data(), p.segs.size() * sizeof(SegDesc)) == 0;
  if (!same_fuse_layout || e->fuse_range != (uint32_t)R || e->fuse_nranges != nr) {
    e->fuse_segs.clear(); e->fuse_ext0.assign(nr + 1, 0);  // (fuse_segs: invalid until the table is on its way)
    for (uint32_t q = 0; q < nr; ++q) {
      const uint64_t t0 = (uint64_t)q * R, t1 = std::min<uint64_t>(t0 + R, p.ntiles) - 1;
      e->fuse_ext0[q + 1] = e->fuse_ext0[q] + (seg_of_tile(p.segs, t1) - seg_of_tile(p.segs, t0) + 1);
    }
    HIPCHK(e, e->d_fext0.ensure((nr + 1) * 4), "alloc fuse ranges");
    HIPCHK(e, hipMemcpyAsync(e->d_fext0.p, e->fuse_ext0.data(), (nr + 1) * 4, hipMemcpyHostToDevice, e->stream),
           "H2D fuse ranges");
    e->fuse_range = (uint32_t)R; e->fuse_nranges = nr; e->fuse_next = e->fuse_ext0[nr];
    e->fuse_segs = p.segs;
  }
  HIPCHK(e, e->d_fext.ensure((size_t)e->fuse_next * 16), "alloc fuse extents");
  HIPCHK(e, e->d_frinfo.ensure((size_t)e->fuse_nranges * 32), "alloc fuse range states");
  return KLF_OK;
}
static int map_workspace(RunPlan& p) {  // what the layout alone sizes, as one allocation
  klf_engine* e = p.e;
  const uint64_t ntiles = p.ntiles;
  BufList ws = {{&e->d_tstat, ntiles * sizeof(klf::TileStat)},
                {&e->d_tile_base, ntiles * 8}, {&e->d_bsum, (ntiles / 1024 + 2) * 4 * 8},
                {&e->d_counters, kCtrBytes + p.nsegs * sizeof(SegOut)} /* + the stream records */,
                {&e->d_wpre, (3 * (size_t)p.nsegs + 2) * 8} /* + wgrp */};
  if (p.want_truns) ws.push_back({&e->d_truns, ntiles * klf::kRunSlots * 4});
  if (p.compact_mode != 1) ws.insert(ws.end(), {{&e->d_trec, ntiles * sizeof(klf::TRec)}, {&e->d_kbase, ntiles * 16}});
  if (p.need_cand) ws.push_back({&e->d_cand, (size_t)e->cand_cap * 16});
  if (p.need_hits)
    ws.insert(ws.end(), {{&e->d_qhits, (size_t)p.qhits_cap * 8}, {&e->d_hslots, (size_t)ntiles * klf::kHitSlots * 2},
                         {&e->d_hflat, (size_t)p.hflat_cap * 8}});
  HIPCHK(e, ensure_all(e->d_block, e->block_users, ws), "alloc workspace");
  p.mark("workspace");
  return KLF_OK;
}
// the buffers indexed by global line, and the compaction's `mcb` blocks and `cmc` copy chunks, for capacity c
static BufList line_sizes(const RunPlan& p, uint64_t c, uint64_t& mcb, uint64_t& cmc) {
  klf_engine* e = p.e;
  mcb = c / klf::kCompactLines + 2;
  // >= sum over blocks of ceil(bytes / chunk): within kCopyChunksTarget chunks unless the chunk is kCopyChunk
  cmc = mcb + std::max<uint64_t>(p.total_bytes / klf::kCopyChunk, klf::kCopyChunksTarget) + 2;
  return {{&e->d_line_off, (c + p.nsegs + 1) * 8}, {&e->d_meta, c * 2 + 16}, {&e->d_bits, (c / 32 + 1) * 4},
          {&e->d_cstatus, (mcb + 1) * 3 * 8}, {&e->d_cmap, cmc * 4}, {&e->d_cseg, (mcb + 1) * 4},
          {&e->d_mpart, (c / klf::kMatchChunk + 2) * 8}};
}
static hipError_t alloc_lines(const RunPlan& p, klf::RunArgs& x, uint64_t c) {
  klf_engine* e = p.e;
  uint64_t mcb, cmc;
  for (auto& q : line_sizes(p, c, mcb, cmc))
    if (const hipError_t h = q.first->ensure(q.second); h != hipSuccess) return h;
  x.line_off = e->d_line_off.as<uint64_t>(); x.meta = e->d_meta.as<uint16_t>(); x.bits = e->d_bits.as<uint32_t>();
  x.csum = e->d_cstatus.as<uint64_t>(); x.cmap = e->d_cmap.as<uint32_t>(); x.cseg = e->d_cseg.as<uint32_t>();
  x.mpart = e->d_mpart.as<uint64_t>(); x.cap_lines = c; x.max_cblocks = (uint32_t)mcb; x.cmap_cap = cmc;
  return hipSuccess;
}
// the slot pool: every tile where two or more lines start (16-B aligned: <= 3 spare slots each),
// dense tiles, and the waves' partly used last chunks; an overflow reruns with what the scan reserved
static uint64_t pool_need(const RunPlan& p, uint64_t c, uint32_t& chunk) {
  chunk = 256;
  if (!p.wave_pool) return p.e->pool_cap;
  const uint64_t nwaves = (uint64_t)p.e->num_cus * 16;
  const uint64_t per_wave = (c + 2 * p.ntiles) / nwaves;
  while (chunk < 4096 && chunk * 4 < per_wave) chunk *= 2;
  return std::max<uint64_t>(p.e->pool_cap, c + 3 * p.ntiles + nwaves * chunk + 1024);
}
// a first run's line arrays, slot pool / records and output buffer as one more allocation
static int map_lines(RunPlan& p, const RunState& s) {
  klf_engine* e = p.e;
  BufList ws2;
  if (p.out_need) ws2.push_back({&e->d_out, p.out_need});
  if (!p.wave_pool) ws2.push_back({&e->d_slots, p.ntiles * klf::kRecStride * 4});
  if (e->line_density == 0.0) {
    uint64_t mcb, cmc;
    uint32_t ch = 0;
    for (auto& x : line_sizes(p, s.cap, mcb, cmc)) ws2.push_back(x);
    ws2.push_back({&e->d_pool, pool_need(p, s.cap, ch) * 4});
  }
  HIPCHK(e, ensure_all(e->d_block2, e->block2_users, ws2), "alloc line arrays / output");
  p.mark("line arrays / output");
  return KLF_OK;
}

// Every RunArgs field but the line arrays (alloc_lines); launch_graph keys on the bytes: zeroed, then filled.
static void fill_args(const RunPlan& p, const RunState& s, int attempt, klf::RunArgs& a) {
  klf_engine* e = p.e;
  const klf_filter* f = p.f;
  const RunKnobs& k = p.k;
  const bool general = p.mode == klf::CompiledSet::kGeneral, none = p.mode == klf::CompiledSet::kNone;
  memset(static_cast<void*>(&a), 0, sizeof(a));
  // the batch and its tile index
  a.bytes = p.d_bytes; a.segs = e->d_segs.as<SegDesc>(); a.nsegs = p.nsegs; a.ntiles = (uint32_t)p.ntiles;
  a.tile_seg = e->d_tile_seg.as<uint32_t>();
  a.build_tiles = (!p.same_layout && attempt == 0) ? 1u : 0u;
  a.tindex_wide = (p.ntiles > klf::kScanSmallTiles || k.tindex_wide) ? 1u : 0u;
  // the filter
  a.since_sec = f->since.sec; a.since_nsec = f->since.nsec; a.tail = f->tail;
  since_digits(f->since.sec, f->since.nsec, a.since_dig);
  a.grep_mode = (uint32_t)p.mode; a.match_all = e->cs.also_all ? 1u : 0u;
  a.lit = e->d_lit.as<uint8_t>(); a.lit_words = e->d_lit.as<uint32_t>(); a.lit_len = (uint32_t)e->cs.literal.size();
  a.lit_anchor = e->cs.literal_anchor;
  a.lit_anchor_byte = e->cs.literal.empty() ? 0u : e->cs.literal[e->cs.literal_anchor];
  a.qf_mul = e->cs.qf_mul;
  memcpy(static_cast<void*>(&a.pats), &e->dpats, sizeof(a.pats));
  // the workspace
  a.tstat = e->d_tstat.as<klf::TileStat>(); a.tile_base = e->d_tile_base.as<uint64_t>(); a.bsum = e->d_bsum.as<uint64_t>();
  a.slots = p.wave_pool ? nullptr : e->d_slots.as<uint32_t>(); a.wave_pool = p.wave_pool ? 1u : 0u;
  a.pool = e->d_pool.as<uint32_t>(); a.pool_cap = e->pool_cap; a.pool_chunk = s.pool_chunk;
  a.counters = e->d_counters.as<uint32_t>(); a.segout = segout_of(e);
  a.wpre = e->d_wpre.as<uint64_t>(); a.wgrp = a.wpre + p.nsegs + 1;
  a.out = e->d_out.as<uint8_t>(); a.out_cap = e->d_out.p ? e->d_out.cap : 0;
  a.stage_times = (f->flags & KLF_FILTER_STAGE_TIMES) && p.evs ? 1u : 0u;
  if (p.need_cand) { a.cand = e->d_cand.as<uint64_t>(); a.cand_cap = e->cand_cap; }
  if (p.need_hits) {
    a.qhits = e->d_qhits.as<uint64_t>(); a.qhits_cap = p.qhits_cap; a.hslots = e->d_hslots.as<uint16_t>();
    a.hflat = e->d_hflat.as<uint64_t>(); a.hflat_cap = p.hflat_cap;
  }
  a.trec = e->d_trec.as<klf::TRec>(); a.kbase = e->d_kbase.as<uint64_t>();
  a.truns = p.want_truns ? e->d_truns.as<uint32_t>() : nullptr;
  a.compact_mode = p.compact_mode; a.lazy_index = p.lazy_index ? 1u : 0u;
  a.plan_runs = (p.lazy_index && p.want_truns && p.compact_mode != 1 && k.plan_runs && !s.fuse_ok) ? 1u : 0u;
  // windowed line index: literal patterns, and prefiltered regex sets, whose candidate lines get their bounds from
  // k_verify; per-pattern counts too (k_fixcount's deferred lines, like k_match's fallback, ask for the whole index)
  a.win_index = (s.win_ok &&
                 (p.mode == klf::CompiledSet::kLiteral1 ||
                  (general && e->cs.qf_on && !e->cs.also_all && ((e->cs.rx_count == 0 && !p.count) || k.win_index_rx))) &&
                 k.win_index) ? 1u : 0u;
  // no launch of kernels that would exit at once: k_match beside a working prefilter, k_tcopy before any run went dense
  a.skip_match = (general && e->cs.qf_on && !e->cs.also_all && !s.force_match && k.skip_idle) ? 1u : 0u;
  a.skip_tcopy = (f->tail >= 0 && !e->dense_tail_seen && p.compact_mode == 0 && k.skip_idle) ? 1u : 0u;
  a.scatter_split = k.scatter_split;
  // a --tail run's sparse gather without patterns: k_tailw plans a window of <= 4 compaction blocks itself (2), else
  // k_cplan's last block runs the prefix (1); a grep run's window needs k_cplan's whole grid (0)
  if (p.compact_mode == 1 && f->tail >= 0 && (none || k.plan_mode)) {
    const bool index_first = !a.win_index && !p.lazy_index;
    a.plan_mode = index_first && none &&
                  (uint64_t)p.nsegs * ((uint64_t)f->tail + 1) <= 4ull * klf::kCompactLines ? 2u : 1u;
    if (k.plan_mode) a.plan_mode = std::min<uint32_t>((uint32_t)atoi(k.plan_mode), index_first ? 2u : 1u);
  }
  if (p.count) { a.count_pats = 1; a.pcount = e->d_pcount.as<uint32_t>(); a.pairs = e->d_pairs.as<uint64_t>(); }
  a.pairs_log2 = e->pairs_log2;
  if (s.fuse_ok) {
    a.fuse = 1; a.fuse_range = e->fuse_range; a.fuse_nranges = e->fuse_nranges;
    a.fuse_ext0 = e->d_fext0.as<uint32_t>(); a.fuse_ext = e->d_fext.as<uint64_t>(); a.fuse_rinfo = e->d_frinfo.as<uint64_t>();
  }
}
static int join_ac(RunPlan& p, klf::RunArgs& a) {  // the literal automaton (klf_open's thread) is read from k_tindex on
  if (const int rc = ensure_ac(p.e); rc != KLF_OK) return rc;
  memcpy(static_cast<void*>(&a.pats), &p.e->dpats, sizeof(a.pats));
  p.mark("automaton");
  return KLF_OK;
}

// One attempt: pool, arguments, launch in its shape, readback; a two-phase run may end at its first readback (phase1).
static int launch_attempt(RunPlan& p, RunState& s, klf_result* r, int attempt, Attempt& at) {
  klf_engine* e = p.e;
  hipStream_t st = e->stream;
  klf::RunArgs& a = at.a;
  if (p.count) {
    HIPCHK(e, e->d_pcount.ensure((size_t)p.nsegs * e->cs.n_cids * 4), "alloc pcount");
    HIPCHK(e, e->d_pairs.ensure((size_t)8 << e->pairs_log2), "alloc pairs");
    HIPCHK(e, hipMemsetAsync(e->d_pcount.p, 0, (size_t)p.nsegs * e->cs.n_cids * 4, st), "zero pcount");
    HIPCHK(e, hipMemsetAsync(e->d_pairs.p, 0, (size_t)8 << e->pairs_log2, st), "zero pairs");
  }
  const bool two_phase = attempt == 0 && e->line_density == 0.0 && !p.density_cap && !p.small_first && !p.k.one_phase;
  e->pool_cap = pool_need(p, s.cap, s.pool_chunk);
  if (e->pool_cap >= (1ull << 31)) return set_err(e, KLF_EINVAL, "batch too large (line slot pool)");
  HIPCHK(e, e->d_pool.ensure(e->pool_cap * 4), "alloc pool");
  fill_args(p, s, attempt, a);
  if (attempt == 0 && p.k.pool_cap) a.pool_cap = std::min<uint64_t>(a.pool_cap, p.k.pool_cap);
  at.shape = two_phase ? "two-phase" : e->ac_pending ? "ac-split" : "plain";
  at.ev_mask = 0; at.phase1 = at.tcopy = at.grown = false;
  at.skip_tcopy = a.skip_tcopy; at.plan_mode = a.plan_mode; at.plan_runs = a.plan_runs;
  r->so.resize(p.nsegs);
  // (+ a one-pass run's extents, read back with the counters: one sync on e->stream)
  const size_t rb_ext = a.fuse ? (size_t)e->fuse_next * 16 : 0;
  HIPCHK(e, e->h_rb.ensure(kCtrBytes + p.nsegs * sizeof(SegOut) + rb_ext), "alloc readback");
  const char* what = "sync phase 1";
  if (two_phase) {
    if (const int rc = join_ac(p, a); rc != KLF_OK) return rc;
    a.cap_lines = 1ull << 40;  // phase 1 indexes no line array (k_tindex: no overflow, no bitmap)
    HIPCHK(e, klf::launch_pipeline(a, st, p.evs, e->num_cus, 1, &at.ev_mask), "launch");
    HIPCHK(e, read_back(e, p.nsegs, 0, 0, at.counters, r->so.data(), &what), what);
    p.mark("phase 1 (launch + sync)");
    if ((at.phase1 = at.counters[2] != 0)) return KLF_OK;  // the dense-tile pool overflowed: a whole rerun
    learn_density(e, r->so, p.total_bytes);  // (the margin later runs size by, so that they fit)
    // the arrays from phase 1's exact line count; a capacity clamped below it fails here, before phase 2 indexes them
    const uint64_t need = r->so[p.nsegs - 1].line_hi + 2;
    s.cap = std::min<uint64_t>(std::max<uint64_t>(std::min<uint64_t>(s.cap, learned_cap(p)), need), p.k.cap_clamp);
    if ((at.phase1 = need > s.cap)) return KLF_OK;
    HIPCHK(e, alloc_lines(p, a, s.cap), "alloc line arrays");
    p.mark("line arrays");
    if (a.grep_mode != klf::CompiledSet::kNone)  // (phase 1's k_tindex zeroes it otherwise)
      HIPCHK(e, hipMemsetAsync(a.bits, 0, (s.cap / 32 + 1) * 4, st), "zero bits");
    HIPCHK(e, klf::launch_pipeline(a, st, p.evs, e->num_cus, 2, &at.ev_mask), "launch");
    p.mark("phase 2 launched");
  } else if (e->ac_pending) {  // joined while the scan runs
    HIPCHK(e, alloc_lines(p, a, s.cap), "alloc line arrays");
    HIPCHK(e, klf::launch_pipeline(a, st, p.evs, e->num_cus, 3, &at.ev_mask), "launch");
    if (const int rc = join_ac(p, a); rc != KLF_OK) return rc;
    HIPCHK(e, klf::launch_pipeline(a, st, p.evs, e->num_cus, 4, &at.ev_mask), "launch");
  } else {
    HIPCHK(e, alloc_lines(p, a, s.cap), "alloc line arrays");
    p.mark("line arrays");
    // KLF_GRAPH=1: a small batch (KLF_GRAPH_MAX_MB, default 256) replays a graph
    const bool graph = !e->graph_off && !a.stage_times && p.total_bytes <= p.k.graph_max && p.k.graph;
    if (graph && launch_graph(e, a, at.ev_mask, p.k.diag)) at.shape = "graph";
    else HIPCHK(e, klf::launch_pipeline(a, st, p.evs, e->num_cus, 0, &at.ev_mask), "launch");
  }
  p.mark("launched");
  what = "sync";
  HIPCHK(e, read_back(e, p.nsegs, rb_ext, 1000 + p.total_bytes / 2000000, at.counters, r->so.data(), &what), what);
  p.mark("pipeline done");
  e->last_segs = p.segs;
  if (p.k.diag)
    fprintf(stderr, "[klf] hits=%u spilled=%u hits_over=%u nfa_queue=%u queue_over=%u deferred=%u\n",
            at.counters[klf::kCtrVerified], at.counters[klf::kCtrHits], at.counters[klf::kCtrHitsOver],
            at.counters[klf::kCtrQueue], at.counters[klf::kCtrQOver], at.counters[5]);
  return KLF_OK;
}
static Outcome judge(const Attempt& at) {  // what a finished attempt asks for, from its counters, in this order
  const klf::RunArgs& a = at.a; const uint32_t* c = at.counters;
  if (at.phase1 || (c[2] & 1u)) return kLines;
  if (a.skip_match && (c[klf::kCtrQOver] || c[klf::kCtrHitsOver])) return kMatch;
  if (a.fuse && c[klf::kCtrFuseBad]) return kFuse;
  if (a.win_index && c[klf::kCtrRedo]) return kIndex;
  if (a.count_pats && c[klf::kCtrPairsOver]) return kPairs;
  return kDone;
}
// changes the state as outcome `o` asks and says what follows the attempt
static Next apply_outcome(const RunPlan& p, RunState& s, Outcome o, const Attempt& at, const std::vector<SegOut>& so) {
  klf_engine* e = p.e; const uint32_t* c = at.counters;
  const uint64_t need = so.back().line_hi + 2;  // (kLines: the exact line count)
  switch (o) {
    case kDone: return kStand;
    case kLines:  // fails if the exact rerun overflowed too (phase 1's is not counted) or phase 1 met a clamped cap
      if (at.phase1 ? !c[2] : s.line_reruns++ > 0) return kFail;
      bump_pool(e, c);
      if (at.phase1) learn_density(e, so, p.total_bytes);
      s.cap = at.phase1 ? std::min<uint64_t>(s.cap, need) : std::min(std::max<uint64_t>(s.cap, need), p.k.cap_clamp);
      return kRedo;
    case kMatch: s.force_match = true; return kRedo;  // redo with k_match
    case kFuse: s.fuse_ok = false; return kRedo;      // the two-pass rerun
    case kIndex: s.win_ok = false; return kRedo;      // rerun with the whole index
    case kPairs: {  // a larger set, twice at most: else the result stands without per-pattern counts
      if (s.pair_reruns >= 2 || e->pairs_log2 >= 28) return kStand;
      ++s.pair_reruns;  // distinct pairs <= the set's capacity + the failed inserts; size for load <= 1/2
      const uint64_t pairs = 2 * (((uint64_t)1 << e->pairs_log2) + c[klf::kCtrPairsOver]);
      uint32_t lg = e->pairs_log2 + 1;
      while (lg < 28 && ((uint64_t)1 << lg) < pairs) ++lg;
      e->pairs_log2 = lg; return kRedo;
    }
  }
  return kFail;
}
static int deferred_tcopy(RunPlan& p, Attempt& at) {  // the dense path without its copy (skip_tcopy): launch it now
  klf_engine* e = p.e;
  if (!(at.a.skip_tcopy && at.counters[klf::kCtrDense])) return KLF_OK;
  uint32_t* rb1 = e->h_rb.as<uint32_t>();
  HIPCHK(e, klf::launch_tcopy(at.a, e->stream, nullptr, e->num_cus, nullptr), "launch tile copy");
  HIPCHK(e, hipMemcpyAsync(rb1, e->d_counters.p, sizeof(at.counters), hipMemcpyDeviceToHost, e->stream), "D2H counters");
  HIPCHK(e, hipStreamSynchronize(e->stream), "sync tile copy");
  at.counters[klf::kCtrOutShort] = rb1[klf::kCtrOutShort];
  at.a.skip_tcopy = 0; at.tcopy = true;  // (klf_retail from this run launches it)
  return KLF_OK;
}
// a one-pass run's extents, in stream order (ranges ascend, and so do a range's streams)
static void fused_extents(const RunPlan& p, klf_result* r) {
  klf_engine* e = p.e; const uint32_t nsegs = p.nsegs;
  r->fused = true;
  r->fx.resize((size_t)e->fuse_next * 2);
  memcpy(r->fx.data(), e->h_rb.as<uint8_t>() + kCtrBytes + nsegs * sizeof(SegOut), (size_t)e->fuse_next * 16);
  r->fx_first.assign(nsegs + 1, e->fuse_next);
  for (uint32_t q = e->fuse_nranges; q-- > 0;) {
    const uint32_t s0 = seg_of_tile(p.segs, (uint64_t)q * e->fuse_range);
    for (uint32_t k = e->fuse_ext0[q]; k < e->fuse_ext0[q + 1]; ++k) r->fx_first[s0 + (k - e->fuse_ext0[q])] = k;
  }
  uint64_t acc = 0;
  for (uint32_t sg = 0; sg < nsegs; ++sg) {
    r->so[sg].sel_lo = 0; r->so[sg].sel_hi = r->so[sg].since_ok;  // (every parsed line since the cutoff)
    r->so[sg].out_lo = acc;
    for (uint32_t k = r->fx_first[sg]; k < r->fx_first[sg + 1]; ++k) acc += r->fx[2 * (size_t)k + 1];
    r->so[sg].out_hi = acc;
  }
}
// the attempt that stands: its output (grown when short), and what the engine remembers of it
static int publish(RunPlan& p, Attempt& at, klf_result* r) {
  klf_engine* e = p.e; klf::RunArgs& a = at.a; const uint32_t* c = at.counters;
  if (c[klf::kCtrOutShort]) {  // the output did not fit: grow, rerun the tail stage
    HIPCHK(e, grow_out_retail(e, a, r->so), "grow output");
    at.grown = true;
    if (p.k.diag) fprintf(stderr, "[klf] output buffer grown to %zu B\n", e->d_out.cap);
  }
  if (a.fuse) fused_extents(p, r);
  e->last_args = a;
  const bool on_demand = a.lazy_index && (c[klf::kCtrDense] || a.fuse);
  if (on_demand || a.win_index) e->index_pending.push_back(a);
  r->index_mode = on_demand ? KLF_INDEX_ON_DEMAND : a.win_index ? KLF_INDEX_WINDOWS : KLF_INDEX_FULL;
  r->compaction = a.fuse ? KLF_COMPACT_ONEPASS : c[klf::kCtrDense] ? KLF_COMPACT_TILES : KLF_COMPACT_GATHER;
  e->last_gen = r->gen;
  learn_density(e, r->so, p.total_bytes);
  if (p.f->tail >= 0 && c[klf::kCtrDense]) e->dense_tail_seen = true;
  return KLF_OK;
}
static void diag_attempt(int attempt, const Attempt& at, const char* outcome) {  // only values two processes share
  const klf::RunArgs& a = at.a;
  fprintf(stderr, "[klf] attempt %d %s grep_mode=%u tail=%lld cap_lines=%llu fuse=%u lazy_index=%u win_index=%u "
          "compact_mode=%u plan_mode=%u plan_runs=%u skip_match=%u skip_tcopy=%u wave_pool=%u pool_chunk=%u "
          "count_pats=%u build_tiles=%u -> %s%s%s\n", attempt, at.shape, a.grep_mode, (long long)a.tail,
          (unsigned long long)a.cap_lines, a.fuse, a.lazy_index, a.win_index, a.compact_mode, at.plan_mode, at.plan_runs,
          a.skip_match, at.skip_tcopy, a.wave_pool, a.pool_chunk, a.count_pats, a.build_tiles, outcome,
          at.tcopy ? " +tcopy" : "", at.grown ? " +grown" : "");
}
// Only the event pairs this run recorded (ev_mask): another would fail the query or time an earlier run.
// Timing is diagnostic: a recorded pair that fails to read leaves -1 in its slot and the result stands.
static void query_timing(const RunPlan& p, klf_result* r, uint32_t ev_mask) {
  klf_engine* e = p.e;
  auto elapsed = [&](int k0, int k1, int slot) {
    if (!((ev_mask >> k0 & 1u) && (ev_mask >> k1 & 1u))) return;
    float ms = 0.f;
    const hipError_t h = hipEventElapsedTime(&ms, e->ev[k0], e->ev[k1]);
    r->ms[slot] = h == hipSuccess ? ms : -1.0;
    if (h == hipSuccess) return;
    (void)hipGetLastError();  // (the failed query's error is not the next call's)
    if (p.k.diag) fprintf(stderr, "[klf] timing events %d/%d unreadable: %s\n", k0, k1, hipGetErrorString(h));
  };
  static const int kPairs[6][3] = {{1, 2, 0}, {2, 3, 1}, {3, 4, 2}, {4, 5, 3}, {0, 5, 4}, {0, 1, 5}};
  const auto t_q0 = Clock::now();
  for (const auto& q : kPairs) elapsed(q[0], q[1], q[2]);
  elapsed(7, 8, 6);   // k_scan's dispatch alone
  elapsed(9, 10, 7);  // k_tcopy's dispatch alone (dense copy)
  if (p.k.diag)
    fprintf(stderr, "[klf] timing queries %.1f us\n", std::chrono::duration<double, std::micro>(Clock::now() - t_q0).count());
  r->ev_mask = ev_mask;
}
static void diag_summary(const RunPlan& p) {
  const double us = std::chrono::duration<double, std::micro>(Clock::now() - p.t_run0).count();
  fprintf(stderr, "[klf] run %.1f us: allocations %.1f us, first-batch tuning %.1f us\n", us,
          (g_alloc_ns.load() - p.alloc0) / 1e3, p.tune_ns / 1e3);
  std::string m = "[klf] run marks (us):";
  auto prev = p.t_run0;
  for (auto& x : p.marks) {
    m += std::string(" ") + x.first + " " + std::to_string((int)std::chrono::duration<double, std::micro>(x.second - prev).count()) + ";";
    prev = x.second;
  }
  fprintf(stderr, "%s\n", m.c_str());
}

static int run_device_impl(klf_engine* e, const uint8_t* d_bytes, uint32_t n_streams, const uint64_t* seg_base,
                           const uint64_t* lens, const klf_filter* f, klf_result** out) {
  if (!e || !f || !out || (n_streams && (!seg_base || !lens))) return KLF_EINVAL;
  if (f->tail < -1) return set_err(e, KLF_EINVAL, "tail must be >= -1");
  if (f->since.nsec < 0 || f->since.nsec >= 1000000000) return set_err(e, KLF_EINVAL, "since.nsec out of range");
  if (reinterpret_cast<uintptr_t>(d_bytes) % 16) return set_err(e, KLF_EINVAL, "device bytes must be 16-B aligned");
  *out = nullptr;
  RunPlan p{e, f, d_bytes, read_knobs()};
  RunState s;
  HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
  std::unique_ptr<klf_result> rp(new (std::nothrow) klf_result());  // freed on every error return
  klf_result* r = rp.get();
  if (!r) return KLF_ENOMEM;
  r->e = e; r->gen = ++e->gen; r->n_streams = n_streams;
  r->seg_of.assign(n_streams, -1);
  // an earlier one-pass result's contiguous copy (klf_result_device_out) is stale from here on, like that result
  if (e->d_out2.p) e->d_out2.release();
  int rc;
  if (e->cs.also_all_pending && (f->flags & KLF_FILTER_PATTERN_COUNTS) && (rc = compile_pending(e)) != KLF_OK) return rc;
  p.mode = e->cs.mode;
  // a set with an always-pattern filters as kAll; its other patterns are evaluated only for per-pattern counts
  if (e->cs.also_all && !(f->flags & KLF_FILTER_PATTERN_COUNTS)) p.mode = klf::CompiledSet::kAll;
  r->has_bits = p.mode != klf::CompiledSet::kNone;
  if ((rc = layout_segments(p, s, r, n_streams, seg_base, lens)) != KLF_OK) return rc;
  // asked-for per-pattern counts are reported even when every stream is empty (all zero)
  r->counted = (f->flags & KLF_FILTER_PATTERN_COUNTS) != 0;
  r->pcount_ok = true;  // no segment reads pcount
  if (p.nsegs == 0) { e->last_gen = r->gen; *out = rp.release(); return KLF_OK; }
  r->pcount_ok = false;
  plan_run(p, s);
  double est_density = 0.0;
  if ((rc = upload_layout(p)) != KLF_OK) return rc;
  if ((rc = start_sample(p)) != KLF_OK) return rc;  // (its readback is in flight while the workspace is mapped)
  if (p.fuse_try && (rc = fuse_ranges(p)) != KLF_OK) return rc;
  e->index_pending.clear();
  if ((rc = map_workspace(p)) != KLF_OK) return rc;
  if ((rc = finish_sample(p, est_density)) != KLF_OK) return rc;
  plan_density(p, s, est_density);
  if ((rc = map_lines(p, s)) != KLF_OK) return rc;
  // each attempt launches the whole run and reads its counters back; apply_outcome changes the state for a redo
  Attempt at;
  Outcome o = kDone;
  Next next = kRedo;
  for (int attempt = 0; attempt < 4 && next == kRedo; ++attempt) {
    if ((rc = launch_attempt(p, s, r, attempt, at)) != KLF_OK) return rc;
    o = judge(at);
    if (o != kLines && o != kMatch && (rc = deferred_tcopy(p, at)) != KLF_OK) return rc;
    next = apply_outcome(p, s, o, at, r->so);
    if (next == kStand && (rc = publish(p, at, r)) != KLF_OK) return rc;
    if (p.k.diag) diag_attempt(attempt, at, kOutcomeName[next == kStand ? kDone : o]);
  }
  if (p.count && next == kStand && o != kPairs) {
    r->pcount.resize((size_t)p.nsegs * e->cs.n_cids);
    HIPCHK(e, hipMemcpy(r->pcount.data(), e->d_pcount.p, r->pcount.size() * 4, hipMemcpyDeviceToHost), "D2H pcount");
    r->pcount_ok = true;
  }
  if (p.k.diag) diag_summary(p);
  if (next == kFail)  // never hand out the aborted run's records
    return set_err(e, KLF_ENOMEM, "line index / dense-tile pool overflow after the exact rerun");
  if (next == kRedo)  // every attempt asked for another
    return set_err(e, KLF_ENOMEM, std::string("run not finished after 4 attempts (the last asked for a redo: ") +
                                      kOutcomeName[o] + ")");
  if (p.k.timeline_out) {  // diagnostic builds only
    std::vector<uint64_t> tl(300000 * 8);
    if (klf::dump_timeline(tl.data(), tl.size() * 8) == hipSuccess) {
      FILE* fp = fopen(p.k.timeline_out, "wb");
      if (fp) { fwrite(tl.data(), 8, std::min<size_t>(tl.size(), p.ntiles * 8), fp); fclose(fp); }
      (void)klf::clear_timeline();
    }
  }
  query_timing(p, r, at.ev_mask);
  r->total_lines = r->so[p.nsegs - 1].line_hi;
  for (auto& so : r->so) r->total_out = std::max(r->total_out, so.out_hi);
  *out = rp.release();
  return KLF_OK;
}

extern "C" int klf_run_device(klf_engine* e, const uint8_t* d_bytes, uint32_t n, const uint64_t* seg_base,
                              const uint64_t* lens, const klf_filter* f, klf_result** out) {
  return run_device_impl(e, d_bytes, n, seg_base, lens, f, out);
}

// klf_retail (o null: over the bitmap the latest result was selected from), klf_regroup
// (o: over G', built first from the run's match bitmap in d_bits) and klf_window (o and tw:
// G' only when o asks for context or inversion, then cut by the time window when a bound is
// closed or the engine has no patterns; always from M).  klf_around (ar, with tw holding its
// bounds and no context): G' from the anchors' time intervals (around_build), then the same cut.
// klf_records (rc, with tw holding its bounds): G' from the records' heads (records_build), then
// the same cut.
static bool window_closed(const klf_window_opts* tw) {
  return tw->from.sec != KLF_TIME_MIN_SEC || tw->until.sec != KLF_TIME_MAX_SEC;
}
int klf_impl::check_latest(klf_engine* e, const klf_result* r, const char* what) {
  if (r->gen != e->gen || e->last_gen != r->gen) return set_err(e, KLF_ESTATE, std::string(what) + ": not the latest run");
  return KLF_OK;
}
const uint32_t* klf_impl::sel_bits(const klf_result* r) {
  return r->grouped ? r->e->d_gbits.as<uint32_t>() : r->has_bits ? r->e->d_bits.as<uint32_t>() : nullptr;
}
klf::SelView klf_impl::sel_view(const klf_result* r) {
  const klf::RunArgs& a = r->e->last_args;
  const uint64_t nchunks = (r->total_lines + klf::kMatchChunk - 1) / klf::kMatchChunk;  // (<= cap_lines / kMatchChunk + 1)
  return {sel_bits(r), a.meta, a.line_off, a.bytes, a.segs, a.segout, (uint32_t)r->so.size(), a.cap_lines, nchunks};
}

static int retail_impl(klf_engine* e, klf_result* prev, const klf_regroup_opts* o, int64_t tail, klf_result** out,
                       const char* what, const klf_window_opts* tw = nullptr, const klf_around_opts* ar = nullptr,
                       const klf_records_opts* rc = nullptr) {
  if (int rc = check_latest(e, prev, what)) return rc;
  if (int rc = ensure_index(e)) return rc;
  HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
  auto* r = new (std::nothrow) klf_result();
  if (!r) return KLF_ENOMEM;
  r->e = e;
  r->n_streams = prev->n_streams;
  r->seg_of = prev->seg_of;
  r->seg_base = prev->seg_base;
  r->has_bits = prev->has_bits;
  // (a window without patterns selects over the parsed lines: the tail stage then runs in
  // bitmap mode, over d_gbits, like a regrouped result)
  const bool regroup = o && (!tw || o->before || o->after || o->flags);
  const bool cut = tw && (window_closed(tw) || !prev->has_bits);
  r->grouped = (o || tw) ? (regroup || cut || ar || rc) : prev->grouped;
  r->total_lines = prev->total_lines;
  r->counted = prev->counted;
  r->pcount_ok = prev->pcount_ok;
  r->pcount = prev->pcount;
  const uint32_t nsegs = (uint32_t)prev->so.size();
  r->so.resize(nsegs);
  if (nsegs) {
    klf::RunArgs a = e->last_args;
    a.tail = tail;
    a.stage_times = 0;
    a.fuse = 0;  // (the two-pass compaction, over the line index)
    a.plan_runs = 0;  // (plans assume --tail -1 and are consumed by the run)
    a.skip_tcopy = 0;  // (another window may take the dense path)
    a.plan_mode = 0;   // (and may be larger: the gather's plan over the whole grid)
    hipStream_t st = e->stream;
    uint32_t rmask = 0;
    hipError_t h = hipSuccess;
    klf::RegroupArgs g{};
    klf::WindowArgs wa{};
    if (o || tw) a.bits = e->d_bits.as<uint32_t>();  // always from M: regroups and windows do not compound
    if (regroup) {
      const uint64_t nw = a.cap_lines / 32 + 1, nc = a.cap_lines / klf::kMatchChunk + 1;
      h = e->d_gbits.ensure(nw * 4);
      if (h == hipSuccess) h = e->d_gsum.ensure(nc * 4 * 8);
      g.v = sel_view(prev);
      g.v.bits_in = a.bits;  // M
      g.bits_out = e->d_gbits.as<uint32_t>();
      g.invert = (o->flags & KLF_REGROUP_INVERT) ? 1u : 0u;
      g.before = o->before;
      g.after = o->after;
      g.csum = e->d_gsum.as<uint64_t>();  // (nc >= g.v.nchunks chunks)
      a.bits = g.bits_out;
    }
    double build_ms = 0.0;
    if (ar) {  // (before the tail stage's bracket: the sort's digit read-back syncs the host)
      h = e->d_gbits.ensure((a.cap_lines / 32 + 1) * 4);
      if (h == hipSuccess)
        if (int rc = around_build(e, prev, ar, build_ms, r->ar_anchors, r->ar_intervals)) { delete r; return rc; }
      a.bits = e->d_gbits.as<uint32_t>();
      r->ar_build_ms = build_ms;
    }
    if (rc) {  // (a bracket of its own, like klf_around's: it reads its two counts back)
      h = e->d_gbits.ensure((a.cap_lines / 32 + 1) * 4);
      if (h == hipSuccess)
        if (int err = records_build(e, prev, rc, build_ms, r->rc_heads, r->rc_conts)) { delete r; return err; }
      a.bits = e->d_gbits.as<uint32_t>();
      r->rc_build_ms = build_ms;
    }
    if (cut) {
      if (h == hipSuccess) h = e->d_gbits.ensure((a.cap_lines / 32 + 1) * 4);
      wa.v = sel_view(prev);
      wa.v.bits_in = prev->has_bits ? a.bits : nullptr;  // G' (d_gbits, in place), M, or the parsed lines
      wa.bits_out = e->d_gbits.as<uint32_t>();
      wa.from_sec = tw->from.sec;
      wa.from_nsec = tw->from.nsec;
      wa.until_sec = tw->until.sec;
      wa.until_nsec = tw->until.nsec;
      since_digits(tw->from.sec, tw->from.nsec, wa.from_dig);
      since_digits(tw->until.sec, tw->until.nsec, wa.until_dig);
      a.bits = wa.bits_out;
      a.grep_mode = prev->has_bits ? a.grep_mode : (uint32_t)klf::kGrepGeneral;  // (a.pats stays empty: unread)
    }
    if (h == hipSuccess)
      h = klf::launch_retail(a, st, e->ev, e->num_cus, &rmask, regroup ? &g : nullptr, cut ? &wa : nullptr);
    uint32_t counters[32] = {0};
    if (h == hipSuccess) h = e->h_rb.ensure(kCtrBytes + nsegs * sizeof(SegOut));
    if (h == hipSuccess) h = read_back(e, nsegs, 0, 0, counters, r->so.data());
    if (h == hipSuccess) r->compaction = counters[klf::kCtrDense] ? KLF_COMPACT_TILES : KLF_COMPACT_GATHER;
    if (h == hipSuccess && counters[klf::kCtrOutShort]) h = grow_out_retail(e, a, r->so);  // a larger window than the buffer holds
    if (h == hipSuccess) e->last_args = a;
    if (h != hipSuccess) { delete r; return hip_err(e, h, what); }
    if ((rmask & 1u) && (rmask >> 5 & 1u)) {
      float ms = 0.f;
      if ((h = hipEventElapsedTime(&ms, e->ev[0], e->ev[5])) != hipSuccess) { delete r; return hip_err(e, h, "re-tail timing"); }
      r->ms[4] = ms + build_ms;
    }
    if ((rmask >> 9 & 1u) && (rmask >> 10 & 1u)) {
      float ms = 0.f;
      if ((h = hipEventElapsedTime(&ms, e->ev[9], e->ev[10])) != hipSuccess) { delete r; return hip_err(e, h, "re-tail timing"); }
      r->ms[7] = ms;
    }
    r->ev_mask = rmask;
  }
  for (auto& s : r->so) r->total_out = std::max(r->total_out, s.out_hi);
  r->gen = ++e->gen;  // prev's output buffer is rewritten: prev is stale from here on
  e->last_gen = r->gen;
  *out = r;
  return KLF_OK;
}

extern "C" int klf_retail(klf_engine* e, klf_result* prev, int64_t tail, klf_result** out) {
  if (!e || !prev || !out || prev->e != e || tail < -1) return KLF_EINVAL;
  *out = nullptr;
  return retail_impl(e, prev, nullptr, tail, out, "klf_retail");
}

extern "C" int klf_regroup(klf_engine* e, klf_result* prev, const klf_regroup_opts* o, int64_t tail,
                           klf_result** out) {
  if (!e || !prev || !o || !out || prev->e != e || tail < -1) return KLF_EINVAL;
  *out = nullptr;
  if ((o->flags & ~KLF_REGROUP_INVERT) || o->_reserved)
    return set_err(e, KLF_EINVAL, "klf_regroup: unknown flag bits or a non-zero _reserved");
  if (!prev->has_bits) return set_err(e, KLF_EINVAL, "klf_regroup: the engine has no patterns");
  return retail_impl(e, prev, o, tail, out, "klf_regroup");
}

extern "C" int klf_window(klf_engine* e, klf_result* prev, const klf_window_opts* o, int64_t tail, klf_result** out) {
  if (!e || !prev || !o || !out || prev->e != e || tail < -1) return KLF_EINVAL;
  *out = nullptr;
  if ((o->flags & ~KLF_REGROUP_INVERT) || o->_reserved || o->from._reserved || o->until._reserved)
    return set_err(e, KLF_EINVAL, "klf_window: unknown flag bits or a non-zero _reserved");
  if (o->from.nsec < 0 || o->from.nsec >= 1000000000 || o->until.nsec < 0 || o->until.nsec >= 1000000000)
    return set_err(e, KLF_EINVAL, "klf_window: nsec outside [0, 1e9)");
  if (!prev->has_bits && (o->before || o->after || o->flags))
    return set_err(e, KLF_EINVAL, "klf_window: context and inversion need a pattern");
  const klf_regroup_opts g{o->before, o->after, o->flags, 0};
  return retail_impl(e, prev, &g, tail, out, "klf_window", o);
}

extern "C" int klf_around(klf_engine* e, klf_result* prev, const klf_around_opts* o, int64_t tail, klf_result** out) {
  if (!e || !prev || !o || !out || prev->e != e || tail < -1) return KLF_EINVAL;
  *out = nullptr;
  if (o->flags || o->_reserved || o->from._reserved || o->until._reserved)
    return set_err(e, KLF_EINVAL, "klf_around: unknown flag bits or a non-zero _reserved");
  if (o->from.nsec < 0 || o->from.nsec >= 1000000000 || o->until.nsec < 0 || o->until.nsec >= 1000000000)
    return set_err(e, KLF_EINVAL, "klf_around: nsec outside [0, 1e9)");
  if (o->before_ns > KLF_AROUND_MAX_NS || o->after_ns > KLF_AROUND_MAX_NS)
    return set_err(e, KLF_EINVAL, "klf_around: a duration above KLF_AROUND_MAX_NS");
  if (!prev->has_bits) return set_err(e, KLF_EINVAL, "klf_around: the engine has no patterns");
  const klf_window_opts w{o->from, o->until, 0, 0, 0, 0};
  return retail_impl(e, prev, nullptr, tail, out, "klf_around", &w, o);
}

extern "C" int klf_records(klf_engine* e, klf_result* prev, const klf_records_opts* o, int64_t tail, klf_result** out) {
  if (!o || !out || tail < -1) return KLF_EINVAL;
  *out = nullptr;
  if (const char* bad = records_opts_error(o))  // (the options first: they need neither an engine nor a device)
    return e ? set_err(e, KLF_EINVAL, std::string("klf_records: ") + bad) : KLF_EINVAL;
  if (!e || !prev || prev->e != e) return KLF_EINVAL;
  if (!prev->has_bits) return set_err(e, KLF_EINVAL, "klf_records: the engine has no patterns");
  const klf_window_opts w{o->from, o->until, 0, 0, 0, 0};
  return retail_impl(e, prev, nullptr, tail, out, "klf_records", &w, nullptr, o);
}

extern "C" int klf_result_records_info(const klf_result* r, uint64_t* heads, uint64_t* conts, double* build_ms) {
  if (!r) return KLF_EINVAL;
  if (heads) *heads = r->rc_heads;
  if (conts) *conts = r->rc_conts;
  if (build_ms) *build_ms = r->rc_build_ms;
  return KLF_OK;
}

extern "C" int klf_result_around_info(const klf_result* r, uint64_t* anchors, uint64_t* intervals, double* build_ms) {
  if (!r) return KLF_EINVAL;
  if (anchors) *anchors = r->ar_anchors;
  if (intervals) *intervals = r->ar_intervals;
  if (build_ms) *build_ms = r->ar_build_ms;
  return KLF_OK;
}

extern "C" int klf_run(klf_engine* e, const klf_filter* f, klf_result** out) {
  if (!e || !f || !out) return KLF_EINVAL;
  HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
  HIPCHK(e, ensure_copy_stream(e), "copy stream");
  std::lock_guard<std::mutex> g(e->mu);
  const uint32_t n = (uint32_t)e->staged.size();
  std::vector<uint64_t> lens(n), base(n);
  for (uint32_t i = 0; i < n; ++i) lens[i] = e->staged[i]->len;
  uint64_t total = 0;
  klf_layout(n, lens.data(), base.data(), &total);
  HIPCHK(e, e->d_batch.ensure(total), "alloc batch");
  uint8_t* batch = e->d_batch.as<uint8_t>();
  std::vector<klf::AsmPiece> pieces;
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t off = base[i];
    for (uint8_t* d : e->staged[i]->dchunks) {
      pieces.push_back({d, off, kStageChunk});
      off += kStageChunk;
    }
  }
  if (!pieces.empty()) HIPCHK(e, upload(e->d_asm, pieces, e->stream), "upload pieces");
  // early DMAs done -> k_assemble moves the device chunks into place, while the copy
  // stream DMAs every stream's partly filled last chunk straight to its place
  HIPCHK(e, hipEventRecord(e->copy_done, e->copy_stream), "record copy");
  HIPCHK(e, hipStreamWaitEvent(e->stream, e->copy_done, 0), "wait copy");
  if (!pieces.empty())
    HIPCHK(e, klf::launch_assemble(e->d_asm.as<klf::AsmPiece>(), (uint32_t)pieces.size(), batch, e->stream),
           "assemble");
  for (uint32_t i = 0; i < n; ++i) {
    const auto& s = *e->staged[i];
    if (s.cur.p && s.cur.used)
      HIPCHK(e, hipMemcpyAsync(batch + base[i] + s.dchunks.size() * kStageChunk, s.cur.p, s.cur.used,
                               hipMemcpyHostToDevice, e->copy_stream), "H2D tail");
  }
  HIPCHK(e, hipEventRecord(e->copy_done, e->copy_stream), "record tail");
  HIPCHK(e, hipStreamWaitEvent(e->stream, e->copy_done, 0), "wait tail");
  e->ran = true;
  return run_device_impl(e, batch, n, base.data(), lens.data(), f, out);
}

// ---------------------------------------------------------------------- results ---

int klf_impl::check_result(klf_result* r, uint32_t id) {
  if (!r || id >= r->n_streams) return KLF_EINVAL;
  if (r->e->gen != r->gen) return KLF_ESTATE;  // workspace reused by a later run
  return KLF_OK;
}

int klf_impl::ensure_index(klf_engine* e) {
  if (e->index_pending.empty()) return KLF_OK;
  HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
  for (auto& x : e->index_pending) {
    x.lazy_index = 0;
    x.win_index = 0;
    x.scatter_mode = 0;
    HIPCHK(e, klf::launch_scatter(x, e->stream, e->num_cus), "launch line index");
  }
  HIPCHK(e, hipStreamSynchronize(e->stream), "sync line index");
  e->index_pending.clear();
  e->last_args.lazy_index = 0;
  e->last_args.win_index = 0;
  return KLF_OK;
}

static void fill_counts(const klf_result* r, int64_t s, const uint64_t len, klf_counts* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  if (s < 0) return;
  const SegOut& so = r->so[s];
  const auto mode = r->e->cs.mode;
  c->lines = so.line_hi - so.line_lo;
  c->parsed = so.parsed;
  c->since_ok = so.since_ok;
  c->matched = mode == klf::CompiledSet::kNone && !r->grouped ? c->lines : so.matched;  // (grouped: |G''|)
  c->selected = so.sel_hi - so.sel_lo;
  c->out_bytes = len;
}

extern "C" int klf_result_stream(klf_result* r, uint32_t id, const uint8_t** bytes, uint64_t* len, klf_counts* counts) {
  int rc = check_result(r, id);
  if (rc) return rc;
  klf_engine* e = r->e;
  if (bytes && !r->have_out) {  // counts only: no D2H
    r->out.resize(r->total_out + 1);
    if (r->total_out && !r->fused) {
      HIPCHK(e, hipMemcpyAsync(r->out.data(), e->d_out.p, r->total_out, hipMemcpyDeviceToHost, e->stream), "D2H out");
      HIPCHK(e, hipStreamSynchronize(e->stream), "sync");
    } else if (r->total_out) {  // one copy per extent, into the stream's place
      const uint8_t* d = e->d_out.as<uint8_t>();
      for (size_t sg = 0; sg < r->so.size(); ++sg) {
        uint64_t o = r->so[sg].out_lo;
        for (uint32_t k = r->fx_first[sg]; k < r->fx_first[sg + 1]; ++k) {
          const uint64_t n = r->fx[2 * (size_t)k + 1];
          if (n) HIPCHK(e, hipMemcpyAsync(r->out.data() + o, d + r->fx[2 * (size_t)k], n, hipMemcpyDeviceToHost, e->stream),
                        "D2H out");
          o += n;
        }
      }
      HIPCHK(e, hipStreamSynchronize(e->stream), "sync");
    }
    r->have_out = true;
  }
  const int64_t s = r->seg_of[id];
  uint64_t n = 0, off = 0;
  if (s >= 0) { off = r->so[s].out_lo; n = r->so[s].out_hi - r->so[s].out_lo; }
  if (bytes) *bytes = r->out.data() + off;
  if (len) *len = n;
  fill_counts(r, s, n, counts);
  return KLF_OK;
}

bool klf_impl::write_all(int fd, const uint8_t* p, uint64_t n) {
  while (n) {
    const ssize_t k = ::write(fd, p, (size_t)std::min<uint64_t>(n, 1u << 30));
    if (k < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    if (k == 0) {
      errno = EIO;
      return false;
    }
    p += k;
    n -= (uint64_t)k;
  }
  return true;
}

// §8f-3: device output -> per-stream files.  The output is one buffer in stream order;
// it crosses PCIe once, through 64 MiB pinned chunks taken from the staging pool, with
// the DMA of the next piece in flight while the host writes the current one.
//
// A page-cache write(2) is a host memcpy under the file's inode lock (≈ 7 GB/s on one
// core, measured), far below the pinned D2H, so with several streams each worker thread
// owns whole streams (files), with its own HIP stream and pinned chunk: files are written
// in parallel and each file still sees one sequential write(2) sequence.  One descriptor
// shared by several streams must see them in stream order: that case (and small outputs)
// runs on the calling thread alone.
static bool copy_piece(klf_engine* e, const uint8_t* d_out, const WPiece& q, uint8_t* buf, uint64_t half,
                hipStream_t st, hipEvent_t ev[2], WErr& werr, uint64_t& total) {
  for (const auto& pt : q.parts)
    if (pt.second && !copy_part(e, d_out, q, pt.first, pt.second, buf, half, st, ev, werr, total)) return false;
  return true;
}
bool klf_impl::copy_part(klf_engine* e, const uint8_t* d_out, const WPiece& q, uint64_t dlo, uint64_t n, uint8_t* buf,
                         uint64_t half, hipStream_t st, hipEvent_t ev[2], WErr& werr, uint64_t& total) {
  auto fail = [&](int err, const std::string& what) {
    int exp = -1;
    if (werr.id.compare_exchange_strong(exp, (int)q.id)) { werr.err = err; werr.what = what; }
    return false;
  };
  const uint64_t nk = (n + half - 1) / half;
  auto issue = [&](uint64_t k) {
    const uint64_t o = k * half, m = std::min(half, n - o);
    return hipMemcpyAsync(buf + (k & 1) * half, d_out + dlo + o, m, hipMemcpyDeviceToHost, st) == hipSuccess &&
           hipEventRecord(ev[k & 1], st) == hipSuccess;
  };
  if (!issue(0)) return fail(0, "D2H");
  for (uint64_t k = 0; k < nk; ++k) {
    if (werr.id.load() >= 0) return false;  // another worker failed: stop early
    if (k + 1 < nk && !issue(k + 1)) return fail(0, "D2H");
    if (hipEventSynchronize(ev[k & 1]) != hipSuccess) return fail(0, "D2H sync");
    const uint64_t o = k * half, m = std::min(half, n - o);
    if (!write_all(q.fd, buf + (k & 1) * half, m)) return fail(errno, "write");
    total += m;
  }
  (void)e;
  return true;
}

extern "C" int klf_result_write(klf_result* r, const int* fds, uint32_t n_fds, uint64_t* written) {
  if (written) *written = 0;
  if (!r || (n_fds && !fds) || n_fds != r->n_streams) return KLF_EINVAL;
  klf_engine* e = r->e;
  if (e->gen != r->gen) return KLF_ESTATE;
  std::vector<WPiece> pcs;
  for (uint32_t i = 0; i < n_fds; ++i) {
    const int64_t s = r->seg_of[i];
    if (fds[i] < 0 || s < 0 || r->so[s].out_hi == r->so[s].out_lo) continue;
    WPiece q{r->so[s].out_lo, r->so[s].out_hi, fds[i], i, {}};
    if (r->fused) {
      for (uint32_t k = r->fx_first[s]; k < r->fx_first[s + 1]; ++k) q.parts.emplace_back(r->fx[2 * (size_t)k], r->fx[2 * (size_t)k + 1]);
    } else {
      q.parts.emplace_back(q.lo, q.hi - q.lo);
    }
    pcs.push_back(std::move(q));
  }
  if (pcs.empty()) return KLF_OK;
  std::sort(pcs.begin(), pcs.end(), [](const WPiece& a, const WPiece& b) { return a.lo < b.lo; });
  uint64_t out_bytes = 0;
  for (const auto& q : pcs) out_bytes += q.hi - q.lo;
  auto eio = [&](const WErr& w) {
    return set_err(e, KLF_EIO, "write stream " + std::to_string(w.id.load()) + ": " + w.what +
                                   (w.err ? std::string(": ") + strerror(w.err) : std::string()));
  };
  if (r->have_out) {  // already on the host (klf_result_stream ran)
    uint64_t total = 0;
    for (const auto& q : pcs) {
      if (!write_all(q.fd, r->out.data() + q.lo, q.hi - q.lo))
        return set_err(e, KLF_EIO, "write stream " + std::to_string(q.id) + ": " + strerror(errno));
      total += q.hi - q.lo;
    }
    if (written) *written = total;
    return KLF_OK;
  }
  int nthr = 8;
  if (const char* v = getenv("KLF_WRITE_THREADS")) nthr = std::max(1, atoi(v));
  nthr = (int)std::min<size_t>((size_t)nthr, pcs.size());
  {
    std::vector<int> f;
    for (const auto& q : pcs) f.push_back(q.fd);
    std::sort(f.begin(), f.end());
    if (std::adjacent_find(f.begin(), f.end()) != f.end()) nthr = 1;  // shared fd: stream order
  }
  if (out_bytes < (8u << 20)) nthr = 1;
  HIPCHK(e, hipStreamSynchronize(e->stream), "sync before write");  // d_out complete
  const uint8_t* d_out = e->d_out.as<uint8_t>();
  WErr werr;
  std::atomic<size_t> next{0};
  std::vector<uint64_t> totals((size_t)nthr, 0);
  std::atomic<int> setup_fail{0};
  auto worker = [&](int t) {
    klf_engine::StageChunk c;
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ok = hipSetDevice(e->device) == hipSuccess && take_chunk(e, &c) &&
              hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      setup_fail = 1;
    } else {
      for (size_t j; (j = next.fetch_add(1)) < pcs.size();)
        if (!copy_piece(e, d_out, pcs[j], c.p, kStageChunk / 2, st, ev, werr, totals[(size_t)t])) break;
    }
    if (st) (void)hipStreamSynchronize(st);  // no DMA into a chunk handed back below
    for (auto& x : ev)
      if (x) (void)hipEventDestroy(x);
    if (st) (void)hipStreamDestroy(st);
    if (c.p) {
      std::lock_guard<std::mutex> g(e->mu);
      c.used = 0;
      e->chunk_pool.push_back(c);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nthr; ++t) th.emplace_back(worker, t);
  worker(0);
  for (auto& x : th) x.join();
  if (setup_fail && werr.id.load() < 0 && next.load() < pcs.size())
    return set_err(e, KLF_ENOMEM, "write worker setup (pinned chunk / HIP stream)");
  if (werr.id.load() >= 0) return eio(werr);
  uint64_t total = 0;
  for (auto x : totals) total += x;
  if (written) *written = total;
  return KLF_OK;
}

extern "C" int klf_result_lines(klf_result* r, uint32_t id, const uint64_t** off, uint64_t* n_lines) {
  int rc = check_result(r, id);
  if (rc) return rc;
  klf_engine* e = r->e;
  const int64_t s = r->seg_of[id];
  static const uint64_t kZero = 0;
  if (s < 0) {
    if (off) *off = &kZero;
    if (n_lines) *n_lines = 0;
    return KLF_OK;
  }
  if (!r->have_lines) {
    if (int rc2 = ensure_index(e)) return rc2;
    const size_t nwords = r->total_lines + r->so.size();
    r->line_off.resize(nwords);
    HIPCHK(e, hipMemcpyAsync(r->line_off.data(), e->d_line_off.p, nwords * 8, hipMemcpyDeviceToHost, e->stream), "D2H lines");
    HIPCHK(e, hipStreamSynchronize(e->stream), "sync");
    r->have_lines = true;
  }
  if (off) *off = r->line_off.data() + r->so[s].line_lo + (uint64_t)s;
  if (n_lines) *n_lines = r->so[s].line_hi - r->so[s].line_lo;
  return KLF_OK;
}

// The per-stream packing of one of the run's line bitmaps: the match bitmap M (d_bits) or,
// with `group`, the bitmap r was selected from (sel_bits: a regrouped result's G' in d_gbits).
static int result_bits(klf_result* r, uint32_t id, const uint8_t** bits, uint64_t* nbytes, bool group) {
  int rc = check_result(r, id);
  if (rc) return rc;
  const int which = group && r->grouped ? 1 : 0;
  if (!r->has_bits && !which) return KLF_EINVAL;  // (no patterns: a window's G'' only)
  klf_engine* e = r->e;
  auto& hb = r->hbits[which];
  if (!hb.have) {
    if (int rc2 = ensure_index(e)) return rc2;
    const size_t nw = r->total_lines / 32 + 1;
    hb.bits.assign(nw, 0);
    if (!r->so.empty()) {
      const void* src = group ? sel_bits(r) : e->d_bits.p;
      HIPCHK(e, hipMemcpyAsync(hb.bits.data(), src, nw * 4, hipMemcpyDeviceToHost, e->stream), "D2H bits");
      HIPCHK(e, hipStreamSynchronize(e->stream), "sync");
    }
    hb.have = true;
    hb.stream_bits.assign(r->n_streams, {});
    hb.have_stream_bits.assign(r->n_streams, 0);
  }
  if (!hb.have_stream_bits[id]) {
    const int64_t s = r->seg_of[id];
    auto& v = hb.stream_bits[id];
    if (s >= 0) {
      const uint64_t lo = r->so[s].line_lo, n = r->so[s].line_hi - lo;
      v.assign((n + 7) / 8, 0);
      for (uint64_t i = 0; i < n; ++i) {
        const uint64_t l = lo + i;
        if ((hb.bits[l >> 5] >> (l & 31)) & 1u) v[i >> 3] |= (uint8_t)(1u << (i & 7));
      }
    }
    hb.have_stream_bits[id] = 1;
  }
  if (bits) *bits = hb.stream_bits[id].data();
  if (nbytes) *nbytes = hb.stream_bits[id].size();
  return KLF_OK;
}

extern "C" int klf_result_match_bits(klf_result* r, uint32_t id, const uint8_t** bits, uint64_t* nbytes) {
  return result_bits(r, id, bits, nbytes, false);
}

extern "C" int klf_result_group_bits(klf_result* r, uint32_t id, const uint8_t** bits, uint64_t* nbytes) {
  return result_bits(r, id, bits, nbytes, true);
}

extern "C" int klf_result_pattern_counts(klf_result* r, uint32_t id, uint64_t* counts, uint32_t cap, uint32_t* n) {
  if (!r || id >= r->n_streams || (cap && !counts)) return KLF_EINVAL;
  klf_engine* e = r->e;
  if (n) *n = e->n_user;
  if (!r->counted) return set_err(e, KLF_ESTATE, "the run did not ask for per-pattern counts (KLF_FILTER_PATTERN_COUNTS)");
  if (e->counts_code != KLF_OK) return set_err(e, e->counts_code, e->counts_err);
  const auto& cs = e->cs;
  const int64_t s = r->seg_of[id];
  const bool general = cs.mode == klf::CompiledSet::kGeneral;
  if (general && !r->pcount_ok)
    return set_err(e, KLF_ETOOBIG, "per-pattern counts: the (line, pattern) pair set overflowed");
  for (uint32_t u = 0; u < std::min(cap, e->n_user); ++u) {
    const int32_t m = u < cs.user_map.size() ? cs.user_map[u] : klf::CompiledSet::kCidNever;
    uint64_t v = 0;
    if (s >= 0) {
      const SegOut& so = r->so[s];
      if (m == klf::CompiledSet::kCidAlways) v = so.parsed;
      else if (m >= 0 && cs.mode == klf::CompiledSet::kLiteral1) v = so.matched;  // the one literal
      else if (m >= 0 && general) v = r->pcount[(size_t)s * cs.n_cids + (size_t)m];
    }
    counts[u] = v;
  }
  return KLF_OK;
}

extern "C" int klf_result_last_unparsed(klf_result* r, uint32_t id, uint64_t* rank) {
  int rc = check_result(r, id);
  if (rc) return rc;
  if (!rank) return KLF_EINVAL;
  *rank = 0;
  const int64_t s = r->seg_of[id];
  if (s < 0) return KLF_OK;
  klf_engine* e = r->e;
  const SegOut& so = r->so[s];
  const uint64_t hi = so.line_hi - (so.frag ? 1 : 0);  // newline-terminated lines only
  if (hi <= so.line_lo) return KLF_OK;
  if (int rc2 = ensure_index(e)) return rc2;
  HIPCHK(e, e->d_scratch.ensure(64), "alloc scratch");
  uint64_t v = 0;
  HIPCHK(e, klf::launch_lastbad(e->last_args, so.line_lo, hi, e->d_scratch.as<uint64_t>(), e->stream), "lastbad");
  HIPCHK(e, hipMemcpyAsync(&v, e->d_scratch.p, 8, hipMemcpyDeviceToHost, e->stream), "D2H lastbad");
  HIPCHK(e, hipStreamSynchronize(e->stream), "sync");
  if (v) *rank = hi - (v - 1);
  return KLF_OK;
}

extern "C" int klf_result_device_out(klf_result* r, uint32_t id, const uint8_t** d_out, uint64_t* off, uint64_t* len) {
  if (r && r->fused && !r->have_dev && check_result(r, id) == KLF_OK) {  // one contiguous copy, on demand
    klf_engine* e = r->e;
    HIPCHK(e, hipSetDevice(e->device), "hipSetDevice");
    HIPCHK(e, e->d_out2.ensure(r->total_out + 64), "alloc contiguous output");
    const uint8_t* d = e->d_out.as<uint8_t>();
    for (size_t sg = 0; sg < r->so.size(); ++sg) {
      uint64_t o = r->so[sg].out_lo;
      for (uint32_t k = r->fx_first[sg]; k < r->fx_first[sg + 1]; ++k) {
        const uint64_t n = r->fx[2 * (size_t)k + 1];
        if (n) HIPCHK(e, hipMemcpyAsync(e->d_out2.as<uint8_t>() + o, d + r->fx[2 * (size_t)k], n, hipMemcpyDeviceToDevice,
                                        e->stream), "D2D contiguous output");
        o += n;
      }
    }
    HIPCHK(e, hipStreamSynchronize(e->stream), "sync");
    r->have_dev = true;
  }
  int rc = check_result(r, id);
  if (rc) return rc;
  const int64_t s = r->seg_of[id];
  if (d_out) *d_out = r->fused ? r->e->d_out2.as<uint8_t>() : r->e->d_out.as<uint8_t>();
  if (off) *off = s >= 0 ? r->so[s].out_lo : 0;
  if (len) *len = s >= 0 ? r->so[s].out_hi - r->so[s].out_lo : 0;
  return KLF_OK;
}

extern "C" int klf_result_timing(const klf_result* r, double* ms, uint32_t cap, uint32_t* n) {
  if (!r || (cap && !ms)) return KLF_EINVAL;
  const uint32_t k = std::min<uint32_t>(cap, 8);
  for (uint32_t i = 0; i < k; ++i) ms[i] = r->ms[i];
  if (n) *n = k;
  return KLF_OK;
}

extern "C" int klf_result_index_mode(const klf_result* r) { return r ? r->index_mode : KLF_EINVAL; }
extern "C" int klf_result_compaction(const klf_result* r) { return r ? r->compaction : KLF_EINVAL; }

extern "C" int klf_result_totals(const klf_result* r, klf_counts* t) {
  if (!r || !t) return KLF_EINVAL;
  memset(t, 0, sizeof(*t));
  for (uint32_t i = 0; i < r->n_streams; ++i) {
    const int64_t s = r->seg_of[i];
    if (s < 0) continue;
    klf_counts c;
    fill_counts(r, s, r->so[s].out_hi - r->so[s].out_lo, &c);
    t->lines += c.lines;
    t->parsed += c.parsed;
    t->since_ok += c.since_ok;
    t->matched += c.matched;
    t->selected += c.selected;
    t->out_bytes += c.out_bytes;
  }
  return KLF_OK;
}

extern "C" void klf_result_free(klf_result* r) { delete r; }

// ------------------------------------------------------------------ follow mode ---

struct klf_follow {
  klf_engine* e = nullptr;
  klf_filter f{};
  std::mutex mu;  // guards the carry table's growth (feeds of different ids run concurrently)
  std::vector<std::unique_ptr<std::string>> carry;
};

static std::string* follow_carry(klf_follow* w, uint32_t id) {
  std::lock_guard<std::mutex> g(w->mu);
  while (w->carry.size() <= id) w->carry.emplace_back(new std::string());
  return w->carry[id].get();
}

extern "C" int klf_follow_open(klf_engine* e, const klf_filter* f, klf_follow** out) {
  if (!e || !f || !out) return KLF_EINVAL;
  *out = nullptr;
  auto* w = new (std::nothrow) klf_follow();
  if (!w) return KLF_ENOMEM;
  w->e = e;
  w->f = *f;
  w->f.tail = -1;  // per-line rules only: the server applies --tail to the backlog
  const int rc = klf_reset(e);
  if (rc) { delete w; return rc; }
  *out = w;
  return KLF_OK;
}

extern "C" int klf_follow_feed(klf_follow* w, uint32_t id, const uint8_t* p, size_t n) {
  if (!w || (n && !p)) return KLF_EINVAL;
  std::string* c;
  try {
    c = follow_carry(w, id);
  } catch (...) {
    return KLF_ENOMEM;
  }
  if (!n) return KLF_OK;
  const uint8_t* nl = static_cast<const uint8_t*>(memrchr(p, '\n', n));
  if (!nl) {  // still inside the open line
    c->append(reinterpret_cast<const char*>(p), n);
    return KLF_OK;
  }
  const size_t cut = (size_t)(nl - p) + 1;
  if (!c->empty()) {
    const int rc = klf_stage(w->e, id, reinterpret_cast<const uint8_t*>(c->data()), c->size());
    if (rc) return rc;
    c->clear();  // staged: a retried feed must not stage it again
  }
  const int rc = klf_stage(w->e, id, p, cut);
  if (rc) return rc;
  c->assign(reinterpret_cast<const char*>(p + cut), n - cut);
  return KLF_OK;
}

extern "C" int klf_follow_flush(klf_follow* w, int final, klf_result** out) {
  if (!w || !out) return KLF_EINVAL;
  *out = nullptr;
  const uint32_t n = (uint32_t)w->carry.size();
  if (final)
    for (uint32_t i = 0; i < n; ++i) {
      std::string& c = *w->carry[i];
      if (c.empty()) continue;
      const int rc = klf_stage(w->e, i, reinterpret_cast<const uint8_t*>(c.data()), c.size());
      if (rc) return rc;
      c.clear();
    }
  int rc = klf_set_streams(w->e, n);
  if (!rc) rc = klf_run(w->e, &w->f, out);
  const int rr = klf_reset(w->e);  // the result keeps its outputs; the staging is released
  return rc ? rc : rr;
}

extern "C" uint64_t klf_follow_open_bytes(const klf_follow* w, uint32_t id) {
  return (w && id < w->carry.size()) ? w->carry[id]->size() : 0;
}

extern "C" void klf_follow_close(klf_follow* w) { delete w; }

// ---------------------------------------------------------------- host helpers ---

extern "C" int klf_parse_rfc3339nano(const uint8_t* s, size_t n, klf_time* out) {
  if (!s || !out) return KLF_EINVAL;
  klf::TsResult r;
  auto get = [&](uint32_t i) -> int { return i < n ? s[i] : -1; };
  if (!klf::parse_rfc3339nano(get, r) || r.len != n) return KLF_EINVAL;
  out->sec = r.sec;
  out->nsec = r.nsec;
  out->_reserved = 0;
  return KLF_OK;
}

extern "C" int klf_debug_match(const klf_pattern* pats, uint32_t n, const uint8_t* content, size_t len, int* match) {
  if ((n && !pats) || (len && !content) || !match) return KLF_EINVAL;
  std::vector<std::vector<uint8_t>> ps;
  std::vector<uint32_t> kinds;
  for (uint32_t i = 0; i < n; ++i) {
    ps.emplace_back(pats[i].bytes, pats[i].bytes + pats[i].len);
    kinds.push_back(pats[i].kind);
  }
  klf::CompiledSet cs;
  std::string err;
  int code = KLF_OK;
  if (!klf::compile_set(ps, kinds, cs, err, code)) return code;
  bool hit = false;
  switch (cs.mode) {
    case klf::CompiledSet::kNone: case klf::CompiledSet::kAll: hit = true; break;
    case klf::CompiledSet::kNever: hit = false; break;
    case klf::CompiledSet::kLiteral1:
      hit = std::search(content, content + len, cs.literal.begin(), cs.literal.end()) != content + len;
      break;
    case klf::CompiledSet::kGeneral: {
      hit = cs.also_all;
      if (cs.ac_states) {  // run the same DFA tables the GPU runs
        uint32_t st = 0;
        for (size_t i = 0; i < len && !hit; ++i) {
          st = cs.ac_next[(size_t)st * cs.ac_classes + cs.ac_class[content[i]]];
          hit = cs.ac_accept[st] != 0;
        }
      }
      for (uint32_t r = 0; r < cs.rx_count && !hit; ++r) {  // the GPU recurrence on host
        const uint32_t fl = cs.rx_flags[r];
        if (len == 0) { hit = fl & 2u; continue; }
        if (fl & 1u) { hit = true; continue; }
        uint64_t d = cs.rx_init0[r];
        for (size_t i = 0; i < len && !hit; ++i) {
          const uint64_t c = d & cs.rx_b[(size_t)r * cs.rx_classes + cs.rx_class[content[i]]];
          if (c & cs.rx_last[r]) { hit = true; break; }
          uint64_t nd = cs.rx_first[r];
          for (int p = 0; p < 64; ++p)
            if (c >> p & 1) nd |= cs.rx_follow[(size_t)r * 64 + p];
          d = nd;
        }
        if (!hit) hit = (d & cs.rx_end[r]) != 0;
      }
      break;
    }
  }
  *match = hit ? 1 : 0;
  return KLF_OK;
}

extern "C" int klf_debug_clock(int device, uint32_t iters, uint32_t reps, double* mhz) {
  if (!mhz || !iters || !reps) return KLF_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return KLF_EHIP;
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0)
    return KLF_EHIP;
  const size_t nb = (size_t)ncu * 4;
  uint64_t* d = nullptr;
  if (hipMalloc(&d, (2 * nb + 1) * 8) != hipSuccess) return KLF_ENOMEM;
  hipStream_t st = nullptr;
  hipError_t h = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (h == hipSuccess) h = klf::clock_probe(ncu, iters, reps, d, st);
  std::vector<uint64_t> v(2 * nb + 1, 0);
  if (h == hipSuccess) h = hipMemcpyAsync(v.data(), d, v.size() * 8, hipMemcpyDeviceToHost, st);
  if (h == hipSuccess) h = hipStreamSynchronize(st);
  if (st) (void)hipStreamDestroy(st);
  (void)hipFree(d);
  if (h != hipSuccess) return KLF_EHIP;
  std::vector<double> f;
  for (size_t b = 0; b < nb; ++b)
    if (v[2 * b + 1]) f.push_back(100.0 * (double)v[2 * b] / (double)v[2 * b + 1]);  // 100 MHz real time
  if (f.empty()) return KLF_EHIP;
  std::sort(f.begin(), f.end());
  mhz[0] = f[f.size() / 2];
  mhz[1] = f.front();
  mhz[2] = f.back();
  return KLF_OK;
}

extern "C" int klf_debug_since_digits(int64_t sec, int32_t nsec, uint32_t* out) {
  if (!out) return KLF_EINVAL;
  since_digits(sec, nsec, out);
  return KLF_OK;
}

extern "C" int klf_debug_prefilter(const klf_pattern* pats, uint32_t n, const uint8_t* content, size_t len,
                                   uint32_t phase, int* match, uint32_t* info) {
  if ((n && !pats) || (len && !content) || !match) return KLF_EINVAL;
  std::vector<std::vector<uint8_t>> ps;
  std::vector<uint32_t> kinds;
  for (uint32_t i = 0; i < n; ++i) {
    ps.emplace_back(pats[i].bytes, pats[i].bytes + pats[i].len);
    kinds.push_back(pats[i].kind);
  }
  klf::CompiledSet cs;
  std::string err;
  int code = KLF_OK;
  if (!klf::compile_set(ps, kinds, cs, err, code)) return code;
  if (info) {
    info[0] = cs.qf_on ? 1u : 0u;
    info[1] = cs.qf_q;
    info[2] = cs.qf_stride;
    info[3] = cs.qf_needles;
    info[4] = cs.qf_anc_on ? 0x100u | cs.qf_anc_byte : 0u;
    info[5] = cs.qf_k;
    info[6] = cs.qf_mul;
  }
  if (cs.mode != klf::CompiledSet::kGeneral || !cs.qf_on) return klf_debug_match(pats, n, content, len, match);
  // also_all: the engine's filter is kAll's (every parsed line); the other patterns' tables
  // only serve the per-pattern counts
  *match = (cs.also_all || klf::prefilter_match(cs, content, len, phase)) ? 1 : 0;
  return KLF_OK;
}

extern "C" int klf_debug_prefilter_hits(const klf_pattern* pats, uint32_t n, const uint8_t* sample, size_t slen,
                                        const uint8_t* data, size_t dlen, uint64_t* out, char* layout, size_t cap) {
  if ((n && !pats) || (slen && !sample) || (dlen && !data) || !out) return KLF_EINVAL;
  std::vector<std::vector<uint8_t>> ps;
  std::vector<uint32_t> kinds;
  for (uint32_t i = 0; i < n; ++i) {
    ps.emplace_back(pats[i].bytes, pats[i].bytes + pats[i].len);
    kinds.push_back(pats[i].kind);
  }
  klf::CompiledSet cs;
  std::string err;
  int code = KLF_OK;
  if (!klf::compile_set(ps, kinds, cs, err, code)) return code;
  if (cs.mode != klf::CompiledSet::kGeneral || !cs.qf_on) return KLF_EINVAL;
  if (slen) {
    klf::DataStats st;
    klf::data_stats(sample, slen, cs.qf_fold, st);
    klf::place_needles(cs, &st);
  }
  const klf::PrefilterHits h = klf::prefilter_hits(cs, data, dlen);
  out[0] = cs.qf_stride;
  out[1] = cs.qf_q;
  out[2] = cs.qf_k;
  out[3] = cs.qf_anc_on ? 0x100u | cs.qf_anc_byte : 0u;
  out[4] = h.probes;
  out[5] = h.bitmap_hits;
  out[6] = h.anchor_hits;
  out[7] = h.verified;
  out[8] = h.pair_pass;
  out[9] = cs.qf_grams;
  out[10] = cs.qf_mul;
  if (layout && cap) { strncpy(layout, cs.qf_layout.c_str(), cap - 1); layout[cap - 1] = 0; }
  return KLF_OK;
}

extern "C" int klf_debug_compile(const klf_pattern* pats, uint32_t n, uint32_t* mode, char* err, size_t err_cap) {
  if ((n && !pats) || !mode) return KLF_EINVAL;
  std::vector<std::vector<uint8_t>> ps;
  std::vector<uint32_t> kinds;
  for (uint32_t i = 0; i < n; ++i) {
    ps.emplace_back(pats[i].bytes, pats[i].bytes + pats[i].len);
    kinds.push_back(pats[i].kind);
  }
  klf::CompiledSet cs;
  std::string e;
  int code = KLF_OK;
  bool ok = klf::compile_set(ps, kinds, cs, e, code);
  if (err && err_cap) { strncpy(err, e.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
  *mode = (uint32_t)cs.mode;
  return ok ? KLF_OK : code;
}

extern "C" int klf_debug_factors(const uint8_t* pat, size_t len, uint32_t want, char* buf, size_t cap, uint32_t* n,
                                 uint32_t* pre, uint32_t* loose) {
  if ((len && !pat) || (cap && !buf) || !n || !pre || !loose) return KLF_EINVAL;
  std::vector<std::string> alts;
  bool l = false;
  uint32_t p = 0;
  if (!klf::regex_factors(pat, len, alts, l, &p, want ? want : SIZE_MAX)) return KLF_EINVAL;
  size_t o = 0;
  for (auto& a : alts) {
    if (o + a.size() + 1 > cap) return KLF_ETOOBIG;
    memcpy(buf + o, a.data(), a.size());
    o += a.size();
    buf[o++] = 0;
  }
  *n = (uint32_t)alts.size();
  *pre = p;
  *loose = l ? 1u : 0u;
  return KLF_OK;
}
