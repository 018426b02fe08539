// klf_analysis.hip — the kernels of the calls on a finished run (SPEC.md S4a .. S4h): regroup,
// time window, histogram, merged timeline and the device sort, grouped counts, field statistics,
// time context across streams, multi-line records.  They read a finished run's line index, meta and bitmaps
// (SelView) and write arrays of their own; none of them touches the run's device state, and
// no kernel of the run (klf_kernels.hip) uses anything defined here.
#include <hip/hip_runtime.h>

#include "klf_analysis.hpp"
#include "klf_device.hpp"
#include "klf_fieldval.hpp"
#include "klf_groupkey.hpp"
#include "klf_ts.hpp"

namespace klf {
namespace {

// ============================ regroup: context lines / inverted match (SPEC.md S4a) ==
// G' = parsed lines within `after` lines behind / `before` lines ahead of a line of S, in
// the same stream; S = M (the run's match bitmap) or, inverted, the parsed lines outside M.
// For line l of stream [lo, hi): with P = the last line of S at or before l and N = the
// first at or after l (over all streams), l is in G' iff it is parsed and
// (P >= lo and l - P <= after) or (N < hi and N - l <= before): the nearest line of S on
// either side decides, and one outside the stream means none inside.  Per kMatchChunk lines
// (256 words, one per thread, like k_mcount):
//   k_rg_sum    per chunk: the last and first line of S
//   k_rg_carry  one block: the same over all chunks before / after each chunk
//   k_rg_build  per chunk: block scans carry P / N from word to word; each word ORs the
//               carried-in masks with the in-word smear of S, per stream part of the word
// The cost is L/8 + 2L bytes read and L/8 written whatever before and after are.  Line
// positions are kept as max-scan keys: P + 1 (0 = none) and ~N (0 = none).
__device__ __forceinline__ uint64_t wave_incl_scan_max64(uint64_t x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up(x, d, 64);
    if (lane >= d) x = x > o ? x : o;
  }
  return x;
}
__device__ __forceinline__ uint64_t wave_incl_rscan_max64(uint64_t x, int lane) {  // over lanes >= lane
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_down(x, d, 64);
    if (lane + d < 64) x = x > o ? x : o;
  }
  return x;
}
// Exclusive block max-scans of x over the threads before (*pre) and after (*post) this one;
// returns the block maximum.  s_w: [2][4].
__device__ __forceinline__ void block_excl_scan_max64(uint64_t x, uint64_t y, uint64_t (*s_w)[4], uint64_t* pre,
                                                      uint64_t* post) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t fi = wave_incl_scan_max64(x, lane), ri = wave_incl_rscan_max64(y, lane);
  uint64_t fe = __shfl_up(fi, 1, 64), re = __shfl_down(ri, 1, 64);
  if (lane == 0) fe = 0;
  if (lane == 63) re = 0;
  __syncthreads();
  if (lane == 63) s_w[0][wv] = fi;
  if (lane == 0) s_w[1][wv] = ri;
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    if (k < wv) fe = fe > s_w[0][k] ? fe : s_w[0][k];
    if (k > wv) re = re > s_w[1][k] ? re : s_w[1][k];
  }
  *pre = fe;
  *post = re;
}

// The parsed bits of word w's 32 lines, or with SINCE their parsed-and-since_ok bits (16-B
// loads of their meta; line by line where the word reaches past the line count).
template <bool SINCE>
__device__ __forceinline__ uint32_t meta_word(const uint16_t* __restrict__ meta, uint64_t w, uint64_t L) {
  const uint64_t l0 = w * 32;
  uint32_t p = 0;
  if (l0 + 32 <= L) {
    const uint4* q = reinterpret_cast<const uint4*>(meta + l0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 v = q[k];
      const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t y = SINCE ? x[j] & (x[j] >> 1) : x[j];  // bit 0 / bit 16: the low / high line's flag(s)
        p |= ((y & 1u) | ((y >> 15) & 2u)) << (8 * k + 2 * j);
      }
    }
  } else {
    for (uint64_t l = l0; l < L; ++l) {
      const uint32_t m = meta[l];
      p |= ((SINCE ? m & (m >> 1) : m) & Meta::kParsed) << (l - l0);
    }
  }
  return p;
}
// Word w of the view's selection (0 past the line count): its bitmap, or without one the
// parsed lines.
__device__ __forceinline__ uint32_t view_word(const SelView& v, uint64_t w, uint64_t L) {
  if (w * 32 >= L) return 0u;
  return v.bits_in ? v.bits_in[w] & word_range_mask(w, 0, L) : meta_word<false>(v.meta, w, L);
}
// Word w of S (0 past the line count).  pw (nullable): the word's parsed bits as well; without
// it the meta is read only when S is inverted.
__device__ __forceinline__ uint32_t rg_s_word(const RegroupArgs& g, uint64_t w, uint64_t L, uint32_t* pw = nullptr) {
  if (pw) *pw = 0u;
  if (w * 32 >= L) return 0u;
  const uint32_t m = g.v.bits_in[w] & word_range_mask(w, 0, L);
  if (!pw && !g.invert) return m;
  const uint32_t p = meta_word<false>(g.v.meta, w, L);
  if (pw) *pw = p;
  return g.invert ? p & ~m : m;
}
// x | x << 1 | ... | x << k (UP) or the same with right shifts, k <= 31: doubling steps.
template <bool UP>
__device__ __forceinline__ uint32_t smear(uint32_t x, uint32_t k) {
  uint32_t cur = 1;
  while (cur * 2 <= k + 1) {
    x |= UP ? x << cur : x >> cur;
    cur *= 2;
  }
  const uint32_t r = k + 1 - cur;  // < cur
  return x | (UP ? x << r : x >> r);
}

__global__ __launch_bounds__(256) void k_rg_sum(RegroupArgs g) {
  __shared__ uint64_t s_w[2][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t;
    const uint32_t s = rg_s_word(g, w, L);
    uint64_t last = s ? w * 32 + (31 - __clz(s)) + 1 : 0, first = s ? ~(w * 32 + (__ffs(s) - 1)) : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const uint64_t a = __shfl_xor(last, d, 64), b = __shfl_xor(first, d, 64);
      last = last > a ? last : a;
      first = first > b ? first : b;
    }
    __syncthreads();
    if (lane == 0) { s_w[0][wv] = last; s_w[1][wv] = first; }
    __syncthreads();
    if (t == 0) {
      uint64_t a = s_w[0][0], b = s_w[1][0];
      for (int k = 1; k < 4; ++k) {
        a = a > s_w[0][k] ? a : s_w[0][k];
        b = b > s_w[1][k] ? b : s_w[1][k];
      }
      g.csum[4 * c] = a;
      g.csum[4 * c + 1] = b;
    }
  }
}

// Thread t owns the chunks [t K, (t + 1) K): their maxima, one block scan, then each chunk's
// exclusive prefix / suffix.
__global__ __launch_bounds__(256) void k_rg_carry(RegroupArgs g) {
  __shared__ uint64_t s_w[2][4];
  const uint64_t K = (g.v.nchunks + 255) / 256;
  const uint64_t c0 = threadIdx.x * K, c1 = c0 + K < g.v.nchunks ? c0 + K : g.v.nchunks;
  uint64_t a = 0, b = 0;
  for (uint64_t c = c0; c < c1; ++c) {
    const uint64_t x = g.csum[4 * c], y = g.csum[4 * c + 1];
    a = a > x ? a : x;
    b = b > y ? b : y;
  }
  uint64_t pre, post;
  block_excl_scan_max64(a, b, s_w, &pre, &post);
  for (uint64_t c = c0; c < c1; ++c) {
    g.csum[4 * c + 2] = pre;
    const uint64_t x = g.csum[4 * c];
    pre = pre > x ? pre : x;
  }
  for (uint64_t c = c1; c > c0; --c) {
    g.csum[4 * (c - 1) + 3] = post;
    const uint64_t y = g.csum[4 * (c - 1) + 1];
    post = post > y ? post : y;
  }
}

__global__ __launch_bounds__(256) void k_rg_build(RegroupArgs g) {
  __shared__ uint64_t s_w[2][4];
  const int t = threadIdx.x;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  const uint64_t nw = g.v.cap_lines / 32 + 1;  // words of the bitmaps
  const uint32_t ka = g.after < 31 ? (uint32_t)g.after : 31u, kb = g.before < 31 ? (uint32_t)g.before : 31u;
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    uint32_t pw;  // (0 past the line count, no bit at or past L)
    const uint32_t sw = rg_s_word(g, w, L, &pw);
    uint64_t pk, nk;  // P + 1 over the words before this one, ~N over the words after it
    block_excl_scan_max64(sw ? l0 + (31 - __clz(sw)) + 1 : 0, sw ? ~(l0 + (__ffs(sw) - 1)) : 0, s_w, &pk, &nk);
    const uint64_t cp = g.csum[4 * c + 2], cn = g.csum[4 * c + 3];
    pk = pk > cp ? pk : cp;
    nk = nk > cn ? nk : cn;
    uint32_t out = 0;
    if (pw) {
      const uint64_t wend = l0 + 32;
      for (uint32_t s = find_seg_by_line(g.v.segout, g.v.nsegs, l0); s < g.v.nsegs; ++s) {
        const uint64_t lo = g.v.segout[s].line_lo, hi = g.v.segout[s].line_hi;
        if (lo >= wend) break;
        const uint32_t pm = word_range_mask(w, lo, hi);
        const uint32_t sp = sw & pm;
        uint32_t m = smear<true>(sp, ka) | smear<false>(sp, kb);
        if (pk && pk - 1 >= lo) {  // (P < l0) the lines up to P + after
          const uint64_t reach = pk - 1 + g.after;
          if (reach >= l0) m |= reach - l0 >= 31 ? ~0u : (2u << (reach - l0)) - 1u;
        }
        if (nk && ~nk < hi) {  // (N >= l0 + 32) the lines from N - before on
          const uint64_t n = ~nk, from = n >= g.before ? n - g.before : 0;
          if (from < wend) m |= from <= l0 ? ~0u : ~0u << (from - l0);
        }
        out |= m & pm;
      }
      out &= pw;  // (pw has no bit at or past L)
    }
    if (w < nw) g.bits_out[w] = out;
  }
}

// ================================================= time window (klf_window, SPEC.md S4b) ==
// G'' = the lines of G' whose instant lies in [from, until).  One block per kMatchChunk
// lines, one thread per bitmap word, like k_rg_build; a wave whose 64 words of G' are zero
// costs their loads only.  A line of G' costs its index entry and the first 32 bytes of the line in the batch
// (every line of G' is parsed: its prefix ends at its first space, inside the line).
// Timestamps need not ascend, so every line is decided on its own.
//
// The canonical kubelet prefix is decided as the scan's parse_fast decides since: the same
// shape test and big-endian digit packing, then two lexicographic compares against the
// bounds' digits (WindowArgs::from_dig / until_dig, clamped to the fast path's years
// 1970..2099 by the host).  The line is parsed already, so its date is valid and the field
// range checks are not repeated.  Every other shape goes to the general parser.
__device__ __forceinline__ bool dig_ge(const uint32_t (&p)[6], const uint32_t (&c)[6]) {
  const uint64_t a0 = (uint64_t)p[0] << 32 | p[1], a1 = (uint64_t)p[2] << 32 | p[3], a2 = (uint64_t)p[4] << 32 | p[5];
  const uint64_t c0 = (uint64_t)c[0] << 32 | c[1], c1 = (uint64_t)c[2] << 32 | c[3], c2 = (uint64_t)c[4] << 32 | c[5];
  return a0 > c0 || (a0 == c0 && (a1 > c1 || (a1 == c1 && a2 >= c2)));
}
// The first 32 bytes of the line at segp + off, packed: true iff they are the canonical
// kubelet prefix with a year in 1970..2099, p = its 23 digits big-endian (Y Y Y Y | M M D D |
// h h m m | s s n0 n1 | n2 n3 n4 n5 | n6 n7 '0' n8).
__device__ __forceinline__ bool tw_canon_digits(const uint8_t* __restrict__ segp, uint64_t off, uint32_t (&p)[6]) {
  // two unaligned 16-B global loads at the line start (inside the allocation: kAllocSlack)
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 x0, x1;
  __builtin_memcpy(&x0, segp + off, 16);
  __builtin_memcpy(&x1, segp + off + 16, 16);
  const uint32_t w[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  // separators: '-' 4, '-' 7, 'T' 10, ':' 13, ':' 16, '.' 19, 'Z' 29, ' ' 30
  const uint32_t sep = ((w[1] ^ 0x2D00002Du) & 0xFF0000FFu) | ((w[2] ^ 0x00540000u) & 0x00FF0000u) |
                       ((w[3] ^ 0x00003A00u) & 0x0000FF00u) | ((w[4] ^ 0x2E00003Au) & 0xFF0000FFu) |
                       ((w[7] ^ 0x00205A00u) & 0x00FFFF00u);
  p[0] = __builtin_amdgcn_perm(0u, w[0], 0x00010203u);                   // Y Y Y Y
  p[1] = __builtin_amdgcn_perm(w[2], w[1], 0x01020405u);                 // M M D D
  p[2] = __builtin_amdgcn_perm(w[3], w[2], 0x03040607u);                 // h h m m
  p[3] = __builtin_amdgcn_perm(w[5], w[4], 0x01020405u);                 // s s n0 n1
  p[4] = __builtin_amdgcn_perm(w[6], w[5], 0x02030405u);                 // n2 n3 n4 n5
  p[5] = __builtin_amdgcn_perm(w[7], w[6], 0x02030C04u) | 0x00003000u;   // n6 n7 0 n8
  const uint32_t hi = ((p[0] ^ 0x30303030u) | (p[1] ^ 0x30303030u) | (p[2] ^ 0x30303030u) | (p[3] ^ 0x30303030u) |
                       (p[4] ^ 0x30303030u) | (p[5] ^ 0x30303030u)) & 0xF0F0F0F0u;
  const uint32_t lo = ((p[0] + 0x06060606u) | (p[1] + 0x06060606u) | (p[2] + 0x06060606u) | (p[3] + 0x06060606u) |
                       (p[4] + 0x06060606u) | (p[5] + 0x06060606u)) & 0x40404040u;
  return (sep | hi | lo) == 0u && p[0] - 0x31393730u <= 0x32303939u - 0x31393730u;  // canonical, year 1970..2099
}
__device__ __forceinline__ bool tw_line_in(const WindowArgs& g, const uint8_t* __restrict__ segp, uint64_t off,
                                           uint64_t seg_len) {
  uint32_t p[6];
  if (tw_canon_digits(segp, off, p)) return dig_ge(p, g.from_dig) && !dig_ge(p, g.until_dig);
  TsResult r;
  uint32_t plen;
  if (!parse_line_prefix(GlobalBytes{segp, (int64_t)off, (int64_t)seg_len}, r, plen)) return false;
  return !time_before(r.sec, r.nsec, g.from_sec, g.from_nsec) && time_before(r.sec, r.nsec, g.until_sec, g.until_nsec);
}

// The n-th (0-based) set bit of w, n < popcount(w): a binary search on popcounts.
__device__ __forceinline__ uint32_t nth_set_bit(uint32_t w, uint32_t n) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t width = 16; width >= 1; width >>= 1) {
    const uint32_t c = (uint32_t)__popc((w >> pos) & ((1u << width) - 1u));
    if (n >= c) { n -= c; pos += width; }
  }
  return pos;
}

// The selected-line walk (k_tw_build, k_hist, k_tl_keys): one block per kMatchChunk lines, one
// thread per bitmap word `in` of the selection (no bit at or past the line count L).  A wave
// shares the lines of its 64 words over its lanes (LDS: the words, the exclusive prefix of
// their popcounts, each word's first stream): lane i of round r takes the wave's (64 r + i)-th
// selected line, so a round reads 64 consecutive selected lines -- consecutive index entries
// and, where the selection is dense, neighbouring bytes of the batch.  One thread per word
// walking its own 32 lines took 2.13 ms on the C3 shape (55.6 M lines, all selected); see
// DESIGN.md.  Per chunk: walk_publish, the kernel's own LDS stores, __syncthreads(),
// walk_rounds.
struct WalkLds {
  uint32_t in[4][64], pre[4][64], seg[4][64];
};
// Publishes the thread's word (first line l0) behind a barrier that ends the previous chunk's
// LDS reads; returns the wave's selected lines (wave-uniform).  The caller's barrier follows.
__device__ __forceinline__ uint32_t walk_publish(WalkLds& ws, const SelView& v, uint32_t in, uint64_t l0) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t cnt = (uint32_t)__popc(in);
  const uint32_t incl = wave_incl_scan_add(cnt, lane);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  __syncthreads();
  ws.in[wv][lane] = in;
  ws.pre[wv][lane] = incl - cnt;
  ws.seg[wv][lane] = in ? find_seg_by_line(v.segout, v.nsegs, l0) : 0u;
  return total;
}
// One selected line of a round: the wave's k-th, bit b of the wave's word j, global line l of
// segment s at stream offset off.  live false: the lane has no line this round; k alone is set.
struct WalkLine {
  bool live;
  uint32_t k, j, b, s;
  uint64_t l, off;
  SegDesc sd;
};
// The rounds: f(const WalkLine&) on every lane of every round (total is wave-uniform), so f may
// use cross-lane operations.
template <class F>
__device__ __forceinline__ void walk_rounds(const WalkLds& ws, const SelView& v, uint32_t total, uint64_t l0, F&& f) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t wl0 = l0 - (uint64_t)lane * 32;  // first line of the wave's words
  for (uint32_t k0 = 0; k0 < total; k0 += 64) {
    WalkLine q;  // (the rest stays unset on a lane without a line: nothing to merge after the branch)
    q.k = k0 + (uint32_t)lane;
    q.live = q.k < total;
    if (q.live) {
      uint32_t j = 0;  // the word holding line k: the last one whose prefix is <= k (its count is > 0)
#pragma unroll
      for (uint32_t step = 32; step >= 1; step >>= 1)
        if (ws.pre[wv][j + step] <= q.k) j += step;
      q.j = j;
      q.b = nth_set_bit(ws.in[wv][j], q.k - ws.pre[wv][j]);
      q.l = wl0 + (uint64_t)j * 32 + q.b;  // (< L: `in` has no bit at or past L)
      q.s = ws.seg[wv][j];
      while (q.l >= v.segout[q.s].line_hi) ++q.s;  // (a word may span streams; s stays < nsegs as l < L)
      q.sd = v.segs[q.s];
      q.off = v.line_off[q.l + q.s];
    }
    f(q);
  }
}

__global__ __launch_bounds__(256) void k_tw_build(WindowArgs g) {
  __shared__ WalkLds ws;
  __shared__ uint32_t s_out[4][64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  const uint64_t nw = g.v.cap_lines / 32 + 1;  // words of the bitmaps
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    const uint32_t total = walk_publish(ws, g.v, view_word(g.v, w, L), l0);  // (the previous chunk's s_out is read)
    s_out[wv][lane] = 0u;
    __syncthreads();
    walk_rounds(ws, g.v, total, l0, [&](const WalkLine& q) {
      if (q.live && tw_line_in(g, g.v.bytes + q.sd.base, q.off, q.sd.len)) atomicOr(&s_out[wv][q.j], 1u << q.b);
    });
    __syncthreads();
    if (w < nw) g.bits_out[w] = s_out[wv][lane];
  }
}

// ====================================== histogram over time (klf_result_histogram, SPEC.md S4c) ==
// Per stream, the lines of a selection bitmap H counted by instant: below `origin`, in one of
// n_buckets buckets of width_ns from `origin` on, or at / above `end` = origin + n_buckets *
// width_ns.  The selected-line walk over H (walk_publish / walk_rounds), reading the first 32
// bytes of each line; in place of a bit per line each line gets a key
// = segment * (n_buckets + 2) + slot (slot n_buckets = below, n_buckets + 1 = above) into the
// u64 table.  The 64 consecutive lines of a round mostly share a key, so a lane adds only when
// its key differs from the previous lane's, and adds the length of its run of equal keys (from
// the ballot of those heads): any order of keys stays exact, at one atomic per line at worst.

// The instant of a canonical prefix from its packed digits (tw_canon_digits; a parsed line,
// so every field is in range): days-from-civil plus h / m / s.
__device__ __forceinline__ uint32_t dig2(uint32_t x) { return (x >> 8 & 15u) * 10u + (x & 15u); }
__device__ __forceinline__ void canon_instant(const uint32_t (&p)[6], int64_t& sec, int32_t& nsec) {
  const int32_t year = (int32_t)(dig2(p[0] >> 16) * 100u + dig2(p[0]));
  const int32_t days = (int32_t)days_from_civil(year, (int)dig2(p[1] >> 16), (int)dig2(p[1]));  // 0 .. 47481
  sec = (int64_t)days * 86400 + (int64_t)(dig2(p[2] >> 16) * 3600u + dig2(p[2]) * 60u + dig2(p[3] >> 16));
  nsec = (int32_t)(dig2(p[3]) * 10000000u + (dig2(p[4] >> 16) * 100u + dig2(p[4])) * 1000u + dig2(p[5] >> 16) * 10u +
                   (p[5] & 15u));
}

// The instant of the line at segp + off: a canonical prefix from its packed digits, every
// other shape through the general parser.  False (sec / nsec untouched): the line has none.
__device__ __forceinline__ bool line_instant(const uint8_t* __restrict__ segp, uint64_t off, uint64_t seg_len,
                                             int64_t& sec, int32_t& nsec) {
  uint32_t p[6];
  if (tw_canon_digits(segp, off, p)) {
    canon_instant(p, sec, nsec);
    return true;
  }
  TsResult r;
  uint32_t plen;
  if (!parse_line_prefix(GlobalBytes{segp, (int64_t)off, (int64_t)seg_len}, r, plen)) return false;
  sec = r.sec;
  nsec = r.nsec;
  return true;
}

// The table slot of the line at segp + off, or ~0u for a line without an instant (none in H).
__device__ __forceinline__ uint32_t hist_slot(const HistArgs& g, const uint8_t* __restrict__ segp, uint64_t off,
                                              uint64_t seg_len) {
  int64_t sec;
  int32_t nsec;
  if (!line_instant(segp, off, seg_len, sec, nsec)) return ~0u;
  if (time_before(sec, nsec, g.org_sec, g.org_nsec)) return g.n_buckets;
  if (!g.end_open && !time_before(sec, nsec, g.end_sec, g.end_nsec)) return g.n_buckets + 1;
  // origin <= ts < end: d = ts - origin in ns lies in [0, n_buckets * width_ns), below 2^63
  const uint64_t ds = (uint64_t)sec - (uint64_t)g.org_sec;
  if (g.width_s)  // whole seconds and a span below 2^32 s: floor(d / 1e9) = ds - borrow, a 32-bit division
    return ((uint32_t)ds - (nsec < g.org_nsec ? 1u : 0u)) / g.width_s;
  const uint64_t d = ds * 1000000000ull + (uint64_t)(int64_t)(nsec - g.org_nsec);
  return (uint32_t)(d / g.width_ns);
}

__global__ __launch_bounds__(256) void k_hist(HistArgs g) {
  __shared__ WalkLds ws;
  const int t = threadIdx.x, lane = t & 63;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  const uint32_t row = g.n_buckets + 2;
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    const uint32_t total = walk_publish(ws, g.v, view_word(g.v, w, L), l0);
    __syncthreads();
    walk_rounds(ws, g.v, total, l0, [&](const WalkLine& q) {
      uint32_t key = ~0u;  // no line, or a line without an instant
      if (q.live) {
        const uint32_t slot = hist_slot(g, g.v.bytes + q.sd.base, q.off, q.sd.len);
        if (slot < row) key = q.s * row + slot;  // (< nsegs * row <= 2^24: the host's size check)
      }
      const uint32_t prev = (uint32_t)__shfl_up((int)key, 1, 64);
      const bool head = lane == 0 || key != prev;
      const uint64_t heads = __ballot(head);
      if (head && key != ~0u) {
        const uint64_t after = lane == 63 ? 0ull : heads >> (lane + 1);  // the heads behind this lane
        const uint32_t run = after ? (uint32_t)__ffsll((long long)after) : 64u - (uint32_t)lane;
        atomicAdd(reinterpret_cast<unsigned long long*>(g.table + key), (unsigned long long)run);
      }
    });
  }
}

// ====================================== merged timeline (klf_result_timeline, SPEC.md S4d) ==
// The emitted lines E of every stream (the lines l of [win_lo, win_hi) with parsed, since_ok
// and their bit in the selection bitmap: window_lines' rule), keyed by instant, sorted by a
// stable LSD radix sort (so equal instants keep their (stream, line) order) and rendered into
// one buffer.  Every step is reduce-then-scan over kernel boundaries; no block waits on another.

// Word w of E (0 past the line count): the selection word, the tail windows of the streams the
// word meets, then the parsed / since_ok flags (read only where something is left).
__device__ __forceinline__ uint32_t tl_e_word(const SelView& v, uint64_t w, uint64_t L) {
  const uint64_t l0 = w * 32;
  if (l0 >= L) return 0u;
  uint32_t x = word_range_mask(w, 0, L);
  if (v.bits_in) x &= v.bits_in[w];
  if (!x) return 0u;
  const uint64_t l1 = l0 + 32 < L ? l0 + 32 : L;
  uint32_t win = 0;
  for (uint32_t s = find_seg_by_line(v.segout, v.nsegs, l0); s < v.nsegs && v.segout[s].line_lo < l1; ++s)
    win |= word_range_mask(w, v.segout[s].win_lo, v.segout[s].win_hi);
  x &= win;
  if (!x) return 0u;
  return x & meta_word<true>(v.meta, w, L);
}

// Per chunk the lines of E (EMITTED: the timeline) or of H (the field statistics).
template <bool EMITTED>
__global__ __launch_bounds__(256) void k_tl_count(SelView v, uint64_t* cbase) {
  __shared__ uint32_t s_w[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t L = v.segout[v.nsegs - 1].line_hi;
  for (uint64_t c = blockIdx.x; c < v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t;
    const uint32_t cnt = wave_sum((uint32_t)__popc(EMITTED ? tl_e_word(v, w, L) : view_word(v, w, L)));
    __syncthreads();  // (the previous chunk's sums are read)
    if (lane == 0) s_w[wv] = cnt;
    __syncthreads();
    if (t == 0) cbase[c] = (uint64_t)s_w[0] + s_w[1] + s_w[2] + s_w[3];
  }
}

// One block: a[0 .. m) becomes its exclusive prefix, a[m] the total.
__global__ __launch_bounds__(256) void k_tl_scan(uint64_t* __restrict__ a, uint64_t m) {
  __shared__ uint64_t s_w[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t per = (m + 255) / 256;
  const uint64_t i0 = (uint64_t)t * per < m ? (uint64_t)t * per : m, i1 = i0 + per < m ? i0 + per : m;
  uint64_t sum = 0;
  for (uint64_t i = i0; i < i1; ++i) sum += a[i];
  const uint64_t incl = wave_incl_scan_add(sum, lane);
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  uint64_t pre = incl - sum;
  for (int k = 0; k < wv; ++k) pre += s_w[k];
  for (uint64_t i = i0; i < i1; ++i) {
    const uint64_t x = a[i];
    a[i] = pre;
    pre += x;
  }
  if (t == 255) a[m] = pre;  // (thread 255's range ends at m)
}

// The selected-line walk over E (EMITTED: the timeline, with a side record per line) or over the
// view's own bitmap (klf_around's anchors: the items alone).  A line's rank in (stream, line)
// order is the chunk's base + the lines of the block's earlier waves + its rank k in the wave.
template <bool EMITTED>
__global__ __launch_bounds__(256) void k_tl_keys(TlArgs g) {
  __shared__ WalkLds ws;
  __shared__ uint32_t s_tot[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    const uint32_t total = walk_publish(ws, g.v, EMITTED ? tl_e_word(g.v, w, L) : view_word(g.v, w, L), l0);
    if (lane == 0) s_tot[wv] = total;
    __syncthreads();
    uint64_t base = g.cbase[c];
    for (int k = 0; k < wv; ++k) base += s_tot[k];
    walk_rounds(ws, g.v, total, l0, [&](const WalkLine& q) {
      if (!q.live) return;
      int64_t sec;
      int32_t nsec;
      if (!line_instant(g.v.bytes + q.sd.base, q.off, q.sd.len, sec, nsec)) sec = 0, nsec = 0;  // (none in E: parsed lines)
      const uint64_t ord = base + q.k;
      if (ord < g.n) {  // (always: n is the scan's total of the same words)
        g.items[0][ord] = TlItem{(uint64_t)sec ^ (1ull << 63), (uint32_t)nsec, (uint32_t)ord};
        if (EMITTED) g.side[ord] = TlSide{q.l, q.s, 0u};
      }
    });
  }
}

__device__ __forceinline__ uint32_t tl_digit(const TlItem& it, uint32_t p) {
  return p < 4 ? (it.nsec >> (8 * p)) & 255u : (uint32_t)(it.sec_key >> (8 * (p - 4))) & 255u;
}

// One count into an LDS histogram per lane with `valid`; a wave whose lanes all hold the same
// digit (the upper bytes of sec; a stream's lines of one second) adds once.  Every lane of the
// wave calls it.
__device__ __forceinline__ void tl_hist_add(uint32_t* h, uint32_t d, bool valid, int lane) {
  const uint64_t act = __ballot(valid);
  if (!act) return;
  const int src = __ffsll((long long)act) - 1;
  const uint32_t first = (uint32_t)__shfl((int)d, src, 64);
  if (__all(!valid || d == first)) {
    if (lane == src) atomicAdd(&h[first], (uint32_t)__popcll(act));
  } else if (valid) {
    atomicAdd(&h[d], 1u);
  }
}

// All twelve digit histograms in one read of the items.
__global__ __launch_bounds__(256) void k_tl_digits(const TlItem* __restrict__ items, uint64_t n,
                                                   uint64_t* __restrict__ dhist) {
  __shared__ uint32_t s_h[kTlDigits * 256];
  const int t = threadIdx.x, lane = t & 63;
  for (uint32_t k = t; k < kTlDigits * 256; k += 256) s_h[k] = 0;
  __syncthreads();
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < n; i0 += (uint64_t)gridDim.x * 256) {
    const uint64_t i = i0 + t;
    const bool valid = i < n;
    TlItem it{};
    if (valid) it = items[i];
#pragma unroll
    for (uint32_t p = 0; p < kTlDigits; ++p) tl_hist_add(s_h + p * 256, tl_digit(it, p), valid, lane);
  }
  __syncthreads();
  for (uint32_t k = t; k < kTlDigits * 256; k += 256)
    if (s_h[k]) atomicAdd(reinterpret_cast<unsigned long long*>(dhist + k), (unsigned long long)s_h[k]);
}

// One radix pass, 1: the digit counts of block b's kTlSortBlock items -> bcnt[d * nb + b].
__global__ __launch_bounds__(256) void k_tl_bcount(const TlItem* __restrict__ items, uint64_t n, uint32_t p,
                                                   uint32_t* __restrict__ bcnt, uint32_t nb) {
  __shared__ uint32_t s_h[256];
  const int t = threadIdx.x, lane = t & 63;
  s_h[t] = 0;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * kTlSortBlock;
  for (uint32_t r = 0; r < kTlSortBlock / 256; ++r) {
    const uint64_t i = i0 + r * 256 + t;
    const bool valid = i < n;
    TlItem it{};
    if (valid) it = items[i];
    tl_hist_add(s_h, tl_digit(it, p), valid, lane);
  }
  __syncthreads();
  bcnt[(size_t)t * nb + blockIdx.x] = s_h[t];
}

// 2: block d turns digit d's row of block counts into the blocks' first output positions: the
// items of smaller digits (the digit histogram k_tl_digits made) + the row's exclusive prefix.
__global__ __launch_bounds__(256) void k_tl_bscan(uint32_t* __restrict__ bcnt, uint32_t nb,
                                                  const uint64_t* __restrict__ dh) {
  __shared__ uint64_t s_w64[4];
  __shared__ uint32_t s_w[4];
  const int t = threadIdx.x;
  const uint32_t d = blockIdx.x;
  uint32_t carry = (uint32_t)block_sum_u64((uint32_t)t < d ? dh[t] : 0ull, s_w64);  // (< n < 2^32)
  uint32_t* row = bcnt + (size_t)d * nb;
  for (uint32_t b0 = 0; b0 < nb; b0 += 256) {
    const uint32_t i = b0 + t;
    const uint32_t x = i < nb ? row[i] : 0u;
    uint32_t tot;
    const uint32_t incl = block_incl_scan_u32(x, s_w, &tot);
    if (i < nb) row[i] = carry + incl - x;
    carry += tot;
  }
}

// 3: the stable scatter.  Rounds of 256 items in order; within a round an item's place among
// those of its digit = the round's items of earlier waves (per-wave LDS counts, prefixed in wave
// order) + the earlier lanes of its own wave (the peer mask of 8 ballots).
__global__ __launch_bounds__(256) void k_tl_scatter(const TlItem* __restrict__ src, TlItem* __restrict__ dst,
                                                    uint64_t n, uint32_t p, const uint32_t* __restrict__ bcnt,
                                                    uint32_t nb) {
  __shared__ uint32_t s_base[256], s_wc[4][256];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  s_base[t] = bcnt[(size_t)t * nb + blockIdx.x];
#pragma unroll
  for (int k = 0; k < 4; ++k) s_wc[k][t] = 0;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * kTlSortBlock;
  for (uint32_t r = 0; r < kTlSortBlock / 256; ++r) {
    const uint64_t i = i0 + r * 256 + t;
    const bool valid = i < n;
    TlItem it{};
    if (valid) it = src[i];
    const uint32_t d = tl_digit(it, p);
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (uint32_t bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const uint64_t bal = __ballot(valid && on);
      peers &= on ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) s_wc[wv][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t pos = s_base[d] + rank;
      for (int k = 0; k < wv; ++k) pos += s_wc[k][d];
      if (pos < n) dst[pos] = it;  // (always: the offsets partition [0, n))
    }
    __syncthreads();
    s_base[t] += s_wc[0][t] + s_wc[1][t] + s_wc[2][t] + s_wc[3][t];
#pragma unroll
    for (int k = 0; k < 4; ++k) s_wc[k][t] = 0;
    __syncthreads();
  }
}

// What the entry of one sorted item copies: `len` bytes from batch offset `src` behind its
// stream's tag, and a '\n' when the line is its stream's unterminated fragment.
struct TlGeom {
  uint64_t src, line;
  uint32_t len, seg, tag_off, tag_len, nl;
};
__device__ __forceinline__ TlGeom tl_geom(const TlArgs& g, const TlItem& it) {
  TlGeom q{};
  if (it.ord >= g.n) return q;  // (never: the sort permutes k_tl_keys' items)
  const TlSide sd = g.side[it.ord];
  const uint32_t s = sd.seg;
  const uint64_t l = sd.line;
  if (s >= g.v.nsegs || l >= g.v.cap_lines) return q;
  const SegDesc seg = g.v.segs[s];
  const uint64_t ls = g.v.line_off[l + s], le = g.v.line_off[l + s + 1];
  const uint32_t plen = g.timestamps ? 0u : line_plen(g, g.v.meta[l], g.v.bytes + seg.base, ls, le);
  q.src = seg.base + ls + plen;
  q.len = (uint32_t)(le - ls - plen);
  q.line = l - g.v.segout[s].line_lo;
  q.seg = s;
  q.tag_off = g.tags ? g.segtab[3 * s + 1] : 0u;
  q.tag_len = g.tags ? g.segtab[3 * s + 2] : 0u;
  q.nl = (le == seg.len && g.v.segout[s].frag) ? 1u : 0u;
  return q;
}

__global__ __launch_bounds__(256) void k_tl_plan(TlArgs g, const TlItem* __restrict__ items) {
  __shared__ uint64_t s_w64[4];
  const uint64_t i = (uint64_t)blockIdx.x * kTlPlanBlock + threadIdx.x;
  uint64_t len = 0;
  if (i < g.n) {
    const TlGeom q = tl_geom(g, items[i]);
    len = (uint64_t)q.tag_len + q.len + q.nl;
  }
  len = block_sum_u64(len, s_w64);
  if (threadIdx.x == 0) g.psum[blockIdx.x] = len;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t x, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src, 64);
  return (uint64_t)hi << 32 | lo;
}

// n bytes from src to dst over the wave's lanes: dwords at the destination's alignment (the
// source dword through gword, which reads at most 4 bytes past the last one it needs), bytes
// at both ends and for short copies.
__device__ __forceinline__ void wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n,
                                          int lane) {
  uint32_t head = (uint32_t)(-reinterpret_cast<intptr_t>(dst)) & 3u;
  if (n < 128 || head > n) head = n;
  for (uint32_t k = lane; k < head; k += 64) dst[k] = src[k];
  const uint32_t nd = (n - head) >> 2;
  uint32_t* d4 = reinterpret_cast<uint32_t*>(dst + head);
  for (uint32_t k = lane; k < nd; k += 64) d4[k] = gword(src + head + 4 * k);
  for (uint32_t k = head + 4 * nd + lane; k < n; k += 64) dst[k] = src[k];
}

// Offsets (in-block scan + the block's base), the entry records, and the gather copy: a wave
// renders its 64 entries one after the other, each spread over its lanes.
__global__ __launch_bounds__(256) void k_tl_copy(TlArgs g, const TlItem* __restrict__ items) {
  __shared__ uint64_t s_w[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * kTlPlanBlock + t;
  TlGeom q{};
  TlItem it{};
  uint64_t len = 0;
  if (i < g.n) {
    it = items[i];
    q = tl_geom(g, it);
    len = (uint64_t)q.tag_len + q.len + q.nl;
  }
  const uint64_t incl = wave_incl_scan_add(len, lane);
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  uint64_t off = g.psum[blockIdx.x] + incl - len;
  for (int k = 0; k < wv; ++k) off += s_w[k];
  if (i < g.n)
    g.entries[i] = TlEntry{(int64_t)(it.sec_key ^ (1ull << 63)), (int32_t)it.nsec, g.segtab[3 * q.seg], q.line, off};
  const uint64_t w0 = (uint64_t)blockIdx.x * kTlPlanBlock + (uint64_t)wv * 64;
  const uint32_t nv = w0 >= g.n ? 0u : (g.n - w0 < 64 ? (uint32_t)(g.n - w0) : 64u);  // (wave-uniform)
  for (uint32_t j = 0; j < nv; ++j) {
    const uint64_t o = shfl64(off, (int)j), src = shfl64(q.src, (int)j);
    const uint32_t n = (uint32_t)__shfl((int)q.len, (int)j, 64), to = (uint32_t)__shfl((int)q.tag_off, (int)j, 64),
                   tl = (uint32_t)__shfl((int)q.tag_len, (int)j, 64), nl = (uint32_t)__shfl((int)q.nl, (int)j, 64);
    for (uint32_t k = lane; k < tl; k += 64) g.out[o + k] = g.tags[to + k];
    wave_copy(g.out + o + tl, g.v.bytes + src, n, lane);
    if (nl && lane == 0) g.out[o + tl + n] = (uint8_t)'\n';
  }
}

// ========================================= grouped counts (klf_result_groups, SPEC.md S4e) ==
// The lines of H grouped by key.  k_gr_insert is the selected-line walk over H, one lane per
// line: the lane runs the normaliser (klf_groupkey.hpp) over its content, 16 bytes a load, folds
// the key bytes into a 64-bit hash and probes the open-addressing table from hash & (P - 1).
// A free slot is claimed with atomicCAS (the word then names this line as the group's
// representative); a slot whose tag is the lane's is settled by comparing the two keys byte
// for byte, both normalised on the fly from the batch.  The hash only chooses where to look:
// groups are exactly the classes of byte-equal keys, for any hash.  The 64 lines of a round
// often share a group, so neighbouring lanes that found one slot add once (k_hist's ballot of
// run heads).  A lane that finds no slot in P probes sets the table-full flag and goes on.

// The content bytes a line's key is made from: S1's content without its '\n', cut to max_key.
struct GrLine {
  const uint8_t* p;
  uint64_t n;
};
// S1's content of line l (of segment s) without its terminating '\n'.
__device__ __forceinline__ GrLine sel_content(const SelView& v, uint64_t l, uint32_t s) {
  const SegDesc sd = v.segs[s];
  const uint64_t ls = v.line_off[l + s], le = v.line_off[l + s + 1];
  const uint8_t* segp = v.bytes + sd.base;
  const uint32_t plen = line_plen(v, v.meta[l], segp, ls, le);
  uint64_t n = le - ls - plen;
  if (n && !(le == sd.len && v.segout[s].frag)) --n;  // the terminating '\n'
  return {segp + ls + plen, n};
}
__device__ __forceinline__ GrLine gr_line(const GroupArgs& g, uint64_t l, uint32_t s) {
  const GrLine q = sel_content(g.v, l, s);
  return {q.p, group_key_span(q.n, g.max_key)};
}
// The key bytes of a line, one after the other.  A 16-B load may reach 15 bytes past the span:
// into the next line, the next stream or the allocation's slack (kAllocSlack), never used.
struct GrCursor {
  const uint8_t* p;
  uint64_t n, pos, lo, hi;
  GroupKeyNorm nm;
  __device__ __forceinline__ GrCursor(const GrLine& q, uint32_t flags) : p(q.p), n(q.n), pos(0), lo(0), hi(0), nm(flags) {}
  __device__ __forceinline__ int next() {  // -1: the key has ended
    while (pos < n) {
      const uint32_t k = (uint32_t)pos & 15u;
      if (k == 0) {
        typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
        u64x2 x;
        __builtin_memcpy(&x, p + pos, 16);
        lo = x.x;
        hi = x.y;
      }
      const uint8_t c = (uint8_t)(k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)));
      ++pos;
      uint8_t out;
      if (nm.step(c, out)) return (int)out;
    }
    return -1;
  }
};
__device__ __forceinline__ uint64_t gr_mix(uint64_t h, uint64_t x) {
  h = (h ^ x) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
// The key's hash: 8 key bytes a step, then the key length.
__device__ __forceinline__ uint64_t gr_hash(const GrLine& q, uint32_t flags) {
  GrCursor cur(q, flags);
  uint64_t h = 0x243F6A8885A308D3ull, acc = 0, len = 0;
  uint32_t na = 0;
  for (int c; (c = cur.next()) >= 0;) {
    acc |= (uint64_t)(uint32_t)c << (8 * na);
    ++len;
    if (++na == 8) {
      h = gr_mix(h, acc);
      acc = 0;
      na = 0;
    }
  }
  h = gr_mix(gr_mix(h, acc), len);
  return h ^ (h >> 32);
}
__device__ __forceinline__ bool gr_keys_equal(const GrLine& a, const GrLine& b, uint32_t flags) {
  GrCursor ca(a, flags), cb(b, flags);
  for (;;) {
    const int x = ca.next(), y = cb.next();
    if (x != y) return false;
    if (x < 0) return true;
  }
}
__device__ __forceinline__ uint64_t* gr_slots(const GroupArgs& g) { return g.table; }
__device__ __forceinline__ uint64_t* gr_count(const GroupArgs& g) { return g.table + (1ull << g.table_log2); }
__device__ __forceinline__ uint64_t* gr_nfirst(const GroupArgs& g) { return g.table + (2ull << g.table_log2); }
__device__ __forceinline__ uint64_t* gr_last(const GroupArgs& g) { return g.table + (3ull << g.table_log2); }
__device__ __forceinline__ uint64_t* gr_stats(const GroupArgs& g) { return g.table + (4ull << g.table_log2); }
constexpr uint64_t kGrLineMask = (1ull << kGrLineBits) - 1ull;

// The slot of line l's group (l of segment s), claimed if the key is new; ~0: the table is full.
__device__ __forceinline__ uint64_t gr_find_slot(const GroupArgs& g, uint64_t l, uint32_t s) {
  const uint64_t pmask = (1ull << g.table_log2) - 1ull;
  const GrLine me = gr_line(g, l, s);
  uint64_t h = gr_hash(me, g.flags);
  if (g.hash_bits < 64) h &= (1ull << g.hash_bits) - 1ull;
  const uint64_t tag = h >> kGrLineBits, mine = tag << kGrLineBits | (l + 1);
  uint64_t* slots = gr_slots(g);
  uint64_t i = h & pmask;
  for (uint64_t probe = 0; probe <= pmask; ++probe, i = (i + 1) & pmask) {
    uint64_t wd = __hip_atomic_load(slots + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wd == 0) {
      wd = atomicCAS(reinterpret_cast<unsigned long long*>(slots + i), 0ull, (unsigned long long)mine);
      if (wd == 0) return i;
    }
    if (wd >> kGrLineBits != tag) continue;
    const uint64_t rep = (wd & kGrLineMask) - 1;
    if (rep >= g.v.cap_lines) continue;  // (never: slot words are written here alone)
    if (gr_keys_equal(me, gr_line(g, rep, find_seg_by_line(g.v.segout, g.v.nsegs, rep)), g.flags)) return i;
  }
  return ~0ull;
}

__device__ __forceinline__ uint64_t shfl64_up1(uint64_t x) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, 1, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), 1, 64);
  return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(256) void k_gr_insert(GroupArgs g) {
  __shared__ WalkLds ws;
  const int t = threadIdx.x, lane = t & 63;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    const uint32_t total = walk_publish(ws, g.v, view_word(g.v, w, L), l0);
    __syncthreads();
    if (lane == 0 && total) atomicAdd(reinterpret_cast<unsigned long long*>(gr_stats(g)), (unsigned long long)total);
    walk_rounds(ws, g.v, total, l0, [&](const WalkLine& q) {
      const uint64_t line = q.live ? q.l : 0ull;
      const uint64_t slot = q.live ? gr_find_slot(g, line, q.s) : ~0ull;  // ~0: no line, or no slot for it
      if (q.live && slot == ~0ull) atomicOr(reinterpret_cast<unsigned long long*>(gr_stats(g) + 1), 1ull);
      // a run of lanes with one slot: its head adds the run's length, its own line (the run's
      // lowest) and the run's last line (lines ascend with the lane)
      const uint64_t prev = shfl64_up1(slot);
      const bool head = lane == 0 || slot != prev;
      const uint64_t heads = __ballot(head);
      const uint64_t after = lane == 63 ? 0ull : heads >> (lane + 1);  // the heads behind this lane
      const uint32_t run = after ? (uint32_t)__ffsll((long long)after) : 64u - (uint32_t)lane;
      const uint64_t tail_line = shfl64(line, lane + (int)run - 1);
      if (head && slot != ~0ull) {
        atomicAdd(reinterpret_cast<unsigned long long*>(gr_count(g) + slot), (unsigned long long)run);
        atomicMax(reinterpret_cast<unsigned long long*>(gr_nfirst(g) + slot), (unsigned long long)~line);
        atomicMax(reinterpret_cast<unsigned long long*>(gr_last(g) + slot), (unsigned long long)tail_line);
      }
    });
  }
}

// Thread t of block b owns the slots b * kGrCountBlock + 8 t .. + 7.
__device__ __forceinline__ uint32_t gr_occupied8(const GroupArgs& g, uint64_t j0) {
  const uint64_t P = 1ull << g.table_log2;
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k)
    if (j0 + k < P && gr_slots(g)[j0 + k]) m |= 1u << k;
  return m;
}
__global__ __launch_bounds__(256) void k_gr_count(GroupArgs g) {
  __shared__ uint64_t s_w64[4];
  const uint64_t j0 = (uint64_t)blockIdx.x * kGrCountBlock + 8ull * threadIdx.x;
  const uint64_t n = block_sum_u64((uint64_t)__popc(gr_occupied8(g, j0)), s_w64);
  if (threadIdx.x == 0) g.bsum[blockIdx.x] = n;
}
// One item per occupied slot, at the block's base + its rank in the block: the sort key is
// (2^40 - 1 - count) in sec_key's upper 40 bits, then the group's lowest line (40 bits) over
// sec_key's lower 24 bits and nsec's lower 16, so ascending keys are (count desc, first asc).
__global__ __launch_bounds__(256) void k_gr_fill(GroupArgs g) {
  __shared__ uint32_t s_w[4];
  const uint64_t j0 = (uint64_t)blockIdx.x * kGrCountBlock + 8ull * threadIdx.x;
  const uint32_t m = gr_occupied8(g, j0), cnt = (uint32_t)__popc(m);
  uint32_t tot;
  uint64_t i = g.bsum[blockIdx.x] + block_incl_scan_u32(cnt, s_w, &tot) - cnt;
  for (uint32_t k = 0; k < 8; ++k) {
    if (!((m >> k) & 1u)) continue;
    const uint64_t j = j0 + k;
    if (i < g.n_groups) {  // (always: n_groups is the scan's total of the same slots)
      const uint64_t cn = gr_count(g)[j] & kGrLineMask, first = ~gr_nfirst(g)[j] & kGrLineMask;
      g.items[i] = TlItem{(kGrLineMask - cn) << 24 | first >> 16, (uint32_t)(first & 0xFFFFu), (uint32_t)i};
      g.gslot[i] = (uint32_t)j;
    }
    ++i;
  }
}

// What entry i of the result is made from: its slot and its representative line.
__device__ __forceinline__ bool gr_top_line(const GroupArgs& g, const TlItem& it, uint64_t* slot, GrLine* q) {
  if (it.ord >= g.n_groups) return false;  // (never: the sort permutes k_gr_fill's items)
  const uint64_t j = g.gslot[it.ord];
  if (j >> g.table_log2) return false;
  const uint64_t rep = (gr_slots(g)[j] & kGrLineMask) - 1;
  if (rep >= g.v.cap_lines) return false;
  *slot = j;
  *q = gr_line(g, rep, find_seg_by_line(g.v.segout, g.v.nsegs, rep));
  return true;
}
// One wave per entry walks the representative's span 64 bytes a step, a byte a lane, by the
// normaliser's rule (group_key_emits: it needs the previous byte alone): f(emit, key byte, its
// position in the key) on every lane of every step; returns the key's length.  Byte loads inside
// the span only.
template <class F>
__device__ __forceinline__ uint64_t gr_wave_key(const GrLine& q, uint32_t flags, int lane, F&& f) {
  uint64_t written = 0;
  int carry = 0;  // the previous step's last byte was a digit
  for (uint64_t base = 0; base < q.n; base += 64) {
    const bool live = base + lane < q.n;
    const uint8_t c = live ? q.p[base + lane] : (uint8_t)0;
    const int dig = live && group_key_digit(c) ? 1 : 0;
    const int up = __shfl_up(dig, 1, 64);
    uint8_t out = 0;
    const bool emit = live && group_key_emits(flags, (lane == 0 ? carry : up) != 0, c, out);
    const uint64_t m = __ballot(emit);
    f(emit, out, written + (uint64_t)__popcll(m & ((1ull << lane) - 1ull)));
    written += (uint64_t)__popcll(m);
    carry = __shfl(dig, 63, 64);
  }
  return written;
}
__global__ __launch_bounds__(256) void k_gr_plan(GroupArgs g, const TlItem* __restrict__ sorted) {
  const int lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);  // (wave-uniform)
  if (i >= g.top) return;
  uint64_t j, len = 0;
  GrLine q;
  if (gr_top_line(g, sorted[i], &j, &q)) len = gr_wave_key(q, g.flags, lane, [](bool, uint8_t, uint64_t) {});
  if (lane == 0) g.klen[i] = len;
}
// The entry record (lane 0), then the key bytes by the same walk.
__global__ __launch_bounds__(256) void k_gr_render(GroupArgs g, const TlItem* __restrict__ sorted) {
  const int lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);  // (wave-uniform)
  if (i >= g.top) return;
  const TlItem it = sorted[i];
  const uint64_t off = g.klen[i], len = g.klen[i + 1] - off;
  uint64_t j;
  GrLine q;
  GrEntry e{};
  e.key_off = off;
  if (gr_top_line(g, it, &j, &q)) {
    const uint64_t first = ((it.sec_key & 0xFFFFFFull) << 16 | (it.nsec & 0xFFFFu)), last = gr_last(g)[j];
    const uint32_t fs = find_seg_by_line(g.v.segout, g.v.nsegs, first), ls = find_seg_by_line(g.v.segout, g.v.nsegs, last);
    e.count = kGrLineMask - (it.sec_key >> 24);
    e.first_line = first - g.v.segout[fs].line_lo;
    e.last_line = last - g.v.segout[ls].line_lo;
    e.first_stream = g.segstream[fs];
    e.last_stream = g.segstream[ls];
    e.key_len = (uint32_t)len;
    gr_wave_key(q, g.flags, lane, [&](bool emit, uint8_t c, uint64_t k) {
      if (emit && k < len) g.keys[off + k] = c;  // (k < len always: the plan walked the same bytes)
    });
  }
  if (lane == 0) g.entries[i] = e;
}

// ================================ numeric field statistics (klf_result_field_stats, SPEC.md S4f) ==
// k_fs_extract is the selected-line walk over H, one lane per line: the lane runs the extractor of
// klf_fieldval.hpp over its content and leaves the line's value and class at the line's rank in H.
// The hits then become sort items keyed by (segment, value); after the value digits of the
// timeline's radix passes the items are in value order (the all-streams row), after the segment
// digits in (segment, value) order (the segments' rows): k_fs_rows reads minimum, maximum and the
// quantile ranks straight out of the sorted items.

// The content's bytes through 16-B loads at multiples of 16 from its start.  A load may reach 15
// bytes past the content: into the next line, the next stream or the allocation's slack
// (kAllocSlack); at(i) is only asked for i inside the content, so none of them is ever looked at.
struct FsBytes {
  const uint8_t* p;
  uint64_t blk, lo, hi;
  __device__ __forceinline__ explicit FsBytes(const uint8_t* q) : p(q), blk(~0ull), lo(0), hi(0) {}
  __device__ __forceinline__ uint8_t at(uint64_t i) {
    const uint64_t b = i >> 4;
    if (b != blk) {
      typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
      u64x2 x;
      __builtin_memcpy(&x, p + (b << 4), 16);
      lo = x.x;
      hi = x.y;
      blk = b;
    }
    const uint32_t k = (uint32_t)i & 15u;
    return (uint8_t)(k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)));
  }
};

__device__ __forceinline__ void fs_add(uint64_t* p, uint64_t x) {
  if (x) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)x);
}

// A wave's counts and sums over a run of lines of one segment: lines / hits / bad are wave-uniform
// (ballot popcounts), the two halves of the sum are per lane until flush() adds them all, once.
struct FsAcc {
  uint32_t seg;  // ~0: none
  uint32_t lines, hits, bad;
  uint64_t hi, lo;
  __device__ __forceinline__ void flush(const FieldArgs& g, int lane) {  // (every lane of the wave calls it)
    if (seg != ~0u) {
      const uint64_t h = wave_sum(hi), l = wave_sum(lo);
      if (lane == 0) {
        const uint64_t ns = g.v.nsegs;
        fs_add(g.tab + seg, lines);
        fs_add(g.tab + ns + seg, hits);
        fs_add(g.tab + 2 * ns + seg, bad);
        fs_add(g.tab + 3 * ns + seg, h);
        fs_add(g.tab + 4 * ns + seg, l);
      }
    }
    seg = ~0u;
    lines = hits = bad = 0;
    hi = lo = 0;
  }
};

__global__ __launch_bounds__(256) void k_fs_extract(FieldArgs g) {
  __shared__ WalkLds ws;
  __shared__ uint32_t s_tot[4], s_hits[4];
  __shared__ uint8_t s_key[kFsMaxKey];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < (int)kFsMaxKey) s_key[t] = g.key[t];
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  const uint64_t ns = g.v.nsegs;
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    const uint32_t total = walk_publish(ws, g.v, view_word(g.v, w, L), l0);  // (its barrier: the last chunk's s_hits is read)
    if (lane == 0) s_tot[wv] = total;
    __syncthreads();  // (s_key too)
    uint64_t base = g.cbase[c];
    for (int k = 0; k < wv; ++k) base += s_tot[k];
    FsAcc acc;
    acc.seg = ~0u;
    acc.flush(g, lane);
    uint32_t chunk_hits = 0;
    walk_rounds(ws, g.v, total, l0, [&](const WalkLine& q) {
      int cls = kFieldMiss;
      int64_t v = 0;
      if (q.live) {
        const GrLine ln = sel_content(g.v, q.l, q.s);
        FsBytes src(ln.p);
        cls = field_classify(src, ln.n, s_key, g.key_len, g.decimals, g.flags, &v);
        if (cls != kFieldHit) v = 0;
        const uint64_t rank = base + q.k;
        if (rank < g.n) {  // (always: n is the scan's total of the same words)
          g.val[rank] = v;
          g.cs[rank] = q.s << 2 | (uint32_t)cls;
        }
      }
      const bool is_hit = q.live && cls == kFieldHit, is_bad = q.live && cls == kFieldBad;
      const uint64_t live = __ballot(q.live), hit = __ballot(is_hit), bad = __ballot(is_bad);
      chunk_hits += (uint32_t)__popcll(hit);
      // (lane 0 has a line in every round)
      const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(q.live ? q.s : 0u));
      const uint32_t s = q.live ? q.s : s0;
      if (__all(s == s0)) {  // one segment: into the wave's run
        if (acc.seg != s0) {
          acc.flush(g, lane);
          acc.seg = s0;
        }
        acc.lines += (uint32_t)__popcll(live);
        acc.hits += (uint32_t)__popcll(hit);
        acc.bad += (uint32_t)__popcll(bad);
        if (is_hit) {
          acc.hi += (uint64_t)(v >> 32);
          acc.lo += (uint64_t)v & 0xFFFFFFFFull;
        }
      } else {  // a round over several (small) streams: a line at a time
        acc.flush(g, lane);
        if (q.live) {
          fs_add(g.tab + s, 1);
          fs_add(g.tab + ns + s, is_hit ? 1 : 0);
          fs_add(g.tab + 2 * ns + s, is_bad ? 1 : 0);
          if (is_hit) {
            fs_add(g.tab + 3 * ns + s, (uint64_t)(v >> 32));
            fs_add(g.tab + 4 * ns + s, (uint64_t)v & 0xFFFFFFFFull);
          }
        }
      }
    });
    acc.flush(g, lane);
    if (lane == 0) s_hits[wv] = chunk_hits;
    __syncthreads();
    if (t == 0) g.hbase[c] = (uint64_t)s_hits[0] + s_hits[1] + s_hits[2] + s_hits[3];
  }
}

// The segments' hits beside the table, for their prefix.
__global__ __launch_bounds__(256) void k_fs_hcopy(FieldArgs g) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s < g.v.nsegs) g.hpre[s] = g.tab[(uint64_t)g.v.nsegs + s];
}

// One item per hit, at the chunk's hit base + its place among the chunk's hits: the ranks of
// chunk c are [cbase[c], cbase[c + 1]).  Key: nsec = the low half of v ^ 2^63, sec_key = its high
// half under the segment, so the digits 0..7 order by value and 8..11 by segment.
__global__ __launch_bounds__(256) void k_fs_compact(FieldArgs g) {
  __shared__ uint32_t s_w[4];
  const int t = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t r0 = g.cbase[c], r1 = g.cbase[c + 1];
    uint64_t out = g.hbase[c];
    for (uint64_t rb = r0; rb < r1; rb += 256) {  // (block-uniform)
      const uint64_t rank = rb + t;
      const bool valid = rank < r1 && rank < g.n;
      const uint32_t x = valid ? g.cs[rank] : (uint32_t)kFieldMiss;
      const uint32_t hit = (x & 3u) == (uint32_t)kFieldHit ? 1u : 0u;
      uint32_t tot;
      const uint32_t incl = block_incl_scan_u32(hit, s_w, &tot);
      const uint64_t pos = out + incl - 1;
      if (hit && pos < g.n_hits) {  // (always: n_hits is the scan's total of the same hits)
        const uint64_t u = (uint64_t)g.val[rank] ^ (1ull << 63);
        g.items[pos] = TlItem{(uint64_t)(x >> 2) << 32 | u >> 32, (uint32_t)u, (uint32_t)rank};
      }
      out += tot;
    }
  }
}

__device__ __forceinline__ int64_t fs_item_value(const TlItem& it) {
  return (int64_t)(((it.sec_key & 0xFFFFFFFFull) << 32 | it.nsec) ^ (1ull << 63));
}
// The global line of rank `rank` of H: its chunk by the chunk bases, then the chunk's words.
__device__ uint64_t fs_rank_line(const FieldArgs& g, uint64_t rank, uint64_t L) {
  uint64_t lo = 0, hi = g.v.nchunks;  // the last chunk whose base is <= rank (a chunk without lines shares the next one's)
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (g.cbase[mid] <= rank) lo = mid; else hi = mid;
  }
  uint64_t r = rank - g.cbase[lo];
  for (uint32_t k = 0; k < kMatchChunk / 32; ++k) {
    const uint64_t w = lo * (kMatchChunk / 32) + k;
    const uint32_t x = view_word(g.v, w, L), cnt = (uint32_t)__popc(x);
    if (r < cnt) return w * 32 + nth_set_bit(x, (uint32_t)r);
    r -= cnt;
  }
  return ~0ull;  // (never: rank < n)
}

// One block per row; its hits are sorted[a .. b) in value order.  Thread j < n_q: quantile j by
// nearest rank; thread n_q: the minimum and its line (the range's first item: equal values keep
// their rank order); thread n_q + 1: the maximum and the first item of its run of equal values.
__global__ __launch_bounds__(64) void k_fs_rows(FieldArgs g, const TlItem* __restrict__ sorted, uint32_t all) {
  const uint32_t row = all ? g.v.nsegs : blockIdx.x, j = threadIdx.x;
  const uint64_t a = all ? 0ull : g.hpre[row], b = all ? g.n_hits : g.hpre[row + 1];
  const uint64_t n = b > a && b <= g.n_hits ? b - a : 0ull;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  if (j < g.n_q) {
    int64_t x = 0;
    if (n) {
      const uint64_t k = ((uint64_t)g.q[j] * n + 9999ull) / 10000ull;  // ceil(q n / 10000) <= n
      x = fs_item_value(sorted[a + (k ? k - 1 : 0)]);
    }
    g.qv[(uint64_t)row * g.n_q + j] = x;
  } else if (j == g.n_q || j == g.n_q + 1) {
    const bool is_max = j != g.n_q;
    int64_t x = 0;
    uint64_t line = ~0ull;
    uint32_t seg = ~0u;
    if (n) {
      uint64_t i = a;
      if (is_max) {
        x = fs_item_value(sorted[b - 1]);
        uint64_t lo = a, hi = b - 1;  // the lowest i with value(i) >= x
        while (lo < hi) {
          const uint64_t mid = (lo + hi) >> 1;
          if (fs_item_value(sorted[mid]) >= x) hi = mid; else lo = mid + 1;
        }
        i = lo;
      } else {
        x = fs_item_value(sorted[a]);
      }
      const uint64_t rank = sorted[i].ord;
      const uint64_t l = rank < g.n ? fs_rank_line(g, rank, L) : ~0ull;
      if (l < L) {
        seg = find_seg_by_line(g.v.segout, g.v.nsegs, l);
        line = l - g.v.segout[seg].line_lo;
      }
    }
    FsRow* r = g.rows + row;
    if (is_max) {
      r->max = x;
      r->max_line = line;
      r->max_seg = seg;
    } else {
      r->min = x;
      r->min_line = line;
      r->min_seg = seg;
    }
  }
}

// ================================ time context across streams (klf_around, SPEC.md S4g) ==
// G' = the parsed lines of any stream whose instant lies in [ts(a) - before, ts(a) + after] for
// some anchor a, a line of M of any stream.  The anchors' instants (k_tl_count<false> /
// k_tl_keys<false> over M) are sorted by the shared sort, then
//   k_ar_heads / k_tl_scan    anchor i opens an interval iff it is the first or its gap to anchor
//                             i - 1 exceeds before + after; heads per kArBlock anchors, their
//                             prefix -> K
//   k_ar_emit                 one record per interval: the head writes the lower end, the last
//                             anchor before the next head the upper end
//   k_ar_build                the selected-line walk over the parsed lines, shaped like k_tw_build:
//                             a binary search for the last interval whose lower end is <= ts
// All arithmetic is on (sec, nsec) pairs with a carry or borrow: the years 0000 and 9999 do not
// fit one 64-bit nanosecond count.  No kernel waits on another block.

// Sorted neighbours prev <= it: the gap between them exceeds the span before + after.
__device__ __forceinline__ bool ar_head(const ArArgs& g, const TlItem& prev, const TlItem& it) {
  uint64_t ds = it.sec_key - prev.sec_key;
  int64_t dn = (int64_t)it.nsec - (int64_t)prev.nsec;
  if (dn < 0) {  // (then ds >= 1: the items are sorted)
    dn += 1000000000;
    ds -= 1;
  }
  return ds > g.span_sec || (ds == g.span_sec && (uint32_t)dn > g.span_nsec);
}
// Bit k: the thread's k-th anchor i0 + k (< n) opens an interval.
__device__ __forceinline__ uint32_t ar_head_mask(const ArArgs& g, uint64_t i0) {
  uint32_t m = 0;
  if (i0 >= g.n) return m;
  TlItem prev = g.sorted[i0 ? i0 - 1 : 0];
  for (uint32_t k = 0; k < kArPer && i0 + k < g.n; ++k) {
    const TlItem it = g.sorted[i0 + k];
    if (i0 + k == 0 || ar_head(g, prev, it)) m |= 1u << k;
    prev = it;
  }
  return m;
}

__global__ __launch_bounds__(256) void k_ar_heads(ArArgs g) {
  __shared__ uint32_t s_w[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t cnt = wave_sum((uint32_t)__popc(ar_head_mask(g, (uint64_t)blockIdx.x * kArBlock + (uint64_t)t * kArPer)));
  if (lane == 0) s_w[wv] = cnt;
  __syncthreads();
  if (t == 0) g.bsum[blockIdx.x] = (uint64_t)s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(256) void k_ar_emit(ArArgs g) {
  __shared__ uint32_t s_w[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t i0 = (uint64_t)blockIdx.x * kArBlock + (uint64_t)t * kArPer;
  const uint32_t mask = ar_head_mask(g, i0), cnt = (uint32_t)__popc(mask);
  const uint32_t incl = wave_incl_scan_add(cnt, lane);
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  uint64_t idx = g.bsum[blockIdx.x] + (incl - cnt);  // the heads ahead of anchor i0
  for (int k = 0; k < wv; ++k) idx += s_w[k];
  for (uint32_t k = 0; k < kArPer && i0 + k < g.n; ++k) {
    const uint64_t i = i0 + k;
    const TlItem it = g.sorted[i];
    const int64_t sec = (int64_t)(it.sec_key ^ (1ull << 63));
    if (mask >> k & 1u) ++idx;
    if (idx == 0 || idx > g.k) continue;  // (never: anchor 0 is a head, K is the scan's total of the same flags)
    ArIval& iv = g.iv[idx - 1];
    if (mask >> k & 1u) {
      int64_t s = sec - (int64_t)g.before_sec;
      int32_t ns = (int32_t)it.nsec - (int32_t)g.before_nsec;
      if (ns < 0) {
        ns += 1000000000;
        s -= 1;
      }
      iv.lo_sec = s;
      iv.lo_nsec = ns;
    }
    const bool last = i + 1 == g.n || (k + 1 < kArPer ? (mask >> (k + 1) & 1u) != 0 : ar_head(g, it, g.sorted[i + 1]));
    if (last) {
      int64_t s = sec + (int64_t)g.after_sec;
      int32_t ns = (int32_t)it.nsec + (int32_t)g.after_nsec;
      if (ns >= 1000000000) {
        ns -= 1000000000;
        s += 1;
      }
      iv.hi_sec = s;
      iv.hi_nsec = ns;
    }
  }
}

// The line at segp + off has an instant inside one of the K >= 1 intervals.  The search keeps
// [lo, lo + len) inside [0, K): it reads neither index -1 nor K.
__device__ __forceinline__ bool ar_line_in(const ArArgs& g, const uint8_t* __restrict__ segp, uint64_t off,
                                           uint64_t seg_len) {
  int64_t sec;
  int32_t nsec;
  if (!g.k || !line_instant(segp, off, seg_len, sec, nsec)) return false;
  uint64_t lo = 0;
  for (uint64_t len = g.k; len > 1;) {
    const uint64_t half = len >> 1;
    const ArIval& m = g.iv[lo + half];
    lo = time_before(sec, nsec, m.lo_sec, m.lo_nsec) ? lo : lo + half;
    len -= half;
  }
  const ArIval iv = g.iv[lo];
  return !time_before(sec, nsec, iv.lo_sec, iv.lo_nsec) && !time_before(iv.hi_sec, iv.hi_nsec, sec, nsec);
}

__global__ __launch_bounds__(256) void k_ar_build(ArArgs g) {
  __shared__ WalkLds ws;
  __shared__ uint32_t s_out[4][64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  const uint64_t nw = g.v.cap_lines / 32 + 1;  // words of the bitmaps
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    const uint32_t total = walk_publish(ws, g.v, view_word(g.v, w, L), l0);  // (the previous chunk's s_out is read)
    s_out[wv][lane] = 0u;
    __syncthreads();
    walk_rounds(ws, g.v, total, l0, [&](const WalkLine& q) {
      if (q.live && ar_line_in(g, g.v.bytes + q.sd.base, q.off, q.sd.len)) atomicOr(&s_out[wv][q.j], 1u << q.b);
    });
    __syncthreads();
    if (w < nw) g.bits_out[w] = s_out[wv][lane];
  }
}

// ======================================== multi-line records (klf_records, SPEC.md S4h) ==
// G' = the parsed lines of every record that holds a line of M (inverted: that holds none).
// k_rc_heads is the selected-line walk over the parsed lines, one lane per line: the classifier of
// klf_recordcls.hpp over the line's content decides head or continuation, and the start bitmap
// gets a bit on every head and on every segment's first line.  The other three kernels are a
// segmented OR of M between start bits over the one sequence of all lines (klf_analysis.hpp,
// RecordArgs): the shape of k_rg_sum / k_rg_carry / k_rg_build, on two bitmaps.

// The kernel's loader for record_class: all 16 bytes of a block in one load.  It may reach 15
// bytes past the content: into the next line, the next stream or the allocation's slack
// (kAllocSlack); record_class masks them away before it compares.
struct RcDevLoad {
  __device__ __forceinline__ void operator()(const uint8_t* c, uint32_t blk, uint32_t, uint64_t& lo, uint64_t& hi) const {
    typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
    u64x2 x;
    __builtin_memcpy(&x, c + 16 * blk, 16);
    lo = x.x;
    hi = x.y;
  }
};

__global__ __launch_bounds__(256) void k_rc_heads(RecordArgs g) {
  __shared__ WalkLds ws;
  __shared__ uint32_t s_out[4][64];
  __shared__ uint64_t s_cnt[2][4];
  __shared__ RecordPrefixes s_pre;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  static_assert(sizeof(RecordPrefixes) % 4 == 0 && sizeof(RecordPrefixes) / 4 <= 256, "one word per thread");
  if (t < (int)(sizeof(RecordPrefixes) / 4))
    reinterpret_cast<uint32_t*>(&s_pre)[t] = reinterpret_cast<const uint32_t*>(&g.pre)[t];
  SelView v = g.v;
  v.bits_in = nullptr;  // the parsed lines
  const uint64_t L = v.segout[v.nsegs - 1].line_hi;
  const uint64_t nw = v.cap_lines / 32 + 1;  // words of the bitmaps
  uint64_t heads = 0, conts = 0;             // the wave's (wave-uniform)
  for (uint64_t c = blockIdx.x; c < v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    const uint32_t total = walk_publish(ws, v, view_word(v, w, L), l0);  // (the previous chunk's s_out is read)
    uint32_t first = 0;  // the first line of every non-empty segment that begins in this word
    if (l0 < L)
      for (uint32_t s = find_seg_by_line(v.segout, v.nsegs, l0); s < v.nsegs; ++s) {
        const uint64_t lo = v.segout[s].line_lo;
        if (lo >= l0 + 32) break;
        if (lo >= l0 && lo < v.segout[s].line_hi) first |= 1u << (lo - l0);
      }
    s_out[wv][lane] = first;
    __syncthreads();  // (s_pre too)
    walk_rounds(ws, v, total, l0, [&](const WalkLine& q) {
      bool head = false;
      if (q.live) {
        const GrLine ln = sel_content(v, q.l, q.s);
        head = record_class(RcDevLoad{}, ln.p, ln.n, g.flags, s_pre) == 0;
        if (head) atomicOr(&s_out[wv][q.j], 1u << q.b);
      }
      const uint32_t nl = (uint32_t)__popcll(__ballot(q.live)), nh = (uint32_t)__popcll(__ballot(head));
      heads += nh;
      conts += nl - nh;
    });
    __syncthreads();
    if (w < nw) g.start[w] = s_out[wv][lane];
  }
  if (lane == 0) { s_cnt[0][wv] = heads; s_cnt[1][wv] = conts; }
  __syncthreads();
  if (t == 0) {
    fs_add(g.counts, s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3]);
    fs_add(g.counts + 1, s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3]);
  }
}

// Word w of M and of the start bitmap (0 past the line count; neither has a bit at or past L).
__device__ __forceinline__ uint32_t rc_m_word(const RecordArgs& g, uint64_t w, uint64_t L) {
  return w * 32 >= L ? 0u : g.v.bits_in[w] & word_range_mask(w, 0, L);
}
__device__ __forceinline__ uint32_t rc_s_word(const RecordArgs& g, uint64_t w, uint64_t L) {
  return w * 32 >= L ? 0u : g.start[w] & word_range_mask(w, 0, L);
}
// The max-scan keys of a word x whose first line is l0: its last line + 1, ~(its first line); 0 = none.
__device__ __forceinline__ uint64_t rc_last_key(uint32_t x, uint64_t l0) { return x ? l0 + (31 - __clz(x)) + 1 : 0; }
__device__ __forceinline__ uint64_t rc_first_key(uint32_t x, uint64_t l0) { return x ? ~(l0 + (__ffs(x) - 1)) : 0; }

__global__ __launch_bounds__(256) void k_rc_sum(RecordArgs g) {
  __shared__ uint64_t s_w[4][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    const uint32_t m = rc_m_word(g, w, L), s = rc_s_word(g, w, L);
    uint64_t k[4] = {rc_last_key(m, l0), rc_first_key(m, l0), rc_last_key(s, l0), rc_first_key(s, l0)};
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint64_t o = __shfl_xor(k[i], d, 64);
        k[i] = k[i] > o ? k[i] : o;
      }
    __syncthreads();
    if (lane == 0)
      for (int i = 0; i < 4; ++i) s_w[i][wv] = k[i];
    __syncthreads();
    if (t < 4) {
      uint64_t a = s_w[t][0];
      for (int j = 1; j < 4; ++j) a = a > s_w[t][j] ? a : s_w[t][j];
      g.csum[8 * c + t] = a;
    }
  }
}

// Thread t owns the chunks [t K, (t + 1) K), as in k_rg_carry: their maxima, a block scan for M's
// keys and one for the start bitmap's, then each chunk's exclusive prefix / suffix.
__global__ __launch_bounds__(256) void k_rc_carry(RecordArgs g) {
  __shared__ uint64_t s_w[2][4];
  const uint64_t K = (g.v.nchunks + 255) / 256;
  const uint64_t c0 = threadIdx.x * K, c1 = c0 + K < g.v.nchunks ? c0 + K : g.v.nchunks;
  uint64_t a[4] = {0, 0, 0, 0};
  for (uint64_t c = c0; c < c1; ++c)
    for (int i = 0; i < 4; ++i) {
      const uint64_t x = g.csum[8 * c + i];
      a[i] = a[i] > x ? a[i] : x;
    }
  uint64_t pre[2], post[2];
  block_excl_scan_max64(a[0], a[1], s_w, &pre[0], &post[0]);
  block_excl_scan_max64(a[2], a[3], s_w, &pre[1], &post[1]);
  for (uint64_t c = c0; c < c1; ++c)
    for (int i = 0; i < 2; ++i) {
      g.csum[8 * c + 4 + 2 * i] = pre[i];
      const uint64_t x = g.csum[8 * c + 2 * i];
      pre[i] = pre[i] > x ? pre[i] : x;
    }
  for (uint64_t c = c1; c > c0; --c)
    for (int i = 0; i < 2; ++i) {
      g.csum[8 * (c - 1) + 5 + 2 * i] = post[i];
      const uint64_t y = g.csum[8 * (c - 1) + 1 + 2 * i];
      post[i] = post[i] > y ? post[i] : y;
    }
}

// Occluded fills of a word: every bit of x spreads upwards (UP) or downwards over the following
// lines that are not starts, so it stops ahead of a start bit going up and on one going down.
template <bool UP>
__device__ __forceinline__ uint32_t rc_fill(uint32_t x, uint32_t start) {
  // p: the bits a neighbour's flag may enter: going up a line that is no start, going down the
  // line below one that is no start
  uint32_t p = UP ? ~start : ~start >> 1;
#pragma unroll
  for (uint32_t d = 1; d < 32; d <<= 1) {
    x |= (UP ? x << d : x >> d) & p;
    p &= UP ? p << d : p >> d;
  }
  return x;
}

__global__ __launch_bounds__(256) void k_rc_build(RecordArgs g) {
  __shared__ uint64_t s_w[2][4];
  const int t = threadIdx.x;
  const uint64_t L = g.v.segout[g.v.nsegs - 1].line_hi;
  const uint64_t nw = g.v.cap_lines / 32 + 1;  // words of the bitmaps
  for (uint64_t c = blockIdx.x; c < g.v.nchunks; c += gridDim.x) {
    const uint64_t w = c * (kMatchChunk / 32) + t, l0 = w * 32;
    const uint32_t m = rc_m_word(g, w, L), s = rc_s_word(g, w, L);
    const uint32_t pw = l0 < L ? meta_word<false>(g.v.meta, w, L) : 0u;  // (no bit at or past L)
    // P + 1 of M and of the starts over the words before this one, ~N of both over the words after it
    uint64_t pm, nm, ps, ns;
    block_excl_scan_max64(rc_last_key(m, l0), rc_first_key(m, l0), s_w, &pm, &nm);
    block_excl_scan_max64(rc_last_key(s, l0), rc_first_key(s, l0), s_w, &ps, &ns);
    const uint64_t* cs = g.csum + 8 * c;
    pm = pm > cs[4] ? pm : cs[4];
    nm = nm > cs[5] ? nm : cs[5];
    ps = ps > cs[6] ? ps : cs[6];
    ns = ns > cs[7] ? ns : cs[7];
    // the record open at the first line holds a match already: the last line of M before the
    // word is at or behind the last start before it (the word's line 0 joins it unless it is a start)
    const bool left = pm != 0 && pm >= ps;
    // the record open at the last line gets one further on: ahead of the next start behind the word
    const bool right = nm > ns;
    uint32_t out = rc_fill<true>(m | (left ? ~s & 1u : 0u), s) | rc_fill<false>(m | (right ? 0x80000000u : 0u), s);
    if (g.flags & kRecordsInvert) out = ~out;
    if (w < nw) g.bits_out[w] = out & pw;
  }
}

}  // namespace

// The grid of a kernel that takes one kMatchChunk chunk per block turn: 16 blocks per CU at
// most, like k_mcount's (launch_tail_stage).
static uint32_t chunk_grid(uint64_t nchunks, int num_cus) {
  const uint64_t gmax = (uint64_t)num_cus * 16;
  return (uint32_t)(nchunks < gmax ? nchunks : gmax);
}

hipError_t launch_regroup(const RegroupArgs& g, hipStream_t st, int num_cus) {
  const uint32_t gc = chunk_grid(g.v.nchunks, num_cus);
  hipError_t e;
  if ((e = launch(k_rg_sum, dim3(gc), dim3(256), 0, st, g)) != hipSuccess) return e;
  if ((e = launch(k_rg_carry, dim3(1), dim3(256), 0, st, g)) != hipSuccess) return e;
  return launch(k_rg_build, dim3(gc), dim3(256), 0, st, g);
}

hipError_t launch_window(const WindowArgs& tw, hipStream_t st, int num_cus) {
  if (!tw.v.nchunks) return hipSuccess;
  return launch(k_tw_build, dim3(chunk_grid(tw.v.nchunks, num_cus)), dim3(256), 0, st, tw);
}

hipError_t launch_hist(const HistArgs& g, hipStream_t st, int num_cus) {
  const hipError_t e = hipMemsetAsync(g.table, 0, (size_t)g.v.nsegs * (g.n_buckets + 2) * 8, st);
  if (e != hipSuccess || !g.v.nchunks) return e;
  return launch(k_hist, dim3(chunk_grid(g.v.nchunks, num_cus)), dim3(256), 0, st, g);
}

hipError_t launch_tl_count(const SelView& v, uint64_t* cbase, bool emitted, hipStream_t st, int num_cus) {
  if (v.nchunks) {
    const dim3 grid(chunk_grid(v.nchunks, num_cus));
    const hipError_t e = emitted ? launch(k_tl_count<true>, grid, dim3(256), 0, st, v, cbase)
                                 : launch(k_tl_count<false>, grid, dim3(256), 0, st, v, cbase);
    if (e != hipSuccess) return e;
  }
  return launch(k_tl_scan, dim3(1), dim3(256), 0, st, cbase, v.nchunks);
}

hipError_t launch_sort_digits(const SortArgs& s, hipStream_t st, int num_cus) {
  hipError_t e = hipMemsetAsync(s.dhist, 0, (size_t)kTlDigits * 256 * 8, st);
  if (e != hipSuccess || !s.n) return e;
  const uint64_t nb = (s.n + 255) / 256, dmax = (uint64_t)num_cus * 8;
  return launch(k_tl_digits, dim3((uint32_t)(nb < dmax ? nb : dmax)), dim3(256), 0, st, s.items[0], s.n, s.dhist);
}

hipError_t launch_sort_pass(const SortArgs& s, uint32_t digit, uint32_t from, hipStream_t st) {
  const uint32_t nb = (uint32_t)((s.n + kTlSortBlock - 1) / kTlSortBlock);
  if (!nb || digit >= kTlDigits) return hipSuccess;
  hipError_t e;
  if ((e = launch(k_tl_bcount, dim3(nb), dim3(256), 0, st, s.items[from & 1], s.n, digit, s.bcnt, nb)) != hipSuccess)
    return e;
  if ((e = launch(k_tl_bscan, dim3(256), dim3(256), 0, st, s.bcnt, nb, s.dhist + (size_t)digit * 256)) != hipSuccess)
    return e;
  return launch(k_tl_scatter, dim3(nb), dim3(256), 0, st, s.items[from & 1], s.items[(from & 1) ^ 1], s.n, digit,
                s.bcnt, nb);
}

hipError_t launch_tl_keys(const TlArgs& g, bool emitted, hipStream_t st, int num_cus) {
  if (!g.n || !g.v.nchunks) return hipSuccess;
  const dim3 grid(chunk_grid(g.v.nchunks, num_cus));
  return emitted ? launch(k_tl_keys<true>, grid, dim3(256), 0, st, g)
                 : launch(k_tl_keys<false>, grid, dim3(256), 0, st, g);
}

hipError_t launch_ar_heads(const ArArgs& g, hipStream_t st) {
  const uint64_t nb = (g.n + kArBlock - 1) / kArBlock;
  if (nb) {
    if (hipError_t e = launch(k_ar_heads, dim3((uint32_t)nb), dim3(256), 0, st, g); e != hipSuccess) return e;
  }
  return launch(k_tl_scan, dim3(1), dim3(256), 0, st, g.bsum, nb);
}

hipError_t launch_ar_build(const ArArgs& g, hipStream_t st, int num_cus) {
  const uint64_t nb = (g.n + kArBlock - 1) / kArBlock;
  if (!nb || !g.k || !g.v.nchunks) return hipSuccess;
  if (hipError_t e = launch(k_ar_emit, dim3((uint32_t)nb), dim3(256), 0, st, g); e != hipSuccess) return e;
  return launch(k_ar_build, dim3(chunk_grid(g.v.nchunks, num_cus)), dim3(256), 0, st, g);
}

hipError_t launch_records(const RecordArgs& g, hipStream_t st, int num_cus) {
  hipError_t e = hipMemsetAsync(g.start, 0, (size_t)(g.v.cap_lines / 32 + 1) * 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(g.counts, 0, 16, st);
  if (e != hipSuccess || !g.v.nchunks) return e;
  const uint32_t gc = chunk_grid(g.v.nchunks, num_cus);
  if ((e = launch(k_rc_heads, dim3(gc), dim3(256), 0, st, g)) != hipSuccess) return e;
  if ((e = launch(k_rc_sum, dim3(gc), dim3(256), 0, st, g)) != hipSuccess) return e;
  if ((e = launch(k_rc_carry, dim3(1), dim3(256), 0, st, g)) != hipSuccess) return e;
  return launch(k_rc_build, dim3(gc), dim3(256), 0, st, g);
}

hipError_t launch_tl_plan(const TlArgs& g, uint32_t which, hipStream_t st) {
  const uint64_t nb = (g.n + kTlPlanBlock - 1) / kTlPlanBlock;
  if (nb) {
    if (hipError_t e = launch(k_tl_plan, dim3((uint32_t)nb), dim3(256), 0, st, g, g.items[which & 1]); e != hipSuccess)
      return e;
  }
  return launch(k_tl_scan, dim3(1), dim3(256), 0, st, g.psum, nb);
}

hipError_t launch_tl_copy(const TlArgs& g, uint32_t which, hipStream_t st) {
  const uint64_t nb = (g.n + kTlPlanBlock - 1) / kTlPlanBlock;
  if (!nb) return hipSuccess;
  return launch(k_tl_copy, dim3((uint32_t)nb), dim3(256), 0, st, g, g.items[which & 1]);
}

static uint32_t gr_count_blocks(const GroupArgs& g) {
  return (uint32_t)(((1ull << g.table_log2) + kGrCountBlock - 1) / kGrCountBlock);
}

hipError_t launch_gr_insert(const GroupArgs& g, hipStream_t st, int num_cus) {
  hipError_t e = hipMemsetAsync(g.table, 0, ((4ull << g.table_log2) + 2) * 8, st);
  if (e != hipSuccess || !g.v.nchunks) return e;
  return launch(k_gr_insert, dim3(chunk_grid(g.v.nchunks, num_cus)), dim3(256), 0, st, g);
}

hipError_t launch_gr_count(const GroupArgs& g, hipStream_t st) {
  const uint32_t nb = gr_count_blocks(g);
  if (hipError_t e = launch(k_gr_count, dim3(nb), dim3(256), 0, st, g); e != hipSuccess) return e;
  return launch(k_tl_scan, dim3(1), dim3(256), 0, st, g.bsum, (uint64_t)nb);
}

hipError_t launch_gr_fill(const GroupArgs& g, hipStream_t st) {
  if (!g.n_groups) return hipSuccess;
  return launch(k_gr_fill, dim3(gr_count_blocks(g)), dim3(256), 0, st, g);
}

hipError_t launch_gr_plan(const GroupArgs& g, const TlItem* sorted, hipStream_t st) {
  if (g.top) {
    if (hipError_t e = launch(k_gr_plan, dim3((g.top + 3) / 4), dim3(256), 0, st, g, sorted); e != hipSuccess) return e;
  }
  return launch(k_tl_scan, dim3(1), dim3(256), 0, st, g.klen, (uint64_t)g.top);
}

hipError_t launch_gr_render(const GroupArgs& g, const TlItem* sorted, hipStream_t st) {
  if (!g.top) return hipSuccess;
  return launch(k_gr_render, dim3((g.top + 3) / 4), dim3(256), 0, st, g, sorted);
}

hipError_t launch_fs_extract(const FieldArgs& g, hipStream_t st, int num_cus) {
  hipError_t e = hipMemsetAsync(g.tab, 0, (size_t)kFsTabRows * g.v.nsegs * 8, st);
  if (e != hipSuccess) return e;
  if (g.n && g.v.nchunks) {
    e = launch(k_fs_extract, dim3(chunk_grid(g.v.nchunks, num_cus)), dim3(256), 0, st, g);
    if (e != hipSuccess) return e;
  } else if ((e = hipMemsetAsync(g.hbase, 0, (size_t)g.v.nchunks * 8, st)) != hipSuccess) {
    return e;
  }
  if ((e = launch(k_tl_scan, dim3(1), dim3(256), 0, st, g.hbase, g.v.nchunks)) != hipSuccess) return e;
  if ((e = launch(k_fs_hcopy, dim3((g.v.nsegs + 255) / 256), dim3(256), 0, st, g)) != hipSuccess) return e;
  return launch(k_tl_scan, dim3(1), dim3(256), 0, st, g.hpre, (uint64_t)g.v.nsegs);
}

hipError_t launch_fs_compact(const FieldArgs& g, hipStream_t st, int num_cus) {
  if (!g.n_hits || !g.v.nchunks) return hipSuccess;
  return launch(k_fs_compact, dim3(chunk_grid(g.v.nchunks, num_cus)), dim3(256), 0, st, g);
}

hipError_t launch_fs_rows(const FieldArgs& g, const TlItem* sorted, uint32_t all, hipStream_t st) {
  return launch(k_fs_rows, dim3(all ? 1u : g.v.nsegs), dim3(64), 0, st, g, sorted, all);
}

}  // namespace klf
