// klf_device.hpp — the device helpers that both kernel files use: the run's (klf_kernels.hip)
// and the finished-run analyses' (klf_analysis.hip), and the host helper their launchers share.
// Everything is in klf's anonymous namespace, so each translation unit has its own copy under
// the names its kernels have always seen.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "klf_kernels.hpp"

namespace klf {
namespace {

// ------------------------------------------------------------------ small helpers ---

template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}
template <class T>
__device__ __forceinline__ T wave_incl_scan_add(T x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(x, d, 64);
    if (lane >= d) x += o;
  }
  return x;
}

// 32-bit wave scans / reductions on DPP (row_shr within 16-lane rows, then the row totals
// through v_readlane): no LDS round trips (the generic __shfl versions above lower to
// ds_bpermute, ~100 cycles each, six in a chain).  Exact-type overloads: every u32 call
// site picks these.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp0(uint32_t x) {  // lanes with no source read 0
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t wave_incl_scan_add(uint32_t x, int lane) {
  x += dpp0<0x111>(x);  // row_shr:1
  x += dpp0<0x112>(x);  // row_shr:2
  x += dpp0<0x114>(x);  // row_shr:4
  x += dpp0<0x118>(x);  // row_shr:8
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)x, 15);
  const uint32_t r1 = r0 + (uint32_t)__builtin_amdgcn_readlane((int)x, 31);
  const uint32_t r2 = r1 + (uint32_t)__builtin_amdgcn_readlane((int)x, 47);
  const int row = lane >> 4;
  return x + (row == 0 ? 0u : row == 1 ? r0 : row == 2 ? r1 : r2);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
  x += dpp0<0x111>(x);
  x += dpp0<0x112>(x);
  x += dpp0<0x114>(x);
  x += dpp0<0x118>(x);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 15) + (uint32_t)__builtin_amdgcn_readlane((int)x, 31) +
         (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
  auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
  x = mx(x, dpp0<0x111>(x));
  x = mx(x, dpp0<0x112>(x));
  x = mx(x, dpp0<0x114>(x));
  x = mx(x, dpp0<0x118>(x));
  return mx(mx((uint32_t)__builtin_amdgcn_readlane((int)x, 15), (uint32_t)__builtin_amdgcn_readlane((int)x, 31)),
            mx((uint32_t)__builtin_amdgcn_readlane((int)x, 47), (uint32_t)__builtin_amdgcn_readlane((int)x, 63)));
}

__device__ __forceinline__ uint32_t find_seg_by_line(const SegOut* so, uint32_t n, uint64_t l) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (so[mid].line_lo <= l) lo = mid; else hi = mid;
  }
  return lo;
}

// Byte source for the general timestamp parser (k_fixup): global memory, -1 past the
// end of the stream.
struct GlobalBytes {
  const uint8_t* seg;  // global stream base
  int64_t p0;          // stream offset of the line start
  int64_t seg_len;
  __device__ __forceinline__ int operator()(uint32_t i) const {
    const int64_t q = p0 + (int64_t)i;
    return q < seg_len ? (int)seg[q] : -1;
  }
};
template <class T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const T o = __shfl_xor(x, d, 64);
    x = o > x ? o : x;
  }
  return x;
}

template <class Args>  // (unread: RunArgs for the run's kernels, TlArgs for the timeline's)
__device__ __forceinline__ uint32_t line_plen(const Args& a, uint16_t meta, const uint8_t* segp,
                                              uint64_t start, uint64_t end) {
  uint32_t plen = meta >> 2;
  if (plen == kPlenEscape) {  // long prefix: find the first space again
    plen = 0;
    for (uint64_t q = start; q < end; ++q)
      if (segp[q] == ' ') { plen = (uint32_t)(q - start) + 1; break; }
  }
  return plen;
}

__device__ __forceinline__ uint32_t gword(const uint8_t* p) {  // 4 bytes at any alignment
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(p);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a0 & ~(uintptr_t)3);
  return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(a0 & 3));
}

__device__ __forceinline__ uint32_t word_range_mask(uint64_t w, uint64_t lo, uint64_t hi) {
  // bits of word w (lines 32w .. 32w+31) inside [lo, hi)
  const uint64_t l0 = w * 32;
  uint32_t m = ~0u;
  if (l0 < lo) m &= lo - l0 >= 32 ? 0u : (~0u << (lo - l0));
  if (l0 + 32 > hi) m &= hi <= l0 ? 0u : ((1u << (hi - l0)) - 1u);
  return m;
}

__device__ uint32_t block_incl_scan_u32(uint32_t x, uint32_t* s_w, uint32_t* total) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t inc = wave_incl_scan_add(x, lane);
  __syncthreads();
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  uint32_t pre = 0;
  for (int k = 0; k < wv; ++k) pre += s_w[k];
  *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  return inc + pre;
}

__device__ uint64_t block_sum_u64(uint64_t x, uint64_t* s_w) {
  const int t = threadIdx.x;
  x = wave_sum(x);
  __syncthreads();
  if ((t & 63) == 0) s_w[t >> 6] = x;
  __syncthreads();
  return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// ------------------------------------------------------------------ host: launch ---
// Launches `kernel` on `st` and returns the launch's error.
template <class K, class... Args>
hipError_t launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return hipGetLastError();
}

}  // namespace
}  // namespace klf
