// klf_recordcls.hpp — head or continuation of a multi-line record in klf_records (SPEC.md S4h),
// shared by the HIP kernels and the host (klf_record_class).  No dependencies: a stand-alone host
// program can include it.
//
// A content C (S1's content without its terminating '\n'; a '\r' stays) is a continuation by its
// bytes alone.  Default mode: C starts with ' ' or '\t' (kRecordsIndent), C is empty
// (kRecordsBlank), or C starts with one of the prefixes.  Head mode (kRecordsPrefixHead): C starts
// with none of the prefixes.  A prefix longer than C does not match, one equal to C does; the
// compare is bytewise.  Only the first kRecordsMaxPrefix bytes of C can matter, so the classifier
// works on them as four little-endian 64-bit words, the prefixes being packed the same way.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KLF_RC_HD __host__ __device__ __forceinline__
#else
#define KLF_RC_HD inline
#endif

namespace klf {

constexpr uint32_t kRecordsIndent = 1u;      // = KLF_RECORDS_INDENT
constexpr uint32_t kRecordsBlank = 2u;       // = KLF_RECORDS_BLANK
constexpr uint32_t kRecordsPrefixHead = 4u;  // = KLF_RECORDS_PREFIX_HEAD
constexpr uint32_t kRecordsInvert = 8u;      // = KLF_RECORDS_INVERT (the selection's, unread here)
constexpr uint32_t kRecordsMaxPrefixes = 8u; // = KLF_RECORDS_MAX_PREFIXES
constexpr uint32_t kRecordsMaxPrefix = 32u;  // = KLF_RECORDS_MAX_PREFIX

// The caller's prefixes, by value: prefix k is the first len[k] bytes of w[k] (byte i of the
// prefix = bits 8 (i % 8) .. of w[k][i / 8]; the bytes behind it are 0).  max_len = the longest.
struct RecordPrefixes {
  uint64_t w[kRecordsMaxPrefixes][4];
  uint32_t len[kRecordsMaxPrefixes];
  uint32_t n, max_len;
};

// Packs prefix k from its bytes (1 .. kRecordsMaxPrefix of them; k = the prefixes so far).
inline void record_prefix_add(RecordPrefixes& p, const uint8_t* bytes, uint32_t len) {
  const uint32_t k = p.n++;
  for (int j = 0; j < 4; ++j) p.w[k][j] = 0;
  for (uint32_t i = 0; i < len; ++i) p.w[k][i >> 3] |= (uint64_t)bytes[i] << (8 * (i & 7u));
  p.len[k] = len;
  if (len > p.max_len) p.max_len = len;
}

// The low `n` bytes of a word (n >= 8: all of it).
KLF_RC_HD uint64_t record_low_bytes(uint32_t n) { return n >= 8 ? ~0ull : (1ull << (8 * n)) - 1ull; }

// The host's loader: block `blk` (16 bytes) of the content at c, of which `avail` (1 .. 16) are
// inside it; only those are read.  The kernel's loader reads all 16 in one load (into the next
// line, the next stream or the allocation's slack) and record_class masks the rest away.
struct RecordHostLoad {
  inline void operator()(const uint8_t* c, uint32_t blk, uint32_t avail, uint64_t& lo, uint64_t& hi) const {
    lo = hi = 0;
    for (uint32_t i = 0; i < avail; ++i) {
      const uint64_t b = (uint64_t)c[16 * blk + i] << (8 * (i & 7u));
      if (i < 8) lo |= b; else hi |= b;
    }
  }
};

// 1: the content c[0 .. len) is a continuation, 0: a head.  At most the first min(len, 32) bytes
// are looked at: block 0 when len > 0, block 1 when len > 16 and a prefix is longer than 16.
template <class Load>
KLF_RC_HD int record_class(const Load& load, const uint8_t* c, uint64_t len, uint32_t flags, const RecordPrefixes& p) {
  const uint32_t n = len < kRecordsMaxPrefix ? (uint32_t)len : kRecordsMaxPrefix;  // the bytes that can matter
  uint64_t h[4] = {0, 0, 0, 0};
  if (n) {
    load(c, 0u, n < 16 ? n : 16u, h[0], h[1]);
    h[0] &= record_low_bytes(n);
    h[1] &= n > 8 ? record_low_bytes(n - 8) : 0ull;
  }
  if (n > 16 && p.max_len > 16) {
    load(c, 1u, n - 16, h[2], h[3]);
    h[2] &= record_low_bytes(n - 16);
    h[3] &= n > 24 ? record_low_bytes(n - 24) : 0ull;
  }
  bool starts = false;  // with one of the prefixes
  for (uint32_t k = 0; k < p.n && k < kRecordsMaxPrefixes; ++k) {
    const uint32_t pl = p.len[k];
    if (pl > n) continue;  // longer than C
    uint64_t d = (h[0] ^ p.w[k][0]) & record_low_bytes(pl);
    if (pl > 8) d |= (h[1] ^ p.w[k][1]) & record_low_bytes(pl - 8);
    if (pl > 16) d |= (h[2] ^ p.w[k][2]) & record_low_bytes(pl - 16);
    if (pl > 24) d |= (h[3] ^ p.w[k][3]) & record_low_bytes(pl - 24);
    starts = starts || d == 0;
  }
  if (flags & kRecordsPrefixHead) return starts ? 0 : 1;
  const uint8_t c0 = (uint8_t)h[0];
  const bool indent = (flags & kRecordsIndent) && n && (c0 == ' ' || c0 == '\t');
  const bool blank = (flags & kRecordsBlank) && !n;
  return (indent || blank || starts) ? 1 : 0;
}

}  // namespace klf
