// klf_groupkey.hpp — the key of a line in klf_result_groups (SPEC.md S4e), shared by the HIP
// kernels and the host (klf_group_key).
//
// The key of a content (S1's content without its terminating '\n'): its first max_key bytes
// (all of them with max_key = 0), then, with KLF_GROUPS_MASK_DIGITS, every maximal run of
// ASCII '0'..'9' in what is left replaced by the single byte '#'.  Truncation comes first:
// "ab123456" with max_key = 5 is "ab123", then "ab#".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KLF_GK_HD __host__ __device__ __forceinline__
#else
#define KLF_GK_HD inline
#endif

namespace klf {

constexpr uint32_t kGroupsMaskDigits = 1u;  // = KLF_GROUPS_MASK_DIGITS

// The content bytes the key is made from.
KLF_GK_HD uint64_t group_key_span(uint64_t content_len, uint32_t max_key) {
  return max_key && content_len > max_key ? (uint64_t)max_key : content_len;
}

KLF_GK_HD bool group_key_digit(uint8_t c) { return (uint32_t)c - (uint32_t)'0' <= 9u; }

// The rule, one content byte at a time: true when byte c of the span adds the key byte `out`,
// false when it continues a digit run.  prev_digit: the span's previous byte was a digit (false
// at the span's first byte).  It needs nothing else, so a wave can apply it to 64 bytes at once.
KLF_GK_HD bool group_key_emits(uint32_t flags, bool prev_digit, uint8_t c, uint8_t& out) {
  if ((flags & kGroupsMaskDigits) && group_key_digit(c)) {
    out = (uint8_t)'#';
    return !prev_digit;
  }
  out = c;
  return true;
}

// The normaliser as a state machine over the span's bytes in order: the rule plus its one bit.
struct GroupKeyNorm {
  uint32_t flags;
  bool prev_digit;
  KLF_GK_HD explicit GroupKeyNorm(uint32_t f) : flags(f), prev_digit(false) {}
  KLF_GK_HD bool step(uint8_t c, uint8_t& out) {
    const bool e = group_key_emits(flags, prev_digit, c, out);
    prev_digit = group_key_digit(c);
    return e;
  }
};

}  // namespace klf
