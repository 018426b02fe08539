// klf_fieldval.hpp — the numeric field of a line in klf_result_field_stats (SPEC.md S4f), shared
// by the HIP kernels and the host (klf_field_value).  No dependencies: a stand-alone host program
// can include it.
//
// A content C (S1's content without its terminating '\n') is a miss when `key` does not occur in
// it.  Otherwise the bytes behind the key's first occurrence are fed, one at a time, to
// FieldNumber: up to four separator bytes, an optional sign, a number (plain mode: cut to
// `decimals` fraction digits) or a Go duration (nanoseconds).  The line is a hit with a value
// |v| < 2^62, or bad: the key is there, a value is not.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KLF_FV_HD __host__ __device__ __forceinline__
#else
#define KLF_FV_HD inline
#endif

namespace klf {

constexpr uint32_t kFieldDuration = 1u;   // = KLF_FIELD_DURATION
constexpr uint32_t kFieldMaxKey = 64u;    // = KLF_FIELD_MAX_KEY
constexpr int kFieldHit = 0, kFieldMiss = 1, kFieldBad = 2;  // = KLF_FIELD_HIT / _MISS / _BAD
constexpr uint64_t kFieldLimit = 1ull << 62;  // magnitudes stay below this

KLF_FV_HD bool field_digit(uint8_t c) { return (uint32_t)c - (uint32_t)'0' <= 9u; }
KLF_FV_HD bool field_separator(uint8_t c) { return c == ' ' || c == '\t' || c == '=' || c == ':' || c == '"'; }

// The number behind the key as a state machine over the content's bytes in order.  step(c) is
// false once the class is settled (no later byte can change it); finish() when the bytes ran out
// or step said so.
struct FieldNumber {
  enum State : uint32_t {
    kSep, kSign, kInt0, kInt, kDot, kFrac,     // the number
    kUnit, kUnitS, kUnitM, kMicro,             // duration: its unit
    kAfter, kDoneHit, kDoneBad
  };
  uint32_t decimals, duration;
  uint32_t state, nsep, nfrac;
  uint64_t acc;      // plain: the digits read as an integer; duration: the component's integer part
  uint64_t frac;     // duration: the component's first 9 fraction digits
  uint64_t total;    // duration: the components before this one
  uint64_t unit_ns;  // kUnitS: the unit an 's' completes
  uint8_t micro2;    // kMicro: the second byte of the micro sign that began
  bool neg, over;

  KLF_FV_HD FieldNumber(uint32_t dec, uint32_t flags)
      : decimals(dec), duration(flags & kFieldDuration), state(kSep), nsep(0), nfrac(0), acc(0), frac(0), total(0),
        unit_ns(0), micro2(0), neg(false), over(false) {}

  // acc = acc * 10 + d while that stays below 2^62
  KLF_FV_HD void push(uint32_t d) {
    if (over || acc > (kFieldLimit - 1) / 10) { over = true; return; }
    acc = acc * 10 + d;  // (<= 10 * floor((2^62 - 1) / 10) + 9 < 2^63)
    if (acc >= kFieldLimit) over = true;
  }
  // The component acc.frac of a unit of `ns` nanoseconds joins the total; `lim` = (2^62 - 1) / ns.
  KLF_FV_HD void add_component(uint64_t ns, uint64_t lim) {
    if (over || acc > lim) { over = true; return; }
    uint64_t f9 = frac;
    for (uint32_t k = nfrac; k < 9; ++k) f9 *= 10;
    const uint64_t part = ns >= 1000000000ull ? f9 * (ns / 1000000000ull) : f9 * ns / 1000000000ull;  // (< ns)
    const uint64_t comp = acc * ns + part;  // (< 2^62 + ns)
    if (comp >= kFieldLimit || total + comp >= kFieldLimit) { over = true; return; }
    total += comp;
  }
#define KLF_FV_UNIT(ns) add_component(ns, (kFieldLimit - 1) / (ns))

  KLF_FV_HD bool step(uint8_t c) {
    for (;;) {  // (a state that does not consume c hands it to the next one)
      switch (state) {
        case kSep:
          if (nsep < 4 && field_separator(c)) { ++nsep; return true; }
          state = kSign;
          continue;
        case kSign:
          state = kInt0;
          if (c == '-' || c == '+') { neg = c == '-'; return true; }
          continue;
        case kInt0:
          if (!field_digit(c)) { state = kDoneBad; return false; }
          state = kInt;
          continue;
        case kInt:
          if (field_digit(c)) { push(c - '0'); return true; }
          if (c == '.') { state = kDot; return true; }
          break;  // the number has ended in front of c
        case kDot:  // a '.' counts only with a digit behind it: else the number ended in front of it
          if (!field_digit(c)) { c = '.'; break; }
          state = kFrac;
          continue;
        case kFrac:
          if (!field_digit(c)) break;
          if (duration) {
            if (nfrac < 9) { frac = frac * 10 + (c - '0'); ++nfrac; }
          } else if (nfrac < decimals) {
            push(c - '0');
            ++nfrac;
          }
          return true;
        case kUnit:  // longest match first: "ms" before "m"
          switch (c) {
            case 'n': state = kUnitS; unit_ns = 1ull; return true;
            case 'u': state = kUnitS; unit_ns = 1000ull; return true;
            case 0xC2: state = kMicro; micro2 = 0xB5; return true;  // U+00B5 micro sign
            case 0xCE: state = kMicro; micro2 = 0xBC; return true;  // U+03BC Greek mu
            case 'm': state = kUnitM; return true;
            case 's': KLF_FV_UNIT(1000000000ull); state = kAfter; return true;
            case 'h': KLF_FV_UNIT(3600000000000ull); state = kAfter; return true;
            default: state = kDoneBad; return false;
          }
        case kMicro:
          if (c != micro2) { state = kDoneBad; return false; }
          state = kUnitS;
          unit_ns = 1000ull;
          return true;
        case kUnitS:
          if (c != 's') { state = kDoneBad; return false; }
          if (unit_ns == 1ull) KLF_FV_UNIT(1ull); else KLF_FV_UNIT(1000ull);
          state = kAfter;
          return true;
        case kUnitM:
          state = kAfter;
          if (c == 's') { KLF_FV_UNIT(1000000ull); return true; }
          KLF_FV_UNIT(60000000000ull);
          continue;
        case kAfter:  // another component follows iff the next byte is a digit
          if (!field_digit(c)) { state = kDoneHit; return false; }
          acc = 0; frac = 0; nfrac = 0;
          state = kInt;
          continue;
        default:
          return false;
      }
      // the number has ended in front of c
      if (!duration) { state = kDoneHit; return false; }
      state = kUnit;
    }
  }

  // The class once the content has ended (or step returned false); *v is set for a hit.
  KLF_FV_HD int finish(int64_t* v) {
    uint64_t mag;
    if (duration) {
      if (state == kUnitM) { KLF_FV_UNIT(60000000000ull); state = kAfter; }
      if (state != kAfter && state != kDoneHit) return kFieldBad;
      mag = total;
    } else {
      if (state != kInt && state != kDot && state != kFrac && state != kDoneHit) return kFieldBad;
      for (; nfrac < decimals; ++nfrac) push(0);  // right-padded with '0'
      mag = acc;
    }
    if (over) return kFieldBad;
    *v = neg ? -(int64_t)mag : (int64_t)mag;
    return kFieldHit;
  }
#undef KLF_FV_UNIT
};

// The class and value of a content of n bytes behind `src`, whose at(i) is byte i (i < n; never
// called past n).  The key's first occurrence alone counts: first-byte filter, then compare.
template <class Src>
KLF_FV_HD int field_classify(Src& src, uint64_t n, const uint8_t* key, uint32_t key_len, uint32_t decimals,
                             uint32_t flags, int64_t* v) {
  if (key_len == 0 || key_len > n) return kFieldMiss;
  const uint8_t k0 = key[0];
  const uint64_t last = n - key_len;
  // The search only finds the place; the number is read behind the loop, so that on the GPU the
  // lanes of a wave, which find their keys at different offsets, parse together and not in turn.
  uint64_t at = ~0ull;
  for (uint64_t i = 0; i <= last; ++i) {
    if (src.at(i) != k0) continue;
    uint32_t j = 1;
    while (j < key_len && src.at(i + j) == key[j]) ++j;
    if (j == key_len) {
      at = i;
      break;
    }
  }
  if (at == ~0ull) return kFieldMiss;
  FieldNumber num(decimals, flags);
  for (uint64_t p = at + key_len; p < n; ++p)
    if (!num.step(src.at(p))) break;
  return num.finish(v);
}

// A content in host memory.
struct FieldHostBytes {
  const uint8_t* p;
  KLF_FV_HD uint8_t at(uint64_t i) const { return p[i]; }
};

}  // namespace klf
