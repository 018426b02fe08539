// patterns_fuzz.cpp — the pattern compiler (klf_patterns.cpp) run stand-alone under
// ASan / UBSan (tests/test_native.py).  Input file: records of
//   u32 pattern length, pattern bytes, u32 n contents, then per content u32 length, bytes.
// Output: one line per record: "big" / "bad" (refused), or per content one character '0' / '1'
// per decision: glushkov_match, then prefilter_match at phases 0..15 (the full matcher's
// answer again when the prefilter is off), then the OR of nfa_window over every factor
// position x in 0..n, which covers every match start ('x': not run, the set is not one
// general-mode regex).
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/klf.h"
#include "../../klogs_amd/csrc/klf_patterns.hpp"

static bool rd32(FILE* f, uint32_t& v) { return fread(&v, 4, 1, f) == 1; }
static bool rdbytes(FILE* f, std::vector<uint8_t>& b) {
  uint32_t n;
  if (!rd32(f, n) || n > (1u << 20)) return false;
  b.resize(n);
  return n == 0 || fread(b.data(), 1, n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> pat, s;
  while (rdbytes(f, pat)) {
    uint32_t nc;
    if (!rd32(f, nc)) return 3;
    std::vector<std::vector<uint8_t>> cs(nc);
    for (auto& c : cs)
      if (!rdbytes(f, c)) return 3;
    klf::GlushkovTables g;
    std::string err;
    int code = 0;
    if (!klf::compile_regex(pat.data(), pat.size(), g, err, code)) {
      puts(code == KLF_ETOOBIG ? "big" : "bad");
      continue;
    }
    std::vector<std::string> alts;
    bool loose = false;
    uint32_t pre = 0;
    for (size_t want : {(size_t)SIZE_MAX, (size_t)4, (size_t)10}) klf::regex_factors(pat.data(), pat.size(), alts, loose, &pre, want);
    klf::CompiledSet set;
    if (!klf::compile_set({pat}, {KLF_PAT_REGEX}, set, err, code)) return 4;
    std::string out;
    for (auto& c : cs) {
      const bool full = klf::glushkov_match(g, c.data(), c.size());
      out += full ? '1' : '0';
      const bool pf = set.mode == klf::CompiledSet::kGeneral && set.qf_on;
      for (uint32_t ph = 0; ph < 16; ++ph) out += (pf ? klf::prefilter_match(set, c.data(), c.size(), ph) : full) ? '1' : '0';
      if (set.mode == klf::CompiledSet::kGeneral && set.rx_count == 1) {
        bool win = false;
        for (size_t x = 0; x <= c.size() && !win; ++x) win = klf::nfa_window(set, 0, c.data(), c.size(), x);
        out += win ? '1' : '0';
      } else {
        out += 'x';
      }
      out += ' ';
    }
    puts(out.c_str());
  }
  fclose(f);
  puts("patterns_fuzz: ok");
  return 0;
}
