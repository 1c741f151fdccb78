// rules_selftest.cpp -- stand-alone host check of csrc/a5x_rules.h (the parser and the
// interpreter k_rules_stream runs) for sanitizer builds:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I hashcat_a5_table_generator_amd/csrc tools/rules_selftest.cpp -o rules_selftest && ./rules_selftest
//
// hashcat's documented examples, then every function with every position over words of the
// boundary lengths (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128) against a byte-wise check of the
// invariants: length <= 128, bytes past the length zero, and for the growth functions the
// no-op at the cap.  The word buffer is an exact-size heap block, so any access outside
// the A5X_RULE_NDW dwords is an AddressSanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "a5x_rules.h"

struct HeapBuf {  // A5X_RULE_NDW dwords on the heap: out-of-range dwords trip the sanitizer
  std::unique_ptr<uint32_t[]> w{new uint32_t[A5X_RULE_NDW]()};
  uint32_t rd(uint32_t k) const { return w[k]; }
  void wr(uint32_t k, uint32_t v) { w[k] = v; }
};

static int fails = 0;

static bool run(const std::string& rule, const std::string& word, std::string* out) {
  uint32_t ops[A5X_RULE_OPS_MAX], nops = 0;
  // (an exact-size copy of the line: the parser must not read past it)
  std::unique_ptr<uint8_t[]> line(new uint8_t[rule.size() ? rule.size() : 1]);
  memcpy(line.get(), rule.data(), rule.size());
  if (rule_parse_line(line.get(), rule.size(), ops, &nops) != RULE_LINE_OK) return false;
  HeapBuf b;
  memcpy(b.w.get(), word.data(), word.size());
  const uint32_t L = rule_apply(b, (uint32_t)word.size(), ops, nops);
  if (L > A5X_RULE_LMAX) { printf("FAIL %s: length %u\n", rule.c_str(), L); fails++; return true; }
  const uint8_t* p = (const uint8_t*)b.w.get();
  for (uint32_t i = L; i < 4u * A5X_RULE_NDW; i++)
    if (p[i]) { printf("FAIL %s on %zu bytes: byte %u past the length %u is not zero\n", rule.c_str(), word.size(), i, L); fails++; break; }
  out->assign((const char*)p, L);
  return true;
}

static void kat(const char* rule, const std::string& word, const std::string& want) {
  std::string got;
  if (!run(rule, word, &got) || got != want) { printf("FAIL %s: got '%s' want '%s'\n", rule, got.c_str(), want.c_str()); fails++; }
}

int main() {
  const std::string W = "p@ssW0rd";
  const struct { const char* r; std::string want; } T[] = {
      {"l", "p@ssw0rd"}, {"u", "P@SSW0RD"}, {"c", "P@ssw0rd"}, {"C", "p@SSW0RD"}, {"t", "P@SSw0RD"}, {"T3", "p@sSW0rd"},
      {"r", "dr0Wss@p"}, {"d", W + W}, {"p2", W + W + W}, {"f", "p@ssW0rddr0Wss@p"}, {"{", "@ssW0rdp"}, {"}", "dp@ssW0r"},
      {"$1", "p@ssW0rd1"}, {"^1", "1p@ssW0rd"}, {"[", "@ssW0rd"}, {"]", "p@ssW0r"}, {"D3", "p@sW0rd"}, {"x04", "p@ss"},
      {"O12", "psW0rd"}, {"i4!", "p@ss!W0rd"}, {"o3$", "p@s$W0rd"}, {"'6", "p@ssW0"}, {"ss$", "p@$$W0rd"}, {"@s", "p@W0rd"},
      {"z2", "ppp@ssW0rd"}, {"Z2", "p@ssW0rddd"}, {"q", "pp@@ssssWW00rrdd"}, {"k", "@pssW0rd"}, {"K", "p@ssW0dr"},
      {"*34", "p@sWs0rd"}, {"L2", "p@\xe6sW0rd"}, {"R2", "p@9sW0rd"}, {"+2", "p@tsW0rd"}, {"-1", "p?ssW0rd"},
      {".1", "psssW0rd"}, {",1", "ppssW0rd"}, {"y2", "p@p@ssW0rd"}, {"Y2", "p@ssW0rdrd"}, {":", W}};
  for (const auto& t : T) kat(t.r, W, t.want);
  kat("E", "p@ssW0rd w0rld", "P@ssw0rd W0rld");
  kat("e-", "p@ssW0rd-w0rld", "P@ssw0rd-W0rld");

  // every function, every position, over the boundary lengths
  const char* pos = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ";
  std::vector<std::string> rules;
  for (const char* f = ":lucCtrdf{}[]qkKE"; *f; f++) rules.push_back(std::string(1, *f));
  for (const char* f = "TpD'zZLR+-.,yY"; *f; f++)
    for (const char* p = pos; *p; p++) rules.push_back(std::string(1, *f) + *p);
  for (const char* f = "$^@e"; *f; f++)
    for (const char* x : {"a", " ", "\xff"}) rules.push_back(std::string(1, *f) + x);
  for (const char* f = "xO*"; *f; f++)
    for (const char* p = pos; *p; p++)
      for (const char* q2 : {"0", "1", "3", "4", "5", "9", "Z"}) rules.push_back(std::string(1, *f) + *p + q2);
  for (const char* f = "io"; *f; f++)
    for (const char* p = pos; *p; p++) rules.push_back(std::string(1, *f) + *p + "!");
  rules.push_back("saa");
  rules.push_back("sab");
  rules.push_back(std::string("s\0a", 3));
  rules.push_back(std::string("@\0", 2));
  // rules of several functions that grow to the cap and shrink again
  for (const char* r : {"dddddddd", "qqqqqqqq", "p9p9", "$1$2$3$4$5$6$7$8$9$0", "^1^2^3^4^5", "fff", "zZzZyZYZ", "d]d]d]d]d]d]d]d]d]",
                        "r$1r^2r", "{{{{}}}}", "dq'Z", "x11x00", "O01O01O01", "c$1$2$3TZ", "E eaE", "[[[[]]]]"})
    rules.push_back(r);
  rules.push_back(std::string(31, ':'));
  size_t runs = 0;
  for (size_t n : {0u, 1u, 2u, 3u, 4u, 5u, 7u, 8u, 9u, 31u, 32u, 33u, 35u, 36u, 37u, 63u, 64u, 65u, 127u, 128u}) {
    std::string w(n, 0);
    for (size_t i = 0; i < n; i++) w[i] = (char)("aZ b\xff@a0"[(i * 5 + n) % 8]);
    for (const auto& r : rules) {
      std::string got;
      if (!run(r, w, &got)) { printf("FAIL: rule '%s' not accepted\n", r.c_str()); fails++; }
      runs++;
    }
  }
  // lines the parser must skip without reading past them
  std::string out;
  for (const char* r : {"s", "sa", "i", "i1", "x", "x1", "$", "T", "Ta", "l$", "<5", "M", "Q", "lX"})
    if (run(r, "word", &out)) { printf("FAIL: rule '%s' accepted\n", r); fails++; }
  if (run(std::string(32, ':'), "word", &out)) { printf("FAIL: 32 functions accepted\n"); fails++; }
  printf("%zu rule x word runs, %d failure(s)\n", runs, fails);
  return fails ? 1 : 0;
}
