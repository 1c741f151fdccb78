// nest_selftest.cpp -- stand-alone host check of csrc/a5x_nest.h (the nested digests the
// stream kernels run) for sanitizer builds:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I hashcat_a5_table_generator_amd/csrc tools/nest_selftest.cpp -o nest_selftest && ./nest_selftest
//
// The seven algorithms over the published "hashcat" vectors and over messages of every length
// 0..300 (the inner digests' padding edges), each message in an exact-size heap block read
// only through a bounded at4(), so an over-read is an AddressSanitizer report; the hex step
// for each of the 256 byte values in every byte lane, both cases and both word orders, against
// snprintf; the nested digests against compositions of the plain cores with a byte-wise hex
// encoder.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>

#include "a5x_nest.h"

static int fails = 0;
static size_t checks = 0;

struct HeapMsg {  // the message bytes, exact size
  std::unique_ptr<uint8_t[]> p;
  uint32_t n;
  explicit HeapMsg(const std::string& s) : p(new uint8_t[s.size() ? s.size() : 1]), n((uint32_t)s.size()) {
    memcpy(p.get(), s.data(), s.size());
  }
  ShaBytes src() const { ShaBytes b; b.p = p.get(); b.n = n; return b; }
};

static std::string hex_of(const uint8_t* d, size_t n, bool upper) {
  std::string s;
  char b[3];
  for (size_t i = 0; i < n; i++) {
    snprintf(b, sizeof b, upper ? "%02X" : "%02x", d[i]);
    s += b;
  }
  return s;
}

// plain digests through the same cores, for the byte-wise composition
static std::string md5_of(const std::string& m) {
  const HeapMsg h(m);
  uint32_t d[4];
  md5_src_hd(h.src(), h.n, d);
  return std::string((const char*)d, 16);
}
template <int ALGO> static std::string sha_of(const std::string& m) {
  const HeapMsg h(m);
  uint32_t d[16];
  sha_digest<ALGO>(h.src(), h.n, d);
  return std::string((const char*)d, 4 * ShaCfg<ALGO>::NW);
}
static std::string hx(const std::string& d, bool upper = false) { return hex_of((const uint8_t*)d.data(), d.size(), upper); }

template <int ALGO> static std::string nest_of(const std::string& m) {
  const HeapMsg h(m);
  uint32_t d[8];
  nest_digest<ALGO>(h.src(), h.n, d);
  return std::string((const char*)d, 4 * NestCfg<ALGO>::NW);
}

static std::string composed(int algo, const std::string& m) {
  switch (algo) {
    case A5X_ALGO_MD5_MD5: return md5_of(hx(md5_of(m)));
    case A5X_ALGO_MD5_MD5_MD5: return md5_of(hx(md5_of(hx(md5_of(m)))));
    case A5X_ALGO_MD5_MD5UP: return md5_of(hx(md5_of(m), true));
    case A5X_ALGO_MD5_SHA1: return md5_of(hx(sha_of<A5X_ALGO_SHA1>(m)));
    case A5X_ALGO_SHA1_SHA1: return sha_of<A5X_ALGO_SHA1>(hx(sha_of<A5X_ALGO_SHA1>(m)));
    case A5X_ALGO_SHA1_MD5: return sha_of<A5X_ALGO_SHA1>(hx(md5_of(m)));
    default: return sha_of<A5X_ALGO_SHA256>(hx(md5_of(m)));
  }
}
static std::string nested(int algo, const std::string& m) {
  switch (algo) {
    case A5X_ALGO_MD5_MD5: return nest_of<A5X_ALGO_MD5_MD5>(m);
    case A5X_ALGO_MD5_MD5_MD5: return nest_of<A5X_ALGO_MD5_MD5_MD5>(m);
    case A5X_ALGO_MD5_MD5UP: return nest_of<A5X_ALGO_MD5_MD5UP>(m);
    case A5X_ALGO_MD5_SHA1: return nest_of<A5X_ALGO_MD5_SHA1>(m);
    case A5X_ALGO_SHA1_SHA1: return nest_of<A5X_ALGO_SHA1_SHA1>(m);
    case A5X_ALGO_SHA1_MD5: return nest_of<A5X_ALGO_SHA1_MD5>(m);
    default: return nest_of<A5X_ALGO_SHA256_MD5>(m);
  }
}

template <bool UPPER, bool BE> static void check_hex_word(uint32_t w) {
  uint32_t m[2];
  nest_hex_word<UPPER, BE>(w, m);
  uint8_t got[8];
  for (int k = 0; k < 8; k++) got[k] = (uint8_t)(BE ? m[k / 4] >> (24 - 8 * (k % 4)) : m[k / 4] >> (8 * (k % 4)));
  const std::string want = hex_of((const uint8_t*)&w, 4, UPPER);
  checks++;
  if (memcmp(got, want.data(), 8) != 0) {
    if (fails < 20) printf("FAIL hex word %08x upper %d big-endian %d\n", w, (int)UPPER, (int)BE);
    fails++;
  }
}

int main() {
  // each of the 256 byte values in each of the four byte lanes, beside other values
  for (uint32_t v = 0; v < 256; v++)
    for (uint32_t lane = 0; lane < 4; lane++)
      for (uint32_t bg : {0x00000000u, 0xffffffffu, 0x9a0f5ca9u}) {
        const uint32_t w = (bg & ~(0xffu << (8 * lane))) | (v << (8 * lane));
        check_hex_word<false, false>(w);
        check_hex_word<true, false>(w);
        check_hex_word<false, true>(w);
        check_hex_word<true, true>(w);
      }
  // the published vectors: each algorithm over "hashcat"
  static const struct { int algo; const char* hex; } V[] = {
      {A5X_ALGO_MD5_MD5, "a936af92b0ae20b1ff6c3347a72e5fbe"},
      {A5X_ALGO_MD5_MD5_MD5, "9882d0778518b095917eb589f6998441"},
      {A5X_ALGO_MD5_MD5UP, "b8c385461bb9f9d733d3af832cf60b27"},
      {A5X_ALGO_MD5_SHA1, "288496df99b33f8f75a7ce4837d1b480"},
      {A5X_ALGO_SHA1_SHA1, "3db9184f5da4e463832b086211af8d2314919951"},
      {A5X_ALGO_SHA1_MD5, "92d85978d884eb1d99a51652b1139c8279fa8663"},
      {A5X_ALGO_SHA256_MD5, "74ee1fae245edd6f27bf36efc3604942479fceefbadab5dc5c0b538c196eb0f1"},
  };
  for (const auto& v : V) {
    checks++;
    const std::string got = hx(nested(v.algo, "hashcat"));
    if (got != v.hex) {
      printf("FAIL vector algo %d: %s, expected %s\n", v.algo, got.c_str(), v.hex);
      fails++;
    }
  }
  // every length through the inner digests' padding edges, against the composition
  for (uint32_t n = 0; n <= 300; n++) {
    std::string m(n, 0);
    for (uint32_t i = 0; i < n; i++) m[i] = (char)((i * 37u + n * 101u + 11u) % 256u);
    for (const auto& v : V) {
      checks++;
      if (nested(v.algo, m) != composed(v.algo, m)) {
        if (fails < 20) printf("FAIL algo %d len %u\n", v.algo, n);
        fails++;
      }
    }
  }
  printf("%zu checks, %d failure(s)\n", checks, fails);
  return fails ? 1 : 0;
}
