// salt_nest_selftest.cpp -- stand-alone host check of csrc/a5x_salt_nest.h (the salted nested
// digests the salted-nested stream kernel runs) for sanitizer builds:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I hashcat_a5_table_generator_amd/csrc tools/salt_nest_selftest.cpp -o salt_nest_selftest && ./salt_nest_selftest
//
// Every (algorithm 32..38, candidate length 0..128, salt length 0..64) through the header's host
// path -- the record preparation, the inner digest and its hex words, the placement of salt .
// text, one or two outer compressions -- against an independent composition: this program's own
// byte-wise MD5 (RFC 1321) and SHA-1 (FIPS 180-4) over the concatenated bytes.  Candidates,
// salts, the placement's working buffer and the record live in exact-size heap blocks, the
// candidate read only through a bounded at4(), so an over-read or over-write is an
// AddressSanitizer report.  The record of every salt length is checked on its own too: the
// salt's bytes, the 0x80 byte, the zeros, the bit length and the block count.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>

#include "a5x_salt_nest.h"

static int fails = 0;
static size_t checks = 0, pairs = 0, records = 0;

// ---- the independent reference: plain byte-wise MD5 and SHA-1 ---------------------------
static uint32_t rol(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

static std::string pad_md(const std::string& m, bool be) {
  std::string p = m;
  p += (char)0x80;
  while (p.size() % 64 != 56) p += (char)0;
  const uint64_t bits = (uint64_t)m.size() * 8;
  for (int i = 0; i < 8; i++) p += (char)(uint8_t)(bits >> (be ? 56 - 8 * i : 8 * i));
  return p;
}

static std::string ref_md5(const std::string& m) {
  static const int S[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9, 14, 20, 5, 9,
                            14, 20, 5, 9, 14, 20, 5, 9, 14, 20, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23,
                            4, 11, 16, 23, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
  uint32_t K[64];
  for (int i = 0; i < 64; i++) {  // floor(2^32 * abs(sin(i + 1))), RFC 1321 3.4
    double s = __builtin_sin((double)(i + 1));
    if (s < 0) s = -s;
    K[i] = (uint32_t)(uint64_t)(s * 4294967296.0);
  }
  uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
  const std::string p = pad_md(m, false);
  for (size_t o = 0; o < p.size(); o += 64) {
    uint32_t X[16];
    for (int j = 0; j < 16; j++) {
      const uint8_t* b = (const uint8_t*)p.data() + o + 4 * j;
      X[j] = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
    for (int i = 0; i < 64; i++) {
      uint32_t f;
      int g;
      if (i < 16) { f = (b & c) | (~b & d); g = i; }
      else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) % 16; }
      else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) % 16; }
      else { f = c ^ (b | ~d); g = (7 * i) % 16; }
      const uint32_t t = d;
      d = c; c = b;
      b = b + rol(a + f + K[i] + X[g], S[i]);
      a = t;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
  }
  std::string out;
  for (int i = 0; i < 4; i++)
    for (int k = 0; k < 4; k++) out += (char)(uint8_t)(h[i] >> (8 * k));
  return out;
}

static std::string ref_sha1(const std::string& m) {
  uint32_t h[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
  const std::string p = pad_md(m, true);
  for (size_t o = 0; o < p.size(); o += 64) {
    uint32_t w[80];
    for (int j = 0; j < 16; j++) {
      const uint8_t* b = (const uint8_t*)p.data() + o + 4 * j;
      w[j] = ((uint32_t)b[0] << 24) | (b[1] << 16) | (b[2] << 8) | b[3];
    }
    for (int j = 16; j < 80; j++) w[j] = rol(w[j - 3] ^ w[j - 8] ^ w[j - 14] ^ w[j - 16], 1);
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
    for (int i = 0; i < 80; i++) {
      uint32_t f, k;
      if (i < 20) { f = (b & c) | (~b & d); k = 0x5a827999u; }
      else if (i < 40) { f = b ^ c ^ d; k = 0x6ed9eba1u; }
      else if (i < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8f1bbcdcu; }
      else { f = b ^ c ^ d; k = 0xca62c1d6u; }
      const uint32_t t = rol(a, 5) + f + e + k + w[i];
      e = d; d = c; c = rol(b, 30); b = a; a = t;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
  }
  std::string out;
  for (int i = 0; i < 5; i++)
    for (int k = 0; k < 4; k++) out += (char)(uint8_t)(h[i] >> (24 - 8 * k));
  return out;
}

static std::string hx(const std::string& d) {
  std::string s;
  char b[3];
  for (unsigned char c : d) {
    snprintf(b, sizeof b, "%02x", c);
    s += b;
  }
  return s;
}

static std::string composed(int algo, const std::string& p, const std::string& salt) {
  switch (algo) {
    case A5X_ALGO_MD5_MD5_SALT: return ref_md5(hx(ref_md5(p)) + salt);
    case A5X_ALGO_MD5_SALT_MD5: return ref_md5(salt + hx(ref_md5(p)));
    case A5X_ALGO_MD5_MD5_MD5SALT: return ref_md5(hx(ref_md5(p)) + hx(ref_md5(salt)));
    case A5X_ALGO_MD5_MD5SALT_MD5: return ref_md5(hx(ref_md5(salt)) + hx(ref_md5(p)));
    case A5X_ALGO_SHA1_SHA1_SALT: return ref_sha1(hx(ref_sha1(p)) + salt);
    case A5X_ALGO_SHA1_SALT_SHA1: return ref_sha1(salt + hx(ref_sha1(p)));
    default: return ref_sha1(hx(ref_md5(p)) + salt);
  }
}

// ---- the code under test, over exact-size heap blocks -----------------------------------
struct HeapBytes {
  std::unique_ptr<uint8_t[]> p;
  uint32_t n;
  explicit HeapBytes(const std::string& s) : p(new uint8_t[s.size() ? s.size() : 1]), n((uint32_t)s.size()) {
    memcpy(p.get(), s.data(), s.size());
  }
};

static std::string under_test(int algo, const std::string& cand, const std::string& salt) {
  const HeapBytes c(cand), s(salt);
  ShaBytes src;
  src.p = c.p.get();
  src.n = c.n;
  const uint32_t nw = snest_out_sha1(algo) ? 5u : 4u;  // outer digest words
  std::unique_ptr<uint32_t[]> w(new uint32_t[A5X_SNEST_PW]), d(new uint32_t[nw]);
  if (!snest_pair_host_any(algo, src, c.n, s.p.get(), s.n, w.get(), d.get())) return std::string();
  return std::string((const char*)d.get(), 4 * nw);
}

// the record of one salt, against its definition byte by byte
static void check_record(int algo, const std::string& salt) {
  const HeapBytes s(salt);
  std::unique_ptr<uint32_t[]> r(new uint32_t[A5X_SNEST_STRIDE]);
  snest_record(algo, s.p.get(), s.n, 7u, r.get());
  const bool be = snest_out_sha1(algo), prefix = snest_order(algo) == A5X_SALT_ORDER_SALT_PASS;
  const uint32_t T = snest_in_sha1(algo) ? 40u : 32u;
  const std::string eff = snest_md5salt(algo) ? hx(ref_md5(salt)) : salt;
  const uint32_t L = T + (uint32_t)eff.size(), nb = L + 9u <= 64u ? 1u : 2u;
  std::string want(128, (char)0);
  memcpy(&want[prefix ? 0 : T], eff.data(), eff.size());
  want[L] = (char)0x80;
  const uint64_t bits = 8ull * L;
  for (int i = 0; i < 8; i++) want[64 * nb - 8 + i] = (char)(uint8_t)(bits >> (be ? 56 - 8 * i : 8 * i));
  std::string got(128, (char)0);
  for (uint32_t k = 0; k < 32; k++)
    for (uint32_t j = 0; j < 4; j++) got[4 * k + j] = (char)(uint8_t)(r[A5X_SNEST_R_MSG + k] >> (be ? 24 - 8 * j : 8 * j));
  uint32_t m[4];
  salt_mask(7u, m);
  records++;
  checks++;
  if (got != want || r[A5X_SNEST_R_LEN] != eff.size() || r[A5X_SNEST_R_INDEX] != 7u || r[A5X_SNEST_R_NB] != nb || r[3] != 0u ||
      memcmp(m, r.get() + A5X_SNEST_R_MASK, 16) != 0) {
    if (fails < 20) printf("FAIL record algo %d salt length %zu\n", algo, salt.size());
    fails++;
  }
}

int main() {
  // the reference itself, on the RFC 1321 / FIPS 180 "abc" vectors
  checks += 2;
  if (hx(ref_md5("abc")) != "900150983cd24fb0d6963f7d28e17f72") { printf("FAIL reference md5\n"); fails++; }
  if (hx(ref_sha1("abc")) != "a9993e364706816aba3e25717850c26c9cd0d89d") { printf("FAIL reference sha1\n"); fails++; }
  for (int algo = A5X_ALGO_MD5_MD5_SALT; algo <= A5X_ALGO_SHA1_MD5_SALT; algo++) {
    for (uint32_t sl = 0; sl <= A5X_SALT_MAX; sl++) {
      std::string salt(sl, 0);
      for (uint32_t i = 0; i < sl; i++) salt[i] = (char)((i * 53u + sl * 29u + 7u) % 256u);
      check_record(algo, salt);
      for (uint32_t n = 0; n <= A5X_RULE_LMAX; n++) {
        std::string m(n, 0);
        for (uint32_t i = 0; i < n; i++) m[i] = (char)((i * 37u + n * 101u + sl * 3u + 11u) % 256u);
        checks++;
        pairs++;
        if (under_test(algo, m, salt) != composed(algo, m, salt)) {
          if (fails < 20) printf("FAIL algo %d candidate length %u salt length %u\n", algo, n, sl);
          fails++;
        }
      }
    }
  }
  printf("%zu checks (%zu pairs, %zu records), %d failure(s)\n", checks, pairs, records, fails);
  return fails ? 1 : 0;
}
