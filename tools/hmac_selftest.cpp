// hmac_selftest.cpp -- stand-alone host check of csrc/a5x_hmac.h (the HMAC pieces the HMAC stream
// kernel runs) for sanitizer builds:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I hashcat_a5_table_generator_amd/csrc tools/hmac_selftest.cpp -o hmac_selftest && ./hmac_selftest
//
// Every (algorithm 48..55, candidate length 0..128, salt length 0..64) through the header's host
// path -- the record preparation, the key states with the pre-hash of a long key, the inner hash
// from the record's words or from the candidate's bytes, the outer block -- against an
// independent composition: this program's own byte-wise MD5 (RFC 1321), SHA-1, SHA-256 and
// SHA-512 (FIPS 180-4, their constants computed here from the primes' roots) and a textbook
// HMAC (RFC 2104) over concatenated bytes.  Candidates, salts and the record live in exact-size
// heap blocks, the candidate read only through a bounded at4(), so an over-read or over-write is
// an AddressSanitizer report.  The record of every salt length is checked on its own too: key =
// pass word by word (the salt's bytes, the 0x80 byte, the zeros, the bit length (B + slen) * 8,
// the block count), key = salt against the reference's own key states.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "a5x_hmac.h"

static int fails = 0;
static size_t checks = 0, pairs = 0, records = 0;

// ---- the independent reference ---------------------------------------------------------
enum { H_MD5, H_SHA1, H_SHA256, H_SHA512 };
static uint32_t hblock(int h) { return h == H_SHA512 ? 128u : 64u; }
static uint32_t hwords(int h) { return h == H_MD5 ? 4u : h == H_SHA1 ? 5u : 8u; }

static uint32_t rol(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }
static uint32_t ror(uint32_t x, int s) { return (x >> s) | (x << (32 - s)); }
static uint64_t ror64(uint64_t x, int s) { return (x >> s) | (x << (64 - s)); }

// floor(2^64 * frac(p^(1/k))), k = 2 or 3, by bisection on exact integers (FIPS 180-4 4.2.2,
// 4.2.3, 5.3.3, 5.3.5: the first 32 or 64 bits of the fractional parts of the primes' roots)
typedef std::vector<uint32_t> Big;  // little-endian limbs
static Big big_mul(const Big& a, const Big& b) {
  Big r(a.size() + b.size(), 0u);
  for (size_t i = 0; i < a.size(); i++) {
    uint64_t c = 0;
    for (size_t j = 0; j < b.size(); j++) {
      c += (uint64_t)a[i] * b[j] + r[i + j];
      r[i + j] = (uint32_t)c;
      c >>= 32;
    }
    r[i + b.size()] = (uint32_t)c;
  }
  return r;
}
static int big_cmp(const Big& a, const Big& b) {
  for (size_t i = (a.size() > b.size() ? a.size() : b.size()); i-- > 0;) {
    const uint32_t x = i < a.size() ? a[i] : 0u, y = i < b.size() ? b[i] : 0u;
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}
static uint64_t root_frac(uint32_t p, int k) {
  Big target((size_t)2 * k + 1, 0u);  // p << (64 * k)
  target[(size_t)2 * k] = p;
  unsigned __int128 lo = 0, hi = (unsigned __int128)1 << 70;  // (roots below 64)
  while (hi - lo > 1) {
    const unsigned __int128 mid = lo + (hi - lo) / 2;
    Big m(3);
    m[0] = (uint32_t)mid; m[1] = (uint32_t)(mid >> 32); m[2] = (uint32_t)(mid >> 64);
    Big x = big_mul(m, m);
    if (k == 3) x = big_mul(x, m);
    if (big_cmp(x, target) <= 0) lo = mid; else hi = mid;
  }
  return (uint64_t)lo;
}
static const std::vector<uint32_t>& primes() {
  static std::vector<uint32_t> P;
  for (uint32_t n = 2; P.size() < 80; n++) {
    bool ok = true;
    for (uint32_t q : P)
      if (n % q == 0) ok = false;
    if (ok) P.push_back(n);
  }
  return P;
}

// the padded message: 0x80, zeros, the bit length in 8 (SHA-512: 16) bytes
static std::string pad_md(int h, const std::string& m) {
  const size_t B = hblock(h), LB = h == H_SHA512 ? 16 : 8;
  std::string p = m;
  p += (char)0x80;
  while (p.size() % B != B - LB) p += (char)0;
  const uint64_t bits = (uint64_t)m.size() * 8;
  for (size_t i = 0; i < LB; i++) {
    const int sh = h == H_MD5 ? (int)(8 * i) : (int)(8 * (LB - 1 - i));
    p += (char)(uint8_t)(sh < 64 ? bits >> sh : 0);
  }
  return p;
}

// the state after the whole blocks of data, from the IV
static std::vector<uint64_t> run(int h, const std::string& data) {
  const uint8_t* D = (const uint8_t*)data.data();
  std::vector<uint64_t> out;
  if (h == H_MD5) {
    static const int S[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9, 14, 20, 5, 9,
                              14, 20, 5, 9, 14, 20, 5, 9, 14, 20, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23,
                              4, 11, 16, 23, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
    uint32_t K[64];
    for (int i = 0; i < 64; i++) {  // floor(2^32 * abs(sin(i + 1))), RFC 1321 3.4
      double s = __builtin_sin((double)(i + 1));
      if (s < 0) s = -s;
      K[i] = (uint32_t)(uint64_t)(s * 4294967296.0);
    }
    uint32_t hh[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    for (size_t o = 0; o + 64 <= data.size(); o += 64) {
      uint32_t X[16];
      for (int j = 0; j < 16; j++) {
        const uint8_t* b = D + o + 4 * j;
        X[j] = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
      }
      uint32_t a = hh[0], b = hh[1], c = hh[2], d = hh[3];
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
      hh[0] += a; hh[1] += b; hh[2] += c; hh[3] += d;
    }
    out.assign(hh, hh + 4);
  } else if (h == H_SHA1) {
    uint32_t hh[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
    for (size_t o = 0; o + 64 <= data.size(); o += 64) {
      uint32_t w[80];
      for (int j = 0; j < 16; j++) {
        const uint8_t* b = D + o + 4 * j;
        w[j] = ((uint32_t)b[0] << 24) | (b[1] << 16) | (b[2] << 8) | b[3];
      }
      for (int j = 16; j < 80; j++) w[j] = rol(w[j - 3] ^ w[j - 8] ^ w[j - 14] ^ w[j - 16], 1);
      uint32_t a = hh[0], b = hh[1], c = hh[2], d = hh[3], e = hh[4];
      for (int i = 0; i < 80; i++) {
        uint32_t f, k;
        if (i < 20) { f = (b & c) | (~b & d); k = 0x5a827999u; }
        else if (i < 40) { f = b ^ c ^ d; k = 0x6ed9eba1u; }
        else if (i < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8f1bbcdcu; }
        else { f = b ^ c ^ d; k = 0xca62c1d6u; }
        const uint32_t t = rol(a, 5) + f + e + k + w[i];
        e = d; d = c; c = rol(b, 30); b = a; a = t;
      }
      hh[0] += a; hh[1] += b; hh[2] += c; hh[3] += d; hh[4] += e;
    }
    out.assign(hh, hh + 5);
  } else if (h == H_SHA256) {
    static uint32_t K[64], IV[8];
    static bool have = false;
    if (!have) {
      for (int i = 0; i < 64; i++) K[i] = (uint32_t)(root_frac(primes()[i], 3) >> 32);
      for (int i = 0; i < 8; i++) IV[i] = (uint32_t)(root_frac(primes()[i], 2) >> 32);
      have = true;
    }
    uint32_t s[8];
    memcpy(s, IV, sizeof s);
    for (size_t o = 0; o + 64 <= data.size(); o += 64) {
      uint32_t w[64];
      for (int j = 0; j < 16; j++) {
        const uint8_t* b = D + o + 4 * j;
        w[j] = ((uint32_t)b[0] << 24) | (b[1] << 16) | (b[2] << 8) | b[3];
      }
      for (int j = 16; j < 64; j++) {
        const uint32_t s0 = ror(w[j - 15], 7) ^ ror(w[j - 15], 18) ^ (w[j - 15] >> 3);
        const uint32_t s1 = ror(w[j - 2], 17) ^ ror(w[j - 2], 19) ^ (w[j - 2] >> 10);
        w[j] = w[j - 16] + s0 + w[j - 7] + s1;
      }
      uint32_t v[8];
      memcpy(v, s, sizeof v);
      for (int i = 0; i < 64; i++) {
        const uint32_t S1 = ror(v[4], 6) ^ ror(v[4], 11) ^ ror(v[4], 25), ch = (v[4] & v[5]) ^ (~v[4] & v[6]);
        const uint32_t t1 = v[7] + S1 + ch + K[i] + w[i];
        const uint32_t S0 = ror(v[0], 2) ^ ror(v[0], 13) ^ ror(v[0], 22), mj = (v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]);
        const uint32_t t2 = S0 + mj;
        for (int q = 7; q > 0; q--) v[q] = v[q - 1];
        v[4] += t1;
        v[0] = t1 + t2;
      }
      for (int i = 0; i < 8; i++) s[i] += v[i];
    }
    out.assign(s, s + 8);
  } else {
    static uint64_t K[80], IV[8];
    static bool have = false;
    if (!have) {
      for (int i = 0; i < 80; i++) K[i] = root_frac(primes()[i], 3);
      for (int i = 0; i < 8; i++) IV[i] = root_frac(primes()[i], 2);
      have = true;
    }
    uint64_t s[8];
    memcpy(s, IV, sizeof s);
    for (size_t o = 0; o + 128 <= data.size(); o += 128) {
      uint64_t w[80];
      for (int j = 0; j < 16; j++) {
        w[j] = 0;
        for (int q = 0; q < 8; q++) w[j] = (w[j] << 8) | D[o + 8 * j + q];
      }
      for (int j = 16; j < 80; j++) {
        const uint64_t s0 = ror64(w[j - 15], 1) ^ ror64(w[j - 15], 8) ^ (w[j - 15] >> 7);
        const uint64_t s1 = ror64(w[j - 2], 19) ^ ror64(w[j - 2], 61) ^ (w[j - 2] >> 6);
        w[j] = w[j - 16] + s0 + w[j - 7] + s1;
      }
      uint64_t v[8];
      memcpy(v, s, sizeof v);
      for (int i = 0; i < 80; i++) {
        const uint64_t S1 = ror64(v[4], 14) ^ ror64(v[4], 18) ^ ror64(v[4], 41), ch = (v[4] & v[5]) ^ (~v[4] & v[6]);
        const uint64_t t1 = v[7] + S1 + ch + K[i] + w[i];
        const uint64_t S0 = ror64(v[0], 28) ^ ror64(v[0], 34) ^ ror64(v[0], 39), mj = (v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]);
        const uint64_t t2 = S0 + mj;
        for (int q = 7; q > 0; q--) v[q] = v[q - 1];
        v[4] += t1;
        v[0] = t1 + t2;
      }
      for (int i = 0; i < 8; i++) s[i] += v[i];
    }
    out.assign(s, s + 8);
  }
  return out;
}

static std::string ref_hash(int h, const std::string& m) {
  const std::vector<uint64_t> s = run(h, pad_md(h, m));
  std::string out;
  for (uint64_t v : s) {
    if (h == H_MD5) for (int k = 0; k < 4; k++) out += (char)(uint8_t)(v >> (8 * k));
    else if (h == H_SHA512) for (int k = 0; k < 8; k++) out += (char)(uint8_t)(v >> (56 - 8 * k));
    else for (int k = 0; k < 4; k++) out += (char)(uint8_t)(v >> (24 - 8 * k));
  }
  return out;
}

// RFC 2104, as written there
static std::string key_block(int h, const std::string& key, uint8_t pad) {
  std::string k = key.size() > hblock(h) ? ref_hash(h, key) : key;
  k.resize(hblock(h), (char)0);
  for (char& c : k) c = (char)((uint8_t)c ^ pad);
  return k;
}
static std::string ref_hmac(int h, const std::string& key, const std::string& msg) {
  return ref_hash(h, key_block(h, key, 0x5c) + ref_hash(h, key_block(h, key, 0x36) + msg));
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

static int hash_of(int algo) { return (algo - A5X_ALGO_HMAC_MD5_KEY_PASS) / 2; }
static bool key_pass(int algo) { return ((algo - A5X_ALGO_HMAC_MD5_KEY_PASS) & 1) == 0; }
static std::string composed(int algo, const std::string& p, const std::string& salt) {
  return key_pass(algo) ? ref_hmac(hash_of(algo), p, salt) : ref_hmac(hash_of(algo), salt, p);
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
  const uint32_t nw = (uint32_t)a5x_algo_hmac(algo) * (hash_of(algo) == H_SHA512 ? 16u : hwords(hash_of(algo)));
  std::unique_ptr<uint32_t[]> d(new uint32_t[nw ? nw : 1]);
  if (!hmac_pair_host_any(algo, src, c.n, s.p.get(), s.n, d.get())) return std::string();
  return std::string((const char*)d.get(), 4 * nw);
}

// the record of one salt, against its definition
static void check_record(int algo, const std::string& salt) {
  const HeapBytes s(salt);
  std::unique_ptr<uint32_t[]> r(new uint32_t[A5X_HMAC_STRIDE]);
  bool ok = hmac_record(algo, s.p.get(), s.n, 7u, r.get());
  const int h = hash_of(algo);
  const uint32_t B = hblock(h), LB = h == H_SHA512 ? 16u : 8u;
  uint32_t m[4];
  salt_mask(7u, m);
  ok = ok && r[A5X_HMAC_R_LEN] == salt.size() && r[A5X_HMAC_R_INDEX] == 7u && r[3] == 0u &&
       memcmp(m, r.get() + A5X_HMAC_R_MASK, 16) == 0;
  if (key_pass(algo)) {
    // word by word: the salt's bytes, 0x80, zeros, the bit length (B + slen) * 8 at the end of the last block
    const uint32_t nb = salt.size() + 1u + LB <= B ? 1u : 2u;
    std::string want(128, (char)0);
    memcpy(&want[0], salt.data(), salt.size());
    want[salt.size()] = (char)0x80;
    const uint64_t bits = 8ull * (B + salt.size());
    for (uint32_t i = 0; i < 8; i++)
      want[B * nb - 8 + i] = (char)(uint8_t)(bits >> (h == H_MD5 ? 8 * i : 56 - 8 * i));
    for (uint32_t k = 0; k < 32; k++) {
      uint32_t w = 0;
      for (uint32_t j = 0; j < 4; j++) w |= (uint32_t)(uint8_t)want[4 * k + j] << (h == H_MD5 ? 8 * j : 24 - 8 * j);
      checks++;
      if (r[A5X_HMAC_R_BODY + k] != w) ok = false;
    }
    ok = ok && r[A5X_HMAC_R_NB] == nb && B * nb <= 128u;
  } else {
    // the reference's own key states: its compression over the one block K0 ^ ipad / K0 ^ opad
    const std::vector<uint64_t> ist = run(h, key_block(h, salt, 0x36)), ost = run(h, key_block(h, salt, 0x5c));
    for (uint32_t i = 0; i < ist.size(); i++) {
      checks++;
      if (h == H_SHA512) {
        const uint32_t* a = r.get() + A5X_HMAC_R_BODY + 2 * i;
        const uint32_t* b = r.get() + A5X_HMAC_R_OST + 2 * i;
        if ((((uint64_t)a[1] << 32) | a[0]) != ist[i] || (((uint64_t)b[1] << 32) | b[0]) != ost[i]) ok = false;
      } else {
        if (r[A5X_HMAC_R_BODY + i] != (uint32_t)ist[i] || r[A5X_HMAC_R_OST + i] != (uint32_t)ost[i]) ok = false;
      }
    }
    // (the words past the states are zero)
    const uint32_t used = h == H_SHA512 ? 16u : (uint32_t)ist.size();
    for (uint32_t k = used; k < 16u; k++)
      if (r[A5X_HMAC_R_BODY + k] || r[A5X_HMAC_R_OST + k]) ok = false;
    ok = ok && r[A5X_HMAC_R_NB] == 0u;
  }
  records++;
  checks++;
  if (!ok) {
    if (fails < 20) printf("FAIL record algo %d salt length %zu\n", algo, salt.size());
    fails++;
  }
}

int main() {
  // the reference itself: the "abc" vectors of RFC 1321 / FIPS 180-4, and RFC 2202 / 4231 test case 2
  const std::string abc = "abc", jefe = "Jefe", what = "what do ya want for nothing?";
  checks += 8;
  if (hx(ref_hash(H_MD5, abc)) != "900150983cd24fb0d6963f7d28e17f72") { printf("FAIL reference md5\n"); fails++; }
  if (hx(ref_hash(H_SHA1, abc)) != "a9993e364706816aba3e25717850c26c9cd0d89d") { printf("FAIL reference sha1\n"); fails++; }
  if (hx(ref_hash(H_SHA256, abc)) != "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad") { printf("FAIL reference sha256\n"); fails++; }
  if (hx(ref_hash(H_SHA512, abc)) !=
      "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f") {
    printf("FAIL reference sha512\n");
    fails++;
  }
  if (hx(ref_hmac(H_MD5, jefe, what)) != "750c783e6ab0b503eaa86e310a5db738") { printf("FAIL reference hmac-md5\n"); fails++; }
  if (hx(ref_hmac(H_SHA1, jefe, what)) != "effcdf6ae5eb2fa2d27416d5f184df9c259a7c79") { printf("FAIL reference hmac-sha1\n"); fails++; }
  if (hx(ref_hmac(H_SHA256, jefe, what)) != "5bdcc146bf60754e6a042426089575c75a003f089d2739839dec58b964ec3843") { printf("FAIL reference hmac-sha256\n"); fails++; }
  if (hx(ref_hmac(H_SHA512, jefe, what)) !=
      "164b7a7bfcf819e2e395fbe73b56e0a387bd64222e831fd610270cd7ea2505549758bf75c05a994a6d034f65f8f0e6fdcaeab1a34d4a6b4b636e070a38bce737") {
    printf("FAIL reference hmac-sha512\n");
    fails++;
  }
  for (int algo = A5X_ALGO_HMAC_MD5_KEY_PASS; algo <= A5X_ALGO_HMAC_SHA512_KEY_SALT; algo++) {
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
