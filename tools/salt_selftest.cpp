// salt_selftest.cpp -- stand-alone host check of csrc/a5x_salt.h (the message assembly
// k_salt_stream runs) for sanitizer builds:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I hashcat_a5_table_generator_amd/csrc tools/salt_selftest.cpp -o salt_selftest && ./salt_selftest
//
// Placement for every (len, slen) with len + slen <= 128 and slen <= 64, in both orders, against
// the byte-wise concatenation; a shorter message after a longer one in the same buffer; the
// kernel's use (pass.salt: one candidate copy, then salt after salt; salt.pass: one candidate
// copy per run of equal salt lengths); bytes past the message zero.  The lane buffer is an
// exact-size heap block of A5X_RULE_NDW dwords, the salt record and the candidate exact-size
// heap blocks too, so any access outside them is an AddressSanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "a5x_salt.h"

struct HeapBuf {  // A5X_RULE_NDW dwords on the heap: out-of-range dwords trip the sanitizer
  std::unique_ptr<uint32_t[]> w{new uint32_t[A5X_RULE_NDW]()};
  uint32_t rd(uint32_t k) const { return w[k]; }
  void wr(uint32_t k, uint32_t v) { w[k] = v; }
};

struct HeapRec {  // one salt record, exact size
  std::unique_ptr<uint32_t[]> r{new uint32_t[A5X_SALT_STRIDE]()};
  explicit HeapRec(const std::string& s) {
    r[A5X_SALT_R_LEN] = (uint32_t)s.size();
    memcpy(r.get() + A5X_SALT_R_BYTES, s.data(), s.size());
  }
  SaltRec rec() const { SaltRec x; x.r = r.get(); return x; }
};

struct HeapCand {  // the candidate bytes, exact size
  std::unique_ptr<uint8_t[]> p;
  uint32_t n;
  explicit HeapCand(const std::string& s) : p(new uint8_t[s.size() ? s.size() : 1]), n((uint32_t)s.size()) {
    memcpy(p.get(), s.data(), s.size());
  }
  SaltCandBytes src() const { SaltCandBytes c; c.p = p.get(); c.n = n; return c; }
};

static int fails = 0;
static size_t checks = 0;

static std::string bytes_of(uint32_t n, uint32_t seed) {
  std::string s(n, 0);
  for (uint32_t i = 0; i < n; i++) s[i] = (char)(1u + (i * 37u + seed * 101u + n * 7u) % 255u);  // never zero
  return s;
}

static void check(const HeapBuf& b, const std::string& want, uint32_t dirty, const char* what, uint32_t len, uint32_t slen) {
  checks++;
  const uint8_t* p = (const uint8_t*)b.w.get();
  bool ok = dirty == rule_ndw((uint32_t)want.size()) && memcmp(p, want.data(), want.size()) == 0;
  for (uint32_t i = (uint32_t)want.size(); ok && i < 4u * A5X_RULE_NDW; i++) ok = p[i] == 0;
  if (!ok) {
    if (fails < 20) printf("FAIL %s len %u slen %u (extent %u)\n", what, len, slen, dirty);
    fails++;
  }
}

int main() {
  // every (len, slen), each placed into a buffer that just held the longest message
  for (uint32_t len = 0; len <= A5X_RULE_LMAX; len++)
    for (uint32_t slen = 0; slen <= A5X_SALT_MAX && len + slen <= A5X_RULE_LMAX; slen++) {
      if (!salt_fits(len, slen)) { printf("FAIL salt_fits(%u, %u)\n", len, slen); fails++; }
      const std::string c = bytes_of(len, 1), s = bytes_of(slen, 2);
      const std::string big = bytes_of(A5X_RULE_LMAX - A5X_SALT_MAX, 3), bigs = bytes_of(A5X_SALT_MAX, 4);
      const HeapCand hc(c), hbig(big);
      const HeapRec hs(s), hbigs(bigs);
      {  // pass.salt
        HeapBuf b;
        uint32_t dirty = salt_copy_cand(b, hbig.src(), hbig.n, 0u);
        dirty = salt_append(b, hbig.n, dirty, hbigs.rec(), A5X_SALT_MAX);
        check(b, big + bigs, dirty, "pass.salt (longest)", hbig.n, A5X_SALT_MAX);
        dirty = salt_copy_cand(b, hc.src(), len, dirty);
        check(b, c, dirty, "candidate copy", len, 0);
        dirty = salt_append(b, len, dirty, hs.rec(), slen);
        check(b, c + s, dirty, "pass.salt", len, slen);
      }
      {  // salt.pass
        HeapBuf b;
        uint32_t dirty = salt_prefix_cand(b, hbig.src(), hbig.n, A5X_SALT_MAX, 0u);
        salt_prefix_salt(b, hbigs.rec(), A5X_SALT_MAX);
        check(b, bigs + big, dirty, "salt.pass (longest)", hbig.n, A5X_SALT_MAX);
        dirty = salt_prefix_cand(b, hc.src(), len, slen, dirty);
        salt_prefix_salt(b, hs.rec(), slen);
        check(b, s + c, dirty, "salt.pass", len, slen);
      }
    }
  if (salt_fits(65, 64) || salt_fits(128, 1) || salt_fits(129, 0) || salt_fits(0xffffffffu, 1) || !salt_fits(128, 0) ||
      !salt_fits(64, 64)) {
    printf("FAIL salt_fits at the 128-byte limit\n");
    fails++;
  }
  // the kernel's loops: one candidate, the salts of a table sorted by length, in one buffer;
  // pairs that do not fit are skipped and leave the buffer as it is
  std::vector<HeapRec> table;
  const uint32_t slens[] = {0, 1, 2, 3, 3, 4, 5, 8, 8, 16, 31, 32, 55, 63, 64, 64};
  for (size_t i = 0; i < sizeof slens / sizeof *slens; i++) table.emplace_back(bytes_of(slens[i], 10 + (uint32_t)i));
  for (int order = 0; order < 2; order++) {
    HeapBuf b;
    uint32_t dirty = 0;
    // candidates longer and shorter in turn: the buffer carries the previous round's extent
    for (uint32_t len : {128u, 0u, 127u, 1u, 100u, 2u, 65u, 3u, 64u, 5u, 63u, 4u, 97u, 96u, 7u}) {
      const std::string c = bytes_of(len, 5);
      const HeapCand hc(c);
      if (order == 0) dirty = salt_copy_cand(b, hc.src(), len, dirty);
      uint32_t run = 0xffffffffu;
      for (const HeapRec& r : table) {
        const uint32_t slen = r.r[A5X_SALT_R_LEN];
        const std::string s((const char*)(r.r.get() + A5X_SALT_R_BYTES), slen);
        const bool act = salt_fits(len, slen);
        if (order == 0) {
          if (!act) continue;
          dirty = salt_append(b, len, dirty, r.rec(), slen);
          check(b, c + s, dirty, "round pass.salt", len, slen);
        } else {
          if (slen != run) {
            if (act) dirty = salt_prefix_cand(b, hc.src(), len, slen, dirty);
            run = slen;
          }
          if (!act) continue;
          salt_prefix_salt(b, r.rec(), slen);
          check(b, s + c, dirty, "round salt.pass", len, slen);
        }
      }
    }
  }
  // masks: distinct, none all zero
  uint32_t m0[4], m1[4];
  salt_mask(0, m0);
  salt_mask(1, m1);
  if (!(m0[0] | m0[1] | m0[2] | m0[3]) || memcmp(m0, m1, 16) == 0) { printf("FAIL salt_mask\n"); fails++; }
  printf("%zu placement checks, %d failure(s)\n", checks, fails);
  return fails ? 1 : 0;
}
