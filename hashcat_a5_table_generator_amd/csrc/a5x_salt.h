// a5x_salt.h -- salted messages, hash(pass.salt) and hash(salt.pass): the salt record and the
// message assembly, host and device (shared by the salt stream kernel, a5x_salt.hip, the
// host hook a5x_debug_digest_salted, a5x_host.cpp, and the stand-alone self-test,
// tools/salt_selftest.cpp: the CPU suite runs the code the kernel runs).
//
// The message lives in the A5X_RULE_NDW-dword buffer of a5x_rules.h, reached only through
// B::rd(k) / B::wr(k, v), so the same code runs on a flat host array and on the kernel's
// dword-interleaved LDS lane buffers.  Invariant kept by every function here: all buffer
// bytes at or past the message length are zero (the hash sources read past the message).
// Placement moves whole dwords: salt (pass.salt) or candidate (salt.pass) dwords are funnel-
// shifted (v_alignbyte_b32 on the device) to the byte offset the other part ends at.
//
// A (candidate, salt) pair whose message would exceed A5X_RULE_LMAX bytes is never placed:
// the caller skips it (salt_fits) and counts it.
#pragma once
#include <stdint.h>

#include "a5x_rules.h"

#define A5X_SALT_MAX 64u
#define A5X_SALT_ORDER_PASS_SALT 0
#define A5X_SALT_ORDER_SALT_PASS 1
// One salt record of the device salt table, in u32: [0] length in bytes, [1] the public salt
// index (first appearance in the caller's order; the table itself is sorted by length),
// [2..3] zero, [4..7] the 128-bit probe mask of the salt index, [8..23] the salt bytes as
// dwords, zero past the length.
#define A5X_SALT_STRIDE 24u
#define A5X_SALT_R_LEN 0u
#define A5X_SALT_R_INDEX 1u
#define A5X_SALT_R_MASK 4u
#define A5X_SALT_R_BYTES 8u

#define SALT_HD RULE_HD

// whether the pair is hashed at all
SALT_HD bool salt_fits(uint32_t len, uint32_t slen) { return len <= A5X_RULE_LMAX && slen <= A5X_RULE_LMAX - len; }

// the salt's dwords out of its record (zero at and past dword 16)
struct SaltRec {
  const uint32_t* r;
  SALT_HD uint32_t dw(uint32_t j) const { return j < A5X_SALT_MAX / 4u ? r[A5X_SALT_R_BYTES + j] : 0u; }
};

// a buffer of exactly A5X_RULE_NDW dwords somewhere else (heap, stack): the host form
struct SaltBuf {
  uint32_t* w;
  SALT_HD uint32_t rd(uint32_t k) const { return w[k]; }
  SALT_HD void wr(uint32_t k, uint32_t v) { w[k] = v; }
  // message source of the digests (a5x_sha.h): 4 bytes at message offset i
  SALT_HD uint32_t at4(uint32_t i) const { return rule_at4(*this, (int)i); }
};

// candidate bytes in plain memory, readable only inside [0, n): the host form of the
// candidate source of salt_copy_cand / salt_prefix_cand (at4(i): 4 bytes at offset i)
struct SaltCandBytes {
  const uint8_t* p;
  uint32_t n;
  SALT_HD uint32_t at4(uint32_t i) const {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4u; k++)
      if (i + k < n) v |= (uint32_t)p[i + k] << (8u * k);
    return v;
  }
};

// zero dwords [nd, dirty) (what an earlier, longer message left); returns nd
template <class B> SALT_HD uint32_t salt_zero_tail(B& b, uint32_t nd, uint32_t dirty) {
  for (uint32_t k = nd; k < dirty; k++) b.wr(k, 0u);
  return nd;
}

// ---- pass.salt -------------------------------------------------------------------
// The candidate (len <= A5X_RULE_LMAX bytes of cand) into the buffer, once per round of
// salts; dirty = the dwords that may be non-zero.  Returns the new dirty extent.
template <class B, class C> SALT_HD uint32_t salt_copy_cand(B& b, const C& cand, uint32_t len, uint32_t dirty) {
  const uint32_t nd = rule_ndw(len);
  for (uint32_t k = 0; k < nd; k++) b.wr(k, cand.at4(4u * k) & rule_keep((int)len - (int)(4u * k)));
  return salt_zero_tail(b, nd, dirty);
}
// The salt behind the candidate that salt_copy_cand placed (another salt may have been
// appended since): its dwords funnel-shifted by len & 3, ORed into the candidate's last
// partial dword and written behind it, zeros up to the previous extent.  salt_fits(len,
// slen) holds.  Returns the new dirty extent, rule_ndw(len + slen).
template <class B, class S>
SALT_HD uint32_t salt_append(B& b, uint32_t len, uint32_t dirty, const S& salt, uint32_t slen) {
  const uint32_t q = len >> 2, r = len & 3u, nd = rule_ndw(len + slen), ns = rule_ndw(slen);
  uint32_t lo = 0u;  // salt dword j - 1
  for (uint32_t j = 0; j <= ns; j++) {
    const uint32_t hi = salt.dw(j);  // (zero at j == ns: the record is zero past the salt)
    const uint32_t k = q + j;
    if (k < nd) {
      uint32_t v = r ? rule_alignbyte(hi, lo, 4u - r) : hi;
      if (j == 0 && r) v |= b.rd(q) & rule_keep((int)r);
      b.wr(k, v);
    }
    lo = hi;
  }
  return salt_zero_tail(b, nd, dirty);
}

// ---- salt.pass -------------------------------------------------------------------
// The candidate at byte offset slen, once per run of salts of slen bytes: dwords
// [slen / 4, ndw(len + slen)), the salt's bytes of the first of them left zero; zeros up to
// the previous extent.  salt_fits(len, slen) holds.  Returns the new dirty extent.
template <class B, class C>
SALT_HD uint32_t salt_prefix_cand(B& b, const C& cand, uint32_t len, uint32_t slen, uint32_t dirty) {
  const uint32_t qs = slen >> 2, rs = slen & 3u, nd = rule_ndw(len + slen);
  for (uint32_t k = qs; k < nd; k++) {
    const uint32_t j = k - qs;
    uint32_t v;
    if (j == 0) v = (cand.at4(0u) & rule_keep((int)len)) << (8u * rs);
    else v = cand.at4(4u * j - rs) & rule_keep((int)len - (int)(4u * j - rs));
    b.wr(k, v);
  }
  return salt_zero_tail(b, nd, dirty);
}
// One salt of the run in front of the candidate salt_prefix_cand placed: whole dwords as
// they are, the last partial one merged with the candidate's first bytes.
template <class B, class S> SALT_HD void salt_prefix_salt(B& b, const S& salt, uint32_t slen) {
  const uint32_t qs = slen >> 2, rs = slen & 3u;
  for (uint32_t k = 0; k < qs; k++) b.wr(k, salt.dw(k));
  if (rs) b.wr(qs, (b.rd(qs) & ~rule_keep((int)rs)) | salt.dw(qs));
}

// ---- the probe mask --------------------------------------------------------------
// A target registered with salt index i is keyed in the prefilter and the table on its first
// 16 digest bytes XOR salt_mask(i): a digest computed under another salt probes another key.
// The mixer's inputs are odd, so no index (0 included) has the all-zero mask the mixer gives
// for input 0.
SALT_HD uint64_t salt_fmix64(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
SALT_HD void salt_mask(uint32_t index, uint32_t* m) {
  const uint64_t a = salt_fmix64(2ull * index + 1ull), b = salt_fmix64((2ull * index + 1ull) ^ 0x9E3779B97F4A7C15ull);
  m[0] = (uint32_t)a; m[1] = (uint32_t)(a >> 32); m[2] = (uint32_t)b; m[3] = (uint32_t)(b >> 32);
}
