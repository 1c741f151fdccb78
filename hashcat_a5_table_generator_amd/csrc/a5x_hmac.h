// a5x_hmac.h -- HMAC (RFC 2104) over MD5 / SHA-1 / SHA-256 / SHA-512 with the candidate as the key
// and the salt as the message, or the reverse; host and device (shared by the HMAC stream kernel,
// a5x_hmac.hip, the host hook a5x_debug_digest_salted, a5x_host.cpp, and the stand-alone
// self-test, tools/hmac_selftest.cpp: the CPU suite runs the code the kernel runs).
//
//   A5X_ALGO_HMAC_MD5_KEY_PASS     HMAC-MD5(K = pass, salt)      hashcat -m 50
//   A5X_ALGO_HMAC_MD5_KEY_SALT     HMAC-MD5(K = salt, pass)      -m 60
//   A5X_ALGO_HMAC_SHA1_KEY_PASS    HMAC-SHA1(K = pass, salt)     -m 150
//   A5X_ALGO_HMAC_SHA1_KEY_SALT    HMAC-SHA1(K = salt, pass)     -m 160
//   A5X_ALGO_HMAC_SHA256_KEY_PASS  HMAC-SHA256(K = pass, salt)   -m 1450
//   A5X_ALGO_HMAC_SHA256_KEY_SALT  HMAC-SHA256(K = salt, pass)   -m 1460
//   A5X_ALGO_HMAC_SHA512_KEY_PASS  HMAC-SHA512(K = pass, salt)   -m 1750
//   A5X_ALGO_HMAC_SHA512_KEY_SALT  HMAC-SHA512(K = salt, pass)   -m 1760
//
// HMAC(K, m) = H((K0 ^ opad) . H((K0 ^ ipad) . m)), K0 = K (its digest if longer than a block of
// B bytes) zero-padded to B.  Both hashes begin with one whole block that depends on the key
// alone, so the two key states ist = H_block(IV, K0 ^ ipad), ost = H_block(IV, K0 ^ opad) are all
// the rest needs of the key (hmac_key_states).
//
//   key = pass: the key states depend only on the candidate: once per candidate, kept across the
//     salts.  The inner message -- salt, 0x80, zeros, the bit length (B + slen) * 8 -- depends
//     only on the salt: the host prepares it as finished message words in the salt record
//     (hmac_record), one or two blocks (SHA-512: always one), and hmac_inner_from_record
//     compresses them from ist.
//   key = salt: the key states depend only on the salt: the host computes them into the record.
//     The inner message is the candidate, padded with its length counted from B
//     (hmac_inner_from_cand; hmac_msg_words gives one block of it, which a caller whose message
//     fits one block builds once and keeps).
//   The outer hash is one more block from ost: the inner digest, then a padding that is a
//   compile-time constant (hmac_outer).
//
// A salt is at most A5X_SALT_MAX = 64 bytes: as a key never longer than a block.  A candidate of
// 65..128 bytes as the key of a 64-byte-block hash is replaced by its digest.
#pragma once
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "a5x.h"
#include "a5x_nest.h"
#include "a5x_salt.h"

#define HMAC_HD NEST_HD

// One record of the device salt table of an HMAC set, in u32.  [0] length of the salt in bytes,
// [1] the public salt index, [2] blocks of the inner message (key = pass: 1 or 2; key = salt: 0,
// the record holds no message), [3] zero, [4..7] the 128-bit probe mask of the salt index --
// length, index and mask where a5x_salt.h has them -- [8..39] the body:
//   key = pass: the 32 words of the padded inner message behind the key block, in the hash's
//     byte order (SHA-512: 64-bit word j as u32 2j = its high half, 2j + 1 = its low half, the
//     big-endian byte order again);
//   key = salt: [8..23] the inner key state, [24..39] the outer key state, state word i at
//     offset i (SHA-512: 64-bit word i as u32 2i = its low half, 2i + 1 = its high half).
// Sorted by [0] as the other salt tables are.
#define A5X_HMAC_STRIDE 40u
#define A5X_HMAC_R_LEN A5X_SALT_R_LEN
#define A5X_HMAC_R_INDEX A5X_SALT_R_INDEX
#define A5X_HMAC_R_NB 2u
#define A5X_HMAC_R_MASK A5X_SALT_R_MASK
#define A5X_HMAC_R_BODY 8u
#define A5X_HMAC_R_OST 24u
static_assert(A5X_HMAC_STRIDE >= A5X_HMAC_R_BODY + 32u, "a record holds two 64-byte blocks, one of 128, or two states");
static_assert(A5X_SALT_MAX + 1u + 8u <= 128u && A5X_SALT_MAX + 1u + 16u <= 128u, "salt, pad byte and bit length fit the record");

constexpr bool a5x_algo_hmac(int algo) { return algo >= A5X_ALGO_HMAC_MD5_KEY_PASS && algo <= A5X_ALGO_HMAC_SHA512_KEY_SALT; }
// the algorithm's own `order` (a5x_algo_salt_order): 0 key = pass, 1 key = salt, -1 not such an algorithm
constexpr int hmac_order(int algo) {
  return !a5x_algo_hmac(algo) ? -1
       : ((algo - A5X_ALGO_HMAC_MD5_KEY_PASS) & 1) ? A5X_SALT_ORDER_SALT_PASS : A5X_SALT_ORDER_PASS_SALT;
}

template <int ALGO> struct HmacCfg {
  static_assert(a5x_algo_hmac(ALGO), "an HMAC algorithm");
  static constexpr int HASH = ALGO <= A5X_ALGO_HMAC_MD5_KEY_SALT ? A5X_ALGO_MD5
                            : ALGO <= A5X_ALGO_HMAC_SHA1_KEY_SALT ? A5X_ALGO_SHA1
                            : ALGO <= A5X_ALGO_HMAC_SHA256_KEY_SALT ? A5X_ALGO_SHA256 : A5X_ALGO_SHA512;
  static constexpr bool KEY_PASS = hmac_order(ALGO) == A5X_SALT_ORDER_PASS_SALT;
  static constexpr bool B64 = HASH == A5X_ALGO_SHA512;  // 64-bit words, 128-byte blocks
  static constexpr bool BE = HASH != A5X_ALGO_MD5;      // big-endian message words
  static constexpr uint32_t B = B64 ? 128u : 64u;       // block bytes
  static constexpr int NS = HASH == A5X_ALGO_MD5 ? 4 : HASH == A5X_ALGO_SHA1 ? 5 : 8;  // state words (of W)
  static constexpr int NW = B64 ? 16 : NS;              // digest words (u32)
  static constexpr uint32_t ONE = B64 ? 111u : 55u;     // the longest message that ends in its first block
  typedef typename std::conditional<B64, uint64_t, uint32_t>::type W;  // a state / message word
};

// ---- the hash from a given state ------------------------------------------------------
template <int ALGO>
HMAC_HD void hmac_iv(typename HmacCfg<ALGO>::W* st) {
  typedef HmacCfg<ALGO> C;
  if constexpr (C::HASH == A5X_ALGO_MD5) {
    st[0] = 0x67452301u; st[1] = 0xefcdab89u; st[2] = 0x98badcfeu; st[3] = 0x10325476u;
  } else if constexpr (C::HASH == A5X_ALGO_SHA1) {
    st[0] = 0x67452301u; st[1] = 0xefcdab89u; st[2] = 0x98badcfeu; st[3] = 0x10325476u; st[4] = 0xc3d2e1f0u;
  } else if constexpr (C::HASH == A5X_ALGO_SHA256) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
  } else {
    st[0] = 0x6a09e667f3bcc908ull; st[1] = 0xbb67ae8584caa73bull; st[2] = 0x3c6ef372fe94f82bull;
    st[3] = 0xa54ff53a5f1d36f1ull; st[4] = 0x510e527fade682d1ull; st[5] = 0x9b05688c2b3e6c1full;
    st[6] = 0x1f83d9abfb41bd6bull; st[7] = 0x5be0cd19137e2179ull;
  }
}
template <int ALGO>
HMAC_HD void hmac_block(typename HmacCfg<ALGO>::W* st, const typename HmacCfg<ALGO>::W* M) {
  typedef HmacCfg<ALGO> C;
  if constexpr (C::HASH == A5X_ALGO_MD5) md5_block_hd(st, M);
  else if constexpr (C::HASH == A5X_ALGO_SHA1) sha1_block(st, M);
  else if constexpr (C::HASH == A5X_ALGO_SHA256) sha256_block(st, M);
  else sha512_block(st, M);
}

// source bytes [b, b + 4) of len as a little-endian word, the bytes at and past len zero (no
// dword at or past len requested); pad: the 0x80 byte placed behind the last one
template <bool PAD, class S>
HMAC_HD uint32_t hmac_word(const S& src, uint32_t len, uint32_t b) {
  const int k = (int)len - (int)b;
  const uint32_t raw = k > 0 ? src.at4(b) : 0u;
  const uint32_t keep = k >= 4 ? 0xffffffffu : (k <= 0 ? 0u : ((1u << (8 * k)) - 1u));
  const uint32_t pad = (PAD && k >= 0 && k < 4) ? (0x80u << (8 * k)) : 0u;
  return (raw & keep) | pad;
}
// 16 words of W from the 2 * 16 (B64) or 16 little-endian u32 that le(j) gives, in the hash's
// byte order
template <int ALGO, class F>
HMAC_HD void hmac_words(F le, typename HmacCfg<ALGO>::W* M) {
  typedef HmacCfg<ALGO> C;
#pragma unroll
  for (uint32_t j = 0; j < 16; j++) {
    if constexpr (C::B64) M[j] = sha_pack64(sha_bswap(le(2u * j + 1u)), sha_bswap(le(2u * j)));
    else if constexpr (C::BE) M[j] = sha_bswap(le(j));
    else M[j] = le(j);
  }
}

// Block blk of the padded message bytes [0, len) of src (the source interface of md_src /
// sha_digest) that follows off bytes already hashed into the state: the 0x80 byte, zeros, and
// in the last block the bit length (off + len) * 8 (off, len <= 128: one u32).  The loops of
// md5_src_hd / sha32_digest / sha512_digest with the length offset.
template <int ALGO, class S>
HMAC_HD void hmac_msg_words(const S& src, uint32_t len, uint32_t off, uint32_t blk, bool last,
                            typename HmacCfg<ALGO>::W* M) {
  typedef HmacCfg<ALGO> C;
  hmac_words<ALGO>([&](uint32_t j) { return hmac_word<true>(src, len, blk * C::B + 4u * j); }, M);
  if (last) {
    const uint32_t bits = (off + len) << 3;
    if constexpr (C::B64) {
      M[14] = 0;
      M[15] = sha_pack64(bits, 0u);
    } else {
      M[14] = C::BE ? 0u : bits;
      M[15] = C::BE ? bits : 0u;
    }
  }
}
// the hash of message bytes [0, len) of src from the state st that has hashed off bytes (a
// multiple of B), st left as the final state
template <int ALGO, class S>
HMAC_HD void hmac_hash_from(const S& src, uint32_t len, uint32_t off, typename HmacCfg<ALGO>::W* st) {
  typedef HmacCfg<ALGO> C;
  const uint32_t nb = (len + (C::B64 ? 16u : 8u)) / C::B + 1u;
  for (uint32_t blk = 0; blk < nb; blk++) {
    typename C::W M[16];
    hmac_msg_words<ALGO>(src, len, off, blk, blk == nb - 1, M);
    hmac_block<ALGO>(st, M);
  }
}

// ---- the pieces of one HMAC -----------------------------------------------------------
// ist = H_block(IV, K0 ^ ipad), ost = H_block(IV, K0 ^ opad) of the key bytes [0, len) of src,
// len <= A5X_RULE_LMAX.  A key over B bytes (64-byte blocks only: 128 is a block of SHA-512) is
// replaced by its digest; on the device that branch diverges by lane, and is rare.
template <int ALGO, class S>
HMAC_HD void hmac_key_states(const S& src, uint32_t len, typename HmacCfg<ALGO>::W* ist, typename HmacCfg<ALGO>::W* ost) {
  typedef HmacCfg<ALGO> C;
  typedef typename C::W W;
  static_assert(A5X_RULE_LMAX <= 128u, "a key of SHA-512 is never longer than its block");
  W K[16], M[16];
  hmac_words<ALGO>([&](uint32_t j) { return hmac_word<false>(src, len, 4u * j); }, K);
  if constexpr (!C::B64) {
    if (len > C::B) {
      W h[C::NS];
      hmac_iv<ALGO>(h);
      hmac_hash_from<ALGO>(src, len, 0u, h);  // (the state words are the digest as message words)
#pragma unroll
      for (int j = 0; j < C::NS; j++) K[j] = h[j];
#pragma unroll
      for (int j = C::NS; j < 16; j++) K[j] = 0u;
    }
  }
  constexpr W IPAD = (W)0x3636363636363636ull, OPAD = (W)0x5c5c5c5c5c5c5c5cull;
#pragma unroll
  for (int j = 0; j < 16; j++) M[j] = K[j] ^ IPAD;
  hmac_iv<ALGO>(ist);
  hmac_block<ALGO>(ist, M);
#pragma unroll
  for (int j = 0; j < 16; j++) M[j] = K[j] ^ OPAD;
  hmac_iv<ALGO>(ost);
  hmac_block<ALGO>(ost, M);
}

// key = salt: a key state out of the record (at: A5X_HMAC_R_BODY the inner, A5X_HMAC_R_OST the outer)
template <int ALGO>
HMAC_HD void hmac_state_from_record(const uint32_t* rec, uint32_t at, typename HmacCfg<ALGO>::W* st) {
  typedef HmacCfg<ALGO> C;
#pragma unroll
  for (int i = 0; i < C::NS; i++) {
    if constexpr (C::B64) st[i] = sha_pack64(rec[at + 2 * i], rec[at + 2 * i + 1]);
    else st[i] = rec[at + i];
  }
}

// key = pass: the inner hash, the record's words compressed from the candidate's inner key
// state; st = its final state.  One block or two by the record (wave-uniform on the device).
template <int ALGO>
HMAC_HD void hmac_inner_from_record(const typename HmacCfg<ALGO>::W* ist, const uint32_t* rec, uint32_t nb,
                                    typename HmacCfg<ALGO>::W* st) {
  typedef HmacCfg<ALGO> C;
  typename C::W M[16];
#pragma unroll
  for (int i = 0; i < C::NS; i++) st[i] = ist[i];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    if constexpr (C::B64) M[k] = sha_pack64(rec[A5X_HMAC_R_BODY + 2 * k + 1], rec[A5X_HMAC_R_BODY + 2 * k]);
    else M[k] = rec[A5X_HMAC_R_BODY + k];
  }
  hmac_block<ALGO>(st, M);
  if constexpr (!C::B64) {
    if (nb > 1u) {
#pragma unroll
      for (int k = 0; k < 16; k++) M[k] = rec[A5X_HMAC_R_BODY + 16 + k];
      hmac_block<ALGO>(st, M);
    }
  }
}

// key = salt: the inner hash, the candidate's bytes [0, len) of src hashed from the salt's inner
// key state with the bit length counted from B; st = its final state
template <int ALGO, class S>
HMAC_HD void hmac_inner_from_cand(const typename HmacCfg<ALGO>::W* ist, const S& src, uint32_t len,
                                  typename HmacCfg<ALGO>::W* st) {
  typedef HmacCfg<ALGO> C;
#pragma unroll
  for (int i = 0; i < C::NS; i++) st[i] = ist[i];
  hmac_hash_from<ALGO>(src, len, C::B, st);
}

// The outer hash: one block from the outer key state -- the inner hash's final state in (its
// words are the digest as message words), the 0x80 byte, zeros, the bit length (B + digest
// bytes) * 8, all but the digest constants.  d = the HMAC in its standard byte order as NW
// little-endian words (what the target table is keyed on and what op 2 stores).
template <int ALGO>
HMAC_HD void hmac_outer(const typename HmacCfg<ALGO>::W* ost, const typename HmacCfg<ALGO>::W* in, uint32_t* d) {
  typedef HmacCfg<ALGO> C;
  typedef typename C::W W;
  constexpr uint32_t BITS = (C::B + 4u * (uint32_t)C::NW) * 8u;
  W st[C::NS], M[16];
#pragma unroll
  for (int i = 0; i < C::NS; i++) st[i] = ost[i];
#pragma unroll
  for (int k = 0; k < 16; k++) M[k] = k < C::NS ? in[k] : (W)0;
  M[C::NS] = C::B64 ? (W)0x8000000000000000ull : C::BE ? (W)0x80000000u : (W)0x80u;
  if constexpr (C::BE) M[15] = BITS; else M[14] = BITS;
  hmac_block<ALGO>(st, M);
#pragma unroll
  for (int i = 0; i < C::NS; i++) {
    if constexpr (C::B64) {
      d[2 * i] = sha_bswap((uint32_t)(st[i] >> 32));
      d[2 * i + 1] = sha_bswap((uint32_t)st[i]);
    } else {
      d[i] = C::BE ? sha_bswap((uint32_t)st[i]) : (uint32_t)st[i];
    }
  }
}

// ---- the host's side: the salt record -------------------------------------------------
template <int ALGO>
inline void hmac_record_of(const uint8_t* salt, uint32_t slen, uint32_t index, uint32_t* r) {
  typedef HmacCfg<ALGO> C;
  for (uint32_t k = 0; k < A5X_HMAC_STRIDE; k++) r[k] = 0u;
  r[A5X_HMAC_R_LEN] = slen;
  r[A5X_HMAC_R_INDEX] = index;
  salt_mask(index, r + A5X_HMAC_R_MASK);
  if constexpr (C::KEY_PASS) {
    uint8_t msg[128];
    const uint32_t nb = (C::B64 || slen <= 55u) ? 1u : 2u;
    memset(msg, 0, sizeof msg);
    if (slen) memcpy(msg, salt, slen);
    msg[slen] = 0x80;
    for (uint32_t k = 0; k < 32u; k++) {
      const uint8_t* p = msg + 4u * k;
      r[A5X_HMAC_R_BODY + k] = C::BE ? ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]
                                     : ((uint32_t)p[3] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0];
    }
    // the bit length (< 2^32: one word): the last word of the last block, MD5 the one before it
    r[A5X_HMAC_R_BODY + (C::B64 ? 32u : 16u * nb) - (C::BE ? 1u : 2u)] = (C::B + slen) << 3;
    r[A5X_HMAC_R_NB] = nb;
  } else {
    typename C::W ist[C::NS], ost[C::NS];
    ShaBytes src;
    src.p = salt;
    src.n = slen;
    hmac_key_states<ALGO>(src, slen, ist, ost);
    for (int i = 0; i < C::NS; i++) {
      if constexpr (C::B64) {
        r[A5X_HMAC_R_BODY + 2 * i] = (uint32_t)ist[i];
        r[A5X_HMAC_R_BODY + 2 * i + 1] = (uint32_t)(ist[i] >> 32);
        r[A5X_HMAC_R_OST + 2 * i] = (uint32_t)ost[i];
        r[A5X_HMAC_R_OST + 2 * i + 1] = (uint32_t)(ost[i] >> 32);
      } else {
        r[A5X_HMAC_R_BODY + i] = ist[i];
        r[A5X_HMAC_R_OST + i] = ost[i];
      }
    }
  }
}

// ---- the host path: one (candidate, salt) pair -------------------------------------------
// The HMAC of ALGO for candidate bytes [0, len) of src and the caller's salt, by the record
// preparation and the pieces above, in the kernel's order.  d gets a5x_digest_size(ALGO) / 4
// words.  len <= A5X_RULE_LMAX, slen <= A5X_SALT_MAX.
template <int ALGO, class S>
inline void hmac_pair_host(const S& src, uint32_t len, const uint8_t* salt, uint32_t slen, uint32_t* d) {
  typedef HmacCfg<ALGO> C;
  typedef typename C::W W;
  uint32_t rec[A5X_HMAC_STRIDE];
  W ist[C::NS], ost[C::NS], st[C::NS];
  hmac_record_of<ALGO>(salt, slen, 0u, rec);
  if constexpr (C::KEY_PASS) {
    hmac_key_states<ALGO>(src, len, ist, ost);
    hmac_inner_from_record<ALGO>(ist, rec, rec[A5X_HMAC_R_NB], st);
  } else {
    hmac_state_from_record<ALGO>(rec, A5X_HMAC_R_BODY, ist);
    hmac_state_from_record<ALGO>(rec, A5X_HMAC_R_OST, ost);
    if (len <= C::ONE) {  // (the kernel: the block built once per candidate when the whole round fits)
      W M[16];
      hmac_msg_words<ALGO>(src, len, C::B, 0u, true, M);
      for (int i = 0; i < C::NS; i++) st[i] = ist[i];
      hmac_block<ALGO>(st, M);
    } else {
      hmac_inner_from_cand<ALGO>(ist, src, len, st);
    }
  }
  hmac_outer<ALGO>(ost, st, d);
}

// the same by value
#define A5X_HMAC_EACH(X)                                                                        \
  X(A5X_ALGO_HMAC_MD5_KEY_PASS) X(A5X_ALGO_HMAC_MD5_KEY_SALT) X(A5X_ALGO_HMAC_SHA1_KEY_PASS)    \
  X(A5X_ALGO_HMAC_SHA1_KEY_SALT) X(A5X_ALGO_HMAC_SHA256_KEY_PASS) X(A5X_ALGO_HMAC_SHA256_KEY_SALT) \
  X(A5X_ALGO_HMAC_SHA512_KEY_PASS) X(A5X_ALGO_HMAC_SHA512_KEY_SALT)

// Record r (A5X_HMAC_STRIDE u32) of the caller's salt for a set of algo; false: no HMAC algorithm
inline bool hmac_record(int algo, const uint8_t* salt, uint32_t slen, uint32_t index, uint32_t* r) {
  switch (algo) {
#define X(A) case A: hmac_record_of<A>(salt, slen, index, r); return true;
    A5X_HMAC_EACH(X)
#undef X
    default: return false;
  }
}
template <class S>
inline bool hmac_pair_host_any(int algo, const S& src, uint32_t len, const uint8_t* salt, uint32_t slen, uint32_t* d) {
  switch (algo) {
#define X(A) case A: hmac_pair_host<A>(src, len, salt, slen, d); return true;
    A5X_HMAC_EACH(X)
#undef X
    default: return false;
  }
}
