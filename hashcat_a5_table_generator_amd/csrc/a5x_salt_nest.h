// a5x_salt_nest.h -- salted nested digests: an outer MD5 / SHA-1 over the hex text of an inner
// digest of the candidate, with a salt in front of or behind the text; host and device (shared
// by the salted-nested stream kernel, a5x_salt_nest.hip, the host hook a5x_debug_digest_salted,
// a5x_host.cpp, and the stand-alone self-test, tools/salt_nest_selftest.cpp: the CPU suite runs
// the code the kernel runs).
//
//   A5X_ALGO_MD5_MD5_SALT     md5(hex(md5(p)) . salt)              hashcat -m 2611 / 2711
//   A5X_ALGO_MD5_SALT_MD5     md5(salt . hex(md5(p)))              -m 3710
//   A5X_ALGO_MD5_MD5_MD5SALT  md5(hex(md5(p)) . hex(md5(salt)))    -m 3910
//   A5X_ALGO_MD5_MD5SALT_MD5  md5(hex(md5(salt)) . hex(md5(p)))    -m 2811
//   A5X_ALGO_SHA1_SHA1_SALT   sha1(hex(sha1(p)) . salt)            -m 4510
//   A5X_ALGO_SHA1_SALT_SHA1   sha1(salt . hex(sha1(p)))            -m 4520
//   A5X_ALGO_SHA1_MD5_SALT    sha1(hex(md5(p)) . salt)             -m 4710
//
// The inner digest and its hex text depend only on the candidate: snest_inner computes them once
// per candidate, as the 8 or 10 message words the outer compression reads (a5x_nest.h's
// nest_hex_word, born in the outer function's byte order).  Everything else of the outer message
// -- the salt, the 0x80 byte, the zeros, the bit length -- depends only on the salt, so the host
// prepares it per salt as finished message words (snest_record): the whole padded message of one
// or two blocks in the outer byte order, with the text's bytes left zero.
//
//   text . salt (pass.salt): the text is message words [0, HW) whatever the salt; the record's
//     words [HW, 16 * blocks) are used as they are (snest_suffix).  No placement at all.
//   salt . text (salt.pass): the text sits at byte offset slen.  Its words are funnel-shifted by
//     slen & 3 (wave-uniform on the device) and moved to word slen / 4 once per run of salts of
//     equal length -- through the lane's working buffer, the one place indexed by a runtime value
//     (snest_place) -- and per salt only ORed with the record's words (snest_prefix).
//     md5(hex(md5(salt)) . text) is the exception: its salt is always 32 bytes, so the text is
//     message words [8, 16) whatever the salt -- text . salt's register form with the roles
//     swapped (snest_prefix_aligned), no placement and no lane buffer.
//
// The MD5SALT forms are the plain ones with the salt replaced by hex(md5(salt)), which the host
// computes when it builds the record (snest_effective_salt): 32 bytes, so the outer message is
// always two blocks, the second pure padding.
#pragma once
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "a5x.h"
#include "a5x_nest.h"
#include "a5x_salt.h"

#define SNEST_HD NEST_HD

// One record of the device salt table of a salted-nested set, in u32.  [0] length of the
// effective salt in bytes (the MD5SALT forms: 32), [1] the public salt index, [2] blocks of the
// outer message (1 or 2), [3] zero, [4..7] the 128-bit probe mask of the salt index -- length,
// index and mask where a5x_salt.h has them -- [8..39] the 32 words of the padded outer message
// in the outer function's byte order, the text's bytes zero.  Sorted by [0] (salt.pass places
// the text once per run of equal lengths).
#define A5X_SNEST_STRIDE 40u
#define A5X_SNEST_R_LEN A5X_SALT_R_LEN
#define A5X_SNEST_R_INDEX A5X_SALT_R_INDEX
#define A5X_SNEST_R_NB 2u
#define A5X_SNEST_R_MASK A5X_SALT_R_MASK
#define A5X_SNEST_R_MSG 8u
// words the placed text of salt.pass can reach: (64 + 40) / 4, and the spill-over word of a shift
#define A5X_SNEST_PW 27u
static_assert(A5X_SNEST_STRIDE >= A5X_SNEST_R_MSG + 32u, "a record holds two whole message blocks");
static_assert(A5X_SALT_MAX + 40u + 1u + 8u <= 128u, "text, salt, pad byte and bit length fit two blocks");
static_assert(A5X_SNEST_PW >= (A5X_SALT_MAX + 40u) / 4u + 1u && A5X_SNEST_PW <= A5X_RULE_NDW, "the placed text fits the lane buffer");

constexpr bool a5x_algo_salt_nested(int algo) { return algo >= A5X_ALGO_MD5_MD5_SALT && algo <= A5X_ALGO_SHA1_MD5_SALT; }

template <int ALGO> struct SaltNestCfg {
  static_assert(a5x_algo_salt_nested(ALGO), "a salted nested algorithm");
  static constexpr bool IN_SHA1 = ALGO == A5X_ALGO_SHA1_SHA1_SALT || ALGO == A5X_ALGO_SHA1_SALT_SHA1;  // else MD5
  static constexpr bool OUT_SHA1 = ALGO >= A5X_ALGO_SHA1_SHA1_SALT;                                    // else MD5
  static constexpr bool PREFIX = ALGO == A5X_ALGO_MD5_SALT_MD5 || ALGO == A5X_ALGO_MD5_MD5SALT_MD5 ||
                                 ALGO == A5X_ALGO_SHA1_SALT_SHA1;  // salt . text
  static constexpr bool MD5SALT = ALGO == A5X_ALGO_MD5_MD5_MD5SALT || ALGO == A5X_ALGO_MD5_MD5SALT_MD5;
  static constexpr bool PLACED = PREFIX && !MD5SALT;  // the text's offset depends on the salt: snest_place
  static constexpr int IW = IN_SHA1 ? 5 : 4;   // inner digest words
  static constexpr int HW = 2 * IW;            // message words of its hex text
  static constexpr int NW = OUT_SHA1 ? 5 : 4;  // outer digest words
};

// the same by value, for the host's record preparation
inline bool snest_in_sha1(int algo) { return algo == A5X_ALGO_SHA1_SHA1_SALT || algo == A5X_ALGO_SHA1_SALT_SHA1; }
inline bool snest_out_sha1(int algo) { return algo >= A5X_ALGO_SHA1_SHA1_SALT && algo <= A5X_ALGO_SHA1_MD5_SALT; }
inline bool snest_md5salt(int algo) { return algo == A5X_ALGO_MD5_MD5_MD5SALT || algo == A5X_ALGO_MD5_MD5SALT_MD5; }
// the algorithm's own placement (a5x_algo_salt_order): 0 text . salt, 1 salt . text, -1 not such an algorithm
inline int snest_order(int algo) {
  if (!a5x_algo_salt_nested(algo)) return -1;
  return algo == A5X_ALGO_MD5_SALT_MD5 || algo == A5X_ALGO_MD5_MD5SALT_MD5 || algo == A5X_ALGO_SHA1_SALT_SHA1
             ? A5X_SALT_ORDER_SALT_PASS : A5X_SALT_ORDER_PASS_SALT;
}

// ---- the host's side: the salt record -------------------------------------------------
// The salt the outer function hashes: the caller's, or for the MD5SALT forms the 32 hex
// characters of its MD5.  out holds A5X_SALT_MAX bytes; returns the length.
inline uint32_t snest_effective_salt(int algo, const uint8_t* salt, uint32_t slen, uint8_t* out) {
  if (!snest_md5salt(algo)) {
    if (slen) memcpy(out, salt, slen);
    return slen;
  }
  ShaBytes src;
  src.p = salt;
  src.n = slen;
  uint32_t d[4], m[8];
  md5_src_hd(src, slen, d);
  for (int i = 0; i < 4; i++) nest_hex_word<false, false>(d[i], m + 2 * i);
  memcpy(out, m, 32);  // (little-endian message words are the text's bytes on a little-endian host)
  return 32u;
}
// Record r (A5X_SNEST_STRIDE u32) of the caller's salt for a set of algo: the padded outer
// message with the text's bytes zero, as words of the outer byte order.
inline void snest_record(int algo, const uint8_t* salt, uint32_t slen, uint32_t index, uint32_t* r) {
  uint8_t eff[A5X_SALT_MAX], msg[128];
  const uint32_t el = snest_effective_salt(algo, salt, slen, eff);
  const uint32_t T = snest_in_sha1(algo) ? 40u : 32u, L = T + el, nb = L <= 55u ? 1u : 2u;
  const bool be = snest_out_sha1(algo);
  memset(msg, 0, sizeof msg);
  if (el) memcpy(msg + (snest_order(algo) == A5X_SALT_ORDER_SALT_PASS ? 0u : T), eff, el);
  msg[L] = 0x80;
  for (uint32_t k = 0; k < A5X_SNEST_STRIDE; k++) r[k] = 0u;
  r[A5X_SNEST_R_LEN] = el;
  r[A5X_SNEST_R_INDEX] = index;
  r[A5X_SNEST_R_NB] = nb;
  salt_mask(index, r + A5X_SNEST_R_MASK);
  for (uint32_t k = 0; k < 32u; k++) {
    const uint8_t* p = msg + 4u * k;
    r[A5X_SNEST_R_MSG + k] = be ? ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]
                                : ((uint32_t)p[3] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0];
  }
  r[A5X_SNEST_R_MSG + 16u * nb - (be ? 1u : 2u)] = L << 3;  // the bit length (< 2^32: one word)
}

// ---- host and device: the digests -----------------------------------------------------
// The inner digest of message bytes [0, len) of src (the source interface of md_src /
// sha_digest) as the HW words of its hex text in the outer function's byte order.
template <int ALGO, class S>
SNEST_HD void snest_inner(const S& src, uint32_t len, uint32_t* hexw) {
  typedef SaltNestCfg<ALGO> C;
  uint32_t in[C::IW];
  if constexpr (C::IN_SHA1) sha_digest<A5X_ALGO_SHA1>(src, len, in);
  else md5_src_hd(src, len, in);
#pragma unroll
  for (int i = 0; i < C::IW; i++) nest_hex_word<false, C::OUT_SHA1>(in[i], hexw + 2 * i);
}

// the outer function from its IV over nb (1 or 2) blocks of M; d = the digest in its standard
// byte order as NW little-endian words.  blk(b, M) fills block b's 16 words (b: the block
// number as a type, so that every index computed from it is a constant).
template <int ALGO, class F>
SNEST_HD void snest_outer(uint32_t nb, F blk, uint32_t* d) {
  typedef SaltNestCfg<ALGO> C;
  uint32_t M[16];
  if constexpr (C::OUT_SHA1) {
    uint32_t st[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
    blk(std::integral_constant<uint32_t, 0u>(), M);
    sha1_block(st, M);
    if (nb > 1u) {
      blk(std::integral_constant<uint32_t, 1u>(), M);
      sha1_block(st, M);
    }
#pragma unroll
    for (int i = 0; i < 5; i++) d[i] = sha_bswap(st[i]);
  } else {
    d[0] = 0x67452301u; d[1] = 0xefcdab89u; d[2] = 0x98badcfeu; d[3] = 0x10325476u;
    blk(std::integral_constant<uint32_t, 0u>(), M);
    md5_block_hd(d, M);
    if (nb > 1u) {
      blk(std::integral_constant<uint32_t, 1u>(), M);
      md5_block_hd(d, M);
    }
  }
}

// text . salt: the text's words, then the record's as they are
template <int ALGO>
SNEST_HD void snest_suffix(const uint32_t* hexw, const uint32_t* rec, uint32_t* d) {
  constexpr int HW = SaltNestCfg<ALGO>::HW;
  snest_outer<ALGO>(rec[A5X_SNEST_R_NB], [&](auto bc, uint32_t* M) {
    constexpr uint32_t b = decltype(bc)::value;
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = (b == 0u && k < HW) ? hexw[k] : rec[A5X_SNEST_R_MSG + 16u * b + k];
  }, d);
}

// text word cur behind text word prev (0 before the first), moved rs = slen & 3 bytes up the
// message: the message word that starts rs bytes before cur's first character
template <bool BE>
SNEST_HD uint32_t snest_shift(uint32_t cur, uint32_t prev, uint32_t rs) {
  if (rs == 0u) return cur;
  if constexpr (BE) return (cur >> (8u * rs)) | (prev << (32u - 8u * rs));
  else return rule_alignbyte(cur, prev, 4u - rs);
}
// salt . text, once per run of salts of slen bytes: the text at byte offset slen of an otherwise
// zero message, as its first A5X_SNEST_PW words Mt.  b: a working buffer of at least
// A5X_SNEST_PW dwords (B::rd / B::wr), the only thing here indexed by a runtime value.
template <int ALGO, class B>
SNEST_HD void snest_place(B& b, const uint32_t* hexw, uint32_t slen, uint32_t* Mt) {
  typedef SaltNestCfg<ALGO> C;
  const uint32_t qs = slen >> 2, rs = slen & 3u;
  for (uint32_t k = 0; k < A5X_SNEST_PW; k++) b.wr(k, 0u);
  uint32_t prev = 0u;
#pragma unroll
  for (int j = 0; j <= C::HW; j++) {
    const uint32_t cur = j < C::HW ? hexw[j] : 0u;
    b.wr(qs + (uint32_t)j, snest_shift<C::OUT_SHA1>(cur, prev, rs));  // (qs + HW <= 26 for slen <= A5X_SALT_MAX)
    prev = cur;
  }
#pragma unroll
  for (uint32_t k = 0; k < A5X_SNEST_PW; k++) Mt[k] = b.rd(k);
}
// one salt of the run: the placed text ORed with the record's words
template <int ALGO>
SNEST_HD void snest_prefix(const uint32_t* Mt, const uint32_t* rec, uint32_t* d) {
  snest_outer<ALGO>(rec[A5X_SNEST_R_NB], [&](auto bc, uint32_t* M) {
    constexpr uint32_t b = decltype(bc)::value;
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) {
      const uint32_t w = 16u * b + k;
      M[k] = rec[A5X_SNEST_R_MSG + w] | (w < A5X_SNEST_PW ? Mt[w] : 0u);
    }
  }, d);
}

// salt . text behind a salt of exactly 32 bytes (the MD5SALT form): the record's words [0, 8),
// the text's as words [8, 16), and a second block that is the record's alone
template <int ALGO>
SNEST_HD void snest_prefix_aligned(const uint32_t* hexw, const uint32_t* rec, uint32_t* d) {
  static_assert(SaltNestCfg<ALGO>::PREFIX && SaltNestCfg<ALGO>::MD5SALT && SaltNestCfg<ALGO>::HW == 8, "a 32-byte salt, a 32-byte text");
  snest_outer<ALGO>(2u, [&](auto bc, uint32_t* M) {
    constexpr uint32_t b = decltype(bc)::value;
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = (b == 0u && k >= 8) ? hexw[k - 8] : rec[A5X_SNEST_R_MSG + 16u * b + k];
  }, d);
}

// ---- the host path: one (candidate, salt) pair -------------------------------------------
// The digest of algo for candidate bytes [0, len) of src under the caller's salt, by the record
// preparation and the functions above; w: a working buffer of A5X_SNEST_PW dwords.  d gets
// a5x_digest_size(algo) / 4 words.  len <= A5X_RULE_LMAX, slen <= A5X_SALT_MAX.
template <int ALGO, class S>
inline void snest_pair_host(const S& src, uint32_t len, const uint8_t* salt, uint32_t slen, uint32_t* w, uint32_t* d) {
  typedef SaltNestCfg<ALGO> C;
  uint32_t rec[A5X_SNEST_STRIDE], hexw[C::HW];
  snest_record(ALGO, salt, slen, 0u, rec);
  snest_inner<ALGO>(src, len, hexw);
  if constexpr (C::PREFIX && !C::PLACED) {
    (void)w;
    snest_prefix_aligned<ALGO>(hexw, rec, d);
  } else if constexpr (C::PLACED) {
    uint32_t Mt[A5X_SNEST_PW];
    SaltBuf b;
    b.w = w;
    snest_place<ALGO>(b, hexw, rec[A5X_SNEST_R_LEN], Mt);
    snest_prefix<ALGO>(Mt, rec, d);
  } else {
    snest_suffix<ALGO>(hexw, rec, d);
  }
}
template <class S>
inline bool snest_pair_host_any(int algo, const S& src, uint32_t len, const uint8_t* salt, uint32_t slen, uint32_t* w,
                                uint32_t* d) {
  switch (algo) {
    case A5X_ALGO_MD5_MD5_SALT: snest_pair_host<A5X_ALGO_MD5_MD5_SALT>(src, len, salt, slen, w, d); return true;
    case A5X_ALGO_MD5_SALT_MD5: snest_pair_host<A5X_ALGO_MD5_SALT_MD5>(src, len, salt, slen, w, d); return true;
    case A5X_ALGO_MD5_MD5_MD5SALT: snest_pair_host<A5X_ALGO_MD5_MD5_MD5SALT>(src, len, salt, slen, w, d); return true;
    case A5X_ALGO_MD5_MD5SALT_MD5: snest_pair_host<A5X_ALGO_MD5_MD5SALT_MD5>(src, len, salt, slen, w, d); return true;
    case A5X_ALGO_SHA1_SHA1_SALT: snest_pair_host<A5X_ALGO_SHA1_SHA1_SALT>(src, len, salt, slen, w, d); return true;
    case A5X_ALGO_SHA1_SALT_SHA1: snest_pair_host<A5X_ALGO_SHA1_SALT_SHA1>(src, len, salt, slen, w, d); return true;
    case A5X_ALGO_SHA1_MD5_SALT: snest_pair_host<A5X_ALGO_SHA1_MD5_SALT>(src, len, salt, slen, w, d); return true;
    default: return false;
  }
}
