// a5x_nest.h -- nested digests: a digest of the hex text of another digest, host and device
// (shared by the two-pass digest stream, a5x_digest_nest.hip, the rules stream,
// a5x_rules_nest.hip, and the host test hook a5x_debug_digest, a5x_host.cpp: the CPU suite
// runs the code the kernels run).
//
//   A5X_ALGO_MD5_MD5      md5(hex(md5(p)))            hashcat -m 2600
//   A5X_ALGO_MD5_MD5_MD5  md5(hex(md5(hex(md5(p)))))  -m 3500
//   A5X_ALGO_MD5_MD5UP    md5(HEX(md5(p)))            -m 4300
//   A5X_ALGO_MD5_SHA1     md5(hex(sha1(p)))           -m 4400
//   A5X_ALGO_SHA1_SHA1    sha1(hex(sha1(p)))          -m 4500
//   A5X_ALGO_SHA1_MD5     sha1(hex(md5(p)))           -m 4700
//   A5X_ALGO_SHA256_MD5   sha256(hex(md5(p)))         -m 20800
//
// Three stages, all in registers.  The inner digest is the length-generic core the plain
// algorithms run (MD5: the padded-source loop of md_src over md5_block; SHA-1: sha_digest),
// over any source with at4().  Its words are turned into hex text two message words per digest
// word: the word is split into its low and high nibbles (two AND, one shift), v_perm_b32
// interleaves them straight into the byte order the outer compression reads -- little-endian
// words for MD5, big-endian for SHA, so no byte swap stands between the stages -- and a SWAR
// step turns four nibbles at once into ASCII.  The outer message is 32 or 40 characters: with
// its 0x80 and its bit length it is always exactly one block whose pad and length words are
// compile-time constants, so the outer digest is one compression from the IV, not the
// length-driven loop.
#pragma once
#include <stdint.h>

#include "a5x.h"
#include "a5x_sha.h"
#if defined(__HIPCC__) || defined(__CUDACC__)
#include "a5x_md.h"
#endif

#define NEST_HD SHA_HD

// RFC 1321 compression on the host (the device core, md5_block of a5x_md.h, is device code)
inline void md5_block_host(uint32_t* st, const uint32_t* M) {
  static const uint32_t K[64] = {
      0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
      0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
      0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
      0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
      0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
      0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
      0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
      0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
  static const uint32_t R[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
  for (uint32_t i = 0; i < 64; i++) {
    uint32_t f, g;
    if (i < 16) { f = (b & c) | (~b & d); g = i; }
    else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
    else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
    else { f = c ^ (b | ~d); g = (7 * i) & 15; }
    const uint32_t x = a + f + K[i] + M[g], s = R[(i >> 4) * 4 + (i & 3)];
    a = d; d = c; c = b;
    b += (x << s) | (x >> (32 - s));
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}

// one MD5 compression: md5_block on the device, md5_block_host on the host
NEST_HD void md5_block_hd(uint32_t* st, const uint32_t* M) {
#if defined(__HIP_DEVICE_COMPILE__)
  md5_block(st, M);
#else
  md5_block_host(st, M);
#endif
}

// MD5 over message bytes [0, len) of src (src.at4(i) = the 4 bytes at message offset i as a
// little-endian word; bytes past len are masked here): RFC 1321 padding (0x80, zeros, 64-bit
// little-endian bit length); d = the digest as 4 little-endian words.  The loop of md_src
// (a5x_md.h) for host and device.
template <class S>
NEST_HD void md5_src_hd(const S& src, uint32_t len, uint32_t* d) {
  d[0] = 0x67452301u; d[1] = 0xefcdab89u; d[2] = 0x98badcfeu; d[3] = 0x10325476u;
  const uint32_t nb = (len + 8u) / 64u + 1u;
  for (uint32_t blk = 0; blk < nb; blk++) {
    uint32_t M[16];
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
      const uint32_t b = blk * 64u + 4u * j;
      const int k = (int)len - (int)b;
      const uint32_t raw = k > 0 ? src.at4(b) : 0u;
      const uint32_t keep = k >= 4 ? 0xffffffffu : (k <= 0 ? 0u : ((1u << (8 * k)) - 1u));
      const uint32_t pad = (k >= 0 && k < 4) ? (0x80u << (8 * k)) : 0u;
      M[j] = (raw & keep) | pad;
    }
    if (blk == nb - 1) {
      M[14] = len << 3;
      M[15] = len >> 29;
    }
    md5_block_hd(d, M);
  }
}

// which digests an algorithm nests, and how the text between them is written
template <int ALGO> struct NestCfg {
  static constexpr bool IN_SHA1 = ALGO == A5X_ALGO_MD5_SHA1 || ALGO == A5X_ALGO_SHA1_SHA1;  // else MD5
  static constexpr int OUT = ALGO == A5X_ALGO_SHA1_SHA1 || ALGO == A5X_ALGO_SHA1_MD5 ? A5X_ALGO_SHA1
                           : ALGO == A5X_ALGO_SHA256_MD5 ? A5X_ALGO_SHA256 : A5X_ALGO_MD5;
  static constexpr bool UPPER = ALGO == A5X_ALGO_MD5_MD5UP;
  static constexpr bool TRIPLE = ALGO == A5X_ALGO_MD5_MD5_MD5;
  static constexpr int IW = IN_SHA1 ? 5 : 4;                                          // inner digest words
  static constexpr int NW = OUT == A5X_ALGO_SHA1 ? 5 : OUT == A5X_ALGO_SHA256 ? 8 : 4;  // outer digest words
};

// bytes sel[0..3] of the eight bytes {hi, lo} (lo = bytes 0-3): v_perm_b32 for selectors < 8
NEST_HD uint32_t nest_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  uint32_t r = 0;
  for (uint32_t i = 0; i < 4; i++) r |= (uint32_t)((v >> (8 * ((sel >> (8 * i)) & 7u))) & 255u) << (8 * i);
  return r;
#endif
}

// four nibbles (one per byte, each <= 15) to their ASCII hex digits: + '0', and + 0x27 ('a' -
// '0' - 10; upper case 0x07) where the nibble is >= 10.  nibble + 6 carries into bit 4 exactly
// then, and per byte nothing exceeds 15 + 48 + 39, so no byte carries into the next.
template <bool UPPER>
NEST_HD uint32_t nest_hex4(uint32_t x) {
  return x + 0x30303030u + (((x + 0x06060606u) >> 4) & 0x01010101u) * (UPPER ? 0x07u : 0x27u);
}

// The 8 hex characters of digest word w (a little-endian word of the digest's byte order:
// byte k of w is digest byte k) as the two message words m[0], m[1] of the outer compression:
// BE false: little-endian words (MD5), character c at bits 8c; BE true: big-endian (SHA).
// Character 2k is the high nibble of byte k, character 2k + 1 its low nibble.
template <bool UPPER, bool BE>
NEST_HD void nest_hex_word(uint32_t w, uint32_t* m) {
  const uint32_t lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;
  // {hi, lo} bytes: 0-3 the low nibbles of bytes 0-3, 4-7 the high nibbles
  const uint32_t a = nest_perm(hi, lo, BE ? 0x04000501u : 0x01050004u);
  const uint32_t b = nest_perm(hi, lo, BE ? 0x06020703u : 0x03070206u);
  m[0] = nest_hex4<UPPER>(a);
  m[1] = nest_hex4<UPPER>(b);
}

// The outer digest: OUT over the 8 * IW hex characters of the IW inner digest words in (32 or
// 40 bytes: with the 0x80 byte and the 64-bit length exactly one block).  M is built in
// registers -- the hex words, the pad word, zeros, the constant bit length -- and compressed
// once from the IV.  d = the digest in its standard byte order as little-endian words.
template <int OUT, int IW, bool UPPER>
NEST_HD void nest_outer(const uint32_t* in, uint32_t* d) {
  constexpr bool BE = OUT != A5X_ALGO_MD5;
  constexpr uint32_t BITS = 64u * IW;  // 8 characters of 8 bits per word
  static_assert(2 * IW + 1 <= 14, "the text, its pad and the length fit one block");
  uint32_t M[16];
#pragma unroll
  for (int i = 0; i < IW; i++) nest_hex_word<UPPER, BE>(in[i], M + 2 * i);
  M[2 * IW] = BE ? 0x80000000u : 0x80u;
#pragma unroll
  for (int i = 2 * IW + 1; i < 14; i++) M[i] = 0u;
  M[14] = BE ? 0u : BITS;
  M[15] = BE ? BITS : 0u;
  if constexpr (OUT == A5X_ALGO_MD5) {
    d[0] = 0x67452301u; d[1] = 0xefcdab89u; d[2] = 0x98badcfeu; d[3] = 0x10325476u;
    md5_block_hd(d, M);
  } else if constexpr (OUT == A5X_ALGO_SHA1) {
    uint32_t st[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
    sha1_block(st, M);
#pragma unroll
    for (int i = 0; i < 5; i++) d[i] = sha_bswap(st[i]);
  } else {
    uint32_t st[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    sha256_block(st, M);
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = sha_bswap(st[i]);
  }
}

// The nested digest ALGO of message bytes [0, len) of src (the source interface of md_src /
// sha_digest: src.at4(i)); d = the outer digest in its standard byte order as NestCfg<ALGO>::NW
// little-endian words (what the target table is keyed on and what op 2 of k_digest_stream
// stores).  The triple form repeats hex + block.
template <int ALGO, class S>
NEST_HD void nest_digest(const S& src, uint32_t len, uint32_t* d) {
  typedef NestCfg<ALGO> C;
  uint32_t in[C::IW];
  if constexpr (C::IN_SHA1) sha_digest<A5X_ALGO_SHA1>(src, len, in);
  else md5_src_hd(src, len, in);
  if constexpr (C::TRIPLE) {
    uint32_t mid[4];
    nest_outer<A5X_ALGO_MD5, 4, false>(in, mid);
    nest_outer<A5X_ALGO_MD5, 4, false>(mid, d);
  } else {
    nest_outer<C::OUT, C::IW, C::UPPER>(in, d);
  }
}
