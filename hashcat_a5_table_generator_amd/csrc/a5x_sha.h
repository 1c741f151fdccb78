// a5x_sha.h -- SHA-1 / SHA-256 (FIPS 180-4) compression and the padded digest of one
// message, host and device (shared by the two-pass digest stream, a5x_digest.hip, and
// the host test hook a5x_debug_digest, a5x_host.cpp: the CPU suite runs the code the
// kernels run).  Message words are big-endian: one byte swap per loaded word, and the
// 64-bit bit length goes big-endian into M[14..15].
//
// Issue cost on gfx950 (DESIGN "Digest roofline"): the rotates are v_alignbit_b32 and the
// byte swaps v_perm_b32 (half rate, no full-rate form); Ch / Maj / Parity and the
// three-way XORs of the schedule and of the sigmas are one v_bitop3_b32 each (full rate).
#pragma once
#include <stdint.h>

#include "a5x.h"

#define SHA_HD __host__ __device__ __forceinline__

SHA_HD uint32_t sha_rotr(uint32_t x, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(x, x, s);
#else
  return (x >> s) | (x << (32u - s));
#endif
}
SHA_HD uint32_t sha_rotl(uint32_t x, uint32_t s) { return sha_rotr(x, 32u - s); }
SHA_HD uint32_t sha_bswap(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(0u, x, 0x00010203u);
#else
  return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
#endif
}

// Three-input bit functions: on the device one v_bitop3_b32 each, by its truth table over
// (x, y, z) = (0xf0, 0xcc, 0xaa).  Left to itself the compiler picks v_bfi_b32 (half rate)
// for Ch and two v_xor_b32 for a three-way XOR.
SHA_HD uint32_t sha_ch(uint32_t x, uint32_t y, uint32_t z) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(x, y, z, 0xca);
#else
  return (x & y) | (~x & z);
#endif
}
SHA_HD uint32_t sha_maj(uint32_t x, uint32_t y, uint32_t z) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(x, y, z, 0xe8);
#else
  return (x & y) | (x & z) | (y & z);
#endif
}
SHA_HD uint32_t sha_par(uint32_t x, uint32_t y, uint32_t z) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(x, y, z, 0x96);
#else
  return x ^ y ^ z;
#endif
}
#define SHA_CH(x, y, z) sha_ch(x, y, z)
#define SHA_MAJ(x, y, z) sha_maj(x, y, z)
#define SHA_PAR(x, y, z) sha_par(x, y, z)

// ---------------------------------------------------------------------------
// SHA-1: 80 steps, W[t] = rotl1(W[t-3] ^ W[t-8] ^ W[t-14] ^ W[t-16]) rolling in 16 words
// ---------------------------------------------------------------------------
#define S1_X(t) (W[(t) & 15] = sha_rotl(SHA_PAR(W[((t) - 3) & 15], W[((t) - 8) & 15], W[((t) - 14) & 15]) ^ W[(t) & 15], 1))
#define S1_W(t) ((t) < 16 ? W[(t) & 15] : S1_X(t))
#define S1_STEP(f, a, b, c, d, e, k, t)            \
  e += sha_rotl(a, 5) + f(b, c, d) + (k) + S1_W(t); \
  b = sha_rotl(b, 30);
#define S1_STEP5(f, k, t)                                                                \
  S1_STEP(f, a, b, c, d, e, k, (t)) S1_STEP(f, e, a, b, c, d, k, (t) + 1)                \
  S1_STEP(f, d, e, a, b, c, k, (t) + 2) S1_STEP(f, c, d, e, a, b, k, (t) + 3)            \
  S1_STEP(f, b, c, d, e, a, k, (t) + 4)

SHA_HD void sha1_block(uint32_t* st, const uint32_t* M) {
  uint32_t W[16];
#pragma unroll
  for (int i = 0; i < 16; i++) W[i] = M[i];
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
  S1_STEP5(SHA_CH, 0x5a827999u, 0) S1_STEP5(SHA_CH, 0x5a827999u, 5)
  S1_STEP5(SHA_CH, 0x5a827999u, 10) S1_STEP5(SHA_CH, 0x5a827999u, 15)
  S1_STEP5(SHA_PAR, 0x6ed9eba1u, 20) S1_STEP5(SHA_PAR, 0x6ed9eba1u, 25)
  S1_STEP5(SHA_PAR, 0x6ed9eba1u, 30) S1_STEP5(SHA_PAR, 0x6ed9eba1u, 35)
  S1_STEP5(SHA_MAJ, 0x8f1bbcdcu, 40) S1_STEP5(SHA_MAJ, 0x8f1bbcdcu, 45)
  S1_STEP5(SHA_MAJ, 0x8f1bbcdcu, 50) S1_STEP5(SHA_MAJ, 0x8f1bbcdcu, 55)
  S1_STEP5(SHA_PAR, 0xca62c1d6u, 60) S1_STEP5(SHA_PAR, 0xca62c1d6u, 65)
  S1_STEP5(SHA_PAR, 0xca62c1d6u, 70) S1_STEP5(SHA_PAR, 0xca62c1d6u, 75)
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e;
}

// ---------------------------------------------------------------------------
// SHA-256: 64 steps, W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16] rolling in 16 words
// ---------------------------------------------------------------------------
#define S256_BS0(x) SHA_PAR(sha_rotr(x, 2), sha_rotr(x, 13), sha_rotr(x, 22))
#define S256_BS1(x) SHA_PAR(sha_rotr(x, 6), sha_rotr(x, 11), sha_rotr(x, 25))
#define S256_SS0(x) SHA_PAR(sha_rotr(x, 7), sha_rotr(x, 18), (x) >> 3)
#define S256_SS1(x) SHA_PAR(sha_rotr(x, 17), sha_rotr(x, 19), (x) >> 10)
#define S256_X(t) \
  (W[(t) & 15] += S256_SS1(W[((t) - 2) & 15]) + W[((t) - 7) & 15] + S256_SS0(W[((t) - 15) & 15]))
#define S256_W(t) ((t) < 16 ? W[(t) & 15] : S256_X(t))
#define S256_STEP(a, b, c, d, e, f, g, h, k, t)                          \
  {                                                                      \
    const uint32_t t1 = h + S256_BS1(e) + SHA_CH(e, f, g) + (k) + S256_W(t); \
    d += t1;                                                             \
    h = t1 + S256_BS0(a) + SHA_MAJ(a, b, c);                             \
  }
#define S256_STEP8(t, k0, k1, k2, k3, k4, k5, k6, k7)                                             \
  S256_STEP(a, b, c, d, e, f, g, h, k0, (t)) S256_STEP(h, a, b, c, d, e, f, g, k1, (t) + 1)       \
  S256_STEP(g, h, a, b, c, d, e, f, k2, (t) + 2) S256_STEP(f, g, h, a, b, c, d, e, k3, (t) + 3)   \
  S256_STEP(e, f, g, h, a, b, c, d, k4, (t) + 4) S256_STEP(d, e, f, g, h, a, b, c, k5, (t) + 5)   \
  S256_STEP(c, d, e, f, g, h, a, b, k6, (t) + 6) S256_STEP(b, c, d, e, f, g, h, a, k7, (t) + 7)

SHA_HD void sha256_block(uint32_t* st, const uint32_t* M) {
  uint32_t W[16];
#pragma unroll
  for (int i = 0; i < 16; i++) W[i] = M[i];
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  S256_STEP8(0, 0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u)
  S256_STEP8(8, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u)
  S256_STEP8(16, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau)
  S256_STEP8(24, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u)
  S256_STEP8(32, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u)
  S256_STEP8(40, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u)
  S256_STEP8(48, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u)
  S256_STEP8(56, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u)
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// 32-bit words of the digest: 5 (SHA-1) / 8 (SHA-256)
template <int ALGO> struct ShaCfg { static constexpr int NW = ALGO == A5X_ALGO_SHA1 ? 5 : 8; };

// Merkle-Damgard over message bytes [0, len) of src (src.at4(i) = the 4 bytes at message
// offset i as a little-endian word; bytes past len are masked here, so a source may
// return anything for them): FIPS 180-4 padding (0x80, zeros, 64-bit big-endian bit
// length).  d = the digest in its standard byte order, as NW little-endian words (what
// the target table is keyed on and what op 2 of k_digest_stream stores).
template <int ALGO, class S>
SHA_HD void sha_digest(const S& src, uint32_t len, uint32_t* d) {
  constexpr int NW = ShaCfg<ALGO>::NW;
  uint32_t st[NW];
  st[0] = ALGO == A5X_ALGO_SHA1 ? 0x67452301u : 0x6a09e667u;
  st[1] = ALGO == A5X_ALGO_SHA1 ? 0xefcdab89u : 0xbb67ae85u;
  st[2] = ALGO == A5X_ALGO_SHA1 ? 0x98badcfeu : 0x3c6ef372u;
  st[3] = ALGO == A5X_ALGO_SHA1 ? 0x10325476u : 0xa54ff53au;
  st[4] = ALGO == A5X_ALGO_SHA1 ? 0xc3d2e1f0u : 0x510e527fu;
  if (NW == 8) {
    st[NW - 3] = 0x9b05688cu; st[NW - 2] = 0x1f83d9abu; st[NW - 1] = 0x5be0cd19u;
  }
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
      M[j] = sha_bswap((raw & keep) | pad);
    }
    if (blk == nb - 1) {
      M[14] = len >> 29;
      M[15] = len << 3;
    }
    if (ALGO == A5X_ALGO_SHA1) sha1_block(st, M); else sha256_block(st, M);
  }
#pragma unroll
  for (int i = 0; i < NW; i++) d[i] = sha_bswap(st[i]);
}

// message bytes in plain memory, readable only inside [0, n)
struct ShaBytes {
  const uint8_t* p;
  uint32_t n;
  SHA_HD uint32_t at4(uint32_t i) const {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; k++)
      if (i + k < n) v |= (uint32_t)p[i + k] << (8 * k);
    return v;
  }
};
