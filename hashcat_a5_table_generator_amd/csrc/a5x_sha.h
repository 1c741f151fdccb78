// a5x_sha.h -- SHA-1 / SHA-224 / SHA-256 / SHA-384 / SHA-512 (FIPS 180-4) compression and
// the padded digest of one message, host and device (shared by the two-pass digest stream,
// a5x_digest.hip, the rules stream, a5x_rules.hip, and the host test hook a5x_debug_digest,
// a5x_host.cpp: the CPU suite runs the code the kernels run).  Message words are
// big-endian: one byte swap per loaded 32-bit word, and the bit length goes big-endian into
// the block's last 64 (SHA-384 / SHA-512: 128) bits.
//
// Issue cost on gfx950 (DESIGN "Digest roofline"): the rotates are v_alignbit_b32 and the
// byte swaps v_perm_b32 (half rate, no full-rate form); Ch / Maj / Parity and the
// three-way XORs of the schedule and of the sigmas are one v_bitop3_b32 each (full rate).
#pragma once
#include <stdint.h>

#include "a5x.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHA_HD __host__ __device__ __forceinline__
#else
#define SHA_HD inline  // (a plain C++ build: tools/nest_selftest.cpp)
#endif

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

// ---------------------------------------------------------------------------
// SHA-512 / SHA-384: 80 steps on 64-bit words over 128-byte blocks,
// W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16] rolling in 16 words.
// gfx950 has no 64-bit rotate and no 64-bit three-input bit op (the plain C++ form, (x >> s) |
// (x << (64 - s)) and ^, goes through 64-bit shifts and two-input ops on each half).
// On the device a 64-bit value is worked on as its (lo, hi) halves: a rotate or
// shift by s < 32 is two v_alignbit_b32 across the halves (s >= 32: the halves swapped
// first, a register renaming), and the Sigmas, sigmas, Ch and Maj are one v_bitop3_b32 per
// half with the truth tables of sha_par / sha_ch / sha_maj.  The adds stay 64-bit
// (v_lshl_add_u64).  The host form is plain uint64_t arithmetic.
// ---------------------------------------------------------------------------
// (the device form is a bitcast of the register pair: written as lo | hi << 32 the compiler
// spends a v_lshl_add_u64 on it)
SHA_HD uint64_t sha_pack64(uint32_t lo, uint32_t hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t sha_u32x2 __attribute__((ext_vector_type(2)));
  const sha_u32x2 v = {lo, hi};
  return __builtin_bit_cast(uint64_t, v);
#else
  return (uint64_t)lo | ((uint64_t)hi << 32);
#endif
}
// x + y.  A5X_SHA512_CARRY (A/B knob): 0 = the compiler's v_lshl_add_u64 on register pairs, 1 =
// v_add_co_u32 + v_addc_co_u32 on the halves.  0 is kept: v_lshl_add_u64 issues like any VOP3
// op (~4 cycles), the pair costs ~8, and the interleaved carry chains through one VCC add
// v_cndmask / s_nop traffic on top (4371 -> 6165 instructions; DESIGN "SHA-224, SHA-384 and SHA-512")
#ifndef A5X_SHA512_CARRY
#define A5X_SHA512_CARRY 0
#endif
SHA_HD uint64_t sha_add64(uint64_t x, uint64_t y) {
#if defined(__HIP_DEVICE_COMPILE__) && A5X_SHA512_CARRY
  uint32_t c0, c1;
  const uint32_t lo = __builtin_addc((uint32_t)x, (uint32_t)y, 0u, &c0);
  const uint32_t hi = __builtin_addc((uint32_t)(x >> 32), (uint32_t)(y >> 32), c0, &c1);
  return sha_pack64(lo, hi);
#else
  return x + y;
#endif
}
// rotr(x, S), 0 < S < 64
template <uint32_t S> SHA_HD uint64_t sha_rotr64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lo = S >= 32u ? (uint32_t)(x >> 32) : (uint32_t)x;
  const uint32_t hi = S >= 32u ? (uint32_t)x : (uint32_t)(x >> 32);
  if (S == 32u) return sha_pack64(lo, hi);
  return sha_pack64(__builtin_amdgcn_alignbit(hi, lo, S & 31u), __builtin_amdgcn_alignbit(lo, hi, S & 31u));
#else
  return (x >> S) | (x << (64u - S));
#endif
}
// x >> S, 0 < S < 32
template <uint32_t S> SHA_HD uint64_t sha_shr64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  return sha_pack64(__builtin_amdgcn_alignbit(hi, lo, S), hi >> S);
#else
  return x >> S;
#endif
}
SHA_HD uint64_t sha_par64(uint64_t x, uint64_t y, uint64_t z) {
  return sha_pack64(sha_par((uint32_t)x, (uint32_t)y, (uint32_t)z),
                    sha_par((uint32_t)(x >> 32), (uint32_t)(y >> 32), (uint32_t)(z >> 32)));
}
SHA_HD uint64_t sha_ch64(uint64_t x, uint64_t y, uint64_t z) {
  return sha_pack64(sha_ch((uint32_t)x, (uint32_t)y, (uint32_t)z),
                    sha_ch((uint32_t)(x >> 32), (uint32_t)(y >> 32), (uint32_t)(z >> 32)));
}
SHA_HD uint64_t sha_maj64(uint64_t x, uint64_t y, uint64_t z) {
  return sha_pack64(sha_maj((uint32_t)x, (uint32_t)y, (uint32_t)z),
                    sha_maj((uint32_t)(x >> 32), (uint32_t)(y >> 32), (uint32_t)(z >> 32)));
}
#define S512_BS0(x) sha_par64(sha_rotr64<28>(x), sha_rotr64<34>(x), sha_rotr64<39>(x))
#define S512_BS1(x) sha_par64(sha_rotr64<14>(x), sha_rotr64<18>(x), sha_rotr64<41>(x))
#define S512_SS0(x) sha_par64(sha_rotr64<1>(x), sha_rotr64<8>(x), sha_shr64<7>(x))
#define S512_SS1(x) sha_par64(sha_rotr64<19>(x), sha_rotr64<61>(x), sha_shr64<6>(x))
#define S512_X(t)                                                                                 \
  (W[(t) & 15] = sha_add64(sha_add64(W[(t) & 15], S512_SS1(W[((t) - 2) & 15])),                   \
                           sha_add64(W[((t) - 7) & 15], S512_SS0(W[((t) - 15) & 15]))))
#define S512_W(t) ((t) < 16 ? W[(t) & 15] : S512_X(t))
#define S512_STEP(a, b, c, d, e, f, g, h, k, t)                                  \
  {                                                                              \
    const uint64_t t1 = sha_add64(sha_add64(sha_add64(h, S512_BS1(e)), sha_ch64(e, f, g)),   \
                                  sha_add64(S512_W(t), (k)));                                \
    d = sha_add64(d, t1);                                                                    \
    h = sha_add64(sha_add64(t1, S512_BS0(a)), sha_maj64(a, b, c));                           \
  }
#define S512_STEP8(t, k0, k1, k2, k3, k4, k5, k6, k7)                                             \
  S512_STEP(a, b, c, d, e, f, g, h, k0, (t)) S512_STEP(h, a, b, c, d, e, f, g, k1, (t) + 1)       \
  S512_STEP(g, h, a, b, c, d, e, f, k2, (t) + 2) S512_STEP(f, g, h, a, b, c, d, e, k3, (t) + 3)   \
  S512_STEP(e, f, g, h, a, b, c, d, k4, (t) + 4) S512_STEP(d, e, f, g, h, a, b, c, k5, (t) + 5)   \
  S512_STEP(c, d, e, f, g, h, a, b, k6, (t) + 6) S512_STEP(b, c, d, e, f, g, h, a, k7, (t) + 7)

SHA_HD void sha512_block(uint64_t* st, const uint64_t* M) {
  uint64_t W[16];
#pragma unroll
  for (int i = 0; i < 16; i++) W[i] = M[i];
  uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  S512_STEP8(0, 0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull)
  S512_STEP8(8, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull)
  S512_STEP8(16, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull)
  S512_STEP8(24, 0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull)
  S512_STEP8(32, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull)
  S512_STEP8(40, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull)
  S512_STEP8(48, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull)
  S512_STEP8(56, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull, 0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull)
  S512_STEP8(64, 0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull)
  S512_STEP8(72, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull)
  st[0] = sha_add64(st[0], a); st[1] = sha_add64(st[1], b); st[2] = sha_add64(st[2], c); st[3] = sha_add64(st[3], d);
  st[4] = sha_add64(st[4], e); st[5] = sha_add64(st[5], f); st[6] = sha_add64(st[6], g); st[7] = sha_add64(st[7], h);
}

// 32-bit words of the digest: 5 (SHA-1) / 7 (SHA-224) / 8 (SHA-256) / 12 (SHA-384) / 16
// (SHA-512); B64: the 64-bit line (SHA-384 / SHA-512)
template <int ALGO> struct ShaCfg {
  static constexpr bool B64 = ALGO == A5X_ALGO_SHA384 || ALGO == A5X_ALGO_SHA512;
  static constexpr int NW = ALGO == A5X_ALGO_SHA1 ? 5 : ALGO == A5X_ALGO_SHA224 ? 7 : ALGO == A5X_ALGO_SHA384 ? 12
                          : ALGO == A5X_ALGO_SHA512 ? 16 : 8;
  static constexpr int NS = ALGO == A5X_ALGO_SHA1 ? 5 : 8;  // 32-bit state words of the 32-bit line
};

// message bytes [b, b + 4) of a message of len bytes as the big-endian word FIPS 180-4
// hashes: the bytes past len masked, the 0x80 pad placed, no dword at or past len requested
template <class S>
SHA_HD uint32_t sha_mword(const S& src, uint32_t len, uint32_t b) {
  const int k = (int)len - (int)b;
  const uint32_t raw = k > 0 ? src.at4(b) : 0u;
  const uint32_t keep = k >= 4 ? 0xffffffffu : (k <= 0 ? 0u : ((1u << (8 * k)) - 1u));
  const uint32_t pad = (k >= 0 && k < 4) ? (0x80u << (8 * k)) : 0u;
  return sha_bswap((raw & keep) | pad);
}

// SHA-512 / SHA-384 of message bytes [0, len) of src: padding 0x80, zeros, the 128-bit
// big-endian bit length (len < 2^32: only its last two 32-bit words are non-zero);
// d = the first NW / 2 state words, each as two byte-swapped halves, high half first
template <int ALGO, class S>
SHA_HD void sha512_digest(const S& src, uint32_t len, uint32_t* d) {
  constexpr int NW = ShaCfg<ALGO>::NW;
  constexpr bool S384 = ALGO == A5X_ALGO_SHA384;
  uint64_t st[8];
  st[0] = S384 ? 0xcbbb9d5dc1059ed8ull : 0x6a09e667f3bcc908ull;
  st[1] = S384 ? 0x629a292a367cd507ull : 0xbb67ae8584caa73bull;
  st[2] = S384 ? 0x9159015a3070dd17ull : 0x3c6ef372fe94f82bull;
  st[3] = S384 ? 0x152fecd8f70e5939ull : 0xa54ff53a5f1d36f1ull;
  st[4] = S384 ? 0x67332667ffc00b31ull : 0x510e527fade682d1ull;
  st[5] = S384 ? 0x8eb44a8768581511ull : 0x9b05688c2b3e6c1full;
  st[6] = S384 ? 0xdb0c2e0d64f98fa7ull : 0x1f83d9abfb41bd6bull;
  st[7] = S384 ? 0x47b5481dbefa4fa4ull : 0x5be0cd19137e2179ull;
  const uint32_t nb = (len + 16u) / 128u + 1u;
  for (uint32_t blk = 0; blk < nb; blk++) {
    uint64_t M[16];
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
      const uint32_t b = blk * 128u + 8u * j;
      const uint32_t hi = sha_mword(src, len, b), lo = sha_mword(src, len, b + 4u);
      M[j] = sha_pack64(lo, hi);
    }
    if (blk == nb - 1) {
      M[14] = 0;
      M[15] = sha_pack64(len << 3, len >> 29);
    }
    sha512_block(st, M);
  }
#pragma unroll
  for (int i = 0; i < NW / 2; i++) {
    d[2 * i] = sha_bswap((uint32_t)(st[i] >> 32));
    d[2 * i + 1] = sha_bswap((uint32_t)st[i]);
  }
}

// Merkle-Damgard over message bytes [0, len) of src (src.at4(i) = the 4 bytes at message
// offset i as a little-endian word; bytes past len are masked here, so a source may
// return anything for them): FIPS 180-4 padding (0x80, zeros, 64-bit big-endian bit
// length).  d = the digest in its standard byte order, as NW little-endian words (what
// the target table is keyed on and what op 2 of k_digest_stream stores).  SHA-224 is
// SHA-256's compression from its own IV, the first 7 state words kept; SHA-384 / SHA-512
// go to sha512_digest (sha_digest below).
template <int ALGO, class S>
SHA_HD void sha32_digest(const S& src, uint32_t len, uint32_t* d) {
  constexpr int NW = ShaCfg<ALGO>::NW;
  constexpr int NS = ShaCfg<ALGO>::NS;
  constexpr bool S224 = ALGO == A5X_ALGO_SHA224;
  uint32_t st[NS];
  st[0] = ALGO == A5X_ALGO_SHA1 ? 0x67452301u : S224 ? 0xc1059ed8u : 0x6a09e667u;
  st[1] = ALGO == A5X_ALGO_SHA1 ? 0xefcdab89u : S224 ? 0x367cd507u : 0xbb67ae85u;
  st[2] = ALGO == A5X_ALGO_SHA1 ? 0x98badcfeu : S224 ? 0x3070dd17u : 0x3c6ef372u;
  st[3] = ALGO == A5X_ALGO_SHA1 ? 0x10325476u : S224 ? 0xf70e5939u : 0xa54ff53au;
  st[4] = ALGO == A5X_ALGO_SHA1 ? 0xc3d2e1f0u : S224 ? 0xffc00b31u : 0x510e527fu;
  if (NS == 8) {
    st[NS - 3] = S224 ? 0x68581511u : 0x9b05688cu;
    st[NS - 2] = S224 ? 0x64f98fa7u : 0x1f83d9abu;
    st[NS - 1] = S224 ? 0xbefa4fa4u : 0x5be0cd19u;
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

template <int ALGO, class S>
SHA_HD void sha_digest(const S& src, uint32_t len, uint32_t* d) {
  if constexpr (ShaCfg<ALGO>::B64) sha512_digest<ALGO>(src, len, d);
  else sha32_digest<ALGO>(src, len, d);
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
