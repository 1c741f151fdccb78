// a5x_pbkdf2.h -- PBKDF2 (RFC 8018) over HMAC-MD5 / -SHA1 / -SHA256 / -SHA512 with the candidate
// as the password; host and device (shared by the iterated kernels, a5x_pbkdf2.hip, the host hook
// a5x_debug_pbkdf2 and the hit check of a5x_format_hits_iterated, a5x_host.cpp, and the
// stand-alone self-test, tools/pbkdf2_selftest.cpp: the CPU suite runs the code the kernels run).
//
//   A5X_ALGO_PBKDF2_HMAC_MD5     hashcat -m 11900
//   A5X_ALGO_PBKDF2_HMAC_SHA1    -m 12000
//   A5X_ALGO_PBKDF2_HMAC_SHA256  -m 10900
//   A5X_ALGO_PBKDF2_HMAC_SHA512  -m 12100
//
// T_i = U_1 ^ U_2 ^ ... ^ U_c, U_1 = HMAC(P, S . INT(i)), U_j = HMAC(P, U_{j-1}).  Everything is
// a5x_hmac.h's key = pass HMAC: the two key states of the candidate (hmac_key_states, once per
// candidate, a key over 64 bytes of a 64-byte-block hash replaced by its digest there), the
// message S . INT(i) as finished padded words in the salt record (pbkdf2_record_of,
// hmac_inner_from_record), and from U_2 on two compressions of one fixed shape: a digest's worth
// of words, the 0x80 byte, zeros, the bit length (B + digest bytes) * 8 -- hmac_outer's block,
// from the inner key state and then from the outer one (pbkdf2_step).  u and t are kept as the
// hash's own state words, so an iteration swaps no byte; the digest's byte order is made once,
// where t is compared or written (pbkdf2_t_words, pbkdf2_t_bytes).
//
// A target matches on the first 16 bytes of T_1 (PBKDF2_KEEP state words): the kernels keep that
// much of t and all of u; the host path keeps all of t and computes every block of any dkLen.
#pragma once
#include "a5x_hmac.h"

// One record of the device salt table of an iterated set: a5x_hmac.h's key = pass record of the
// message salt . INT(1) -- [0] the length of the salt alone, [1] the public index of the (salt,
// iterations) pair, [2] the blocks of the padded message (1 up to a 51-byte salt, then 2;
// SHA-512: 1), [4..7] the probe mask, [8..39] the padded words -- with the iteration count in [3].
#define A5X_PBKDF2_STRIDE A5X_HMAC_STRIDE
#define A5X_PBKDF2_R_ITERS 3u
#define A5X_PBKDF2_KEEP_BYTES 16u

constexpr bool a5x_algo_pbkdf2(int algo) {
  return algo >= A5X_ALGO_PBKDF2_HMAC_MD5 && algo <= A5X_ALGO_PBKDF2_HMAC_SHA512;
}

template <int ALGO> struct Pbkdf2Cfg {
  static_assert(a5x_algo_pbkdf2(ALGO), "a PBKDF2 algorithm");
  // the HMAC underneath: its key = pass form
  static constexpr int HM = ALGO == A5X_ALGO_PBKDF2_HMAC_MD5 ? A5X_ALGO_HMAC_MD5_KEY_PASS
                          : ALGO == A5X_ALGO_PBKDF2_HMAC_SHA1 ? A5X_ALGO_HMAC_SHA1_KEY_PASS
                          : ALGO == A5X_ALGO_PBKDF2_HMAC_SHA256 ? A5X_ALGO_HMAC_SHA256_KEY_PASS
                                                                : A5X_ALGO_HMAC_SHA512_KEY_PASS;
  typedef HmacCfg<HM> C;
  typedef typename C::W W;
  static constexpr int NS = C::NS;
  static constexpr int KEEP = C::B64 ? 2 : 4;            // state words of the 16 compared bytes
  static constexpr uint32_t NSW = C::B64 ? 16u : (uint32_t)C::NS;  // u32 of one state
  static constexpr uint32_t HLEN = 4u * (uint32_t)C::NW;  // bytes of one block T_i
  // u32 of one pair's state in HBM: block, ordinal in block, ist, ost, u, t[0..16 B)
  static constexpr uint32_t STATE_WORDS = 2u + 3u * NSW + 4u;
};

// the record of salt . INT(blockno) for a set of ALGO (the device table: blockno 1)
template <int ALGO>
inline void pbkdf2_record_of(const uint8_t* salt, uint32_t slen, uint32_t index, uint32_t iters, uint32_t blockno,
                             uint32_t* r) {
  uint8_t msg[A5X_SALT_MAX + 4u];
  if (slen) memcpy(msg, salt, slen);
  msg[slen] = (uint8_t)(blockno >> 24);
  msg[slen + 1] = (uint8_t)(blockno >> 16);
  msg[slen + 2] = (uint8_t)(blockno >> 8);
  msg[slen + 3] = (uint8_t)blockno;
  hmac_record_of<Pbkdf2Cfg<ALGO>::HM>(msg, slen + 4u, index, r);
  r[A5X_HMAC_R_LEN] = slen;
  r[A5X_PBKDF2_R_ITERS] = iters;
}

// One compression of the iteration's fixed shape from a key state: hmac_outer's block, the
// result left as state words.
template <int ALGO>
HMAC_HD void pbkdf2_step(const typename Pbkdf2Cfg<ALGO>::W* kst, const typename Pbkdf2Cfg<ALGO>::W* in,
                         typename Pbkdf2Cfg<ALGO>::W* out) {
  typedef typename Pbkdf2Cfg<ALGO>::C C;
  typedef typename C::W W;
  constexpr uint32_t BITS = (C::B + 4u * (uint32_t)C::NW) * 8u;
  W M[16];
#pragma unroll
  for (int k = 0; k < 16; k++) M[k] = k < C::NS ? in[k] : (W)0;
  M[C::NS] = C::B64 ? (W)0x8000000000000000ull : C::BE ? (W)0x80000000u : (W)0x80u;
  if constexpr (C::BE) M[15] = BITS; else M[14] = BITS;
#pragma unroll
  for (int i = 0; i < C::NS; i++) out[i] = kst[i];
  hmac_block<Pbkdf2Cfg<ALGO>::HM>(out, M);
}

// U_1 from the candidate's key states and the record; t starts as its first TN words
template <int ALGO, int TN>
HMAC_HD void pbkdf2_first(const typename Pbkdf2Cfg<ALGO>::W* ist, const typename Pbkdf2Cfg<ALGO>::W* ost,
                          const uint32_t* rec, uint32_t nb, typename Pbkdf2Cfg<ALGO>::W* u,
                          typename Pbkdf2Cfg<ALGO>::W* t) {
  typedef Pbkdf2Cfg<ALGO> P;
  typename P::W st[P::NS];
  hmac_inner_from_record<P::HM>(ist, rec, nb, st);
  pbkdf2_step<ALGO>(ost, st, u);
#pragma unroll
  for (int i = 0; i < TN; i++) t[i] = u[i];
}

// one iteration: u = outer(ost, outer-shaped inner(ist, u)), the first TN words of it into t
template <int ALGO, int TN>
HMAC_HD void pbkdf2_iter(const typename Pbkdf2Cfg<ALGO>::W* ist, const typename Pbkdf2Cfg<ALGO>::W* ost,
                         typename Pbkdf2Cfg<ALGO>::W* u, typename Pbkdf2Cfg<ALGO>::W* t) {
  typedef Pbkdf2Cfg<ALGO> P;
  typename P::W x[P::NS];
  pbkdf2_step<ALGO>(ist, u, x);
  pbkdf2_step<ALGO>(ost, x, u);
#pragma unroll
  for (int i = 0; i < TN; i++) t[i] ^= u[i];
}

// the first 16 bytes of t in the digest's byte order as four little-endian words (what the
// target table is keyed on, what a hit holds and what op 2 stores)
template <int ALGO>
HMAC_HD void pbkdf2_t_words(const typename Pbkdf2Cfg<ALGO>::W* t, uint32_t* d) {
  typedef typename Pbkdf2Cfg<ALGO>::C C;
  if constexpr (C::B64) {
    d[0] = sha_bswap((uint32_t)(t[0] >> 32)); d[1] = sha_bswap((uint32_t)t[0]);
    d[2] = sha_bswap((uint32_t)(t[1] >> 32)); d[3] = sha_bswap((uint32_t)t[1]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) d[i] = C::BE ? sha_bswap((uint32_t)t[i]) : (uint32_t)t[i];
  }
}

// ---- the host path -----------------------------------------------------------------------
// the HLEN bytes of a whole block T
template <int ALGO>
inline void pbkdf2_t_bytes(const typename Pbkdf2Cfg<ALGO>::W* t, uint8_t* out) {
  typedef Pbkdf2Cfg<ALGO> P;
  typedef typename P::C C;
  constexpr int WB = C::B64 ? 8 : 4;
  for (int i = 0; i < P::NS; i++)
    for (int b = 0; b < WB; b++) out[WB * i + b] = (uint8_t)(t[i] >> (C::BE ? 8 * (WB - 1 - b) : 8 * b));
}

// The derived key of dklen bytes for candidate bytes [0, len) of src, the caller's salt and c >= 1
// iterations: every block T_1..T_n by the record preparation and the pieces above, in the
// kernels' order.  len <= A5X_RULE_LMAX, slen <= A5X_SALT_MAX.
template <int ALGO, class S>
inline void pbkdf2_host(const S& src, uint32_t len, const uint8_t* salt, uint32_t slen, uint32_t c, uint8_t* out,
                        size_t dklen) {
  typedef Pbkdf2Cfg<ALGO> P;
  typedef typename P::W W;
  W ist[P::NS], ost[P::NS], u[P::NS], t[P::NS];
  hmac_key_states<P::HM>(src, len, ist, ost);
  uint32_t blockno = 1;
  for (size_t done = 0; done < dklen; done += P::HLEN, blockno++) {
    uint32_t rec[A5X_PBKDF2_STRIDE];
    uint8_t tb[64];
    pbkdf2_record_of<ALGO>(salt, slen, 0u, c, blockno, rec);
    pbkdf2_first<ALGO, P::NS>(ist, ost, rec, rec[A5X_HMAC_R_NB], u, t);
    for (uint32_t j = 1; j < c; j++) pbkdf2_iter<ALGO, P::NS>(ist, ost, u, t);
    pbkdf2_t_bytes<ALGO>(t, tb);
    const size_t n = dklen - done < P::HLEN ? dklen - done : (size_t)P::HLEN;
    memcpy(out + done, tb, n);
  }
}

#define A5X_PBKDF2_EACH(X) \
  X(A5X_ALGO_PBKDF2_HMAC_MD5) X(A5X_ALGO_PBKDF2_HMAC_SHA1) X(A5X_ALGO_PBKDF2_HMAC_SHA256) X(A5X_ALGO_PBKDF2_HMAC_SHA512)

// the same by value; false: no PBKDF2 algorithm
inline bool pbkdf2_record(int algo, const uint8_t* salt, uint32_t slen, uint32_t index, uint32_t iters, uint32_t* r) {
  switch (algo) {
#define X(A) case A: pbkdf2_record_of<A>(salt, slen, index, iters, 1u, r); return true;
    A5X_PBKDF2_EACH(X)
#undef X
    default: return false;
  }
}
template <class S>
inline bool pbkdf2_host_any(int algo, const S& src, uint32_t len, const uint8_t* salt, uint32_t slen, uint32_t c,
                            uint8_t* out, size_t dklen) {
  switch (algo) {
#define X(A) case A: pbkdf2_host<A>(src, len, salt, slen, c, out, dklen); return true;
    A5X_PBKDF2_EACH(X)
#undef X
    default: return false;
  }
}
// u32 of one pair's state (Pbkdf2Cfg::STATE_WORDS); 0: no PBKDF2 algorithm
constexpr uint32_t pbkdf2_state_words(int algo) {
  return algo == A5X_ALGO_PBKDF2_HMAC_MD5 ? Pbkdf2Cfg<A5X_ALGO_PBKDF2_HMAC_MD5>::STATE_WORDS
       : algo == A5X_ALGO_PBKDF2_HMAC_SHA1 ? Pbkdf2Cfg<A5X_ALGO_PBKDF2_HMAC_SHA1>::STATE_WORDS
       : algo == A5X_ALGO_PBKDF2_HMAC_SHA256 ? Pbkdf2Cfg<A5X_ALGO_PBKDF2_HMAC_SHA256>::STATE_WORDS
       : algo == A5X_ALGO_PBKDF2_HMAC_SHA512 ? Pbkdf2Cfg<A5X_ALGO_PBKDF2_HMAC_SHA512>::STATE_WORDS : 0u;
}
