// a5x_hmac.hip -- HMAC target lists in the digest + lookup stage: HMAC-MD5 / -SHA1 / -SHA256 /
// -SHA512 with the candidate as the key and the salt as the message (hashcat -m 50 / 150 / 1450 /
// 1750) or the reverse (-m 60 / 160 / 1460 / 1760); a5x_hmac.h has the table and the split.
//
// k_hmac_stream has k_salt_nest_stream's shape (a5x_salt_nest.hip): one wave stages a 4 KiB
// block of the "cand\n" stream (+256 B of the next) in LDS once, and for each round of 64
// candidates (lane = candidate) does the candidate's share of the work once, straight from the
// staged line, and keeps it in registers; then it runs every salt of the target set over it.
//   key = pass: the two key states (8 / 10 / 16 / 32 dwords).  Per salt the record (wave-
//     uniform: scalar loads) is the whole padded inner message: one compression or two from the
//     inner key state, by a wave-uniform branch on the record's block count, then the outer block.
//   key = salt: the candidate's padded message block, when every candidate of the round ends in
//     its first block (a wave-uniform vote) -- else the candidate is hashed from the staged line
//     per salt.  Per salt the record holds both key states: the inner hash starts from a wave-
//     uniform state, then the outer block.
// Nothing is placed at a runtime byte offset, so no kernel here has a lane buffer: all launch
// with the staged block and the start list alone.  The digest is XORed with the salt's 128-bit
// mask and probed exactly as in k_salt_stream.
//
// The front half (staging, SWAR newline scan, per-round start lists) is k_salt_stream's text,
// for the reason a5x_stream.h gives; the geometry, the hit record and k_hits_resolve's block
// ordinals are a5x_stream.h's.
#include "a5x_stream.h"

#include "a5x_hmac.h"

namespace {

// the candidate in the staged stream: 4 bytes at candidate offset i (line starts are byte
// aligned: funnel reads; the bytes past the candidate are masked by the message loops)
struct HmCand {
  const uint8_t* base;
  u32 s;
  __device__ __forceinline__ u32 at4(u32 i) const { return lds4(base, s + i); }
};

// a wave's LDS: the staged block and the round's start list (SnWaveSmall's layout)
struct HmWave {
  uint8_t data[STREAM_BUF<STREAM_BLK>];
  uint16_t starts[72];  // the round's 64 line starts + the next one
};
static_assert(sizeof(HmWave) == 4576, "eight workgroups of STREAM_WAVES waves fit a CU's LDS");
constexpr u32 HM_WAVE_BYTES = ((u32)sizeof(HmWave) + 15u) & ~15u;


// key = salt, the round's one-block form: the candidate's block M1 does not change over the salt
// loop, and left to itself the compiler hoists everything of the inner compression that depends
// on M1 alone out of that loop -- the whole message schedule of the SHA functions, MD5's M + K
// sums -- and holds it in registers.  Where that is wanted the loop is left alone; where not, M1
// is passed through an empty asm per salt, which costs no instruction and makes it opaque.
// Measured on C5 under 64 salts / one salt, 1e9 pairs/s, hoisted against opaque (DESIGN "HMAC
// target lists"): SHA-1 26.4 / 14.2 against 25.1 / 17.6 (199 against 125 VGPRs), SHA-256 13.2 /
// 8.5 against 11.4 / 9.2 (198 against 130): hoisted, for the lists with many salts.  MD5 37.5 /
// 18.7 against 42.9 / 24.7 (184 against 122 VGPRs: it saves one add a step and loses two waves
// a SIMD): opaque.  SHA-512: 160 schedule dwords do not fit (256 VGPRs and 114 more held in
// AGPRs, one wave a SIMD): opaque.
template <int ALGO>
constexpr bool HM_HOIST = HmacCfg<ALGO>::HASH == A5X_ALGO_SHA1 || HmacCfg<ALGO>::HASH == A5X_ALGO_SHA256;

// op 0: every (candidate, salt) hashed and probed under the salt's mask, hits recorded with
// their salt index; op 1: count line starts per block; op 2: every digest written at
// dig_out[4 * DW * ((blk_pre[blk] + i) * S + salt index)], zeros for a line over A5X_RULE_LMAX
template <int ALGO>
__global__ void __launch_bounds__(64 * STREAM_WAVES) k_hmac_stream(A5xSaltLaunch q, int op) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  typedef HmacCfg<ALGO> C;
  typedef typename C::W HW;
  const A5xDigLaunch& a = q.d;
  const u32 wv = threadIdx.x / 64, lane = __lane_id();
  const u32 nwv = blockDim.x / 64;
  constexpr u32 DW = StreamCfg<ALGO>::DW;
  constexpr u32 HT = StreamCfg<ALGO>::HT;
  static_assert(DW == (u32)C::NW, "the digest's width");
  constexpr u32 NM = STREAM_BLK / 2048u;  // 32-bit newline masks per lane (32 B each)
  static_assert(NM == 2, "a lane's starts are kept in one 64-bit mask");
  HmWave& W = *(HmWave*)(s_dyn + wv * HM_WAVE_BYTES);
  const u64 nblk = (a.nbytes + STREAM_BLK - 1) / STREAM_BLK;
  const u32 S = q.nsalts;
  u32 err = 0, nskip = 0;
  for (u64 blk = (u64)blockIdx.x * nwv + wv; blk < nblk; blk += (u64)gridDim.x * nwv) {
    const u64 bs = blk * STREAM_BLK;
    const u32 bl = (u32)min<u64>(STREAM_BLK, a.nbytes - bs);             // block bytes
    const u32 sl = (u32)min<u64>(STREAM_BLK + STREAM_MARGIN, a.nbytes - bs);   // staged bytes
    __builtin_amdgcn_wave_barrier();
    const uint4* g16 = (const uint4*)(a.out + bs);
    uint4* l16 = (uint4*)W.data;
    for (u32 i = lane; i < sl / 16; i += 64) l16[i] = g16[i];
    for (u32 i = (sl & ~15u) + lane; i < sl; i += 64) W.data[i] = a.out[bs + i];
    for (u32 i = sl + lane; i < STREAM_BUF<STREAM_BLK>; i += 64) W.data[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // newline bits of this lane's slice (NM x 32 bytes), as k_digest_stream
    const u32 q0 = lane * 32u * NM;
    u32 nl[NM], sm[NM];
#pragma unroll
    for (u32 h = 0; h < NM; h++) nl[h] = 0;
#pragma unroll
    for (u32 j = 0; j < 8 * NM; j++) {
      const u32 x = ((const u32*)W.data)[lane * 8 * NM + j] ^ 0x0a0a0a0au;
      const u32 t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);  // 0x80 where the byte is '\n'
      const u32 f = ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
      nl[j >> 3] |= f << (4 * (j & 7));
    }
    auto keep = [&](u32 base) -> u32 {
      return base >= bl ? 0u : (base + 32u <= bl ? 0xffffffffu : ((1u << (bl - base)) - 1u));
    };
#pragma unroll
    for (u32 h = 0; h < NM; h++) nl[h] &= keep(q0 + 32u * h);
    // line starts: byte 0 of the stream, and every byte after a '\n'
    u32 carry = (u32)__shfl_up((int)(nl[NM - 1] >> 31), 1, 64);
    if (lane == 0) carry = bs == 0 ? 1u : (a.out[bs - 1] == '\n' ? 1u : 0u);
    u32 m = 0;
#pragma unroll
    for (u32 h = 0; h < NM; h++) {
      sm[h] = ((nl[h] << 1) | (h ? (nl[h - 1] >> 31) : carry)) & keep(q0 + 32u * h);
      m += (u32)__builtin_popcount(sm[h]);
    }
    const u32 incl = wave_incl_scan(m);
    const u32 nst = (u32)__builtin_amdgcn_readlane((int)incl, 63);
    u32 ord = incl - m;  // ordinal of this lane's next unlisted start
    u64 sm64 = (u64)sm[0] | ((u64)sm[1] << 32);  // this lane's unlisted starts (bit = byte of its 64-B slice)
    if (lane == 0 && a.blk_cnt) a.blk_cnt[blk] = nst;  // ordinals of hits (k_hits_resolve)
    if (op == 1) continue;
    // end of the block's last line: the first '\n' at or after the last start, in the staged
    // bytes; the stream's end for an unterminated last line; none: longer than the margin
    u32 last_start = 0;
    {
      const u32 ls = sm64 ? q0 + 63u - (u32)__builtin_clzll(sm64) : 0u;
      const u64 bal = __ballot(m != 0);
      if (bal) last_start = (u32)__builtin_amdgcn_readlane((int)ls, 63 - __builtin_clzll(bal));
    }
    u32 tail_end = 0xffffffffu;
    if (nst) {
      for (u32 base = last_start; base < sl && tail_end == 0xffffffffu; base += 64) {
        const u32 p = base + lane;
        const u64 bal = __ballot(p < sl && W.data[p] == '\n');
        if (bal) tail_end = base + (u32)__builtin_ctzll(bal);
      }
      if (tail_end == 0xffffffffu && sl < STREAM_BLK + STREAM_MARGIN) tail_end = sl;
    }
    for (u32 r0 = 0; r0 < nst; r0 += 64) {
      // the round's starts: every lane lists its own whose ordinal is in [r0, r0 + 64]
      __builtin_amdgcn_wave_barrier();
      while (sm64 && ord <= r0 + 64u) {
        W.starts[ord - r0] = (uint16_t)(q0 + (u32)__builtin_ctzll(sm64));
        if (ord == r0 + 64u) break;  // the next round's first start: listed there again
        sm64 &= sm64 - 1u;
        ord++;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const u32 i = r0 + lane;
      const bool valid = i < nst;
      u32 s = 0, len = 0;
      if (valid) {
        s = W.starts[lane];
        const u32 e = i + 1 < nst ? (u32)W.starts[lane + 1] - 1u : tail_end;  // '\n' position
        len = e == 0xffffffffu ? 0xffffffffu : e - s;
      }
      // a line over A5X_RULE_LMAX may end past the staged bytes: hashed under no salt, S skipped pairs
      const bool act = valid && len <= A5X_RULE_LMAX;
      nskip += (valid && !act) ? S : 0u;
      u64 row = 0;
      if (op == 2 && valid) row = (a.blk_pre[blk] + i) * S;
      HmCand cand;
      cand.base = W.data;
      cand.s = act ? s : 0u;
      const u32 clen = act ? len : 0u;
      // the candidate's share, once for the round's salts
      [[maybe_unused]] HW kist[C::NS], kost[C::NS];  // key = pass: the key states
      [[maybe_unused]] HW M1[16];                    // key = salt: the candidate's one block
      [[maybe_unused]] bool one = false;             // ... which every lane of the round has (wave-uniform)
      if constexpr (C::KEY_PASS) {
        hmac_key_states<ALGO>(cand, clen, kist, kost);
      } else {
        one = __builtin_amdgcn_ballot_w64(clen > C::ONE) == 0ull;
        if (one) hmac_msg_words<ALGO>(cand, clen, C::B, 0u, true, M1);
      }
      for (u32 si = 0; si < S; si++) {
        const u32* rec = q.salts + (u64)si * A5X_HMAC_STRIDE;  // wave-uniform: scalar loads
        u32 d[DW];
        HW st[C::NS];
        if constexpr (C::KEY_PASS) {
          // (the block count through readfirstlane: the branch on it is uniform by construction)
          const u32 nb = (u32)__builtin_amdgcn_readfirstlane((int)rec[A5X_HMAC_R_NB]);
          hmac_inner_from_record<ALGO>(kist, rec, nb, st);
          hmac_outer<ALGO>(kost, st, d);
        } else {
          HW ost[C::NS];
          hmac_state_from_record<ALGO>(rec, A5X_HMAC_R_BODY, st);
          if (one) {
            if constexpr (!HM_HOIST<ALGO>) {
#pragma unroll
              for (int k = 0; k < 16; k++) asm volatile("" : "+v"(M1[k]));
            }
            hmac_block<ALGO>(st, M1);
          } else {
            hmac_hash_from<ALGO>(cand, clen, C::B, st);
          }
          hmac_state_from_record<ALGO>(rec, A5X_HMAC_R_OST, ost);
          hmac_outer<ALGO>(ost, st, d);
        }
        const u32 sidx = rec[A5X_HMAC_R_INDEX];
        if (op == 2) {
          if (valid) {
            u32* o1 = (u32*)(a.dig_out + 4ull * DW * (row + sidx));
#pragma unroll
            for (u32 k = 0; k < DW; k++) o1[k] = act ? d[k] : 0u;
          }
          continue;
        }
        bool hit = false;
        if (act) {
          // the probe key: the salt's mask over the first four words, the tail as it is
          u32 key[DW];
#pragma unroll
          for (u32 k = 0; k < DW; k++) key[k] = k < 4 ? d[k] ^ rec[A5X_HMAC_R_MASK + k] : d[k];
          if constexpr (DW == 4)
            hit = md_probe(a.bitmap, a.bm_mask, a.table, a.tmask, a.has_zero_target != 0, key);
          else
            hit = md_probe_wide<(int)DW - 4>(a.bitmap, a.bm_mask, a.table, a.tails, a.tmask, a.has_zero_target != 0,
                                             a.ztails, a.nztails, key);
        }
        if (hit) {
          const u32 h = atomicAdd(a.nhits, 1u);
          if (h < a.hit_cap) stream_write_hit<DW, HT, true>(a.hits, a.hit_tail, h, blk, i, d, q.hit_salt, sidx);
          else err |= STREAM_ERR_HITCAP;
        }
      }
    }
  }
  if (nskip) atomicAdd(q.skipped, (unsigned long long)nskip);
  if (err) atomicOr(a.err, err);
}

// stream_launch (a5x_stream.h) with the kernel's own LDS size: the grid is exactly the waves
// the device holds at once
template <int ALGO>
hipError_t hmac_launch(const A5xSaltLaunch& l, int op, u32 cus, hipStream_t st) {
  const u64 want = (a5x_stream_blocks(l.d.nbytes) + STREAM_WAVES - 1) / STREAM_WAVES;
  const size_t lds = (size_t)STREAM_WAVES * HM_WAVE_BYTES;
  static int per_cu = 0;  // workgroups of the kernel one CU holds at once (LDS or registers, whichever is fewer)
  if (!per_cu) {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_hmac_stream<ALGO>, 64 * STREAM_WAVES, lds) != hipSuccess || v < 1)
      v = 2;  // (2 waves per SIMD)
    per_cu = v;
  }
  const u64 grid = (u64)(cus ? cus : 1u) * (u32)per_cu;
  const u32 g = (u32)(want < grid ? want : grid);
  hipLaunchKernelGGL(k_hmac_stream<ALGO>, dim3(g), dim3(64 * STREAM_WAVES), lds, st, l, op);
  return hipGetLastError();
}

}  // namespace

hipError_t a5x_launch_hmac_stream(const A5xSaltLaunch& L, int op, uint32_t cus, hipStream_t st) {
  if (L.d.nbytes == 0) return hipSuccess;
  if (((uintptr_t)L.d.out & 15u) != 0) return hipErrorInvalidValue;
  if (L.order != hmac_order(L.d.algo)) return hipErrorInvalidValue;  // (also: not one of these algorithms)
  if (op != 1 && (!L.salts || !L.nsalts || !L.skipped)) return hipErrorInvalidValue;
  if (op == 0 && (!L.hit_salt || (a5x_algo_wide(L.d.algo) && (!L.d.hit_tail || !L.d.tails)))) return hipErrorInvalidValue;
  switch (L.d.algo) {
#define X(A) case A: return hmac_launch<A>(L, op, cus, st);
    A5X_HMAC_EACH(X)
#undef X
    default: return hipErrorInvalidValue;  // a missing kernel is an error
  }
}
