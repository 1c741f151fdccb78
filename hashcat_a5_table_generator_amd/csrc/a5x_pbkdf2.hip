// a5x_pbkdf2.hip -- iterated target lists in the digest + lookup stage: PBKDF2-HMAC-MD5 / -SHA1 /
// -SHA256 / -SHA512 (hashcat -m 11900 / 12000 / 10900 / 12100); a5x_pbkdf2.h has the core.
//
// A (candidate, salt) pair costs 2 * c compressions, c in the thousands, so the stream kernels'
// shape -- lane = candidate, every salt inside one launch over a range of up to 2 GiB -- would run
// for minutes in one launch.  The pair's state lives in HBM instead and three kernels work on a
// pass of at most P pair slots (A5xPbkdf2Launch, a5x_launch.h):
//   k_pbkdf2_init     the line-stream shape (k_hmac_stream's front half, its LDS layout: nothing
//                     here is placed at a runtime byte offset, so there is no lane buffer) over the
//                     pass's blocks: per candidate the two key states once, per salt record of the
//                     pass U1; ist, ost, u, t[0..16 B) and the pair's name (block, ordinal in
//                     block) go to the state buffer, word-major, pairs salt-major.
//   k_pbkdf2_loop     flat, one lane per pair slot, no LDS: iterations [k0, k1) clipped to the
//                     pair's own count, u and t stored back.  The host bounds pairs x (k1 - k0),
//                     and with it the time of one launch.
//   k_pbkdf2_compare  flat: the salt's mask over t, md_probe, the hit through stream_write_hit as
//                     (block, ordinal, salt index) for k_hits_resolve; op 2 writes the 16 bytes.
// The front half (staging, SWAR newline scan, per-round start lists) is k_salt_stream's text, for
// the reason a5x_stream.h gives.
#include "a5x_stream.h"

#include "a5x_pbkdf2.h"

namespace {

constexpr u32 PB_DEAD = 0xffffffffu;  // state word 1 of a slot that holds no pair
constexpr u32 PB_ERR_SLOT = 1u << 11;  // a line of the pass beyond its np slots (the host's plan is wrong)
constexpr u32 PB_FLAT = 256;           // lanes of a workgroup of the flat kernels

struct PbCand {
  const uint8_t* base;
  u32 s;
  __device__ __forceinline__ u32 at4(u32 i) const { return lds4(base, s + i); }
};

struct PbWave {
  uint8_t data[STREAM_BUF<STREAM_BLK>];
  uint16_t starts[72];  // the round's 64 line starts + the next one
};
static_assert(sizeof(PbWave) == 4576, "eight workgroups of STREAM_WAVES waves fit a CU's LDS");
constexpr u32 PB_WAVE_BYTES = ((u32)sizeof(PbWave) + 15u) & ~15u;

// a state of NS words of W to / from the word-major buffer at u32 word k0 of slot p
template <int ALGO>
__device__ __forceinline__ void pb_store(u32* state, u64 pairs, u64 p, u32 k0, const typename Pbkdf2Cfg<ALGO>::W* st, int n) {
  typedef typename Pbkdf2Cfg<ALGO>::C C;
#pragma unroll
  for (int i = 0; i < Pbkdf2Cfg<ALGO>::NS; i++) {
    if (i >= n) break;
    if constexpr (C::B64) {
      state[(u64)(k0 + 2 * i) * pairs + p] = (u32)st[i];
      state[(u64)(k0 + 2 * i + 1) * pairs + p] = (u32)(st[i] >> 32);
    } else {
      state[(u64)(k0 + i) * pairs + p] = st[i];
    }
  }
}
template <int ALGO>
__device__ __forceinline__ void pb_load(const u32* state, u64 pairs, u64 p, u32 k0, typename Pbkdf2Cfg<ALGO>::W* st, int n) {
  typedef typename Pbkdf2Cfg<ALGO>::C C;
#pragma unroll
  for (int i = 0; i < Pbkdf2Cfg<ALGO>::NS; i++) {
    if (i >= n) break;
    if constexpr (C::B64) {
      st[i] = sha_pack64(state[(u64)(k0 + 2 * i) * pairs + p], state[(u64)(k0 + 2 * i + 1) * pairs + p]);  // (low, high)
    } else {
      st[i] = state[(u64)(k0 + i) * pairs + p];
    }
  }
}
// the u32 word of a slot where each part of the state begins
template <int ALGO> struct PbAt {
  static constexpr u32 NSW = Pbkdf2Cfg<ALGO>::NSW;
  static constexpr u32 BLK = 0, ORD = 1, IST = 2, OST = 2 + NSW, U = 2 + 2 * NSW, T = 2 + 3 * NSW;
  static_assert(T + 4 == Pbkdf2Cfg<ALGO>::STATE_WORDS, "the state's words");
};

// op 0: the pass's pairs initialised; op 1: line starts per block
template <int ALGO>
__global__ void __launch_bounds__(64 * STREAM_WAVES) k_pbkdf2_init(A5xPbkdf2Launch q, int op) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  typedef Pbkdf2Cfg<ALGO> P;
  typedef typename P::W HW;
  typedef PbAt<ALGO> At;
  const A5xDigLaunch& a = q.s.d;
  const u32 wv = threadIdx.x / 64, lane = __lane_id();
  const u32 nwv = blockDim.x / 64;
  constexpr u32 NM = STREAM_BLK / 2048u;  // 32-bit newline masks per lane (32 B each)
  static_assert(NM == 2, "a lane's starts are kept in one 64-bit mask");
  PbWave& W = *(PbWave*)(s_dyn + wv * PB_WAVE_BYTES);
  const u32 S = q.s1 - q.s0;
  u32 err = 0, nskip = 0;
  const u64 ord0 = op == 1 ? 0 : a.blk_pre[q.b0];
  for (u64 blk = q.b0 + (u64)blockIdx.x * nwv + wv; blk < q.b1; blk += (u64)gridDim.x * nwv) {
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
    if (op == 1) {
      if (lane == 0) a.blk_cnt[blk] = nst;  // ordinals of hits (k_hits_resolve)
      continue;
    }
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
    const u64 blk_ord = a.blk_pre[blk] - ord0;  // the block's first line in the pass
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
      // a line over A5X_RULE_LMAX may end past the staged bytes: no pair under any salt, S skipped pairs
      bool act = valid && len <= A5X_RULE_LMAX;
      nskip += (valid && !act) ? S : 0u;
      const u64 po = blk_ord + i;  // the line's ordinal in the pass: its slot in every salt's row
      if (act && po >= q.np) {
        err |= PB_ERR_SLOT;
        act = false;
      }
      PbCand cand;
      cand.base = W.data;
      cand.s = act ? s : 0u;
      const u32 clen = act ? len : 0u;
      HW kist[P::NS], kost[P::NS];
      hmac_key_states<P::HM>(cand, clen, kist, kost);
      for (u32 si = 0; si < S; si++) {
        const u32* rec = q.s.salts + (u64)(q.s0 + si) * A5X_PBKDF2_STRIDE;  // wave-uniform: scalar loads
        const u32 nb = (u32)__builtin_amdgcn_readfirstlane((int)rec[A5X_HMAC_R_NB]);
        HW u[P::NS], t[P::KEEP];
        pbkdf2_first<ALGO, P::KEEP>(kist, kost, rec, nb, u, t);
        if (act) {
          const u64 p = (u64)si * q.np + po;
          q.state[(u64)At::BLK * q.pairs + p] = (u32)blk;
          q.state[(u64)At::ORD * q.pairs + p] = i;
          pb_store<ALGO>(q.state, q.pairs, p, At::IST, kist, P::NS);
          pb_store<ALGO>(q.state, q.pairs, p, At::OST, kost, P::NS);
          pb_store<ALGO>(q.state, q.pairs, p, At::U, u, P::NS);
          pb_store<ALGO>(q.state, q.pairs, p, At::T, t, P::KEEP);
        }
      }
    }
  }
  if (nskip) atomicAdd(q.s.skipped, (unsigned long long)nskip);
  if (err) atomicOr(a.err, err);
}

// iterations [k0, k1) of every pair of the pass whose count reaches k0
template <int ALGO>
__global__ void __launch_bounds__(PB_FLAT) k_pbkdf2_loop(A5xPbkdf2Launch q) {
  typedef Pbkdf2Cfg<ALGO> P;
  typedef typename P::W HW;
  typedef PbAt<ALGO> At;
  const u64 p = (u64)blockIdx.x * PB_FLAT + threadIdx.x;
  if (p >= q.pairs) return;
  // (the row's record: one for the whole wave, np is a multiple of 64)
  const u32 row = (u32)__builtin_amdgcn_readfirstlane((int)(p / q.np));
  const u32 c = q.s.salts[(u64)(q.s0 + row) * A5X_PBKDF2_STRIDE + A5X_PBKDF2_R_ITERS];
  const u32 k1 = q.k1 < c ? q.k1 : c;
  if (q.k0 >= k1) return;
  if (q.state[(u64)At::ORD * q.pairs + p] == PB_DEAD) return;
  HW ist[P::NS], ost[P::NS], u[P::NS], t[P::KEEP];
  pb_load<ALGO>(q.state, q.pairs, p, At::IST, ist, P::NS);
  pb_load<ALGO>(q.state, q.pairs, p, At::OST, ost, P::NS);
  pb_load<ALGO>(q.state, q.pairs, p, At::U, u, P::NS);
  pb_load<ALGO>(q.state, q.pairs, p, At::T, t, P::KEEP);
#pragma unroll 1
  for (u32 k = q.k0; k < k1; k++) pbkdf2_iter<ALGO, P::KEEP>(ist, ost, u, t);
  pb_store<ALGO>(q.state, q.pairs, p, At::U, u, P::NS);
  pb_store<ALGO>(q.state, q.pairs, p, At::T, t, P::KEEP);
}

// op 0: probe and record; op 2: the 16 bytes to dig_out
template <int ALGO>
__global__ void __launch_bounds__(PB_FLAT) k_pbkdf2_compare(A5xPbkdf2Launch q, int op) {
  typedef Pbkdf2Cfg<ALGO> P;
  typedef typename P::W HW;
  typedef PbAt<ALGO> At;
  const A5xDigLaunch& a = q.s.d;
  const u64 p = (u64)blockIdx.x * PB_FLAT + threadIdx.x;
  if (p >= q.pairs) return;
  const u32 i = q.state[(u64)At::ORD * q.pairs + p];
  if (i == PB_DEAD) return;
  const u64 blk = q.state[(u64)At::BLK * q.pairs + p];
  const u32 row = (u32)__builtin_amdgcn_readfirstlane((int)(p / q.np));
  const u32* rec = q.s.salts + (u64)(q.s0 + row) * A5X_PBKDF2_STRIDE;
  const u32 sidx = rec[A5X_HMAC_R_INDEX];
  HW t[P::KEEP];
  u32 d[4];
  pb_load<ALGO>(q.state, q.pairs, p, At::T, t, P::KEEP);
  pbkdf2_t_words<ALGO>(t, d);
  if (op == 2) {
    u32* o1 = (u32*)(a.dig_out + 16ull * ((a.blk_pre[blk] + i) * q.s.nsalts + sidx));
#pragma unroll
    for (u32 k = 0; k < 4; k++) o1[k] = d[k];
    return;
  }
  u32 key[4];
#pragma unroll
  for (u32 k = 0; k < 4; k++) key[k] = d[k] ^ rec[A5X_HMAC_R_MASK + k];
  if (md_probe(a.bitmap, a.bm_mask, a.table, a.tmask, a.has_zero_target != 0, key)) {
    const u32 h = atomicAdd(a.nhits, 1u);
    if (h < a.hit_cap) stream_write_hit<4, 4, true>(a.hits, a.hit_tail, h, blk, i, d, q.s.hit_salt, sidx);
    else atomicOr(a.err, STREAM_ERR_HITCAP);
  }
}

template <int ALGO>
hipError_t pb_init_launch(const A5xPbkdf2Launch& l, int op, u32 cus, hipStream_t st) {
  const u64 want = (l.b1 - l.b0 + STREAM_WAVES - 1) / STREAM_WAVES;
  const size_t lds = (size_t)STREAM_WAVES * PB_WAVE_BYTES;
  static int per_cu = 0;  // workgroups of the kernel one CU holds at once (LDS or registers, whichever is fewer)
  if (!per_cu) {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_pbkdf2_init<ALGO>, 64 * STREAM_WAVES, lds) != hipSuccess || v < 1)
      v = 2;  // (2 waves per SIMD)
    per_cu = v;
  }
  const u64 grid = (u64)(cus ? cus : 1u) * (u32)per_cu;
  const u32 g = (u32)(want < grid ? want : grid);
  hipLaunchKernelGGL(k_pbkdf2_init<ALGO>, dim3(g), dim3(64 * STREAM_WAVES), lds, st, l, op);
  return hipGetLastError();
}

// what every launch of a pass needs to be in bounds
bool pb_pass_ok(const A5xPbkdf2Launch& L) {
  const uint64_t nblk = a5x_stream_blocks(L.s.d.nbytes);
  return a5x_algo_pbkdf2(L.s.d.algo) && L.state && L.s.salts && L.s0 < L.s1 && L.s1 <= L.s.nsalts && L.b0 < L.b1 &&
         L.b1 <= nblk && nblk <= 0xffffffffull && L.np && (L.np & 63u) == 0 &&
         L.pairs == (uint64_t)(L.s1 - L.s0) * L.np && (L.pairs + PB_FLAT - 1) / PB_FLAT <= 0x7fffffffull;
}

}  // namespace

hipError_t a5x_launch_pbkdf2_init(const A5xPbkdf2Launch& L, int op, uint32_t cus, hipStream_t st) {
  if (L.s.d.nbytes == 0) return hipSuccess;
  if (((uintptr_t)L.s.d.out & 15u) != 0 || (op != 0 && op != 1)) return hipErrorInvalidValue;
  if (op == 1) {
    if (!L.s.d.blk_cnt || L.b0 != 0 || L.b1 != a5x_stream_blocks(L.s.d.nbytes)) return hipErrorInvalidValue;
  } else if (!pb_pass_ok(L) || !L.s.d.blk_pre || !L.s.skipped) {
    return hipErrorInvalidValue;
  }
  switch (L.s.d.algo) {
#define X(A) case A: return pb_init_launch<A>(L, op, cus, st);
    A5X_PBKDF2_EACH(X)
#undef X
    default: return hipErrorInvalidValue;  // a missing kernel is an error
  }
}

hipError_t a5x_launch_pbkdf2_loop(const A5xPbkdf2Launch& L, hipStream_t st) {
  if (!pb_pass_ok(L) || L.k0 < 1 || L.k1 <= L.k0) return hipErrorInvalidValue;
  const uint32_t g = (uint32_t)((L.pairs + PB_FLAT - 1) / PB_FLAT);
  switch (L.s.d.algo) {
#define X(A) case A: hipLaunchKernelGGL(k_pbkdf2_loop<A>, dim3(g), dim3(PB_FLAT), 0, st, L); break;
    A5X_PBKDF2_EACH(X)
#undef X
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t a5x_launch_pbkdf2_compare(const A5xPbkdf2Launch& L, int op, hipStream_t st) {
  if (!pb_pass_ok(L) || (op != 0 && op != 2)) return hipErrorInvalidValue;
  if (op == 0 && (!L.s.hit_salt || !L.s.d.hits || !L.s.d.nhits)) return hipErrorInvalidValue;
  if (op == 2 && (!L.s.d.dig_out || !L.s.d.blk_pre)) return hipErrorInvalidValue;
  const uint32_t g = (uint32_t)((L.pairs + PB_FLAT - 1) / PB_FLAT);
  switch (L.s.d.algo) {
#define X(A) case A: hipLaunchKernelGGL(k_pbkdf2_compare<A>, dim3(g), dim3(PB_FLAT), 0, st, L, op); break;
    A5X_PBKDF2_EACH(X)
#undef X
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
