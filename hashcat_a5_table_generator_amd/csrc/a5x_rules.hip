// a5x_rules.hip -- hashcat rules applied on the device in the digest + lookup stage.
//
// The reference's pipeline ends in "| hashcat -m 100 left.txt -r best66.rule" (README.MD:69,
// :163): hashcat applies every rule of the file to every candidate, then hashes.  Here
// k_rules_stream does that over the "cand\n" stream the expansion kernels leave in HBM: one
// wave stages a 4 KiB stream block (+256 B of the next) in LDS once, and for each round of
// 64 candidates (lane = candidate) runs every rule: copy the candidate into the lane's
// working buffer, interpret the rule's functions (a5x_rules.h; the function is the same for
// all 64 lanes, so the interpreter's switch is a scalar branch), hash the ruled bytes, probe
// the target set.  The block's HBM read is spread over R hashes.
//
// LDS per wave (RWave): 4432 B staged stream, 144 B round start list, 8704 B lane buffers
// (34 dwords x 64 lanes, dword k of lane l at (k * 64 + l) * 4: a wave's access to dword k
// touches 64 consecutive banks) = 13280 B; a 256-thread workgroup takes 53120 B, so three fit
// the CU's 160 KiB: 12 waves, 3 on every SIMD (DESIGN "Rules").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "a5x.h"
#include "a5x_launch.h"
#include "a5x_md.h"
#include "a5x_rules.h"
#include "a5x_sha.h"
#ifdef A5X_RULES_NEST
#include "a5x_nest.h"
#endif

namespace {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr u32 RBLK = 4096;     // stream bytes per wave: C5's ~23-byte lines fill 3 rounds of 64 lanes to 93 %
constexpr u32 RMARGIN = 256;   // next-block bytes staged for straddling lines
constexpr u32 RWAVES = 4;      // waves per workgroup: one per SIMD, so a CU's resident workgroups load its SIMDs alike
constexpr u32 R_ERR_HITCAP = 1u << 10;
// a line that starts in the block and is at most A5X_RULE_LMAX bytes has its '\n' staged:
// longer lines are rejected, so no line is ever read from HBM
static_assert(RMARGIN >= A5X_RULE_LMAX + 1u, "a rule-sized line that starts in a block must end in the staged margin");
static_assert(A5X_RULE_NDW * 4u >= A5X_RULE_LMAX + 8u, "the hash sources read up to 8 bytes past the message");

template <int ALGO> struct RCfg {
  static constexpr u32 DW = a5x_algo_words(ALGO);
  static constexpr u32 HT = a5x_hit_tail_stride(ALGO);  // words of a hit's tail record
  static_assert(DW <= 4u || DW - 4u <= HT, "the hit's tail record holds the whole tail");
};

struct RWave {
  static constexpr u32 BUF = RBLK + RMARGIN + 80;  // + slack for the over-reads of the copy
  uint8_t data[BUF];
  uint16_t starts[72];              // the round's 64 line starts + the next one
  u32 lanes[A5X_RULE_NDW * 64];     // working buffers, dword-interleaved
};

__device__ __forceinline__ u32 r_incl_scan(u32 x) {
  const u32 lane = __lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u32 y = (u32)__shfl_up((int)x, d, 64);
    if ((int)lane >= d) x += y;
  }
  return x;
}

// the lane's working buffer: dword k at lanes[k * 64 + lane]
struct RLane {
  u32* p;  // &lanes[lane]
  __device__ __forceinline__ u32 rd(u32 k) const { return p[k * 64u]; }
  __device__ __forceinline__ void wr(u32 k, u32 v) { p[k * 64u] = v; }
  // message source of the digests: 4 bytes at message offset i (zero past the word)
  __device__ __forceinline__ u32 at4(u32 i) const {
    const u32 lo = p[(i >> 2) * 64u];
    return (i & 3u) ? __builtin_amdgcn_alignbyte(p[((i >> 2) + 1u) * 64u], lo, i & 3u) : lo;
  }
};

// MD5 over message bytes [0, len) of src (md_lds of a5x_md.h with a message source)
template <class S>
__device__ __forceinline__ void md5_src(const S& src, u32 len, u32* d) {
  d[0] = 0x67452301u; d[1] = 0xefcdab89u; d[2] = 0x98badcfeu; d[3] = 0x10325476u;
  const u32 nb = (len + 8u) / 64u + 1u;
  for (u32 blk = 0; blk < nb; blk++) {
    u32 M[16];
#pragma unroll
    for (u32 j = 0; j < 16; j++) {
      const u32 b = blk * 64u + 4u * j;
      const int k = (int)len - (int)b;
      const u32 raw = k > 0 ? src.at4(b) : 0u;
      const u32 keep = k >= 4 ? 0xffffffffu : (k <= 0 ? 0u : ((1u << (8 * k)) - 1u));
      const u32 pad = (k >= 0 && k < 4) ? (0x80u << (8 * k)) : 0u;
      M[j] = (raw & keep) | pad;
    }
    if (blk == nb - 1) {
      M[14] = len << 3;
      M[15] = len >> 29;
    }
    md5_block(d, M);
  }
}

// op 0: every (candidate, rule) hashed and probed, hits recorded with their rule; op 1:
// count line starts per block; op 2: every digest written at
// dig_out[4 * DW * ((blk_pre[blk] + i) * R + r)], zeros for a rejected line
template <int ALGO>
__global__ void __launch_bounds__(64 * RWAVES) k_rules_stream(A5xRuleLaunch q, int op) {
  extern __shared__ __attribute__((aligned(16))) uint8_t r_dyn[];
  const A5xDigLaunch& a = q.d;
  const u32 wv = threadIdx.x / 64, lane = __lane_id();
  const u32 nwv = blockDim.x / 64;
  constexpr u32 DW = RCfg<ALGO>::DW;
  constexpr u32 HT = RCfg<ALGO>::HT;
  constexpr u32 DBUF = RWave::BUF;
  constexpr u32 NM = RBLK / 2048u;  // 32-bit newline masks per lane (32 B each)
  static_assert(NM == 2, "a lane's starts are kept in one 64-bit mask");
  RWave& W = *(RWave*)(r_dyn + wv * ((sizeof(RWave) + 15u) & ~15u));
  RLane buf;
  buf.p = W.lanes + lane;
  for (u32 k = 0; k < A5X_RULE_NDW; k++) buf.wr(k, 0u);
  u32 dirty = 0;  // dwords of the lane buffer that may be non-zero
  const u64 nblk = (a.nbytes + RBLK - 1) / RBLK;
  const u32 R = q.nrules;
  u32 err = 0, nrej = 0;
  for (u64 blk = (u64)blockIdx.x * nwv + wv; blk < nblk; blk += (u64)gridDim.x * nwv) {
    const u64 bs = blk * RBLK;
    const u32 bl = (u32)min<u64>(RBLK, a.nbytes - bs);             // block bytes
    const u32 sl = (u32)min<u64>(RBLK + RMARGIN, a.nbytes - bs);   // staged bytes
    __builtin_amdgcn_wave_barrier();
    const uint4* g16 = (const uint4*)(a.out + bs);
    uint4* l16 = (uint4*)W.data;
    for (u32 i = lane; i < sl / 16; i += 64) l16[i] = g16[i];
    for (u32 i = (sl & ~15u) + lane; i < sl; i += 64) W.data[i] = a.out[bs + i];
    for (u32 i = sl + lane; i < DBUF; i += 64) W.data[i] = 0;
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
    const u32 incl = r_incl_scan(m);
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
      if (tail_end == 0xffffffffu && sl < RBLK + RMARGIN) tail_end = sl;
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
      const bool rej = valid && len > A5X_RULE_LMAX;
      nrej += rej ? 1u : 0u;
      const bool act = valid && !rej;
      const u32 nd0 = act ? rule_ndw(len) : 0u;
      u64 row = 0;
      if (op == 2 && valid) row = (a.blk_pre[blk] + i) * R;
      for (u32 r = 0; r < R; r++) {
        const u32* ops = q.rules + (u64)r * A5X_RULE_STRIDE;
        const u32 nops = min(ops[0], A5X_RULE_OPS_MAX);
        u32 L = 0;
        if (act) {
          // the candidate into the lane buffer (line starts are byte aligned: funnel reads),
          // zeros over whatever the previous rule left past it
          const u32 lim = nd0 > dirty ? nd0 : dirty;
          for (u32 k = 0; k < lim; k++)
            buf.wr(k, k < nd0 ? (lds4(W.data, s + 4u * k) & rule_keep((int)len - (int)(4u * k))) : 0u);
          L = len;
        }
        for (u32 j = 0; j < nops; j++) {
          const u32 f = ops[1 + j];
          if (act) L = rule_apply_op(buf, L, f);
        }
        dirty = act ? rule_ndw(L) : dirty;
        u32 d[DW];
        if constexpr (ALGO == A5X_ALGO_MD5) md5_src(buf, L, d);
        else if constexpr (ALGO == A5X_ALGO_NTLM) ntlm_stream(buf, L, d);
#ifdef A5X_RULES_NEST
        else if constexpr (a5x_algo_nested(ALGO)) nest_digest<ALGO>(buf, L, d);
#endif
        else sha_digest<ALGO>(buf, L, d);
        if (op == 2) {
          if (valid) {
            u32* o1 = (u32*)(a.dig_out + 4ull * DW * (row + r));
#pragma unroll
            for (u32 k = 0; k < DW; k++) o1[k] = act ? d[k] : 0u;
          }
          continue;
        }
        bool hit = false;
        if (act) {
          if constexpr (DW == 4)
            hit = md_probe(a.bitmap, a.bm_mask, a.table, a.tmask, a.has_zero_target != 0, d);
          else
            hit = md_probe_wide<(int)DW - 4>(a.bitmap, a.bm_mask, a.table, a.tails, a.tmask, a.has_zero_target != 0,
                                             a.ztails, a.nztails, d);
        }
        if (hit) {
          const u32 h = atomicAdd(a.nhits, 1u);
          if (h < a.hit_cap) {
            A5xHitRaw hr;
            hr.blk = blk; hr.idx = i; hr.d[0] = d[0]; hr.d[1] = d[1]; hr.d[2] = d[2]; hr.d[3] = d[3];
            a.hits[h] = hr;
            q.hit_rule[h] = r;
            if constexpr (DW > 4) {
#pragma unroll
              for (u32 k = 0; k < HT; k++) a.hit_tail[(u64)HT * h + k] = k < DW - 4 ? d[4 + k] : 0u;
            }
          } else {
            err |= R_ERR_HITCAP;
          }
        }
      }
    }
  }
  if (nrej) atomicAdd(q.rejected, (unsigned long long)nrej);
  if (err) atomicOr(a.err, err);
}

}  // namespace

// grid and launch of one instantiation.  The grid is exactly the waves the device holds at
// once (cus x resident workgroups): every wave takes the same share of the blocks in its
// grid-stride loop.  A larger grid runs a second, part-empty residency round -- 16 waves per
// CU launched against 12 resident cost 0.72-0.85 of the no-rule stream's hash rate where this
// gives DESIGN "Rules"'s figures.
template <int ALGO>
static hipError_t rules_launch(const A5xRuleLaunch& L, int op, uint32_t cus, hipStream_t st) {
  const u64 want = (a5x_rules_blocks(L.d.nbytes) + RWAVES - 1) / RWAVES;
  const size_t lds = a5x_rules_lds();
  // workgroups of k_rules_stream<ALGO> one CU holds at once (LDS: 3; fewer if the registers say so)
  static int per_cu = 0;
  if (!per_cu) {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k_rules_stream<ALGO>, 64 * RWAVES, lds) != hipSuccess || v < 1)
      v = 2;  // (2 waves per SIMD)
    per_cu = v;
  }
  const u64 grid = (u64)(cus ? cus : 1u) * (u32)per_cu;
  const u32 g = (u32)(want < grid ? want : grid);
  hipLaunchKernelGGL(k_rules_stream<ALGO>, dim3(g), dim3(64 * RWAVES), lds, st, L, op);
  return hipGetLastError();
}

// The instantiations live in two translation units: MD5 / NTLM / SHA-1 / SHA-256 here, SHA-224
// / SHA-384 / SHA-512 in a5x_rules_wide.hip, which includes this file with A5X_RULES_WIDE
// defined.  The compiler's inlining of the rule interpreter depends on how many kernels of a
// module call it: with seven in one module the first four's code changed, in a module of their
// own it is instruction-identical to what it was (DESIGN "SHA-224, SHA-384 and SHA-512").
// The seven nested algorithms (a5x_nest.h) have a third, a5x_rules_nest.hip (A5X_RULES_NEST).
#if defined(A5X_RULES_NEST)
// (arguments checked by a5x_launch_rules_stream)
hipError_t a5x_launch_rules_stream_nest(const A5xRuleLaunch& L, int op, uint32_t cus, hipStream_t st) {
  switch (L.d.algo) {
    case A5X_ALGO_MD5_MD5: return rules_launch<A5X_ALGO_MD5_MD5>(L, op, cus, st);
    case A5X_ALGO_MD5_MD5_MD5: return rules_launch<A5X_ALGO_MD5_MD5_MD5>(L, op, cus, st);
    case A5X_ALGO_MD5_MD5UP: return rules_launch<A5X_ALGO_MD5_MD5UP>(L, op, cus, st);
    case A5X_ALGO_MD5_SHA1: return rules_launch<A5X_ALGO_MD5_SHA1>(L, op, cus, st);
    case A5X_ALGO_SHA1_SHA1: return rules_launch<A5X_ALGO_SHA1_SHA1>(L, op, cus, st);
    case A5X_ALGO_SHA1_MD5: return rules_launch<A5X_ALGO_SHA1_MD5>(L, op, cus, st);
    case A5X_ALGO_SHA256_MD5: return rules_launch<A5X_ALGO_SHA256_MD5>(L, op, cus, st);
    default: return hipErrorInvalidValue;
  }
}
#elif !defined(A5X_RULES_WIDE)
size_t a5x_rules_lds() { return RWAVES * ((sizeof(RWave) + 15u) & ~15u); }

uint64_t a5x_rules_blocks(uint64_t nbytes) { return (nbytes + RBLK - 1) / RBLK; }

hipError_t a5x_launch_rules_stream_wide(const A5xRuleLaunch& L, int op, uint32_t cus, hipStream_t st);
hipError_t a5x_launch_rules_stream_nest(const A5xRuleLaunch& L, int op, uint32_t cus, hipStream_t st);

hipError_t a5x_launch_rules_stream(const A5xRuleLaunch& L, int op, uint32_t cus, hipStream_t st) {
  if (L.d.nbytes == 0) return hipSuccess;
  if (((uintptr_t)L.d.out & 15u) != 0) return hipErrorInvalidValue;
  if (op != 1 && (!L.rules || !L.nrules || !L.rejected)) return hipErrorInvalidValue;
  if (op == 0 && (!L.hit_rule || (a5x_algo_wide(L.d.algo) && (!L.d.hit_tail || !L.d.tails)))) return hipErrorInvalidValue;
  switch (L.d.algo) {
    case A5X_ALGO_MD5: return rules_launch<A5X_ALGO_MD5>(L, op, cus, st);
    case A5X_ALGO_NTLM: return rules_launch<A5X_ALGO_NTLM>(L, op, cus, st);
    case A5X_ALGO_SHA1: return rules_launch<A5X_ALGO_SHA1>(L, op, cus, st);
    case A5X_ALGO_SHA256: return rules_launch<A5X_ALGO_SHA256>(L, op, cus, st);
    case A5X_ALGO_SHA224: case A5X_ALGO_SHA384: case A5X_ALGO_SHA512:
      return a5x_launch_rules_stream_wide(L, op, cus, st);
    case A5X_ALGO_MD5_MD5: case A5X_ALGO_MD5_MD5_MD5: case A5X_ALGO_MD5_MD5UP: case A5X_ALGO_MD5_SHA1:
    case A5X_ALGO_SHA1_SHA1: case A5X_ALGO_SHA1_MD5: case A5X_ALGO_SHA256_MD5:
      return a5x_launch_rules_stream_nest(L, op, cus, st);
    default: return hipErrorInvalidValue;  // a missing kernel is an error, never another algorithm's digest
  }
}
#else
// (arguments checked by a5x_launch_rules_stream)
hipError_t a5x_launch_rules_stream_wide(const A5xRuleLaunch& L, int op, uint32_t cus, hipStream_t st) {
  switch (L.d.algo) {
    case A5X_ALGO_SHA224: return rules_launch<A5X_ALGO_SHA224>(L, op, cus, st);
    case A5X_ALGO_SHA384: return rules_launch<A5X_ALGO_SHA384>(L, op, cus, st);
    case A5X_ALGO_SHA512: return rules_launch<A5X_ALGO_SHA512>(L, op, cus, st);
    default: return hipErrorInvalidValue;
  }
}
#endif
