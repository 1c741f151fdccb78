// a5x_rules.hip -- hashcat rules applied on the device in the digest + lookup stage.
//
// The reference's pipeline ends in "| hashcat -m 100 left.txt -r best66.rule" (README.MD:69,
// :163): hashcat applies every rule of the file to every candidate, then hashes.  Here
// k_rules_stream does that over the "cand\n" stream the expansion kernels leave in HBM: one
// wave stages a 4 KiB stream block (+256 B of the next) in LDS once, and for each round of
// 64 candidates (lane = candidate) runs every rule: copy the candidate into the lane's
// working buffer, interpret the rule's functions (a5x_rules.h; the function is the same for
// all 64 lanes, so the interpreter's switch is a scalar branch), hash the ruled bytes, probe
// the target set.  The block's HBM read is spread over R hashes.  The geometry, the LDS
// layout, the lane buffer, the hit record and the launch are a5x_stream.h's.
#include "a5x_stream.h"

#include "a5x_sha.h"
#ifdef A5X_RULES_NEST
#include "a5x_nest.h"
#endif

namespace {

// op 0: every (candidate, rule) hashed and probed, hits recorded with their rule; op 1:
// count line starts per block; op 2: every digest written at
// dig_out[4 * DW * ((blk_pre[blk] + i) * R + r)], zeros for a rejected line
template <int ALGO>
__global__ void __launch_bounds__(64 * STREAM_WAVES) k_rules_stream(A5xRuleLaunch q, int op) {
  extern __shared__ __attribute__((aligned(16))) uint8_t r_dyn[];
  const A5xDigLaunch& a = q.d;
  const u32 wv = threadIdx.x / 64, lane = __lane_id();
  const u32 nwv = blockDim.x / 64;
  constexpr u32 DW = StreamCfg<ALGO>::DW;
  constexpr u32 HT = StreamCfg<ALGO>::HT;
  constexpr u32 NM = STREAM_BLK / 2048u;  // 32-bit newline masks per lane (32 B each)
  static_assert(NM == 2, "a lane's starts are kept in one 64-bit mask");
  StreamWave& W = *(StreamWave*)(r_dyn + wv * ((sizeof(StreamWave) + 15u) & ~15u));
  StreamLane buf;
  buf.p = W.lanes + lane;
  for (u32 k = 0; k < A5X_RULE_NDW; k++) buf.wr(k, 0u);
  u32 dirty = 0;  // dwords of the lane buffer that may be non-zero
  const u64 nblk = (a.nbytes + STREAM_BLK - 1) / STREAM_BLK;
  const u32 R = q.nrules;
  u32 err = 0, nrej = 0;
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
        if constexpr (ALGO == A5X_ALGO_MD5) md_src<true>(buf, L, d);
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
          if (h < a.hit_cap) stream_write_hit<DW, HT, true>(a.hits, a.hit_tail, h, blk, i, d, q.hit_rule, r);
          else err |= STREAM_ERR_HITCAP;
        }
      }
    }
  }
  if (nrej) atomicAdd(q.rejected, (unsigned long long)nrej);
  if (err) atomicOr(a.err, err);
}

template <int ALGO>
hipError_t rules_launch(const A5xRuleLaunch& L, int op, uint32_t cus, hipStream_t st) {
  return stream_launch<k_rules_stream<ALGO>>(L, op, cus, st);
}

}  // namespace

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
size_t a5x_stream_lds() { return STREAM_WAVES * ((sizeof(StreamWave) + 15u) & ~15u); }

uint64_t a5x_stream_blocks(uint64_t nbytes) { return (nbytes + STREAM_BLK - 1) / STREAM_BLK; }

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
