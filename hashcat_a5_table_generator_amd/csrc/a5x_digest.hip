// a5x_digest.hip -- fused digest + lookup over an expanded candidate stream.
//
// No counterpart in the reference: main.go only prints candidates (main.go:66) and
// hashcat hashes them (README.MD:69).  Here the "cand\n" stream that the expansion
// kernels leave in HBM is hashed on the device, so candidates never round-trip to the
// host:
//   MD5   RFC 1321 over the candidate bytes (== Go crypto/md5);
//   NTLM  MD4 (RFC 1320) over UTF-16LE of the candidate decoded as Go does for
//         []rune(string): invalid UTF-8 byte -> U+FFFD, runes > U+FFFF -> surrogate
//         pairs (unicode/utf16.Encode);
//   SHA-1 / SHA-224 / SHA-256 / SHA-384 / SHA-512  FIPS 180-4 over the candidate bytes
//         (a5x_sha.h).
// Each digest is probed against a device-resident target set: a 2^k-bit prefilter
// indexed by digest word 0, then an open-addressing table of the first 16 digest bytes
// (wide digests: the remaining words in a parallel array, compared too).
//
// Work unit: one wave per 2 or 4 KiB block of the stream (DCfg).  The wave stages the block (+256 B
// of the next one) in LDS, finds line starts with a SWAR newline test (exact per byte),
// compacts them into an ordered start list, and every lane hashes one candidate at a
// time; the candidate owned by a block is the one STARTING in it.  A hit records
// (block, ordinal in block, digest); a per-block start count + scan turns that into
// the global candidate index afterwards (hits are rare).  The geometry, the wave
// scan and the hit record are a5x_stream.h's, shared with the rules and salt kernels.
#include "a5x_stream.h"

#include "a5x_format.h"
#include "a5x_sha.h"
#ifdef A5X_DIGEST_NEST
#include "a5x_nest.h"
#endif

namespace {

// stream bytes per wave: 4 KiB for MD5 (lanes stay busy over ~3 rounds of candidates),
// 2 KiB for NTLM (the MD4 of UTF-16LE costs about twice per candidate byte), 4 KiB for
// the SHA algorithms: their time is the hash rounds, and a block's last round of 64 lanes is
// only part full -- C5's ~23-byte lines give 2 rounds per 2 KiB block, the second 40 %
// full, against 3 rounds (the third 80 % full) per 4 KiB block; measured on C5 the digest
// pass takes 83.4 vs 97.3 ms (SHA-1) and 132.4 vs 161.7 ms (SHA-256) at 4 vs 2 KiB
// (profiles/r07_ab_sha_stream_block.json)
#ifndef A5X_SHA_DBLK
#define A5X_SHA_DBLK 4096u  // (A/B knob: 2048u or 4096u)
#endif
template <int ALGO> struct DCfg {
  static constexpr u32 BLK = ALGO == A5X_ALGO_MD5 ? 4096u : (ALGO == A5X_ALGO_NTLM ? 2048u : A5X_SHA_DBLK);
};

__device__ __forceinline__ u32 glob4(const uint8_t* base, u64 off, u64 lim) {
  u32 v = 0;
  for (u32 k = 0; k < 4; k++)
    if (off + k < lim) v |= (u32)base[off + k] << (8 * k);
  return v;
}

// message bytes in HBM (lines that run past the staged bytes): 4 bytes at message
// offset i, zero past the stream end
struct MdGlob {
  const uint8_t* g;
  u64 off, lim;
  __device__ __forceinline__ u32 at4(u32 i) const { return glob4(g, off + i, lim); }
};

// message bytes of a line for md_src, sha_digest and nest_digest: the staged LDS bytes, or HBM
// for a line that runs past them
struct ShaLine {
  const uint8_t* lbase;
  u32 loff;
  const uint8_t* gbase;
  u64 goff, glim;
  bool lds;
  __device__ __forceinline__ u32 at4(u32 i) const { return lds ? lds4(lbase, loff + i) : glob4(gbase, goff + i, glim); }
};

template <u32 BLK>
struct DWave {
  uint8_t data[STREAM_BUF<BLK>];
  uint16_t starts[BLK + 2];
};

// op 0: probe targets, record hits; op 1: count line starts per block; op 2: write
// every candidate's digest at dig_out[4 * DW * (blk_pre[blk] + i)] (16 to 64 bytes)
template <int ALGO>
__global__ void __launch_bounds__(256) k_digest_stream(A5xDigLaunch a, int op) {
  static_assert(DCfg<ALGO>::BLK == 2048u || DCfg<ALGO>::BLK == 4096u, "a5x_digest_lds sizes these two");
  extern __shared__ __attribute__((aligned(16))) uint8_t d_dyn[];
  const u32 wv = threadIdx.x / 64, lane = __lane_id();
  const u32 nwv = blockDim.x / 64;
  constexpr u32 DBLK = DCfg<ALGO>::BLK;
  constexpr u32 DW = StreamCfg<ALGO>::DW;
  constexpr u32 HT = StreamCfg<ALGO>::HT;
  typedef DWave<DBLK> WT;
  constexpr u32 DBUF = STREAM_BUF<DBLK>;
  constexpr u32 NM = DBLK / 2048u;  // 32-bit newline masks per lane (32 B each)
  const u32 per = (u32)sizeof(WT);
  WT& W = *(WT*)(d_dyn + wv * ((per + 15u) & ~15u));
  const u64 nblk = (a.nbytes + DBLK - 1) / DBLK;
  u32 err = 0;
  for (u64 blk = (u64)blockIdx.x * nwv + wv; blk < nblk; blk += (u64)gridDim.x * nwv) {
    const u64 bs = blk * DBLK;
    const u32 bl = (u32)min<u64>(DBLK, a.nbytes - bs);                  // block bytes
    const u32 sl = (u32)min<u64>(DBLK + STREAM_MARGIN, a.nbytes - bs);        // staged bytes
    __builtin_amdgcn_wave_barrier();
    // stage [bs, bs + sl) (16-B loads; the stream base is 16-B aligned, see the launcher)
    const uint4* g16 = (const uint4*)(a.out + bs);
    uint4* l16 = (uint4*)W.data;
    for (u32 i = lane; i < sl / 16; i += 64) l16[i] = g16[i];
    for (u32 i = (sl & ~15u) + lane; i < sl; i += 64) W.data[i] = a.out[bs + i];
    for (u32 i = sl + lane; i < DBUF; i += 64) W.data[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // newline bits of this lane's slice (NM x 32 bytes)
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
    u32 o = incl - m;
#pragma unroll
    for (u32 h = 0; h < NM; h++)
      for (u32 x = sm[h]; x; x &= x - 1) W.starts[o++] = (uint16_t)(q0 + 32u * h + (u32)__builtin_ctz(x));
    if (lane == 0 && a.blk_cnt) a.blk_cnt[blk] = nst;  // ordinals of hits (k_hits_resolve)
    if (op == 1) continue;
    // end of the last line starting here: first '\n' at or after it
    u64 tail_end = 0;
    if (nst) {
      const u32 s_last = W.starts[nst - 1];
      const u32 lim = min(sl, DBLK + STREAM_MARGIN);
      // lanes look at 64 consecutive bytes at a time
      u64 found = ~0ull;
      for (u32 base = s_last; base < lim && found == ~0ull; base += 64) {
        const u32 q = base + lane;
        const bool hit = q < lim && W.data[q] == '\n';
        const u64 bal = __ballot(hit);
        if (bal) found = base + (u32)__builtin_ctzll(bal);
      }
      if (found == ~0ull) {  // the line runs past the staged bytes: scan HBM
        u64 g = bs + lim;
        for (;; g += 64) {
          const u64 q = g + lane;
          const bool hit = q < a.nbytes && a.out[q] == '\n';
          const u64 bal = __ballot(hit);
          if (bal) { found = g - bs + (u32)__builtin_ctzll(bal); break; }
          if (g + 64 >= a.nbytes) { found = a.nbytes - bs; break; }  // unterminated (not produced here)
        }
      }
      tail_end = found;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (u32 i = lane; i < nst; i += 64) {
      const u32 s = W.starts[i];
      const u64 e = i + 1 < nst ? (u64)W.starts[i + 1] - 1 : tail_end;  // '\n' position
      const u32 len = (u32)(e - s);
      // every byte of the line staged (bytes past sl are zero-filled) and the 8-B
      // over-read of the last message word inside the buffer
      const bool in_lds = e <= sl && e + 8 <= DBUF;
      u32 d[DW];
      if constexpr (ALGO != A5X_ALGO_NTLM) {
        ShaLine src;
        src.lbase = W.data; src.loff = s;
        src.gbase = a.out; src.goff = bs + s; src.glim = a.nbytes;
        src.lds = in_lds;
        if constexpr (ALGO == A5X_ALGO_MD5) md_src<true>(src, len, d);
#ifdef A5X_DIGEST_NEST
        else if constexpr (a5x_algo_nested(ALGO)) nest_digest<ALGO>(src, len, d);
#endif
        else sha_digest<ALGO>(src, len, d);
      } else if (in_lds) {  // any length: the UTF-16LE units are made as MD4 blocks fill
        MdLds src;
        src.base = W.data;
        src.off = s;
        ntlm_stream(src, len, d);
      } else {
        MdGlob src;
        src.g = a.out;
        src.off = bs + s;
        src.lim = a.nbytes;
        ntlm_stream(src, len, d);
      }
      bool hit = false;
      if (op == 2) {
        if constexpr (DW == 4) {
          uint4* o4 = (uint4*)(a.dig_out + 16 * (a.blk_pre[blk] + i));
          *o4 = make_uint4(d[0], d[1], d[2], d[3]);
        } else {  // a 20-B (28-B) stride is only 4-B aligned: dword stores
          u32* o1 = (u32*)(a.dig_out + 4ull * DW * (a.blk_pre[blk] + i));
#pragma unroll
          for (u32 k = 0; k < DW; k++) o1[k] = d[k];
        }
      } else if constexpr (DW == 4) {
        hit = md_probe(a.bitmap, a.bm_mask, a.table, a.tmask, a.has_zero_target != 0, d);
      } else {
        hit = md_probe_wide<(int)DW - 4>(a.bitmap, a.bm_mask, a.table, a.tails, a.tmask, a.has_zero_target != 0, a.ztails,
                                         a.nztails, d);
      }
      if (hit) {
        const u32 h = atomicAdd(a.nhits, 1u);
        if (h < a.hit_cap) stream_write_hit<DW, HT, false>(a.hits, a.hit_tail, h, blk, i, d, nullptr, 0u);
        else err |= STREAM_ERR_HITCAP;
      }
    }
  }
  if (err) atomicOr(a.err, err);
}

#ifndef A5X_DIGEST_NEST
// hits: (block, ordinal) -> global candidate index -> (word, candidate in word)
__global__ void __launch_bounds__(64) k_hits_resolve(A5xHitRaw* hits, u32 n, const u64* blk_pre, u64 cand_base,
                                                      const u64* cand_off, u64 nw) {
  for (u32 h = blockIdx.x * 64 + threadIdx.x; h < n; h += gridDim.x * 64) {
    A5xHitRaw r = hits[h];
    const u64 g = cand_base + blk_pre[r.blk] + r.idx;
    u64 lo = 0, hi = nw;  // largest w with cand_off[w] <= g
    while (hi - lo > 1) {
      const u64 mid = (lo + hi) / 2;
      if (cand_off[mid] <= g) lo = mid; else hi = mid;
    }
    r.blk = lo;
    r.idx = g - cand_off[lo];
    hits[h] = r;
  }
}

// Hybrid fused digest: the candidate-bearing words the fused kernel leaves out (not
// FAST: slow / BIG / pass-G words) are listed, then gathered into a compact sub-batch
// that the two-pass path digests.
__global__ void __launch_bounds__(256) k_nonfast_list(const u32* flags, const u64* cand_off, u64 nw, u64 cb, u64 ce,
                                                       u32* list, u32* n) {
  // (words with candidates inside [cb, ce))
  for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < nw; w += (u64)gridDim.x * 256)
    if (cand_off[w + 1] > cand_off[w] && cand_off[w] < ce && cand_off[w + 1] > cb && !(flags[w] & A5X_WF_FAST))
      list[atomicAdd(n, 1u)] = (u32)w;
}

__global__ void __launch_bounds__(256) k_gather_lens(const u64* woff, const u32* idx, u32 m, u64* lens) {
  for (u32 k = blockIdx.x * 256 + threadIdx.x; k < m; k += gridDim.x * 256) lens[k] = woff[idx[k] + 1] - woff[idx[k]];
}

__global__ void __launch_bounds__(64) k_gather_words(const uint8_t* words, const u64* woff, const u32* idx, u32 m,
                                                      const u64* sub_off, uint8_t* out) {
  for (u32 k = blockIdx.x; k < m; k += gridDim.x) {
    const u64 s = woff[idx[k]], L = woff[idx[k] + 1] - s, d = sub_off[k];
    for (u64 i = threadIdx.x; i < L; i += 64) out[d + i] = words[s + i];
  }
}

#endif  // A5X_DIGEST_NEST

}  // namespace

// The nested instantiations live in a translation unit of their own, a5x_digest_nest.hip,
// which includes this file with A5X_DIGEST_NEST defined, for the reason recorded above
// a5x_launch_rules_stream (a5x_rules.hip): the kernels of this module keep their code.
#ifdef A5X_DIGEST_NEST
template <int ALGO>
static hipError_t nest_launch(const A5xDigLaunch& L, int op, uint32_t g, hipStream_t st) {
  static_assert(DCfg<ALGO>::BLK == 4096u, "the nested algorithms take the MD5 / SHA stream block and its LDS layout");
  hipLaunchKernelGGL(k_digest_stream<ALGO>, dim3(g), dim3(256), a5x_digest_lds(L.algo), st, L, op);
  return hipGetLastError();
}
// (arguments checked and the grid sized by a5x_launch_digest_stream)
hipError_t a5x_launch_digest_stream_nest(const A5xDigLaunch& L, int op, uint32_t g, hipStream_t st) {
  switch (L.algo) {
    case A5X_ALGO_MD5_MD5: return nest_launch<A5X_ALGO_MD5_MD5>(L, op, g, st);
    case A5X_ALGO_MD5_MD5_MD5: return nest_launch<A5X_ALGO_MD5_MD5_MD5>(L, op, g, st);
    case A5X_ALGO_MD5_MD5UP: return nest_launch<A5X_ALGO_MD5_MD5UP>(L, op, g, st);
    case A5X_ALGO_MD5_SHA1: return nest_launch<A5X_ALGO_MD5_SHA1>(L, op, g, st);
    case A5X_ALGO_SHA1_SHA1: return nest_launch<A5X_ALGO_SHA1_SHA1>(L, op, g, st);
    case A5X_ALGO_SHA1_MD5: return nest_launch<A5X_ALGO_SHA1_MD5>(L, op, g, st);
    case A5X_ALGO_SHA256_MD5: return nest_launch<A5X_ALGO_SHA256_MD5>(L, op, g, st);
    default: return hipErrorInvalidValue;
  }
}
#else
hipError_t a5x_launch_digest_stream_nest(const A5xDigLaunch& L, int op, uint32_t g, hipStream_t st);

hipError_t a5x_launch_nonfast_list(const uint32_t* flags, const uint64_t* cand_off, uint64_t nw, uint64_t cb,
                                   uint64_t ce, uint32_t* list, uint32_t* n, hipStream_t st) {
  if (!nw) return hipSuccess;
  const u64 b = (nw + 255) / 256;
  hipLaunchKernelGGL(k_nonfast_list, dim3((u32)(b < 16384 ? b : 16384)), dim3(256), 0, st, flags, cand_off, nw, cb, ce,
                     list, n);
  return hipGetLastError();
}

hipError_t a5x_launch_gather_words(const uint8_t* words, const uint64_t* woff, const uint32_t* idx, uint32_t m,
                                   uint64_t* lens, const uint64_t* sub_off, uint8_t* out, hipStream_t st) {
  if (!m) return hipSuccess;
  if (lens) {  // pass 1: the lengths
    hipLaunchKernelGGL(k_gather_lens, dim3((m + 255) / 256 < 4096 ? (m + 255) / 256 : 4096), dim3(256), 0, st, woff, idx,
                       m, lens);
  } else {     // pass 2: the bytes at the scanned offsets
    hipLaunchKernelGGL(k_gather_words, dim3(m < 65536 ? m : 65536), dim3(64), 0, st, words, woff, idx, m, sub_off, out);
  }
  return hipGetLastError();
}

// the algorithm's stream block (0: not an algorithm)
static u32 digest_blk(int algo) {
  return algo == A5X_ALGO_MD5 ? DCfg<A5X_ALGO_MD5>::BLK : algo == A5X_ALGO_NTLM ? DCfg<A5X_ALGO_NTLM>::BLK
       : algo == A5X_ALGO_SHA1 ? DCfg<A5X_ALGO_SHA1>::BLK : algo == A5X_ALGO_SHA256 ? DCfg<A5X_ALGO_SHA256>::BLK
       : algo == A5X_ALGO_SHA224 ? DCfg<A5X_ALGO_SHA224>::BLK : algo == A5X_ALGO_SHA384 ? DCfg<A5X_ALGO_SHA384>::BLK
       : algo == A5X_ALGO_SHA512 ? DCfg<A5X_ALGO_SHA512>::BLK
       : a5x_algo_nested(algo) ? DCfg<A5X_ALGO_MD5_MD5>::BLK : 0u;  // (one block for every nested form: nest_launch)
}
size_t a5x_digest_lds(int algo) {
  const u32 blk = digest_blk(algo);
  const u32 per = blk == 4096u ? (u32)sizeof(DWave<4096u>) : (u32)sizeof(DWave<2048u>);
  return 4u * ((per + 15u) & ~15u);
}

hipError_t a5x_launch_digest_stream(const A5xDigLaunch& L, int op, uint32_t grid, hipStream_t st) {
  if (L.nbytes == 0) return hipSuccess;
  if (((uintptr_t)L.out & 15u) != 0) return hipErrorInvalidValue;
  // op 0 of a wide digest compares the slots' tails and records each hit's tail
  if (op == 0 && a5x_algo_wide(L.algo) && (!L.hit_tail || !L.tails)) return hipErrorInvalidValue;
  const u64 nblk = a5x_digest_blocks(L.nbytes, L.algo);
  const u64 want = (nblk + 3) / 4;
  const u32 g = (u32)(want < grid ? want : grid);
  if (L.algo == A5X_ALGO_MD5)
    hipLaunchKernelGGL(k_digest_stream<A5X_ALGO_MD5>, dim3(g), dim3(256), a5x_digest_lds(L.algo), st, L, op);
  else if (L.algo == A5X_ALGO_NTLM)
    hipLaunchKernelGGL(k_digest_stream<A5X_ALGO_NTLM>, dim3(g), dim3(256), a5x_digest_lds(L.algo), st, L, op);
  else if (L.algo == A5X_ALGO_SHA1)
    hipLaunchKernelGGL(k_digest_stream<A5X_ALGO_SHA1>, dim3(g), dim3(256), a5x_digest_lds(L.algo), st, L, op);
  else if (L.algo == A5X_ALGO_SHA256)
    hipLaunchKernelGGL(k_digest_stream<A5X_ALGO_SHA256>, dim3(g), dim3(256), a5x_digest_lds(L.algo), st, L, op);
  else if (L.algo == A5X_ALGO_SHA224)
    hipLaunchKernelGGL(k_digest_stream<A5X_ALGO_SHA224>, dim3(g), dim3(256), a5x_digest_lds(L.algo), st, L, op);
  else if (L.algo == A5X_ALGO_SHA384)
    hipLaunchKernelGGL(k_digest_stream<A5X_ALGO_SHA384>, dim3(g), dim3(256), a5x_digest_lds(L.algo), st, L, op);
  else if (L.algo == A5X_ALGO_SHA512)
    hipLaunchKernelGGL(k_digest_stream<A5X_ALGO_SHA512>, dim3(g), dim3(256), a5x_digest_lds(L.algo), st, L, op);
  else if (a5x_algo_nested(L.algo))
    return a5x_launch_digest_stream_nest(L, op, g, st);
  else
    return hipErrorInvalidValue;  // a missing kernel is an error, never another algorithm's digest
  return hipGetLastError();
}

uint64_t a5x_digest_blocks(uint64_t nbytes, int algo) {
  const u64 b = digest_blk(algo) ? digest_blk(algo) : DCfg<A5X_ALGO_MD5>::BLK;
  return (nbytes + b - 1) / b;
}

hipError_t a5x_launch_hits_resolve(A5xHitRaw* hits, uint32_t n, const uint64_t* blk_pre, uint64_t cand_base,
                                   const uint64_t* cand_off, uint64_t nw, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_hits_resolve, dim3((n + 63) / 64 < 4096 ? (n + 63) / 64 : 4096), dim3(64), 0, st, hits, n,
                     blk_pre, cand_base, cand_off, nw);
  return hipGetLastError();
}
#endif  // A5X_DIGEST_NEST
