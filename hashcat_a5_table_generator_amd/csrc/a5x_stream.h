// a5x_stream.h -- what the three line-stream kernels of the digest + lookup stage share:
// k_digest_stream (a5x_digest.hip), k_rules_stream (a5x_rules.hip), k_salt_stream (a5x_salt.hip).
// The geometry (block, margin, staged bytes, waves), the digest widths, the wave scan, the
// rules / salt wave's LDS layout and lane buffer, the hit record and the occupancy-sized launch
// live here once.
//
// The block staging, the SWAR newline scan and the round lister are NOT here: each kernel keeps
// its own text of them, and the rules and salt kernels their own probe and op 2 store.  As
// forced-inline helpers they compute the same, but the compiler simplifies a helper on its own
// before it inlines it, and every kernel came out with other code (scan scheduled and
// SLP-vectorized differently) whose digest pass was up to 3 % off in either direction.  What is
// shared leaves all three families' code instruction for instruction what it was; a fix to the
// scanner is still made in three places (DESIGN "The line-stream front end").
//
// LDS per wave on the rules / salt routes (StreamWave): 4432 B staged stream, 144 B round
// start list, 8704 B lane buffers (34 dwords x 64 lanes, dword k of lane l at (k * 64 + l) * 4:
// a wave's access to dword k touches 64 consecutive banks) = 13280 B; a workgroup of
// STREAM_WAVES waves takes 53120 B, so three fit the CU's 160 KiB: 12 waves, 3 on every SIMD
// (DESIGN "Rules").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "a5x_launch.h"
#include "a5x_md.h"
#include "a5x_rules.h"

typedef uint64_t u64;
typedef uint32_t u32;

constexpr u32 STREAM_MARGIN = 256;            // next-block bytes staged for straddling lines
constexpr u32 STREAM_ERR_HITCAP = 1u << 10;   // more hits than the caller's buffer
// the rules / salt routes: stream bytes per wave (C5's ~23-byte lines fill 3 rounds of 64 lanes
// to 93 %; k_hits_resolve's ordinals count these blocks) and waves per workgroup (one per SIMD,
// so a CU's resident workgroups load its SIMDs alike)
constexpr u32 STREAM_BLK = 4096;
constexpr u32 STREAM_WAVES = 4;
// a line that starts in the block and is at most A5X_RULE_LMAX bytes has its '\n' staged:
// longer lines are rejected, so those routes never read a line from HBM
static_assert(STREAM_MARGIN >= A5X_RULE_LMAX + 1u, "a message-sized line that starts in a block must end in the staged margin");
static_assert(A5X_RULE_NDW * 4u >= A5X_RULE_LMAX + 8u, "the hash sources read up to 8 bytes past the message");

// staged bytes of a wave: block, margin, slack for the 8-B over-reads of the message loads
template <u32 BLK> constexpr u32 STREAM_BUF = BLK + STREAM_MARGIN + 80;

// digest width of an algorithm: DW = its 32-bit words, HT = words of a hit's tail record
template <int ALGO> struct StreamCfg {
  static constexpr u32 DW = a5x_algo_words(ALGO);
  static constexpr u32 HT = a5x_hit_tail_stride(ALGO);
  static_assert(DW <= 4u || DW - 4u <= HT, "the hit's tail record holds the whole tail");
};

__device__ __forceinline__ u32 wave_incl_scan(u32 x) {
  const u32 lane = __lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u32 y = (u32)__shfl_up((int)x, d, 64);
    if ((int)lane >= d) x += y;
  }
  return x;
}

// ---- the rules / salt routes: lane buffers and rounds of 64 candidates -----------------
struct StreamWave {
  uint8_t data[STREAM_BUF<STREAM_BLK>];
  uint16_t starts[72];           // the round's 64 line starts + the next one
  u32 lanes[A5X_RULE_NDW * 64];  // working buffers, dword-interleaved
};
static_assert(sizeof(StreamWave) == 13280, "three workgroups of STREAM_WAVES waves fit a CU's LDS");

// the lane's working buffer: dword k at lanes[k * 64 + lane] (whatever k: the bank is the lane)
struct StreamLane {
  u32* p;  // &lanes[lane]
  __device__ __forceinline__ u32 rd(u32 k) const { return p[k * 64u]; }
  __device__ __forceinline__ void wr(u32 k, u32 v) { p[k * 64u] = v; }
  // message source of the digests: 4 bytes at message offset i (zero past the message)
  __device__ __forceinline__ u32 at4(u32 i) const {
    const u32 lo = p[(i >> 2) * 64u];
    return (i & 3u) ? __builtin_amdgcn_alignbyte(p[((i >> 2) + 1u) * 64u], lo, i & 3u) : lo;
  }
};

// ---- the hit record ----------------------------------------------------------------------
// op 0: hit h of the hit buffer (block, ordinal in block, digest), its tail, and on the rules /
// salt routes (SIDE) its rule or salt index tag in side[], the u32 array beside the hit buffer.
// The caller draws h from the hit counter and checks it against the buffer's size.
template <u32 DW, u32 HT, bool SIDE>
__device__ __forceinline__ void stream_write_hit(A5xHitRaw* hits, u32* hit_tail, u32 h, u64 blk, u32 i, const u32* d,
                                                 u32* side, u32 tag) {
  A5xHitRaw r;
  r.blk = blk; r.idx = i; r.d[0] = d[0]; r.d[1] = d[1]; r.d[2] = d[2]; r.d[3] = d[3];
  hits[h] = r;
  if constexpr (SIDE) side[h] = tag;
  if constexpr (DW > 4) {
#pragma unroll
    for (u32 k = 0; k < HT; k++) hit_tail[(u64)HT * h + k] = k < DW - 4 ? d[4 + k] : 0u;
  }
}

// ---- launch of one rules / salt kernel instantiation K --------------------------------
// The grid is exactly the waves the device holds at once (cus x resident workgroups): every
// wave takes the same share of the blocks in its grid-stride loop.  A larger grid runs a
// second, part-empty residency round -- 16 waves per CU launched against 12 resident cost
// 0.72-0.85 of the no-rule stream's hash rate where this gives DESIGN "Rules"'s figures.
// (K is a template argument, not a function argument, so that per_cu is cached per kernel.)
template <auto K, class L>
static hipError_t stream_launch(const L& l, int op, u32 cus, hipStream_t st) {
  const u64 want = (a5x_stream_blocks(l.d.nbytes) + STREAM_WAVES - 1) / STREAM_WAVES;
  const size_t lds = a5x_stream_lds();
  static int per_cu = 0;  // workgroups of K one CU holds at once (LDS: 3; fewer if the registers say so)
  if (!per_cu) {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, K, 64 * STREAM_WAVES, lds) != hipSuccess || v < 1)
      v = 2;  // (2 waves per SIMD)
    per_cu = v;
  }
  const u64 grid = (u64)(cus ? cus : 1u) * (u32)per_cu;
  const u32 g = (u32)(want < grid ? want : grid);
  hipLaunchKernelGGL(K, dim3(g), dim3(64 * STREAM_WAVES), lds, st, l, op);
  return hipGetLastError();
}
