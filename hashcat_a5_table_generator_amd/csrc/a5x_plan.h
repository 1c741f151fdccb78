// a5x_plan.h -- per-word unit scan, keyspace closed form and piece plan of the
// FAST expansion path.  Host + device: the kernels (a5x_kernels.hip) run it per
// lane; the host library runs the same code for a5x_debug_fast_word(), which the
// CPU test suite compares against the oracle (tests/test_plan.py).
//
// Reference semantics (processWord, /root/reference/main.go:168-205): a candidate
// is a set of non-overlapping key matches of the ORIGINAL word plus one value per
// match.  Matches are grouped into *units*: a lone match (R = 1 + nvals choices,
// choice 0 = the key itself) or a *cluster* of overlapping matches (e.g. "s"/"ss"
// over "ss", czech+german), whose choices are all non-overlapping subsets of its
// matches times their values (choice 0 = no match).  Units are disjoint, so the
// candidates are the mixed-radix product of the units minus the all-zero
// (unchanged) combination, whenever the substitution-count window is free
// (min <= 1 and every candidate's count <= max).
#pragma once
#include <stdint.h>

#include "a5x_format.h"

#define A5X_HD __host__ __device__ inline

typedef uint64_t u64;
typedef uint32_t u32;
typedef int64_t i64;

// ---------------------------------------------------------------------------
// the device table (see a5x_format.h)
// ---------------------------------------------------------------------------
struct Tab {
  const A5xTableHdr* hdr;
  const uint16_t* bucket;
  const A5xKey* keys;
  const A5xChoice* ch;
  const uint8_t* blob;
  const u64* kmatch;   // first min(klen, 4) key bytes | klen << 32
  const u32* bucket2;  // bucket[b] | bucket[b + 1] << 16
  const u64* cval;     // choice bytes (<= 7) | len << 56
};

A5X_HD Tab tab_view(const uint8_t* base) {
  Tab t;
  t.hdr = (const A5xTableHdr*)base;
  t.bucket = (const uint16_t*)(base + t.hdr->off_bucket);
  t.keys = (const A5xKey*)(base + t.hdr->off_keys);
  t.ch = (const A5xChoice*)(base + t.hdr->off_choices);
  t.blob = base + t.hdr->off_blob;
  t.kmatch = (const u64*)(base + t.hdr->off_kmatch);
  t.bucket2 = (const u32*)(base + t.hdr->off_bucket2);
  t.cval = (const u64*)(base + t.hdr->off_cval);
  return t;
}

A5X_HD u64 mul_ovf(u64 a, u64 b, bool& ovf) {
  u64 r;
  ovf |= __builtin_mul_overflow(a, b, &r);
  return r;
}
A5X_HD u64 add_ovf(u64 a, u64 b, bool& ovf) {
  u64 r = a + b;
  ovf |= r < a;
  return r;
}
A5X_HD u32 umin32(u32 a, u32 b) { return a < b ? a : b; }
A5X_HD u32 umax32(u32 a, u32 b) { return a > b ? a : b; }

// libdivide u32 branch-free division (d >= 2): l = ceil(log2 d), M = floor(2^32 (2^l - d) / d) + 1
A5X_HD void divmagic(u32 d, u32& magic, u32& shift) {
  const u32 l = 32 - (u32)__builtin_clz(d - 1);
  const u64 m = (((u64)1 << 32) * (((u64)1 << l) - d)) / d + 1;
  magic = (u32)m;
  shift = l - 1;
}
A5X_HD u32 fastdiv_hd(u32 n, u32 magic, u32 shift) {
  const u32 q = (u32)(((u64)n * magic) >> 32);
  return (((n - q) >> 1) + q) >> shift;
}

// ---------------------------------------------------------------------------
// FAST plan records (built once per word by k_keyspace_thread, streamed by
// k_expand_fast).  A record is a run of u64 in HBM:
//   [0]               header  (fr_hdr)
//   [1, 1+np)         piece descriptors, pieces in byte order (fr_desc)
//   [1+np, 1+np+ne)   piece entries: the R entries of a piece consecutive, pieces
//                     in order; entry = 7 content bytes + meta byte (len | (R-1) << 3)
// A word is cut left to right into pieces of <= FW_PLEN bytes: a *group* piece
// holds one or more consecutive substitution units (a key match with its R =
// 1 + nvals choices, or a cluster of overlapping matches) with the literal bytes
// around them, all R_1 x R_2 x ... <= FW_UMAXR combinations precombined; a
// *literal* piece holds plain bytes (R = 1).  Combination a_1 + R_1 (a_2 + ...)
// of a group is the mixed-radix digit order of its units (left unit least
// significant), and pieces are digits of the word's candidate index n = rank + 1
// in the same order, so candidate numbering equals the per-unit radix order of
// the other expansion kernels.
// ---------------------------------------------------------------------------
#define FW_PLEN 7    // bytes per piece
#define FW_UMAXM 8   // matches per cluster unit
#define FW_UMAXR 16  // choices per unit / group (4-bit R-1 fields)
#define FW_PMAX 8    // pieces per word
#define FW_RMAX 250  // record u64 per word (window budget)
#define FW_TILE 256  // words per keyspace tile (one workgroup)
#define FW_TILE_REC (FW_TILE * 40)  // record u64 budget per tile (avg 320 B / word)
#define FW_MAXL 1000 // longest candidate (+ newline) of a FAST word
#define FW_PMAX_CNT (1u << 24)  // candidates per FAST word: exact magic division (n (R-1) < 2^32)
                                // and 24-bit digit products (v_mad_u32_u24)
// big pieces (k_expand_fast window setup): consecutive small pieces combined into
// <= FB_PLEN bytes with <= FB_RMAX combinations, entries of 16 B (15 bytes + length)
#define FB_PLEN 15
#define FB_RMAX 64
#define FB_SPAN 4    // small pieces per big piece
#define FB_NMAX 4    // big pieces per word
#ifndef FB_EMAX
#define FB_EMAX 254  // big entries per word (window budget)
#endif

#define FW_M56 0x00FFFFFFFFFFFFFFull
A5X_HD u64 fw_meta(u32 len, u32 R) { return (u64)(len | ((R - 1u) << 3)) << 56; }
A5X_HD u32 fw_len(u64 e) { return (u32)(e >> 56) & 7u; }
A5X_HD u64 keep_bytes64(u64 v, u32 n) { return n >= 8 ? v : (v & ((1ull << (8 * n)) - 1ull)); }

// header: np | ng << 4 | ne << 8 | maxl << 16 | nbig << 28 | first small piece of
//         big pieces 1..3 << 31 (3 bits each) | R - 1 of big pieces 0..3 << 40 (6 bits
//         each; 0 past nbig, i.e. R = 1)
A5X_HD u64 fr_hdr(u32 np, u32 ng, u32 ne, u32 maxl, u32 nbig, u32 bstarts, u32 bRp) {
  return (u64)np | ((u64)ng << 4) | ((u64)ne << 8) | ((u64)maxl << 16) | ((u64)nbig << 28) | ((u64)bstarts << 31) |
         ((u64)bRp << 40);
}
A5X_HD u32 frh_nbig(u64 h) { return (u32)(h >> 28) & 7u; }
A5X_HD u32 frh_bstart(u64 h, u32 b) { return b == 0 ? 0u : (b > 3 ? 15u : (u32)(h >> (31 + 3 * (b - 1))) & 7u); }
A5X_HD u32 frh_np(u64 h) { return (u32)h & 15u; }
A5X_HD u32 frh_ng(u64 h) { return (u32)(h >> 4) & 15u; }
A5X_HD u32 frh_ne(u64 h) { return (u32)(h >> 8) & 255u; }
A5X_HD u32 frh_maxl(u64 h) { return (u32)(h >> 16) & 4095u; }
A5X_HD u32 frh_R(u64 h, u32 b) { return ((u32)(h >> (40 + 6 * b)) & 63u) + 1u; }  // R of big piece b

// piece descriptor: magic = ceil(2^32 / R) (0 for R = 1) | first entry (relative
// to the entries) << 32 | (R-1) << 40 | (R == 1) << 63.  The digit of n is
// d = n - q R with q = umulhi(n, magic) (+ n when R = 1): exact for n (R - 1) <
// 2^32 (FW_PMAX_CNT bound).
A5X_HD u32 fr_magic(u32 R) { return R > 1 ? 0xFFFFFFFFu / R + 1u : 0u; }  // (= ceil(2^32 / R): a 32-bit division)
A5X_HD u64 fr_desc(u32 R, u32 ebase) {
  return (u64)fr_magic(R) | ((u64)(ebase & 255u) << 32) | ((u64)(R - 1) << 40) | ((u64)(R == 1) << 63);
}
A5X_HD u32 frd_R(u64 G) { return ((u32)(G >> 40) & 31u) + 1u; }
A5X_HD u32 frd_ebase(u64 G) { return (u32)(G >> 32) & 255u; }

// FAST flag fields (written by the keyspace pass): record size = 1 + np + ne
A5X_HD u32 ff_ng(u32 f) { return (f >> 10) & 31u; }
A5X_HD u32 ff_ne(u32 f) { return (f >> 16) & 255u; }
A5X_HD u32 ff_np(u32 f) { return (f >> 24) & 31u; }
A5X_HD u32 ff_rsize(u32 f) { return 1u + ff_np(f) + ff_ne(f); }

// k_expand_fast window: records at wrec[0, FX_ZSLOT), wrec[FX_ZSLOT] = 0 (the
// empty entry every piece past a word's last one reads).
#define FX_WREC 256
#define FX_ZSLOT 255

// A word's bytes in global memory (or host memory).
struct GWord {
  const uint8_t* p;
  A5X_HD u32 at(u32 i) const { return p[i]; }
  A5X_HD u64 ld(u32 i, u32 n) const {  // n <= 7
    u64 v = 0;
    for (u32 k = 0; k < n; k++) v |= (u64)p[i + k] << (8 * k);
    return v;
  }
};

template <class W>
A5X_HD bool key_match_w(const W& wd, u32 p, const A5xKey& key, const Tab& T) {
  const A5xChoice c0 = T.ch[key.choice_base];
  for (u32 i = 1; i < key.klen; i++) {  // byte 0 matched by the bucket
    const u32 kb = i < 4 ? ((c0.first4 >> (8 * i)) & 255u) : T.blob[c0.blob_off + i];
    if (wd.at(p + i) != kb) return false;
  }
  return true;
}

// <= 7 bytes of choice ci as a u64
A5X_HD u64 choice7(const Tab& T, u32 ci) {
  const A5xChoice c = T.ch[ci];
  u64 v = c.first4;
  for (u32 k = 4; k < c.len && k < 8; k++) v |= (u64)T.blob[c.blob_off + k] << (8 * k);
  return v;
}

// ---------------------------------------------------------------------------
// units
// ---------------------------------------------------------------------------
struct Unit {
  u32 s, e;        // byte span [s, e) of the original word
  u32 R;           // choices; choice 0 = the span unchanged
  u32 ml;          // longest choice (bytes)
  u32 mnl;         // shortest choice (bytes)
  u32 spos, sneg;  // sums over choices of max(len - span, 0) and max(span - len, 0)
  int maxd;        // longest choice - span
  u32 nm;          // key matches in the unit (bounds the substitutions of a choice)
  u32 key;         // lone match: its key index
  u32 cb;          // lone match: the key's choice_base (choices cb + a, a < R)
  u32 k;           // cluster: number of matches (0 for a lone match)
  u64 m0, m1;      // cluster matches 0-3 / 4-7, 16 bits each: (pos - s) << 10 | key index
  bool ok;         // cluster fits FW_UMAXM matches, FW_UMAXR choices of <= FW_PLEN bytes
};

A5X_HD u32 unit_mkey(const Unit& U, u32 j) { return (u32)((j < 4 ? U.m0 : U.m1) >> (16 * (j & 3))) & 1023u; }
A5X_HD u32 unit_mpos(const Unit& U, u32 j) { return U.s + ((u32)((j < 4 ? U.m0 : U.m1) >> (16 * (j & 3) + 10)) & 63u); }

// Enumerate the choices of a cluster in a fixed order (match subsets by increasing
// bitmask, then values as an odometer, first match fastest); choice 0 is the empty
// subset.  target -1: statistics only (R, ml, spos, sneg, maxd, ok); target -2:
// also every choice a into content[a * cstride] (bytes | len << 56); else stop at
// choice `target` and return its bytes (len <= FW_PLEN) in *content / *len.
template <class W>
A5X_HD void cluster_choices(const W& wd, Unit& U, const Tab& T, int target, u64* content, u32* len,
                            u32 cstride = 1) {
  const u32 span = U.e - U.s;
  u32 R = 0, ml = 0, mnl = 0xffffffffu, spos = 0, sneg = 0;
  int maxd = -(int)span;
  bool ok = U.ok;
  for (u32 mask = 0; mask < (1u << U.k) && ok; mask++) {
    // valid = chosen matches pairwise disjoint (matches are in position order)
    u32 last = 0, nch = 0;
    bool valid = true;
    for (u32 j = 0; j < U.k; j++) {
      if (!((mask >> j) & 1u)) continue;
      const u32 pj = unit_mpos(U, j);
      if (nch && pj < last) { valid = false; break; }
      last = pj + T.keys[unit_mkey(U, j)].klen;
      nch++;
    }
    if (!valid) continue;
    // value odometer over the chosen matches: 4-bit digit j in [0, nvals_j)
    u32 odo = 0;
    while (true) {
      // bytes of this choice
      u64 v = 0;
      u32 n = 0, cur = U.s;
      for (u32 j = 0; j < U.k; j++) {
        if (!((mask >> j) & 1u)) continue;
        const u32 pj = unit_mpos(U, j);
        const A5xKey key = T.keys[unit_mkey(U, j)];
        for (; cur < pj; cur++, n++) if (n < 8) v |= (u64)wd.at(cur) << (8 * n);
        const u32 ci = key.choice_base + 1u + ((odo >> (4 * j)) & 15u);
        const u32 cl = T.ch[ci].len;
        if (n < 8) v |= choice7(T, ci) << (8 * n);
        n += cl;
        cur = pj + key.klen;
      }
      for (; cur < U.e; cur++, n++) if (n < 8) v |= (u64)wd.at(cur) << (8 * n);
      if (n > FW_PLEN || R >= FW_UMAXR) { ok = false; break; }
      if ((int)R == target) {
        *content = keep_bytes64(v, n);
        *len = n;
        U.ok = true;
        return;
      }
      if (target == -2) content[R * cstride] = keep_bytes64(v, n) | ((u64)n << 56);
      R++;
      ml = umax32(ml, n);
      mnl = umin32(mnl, n);
      if (n > span) spos += n - span; else sneg += span - n;
      maxd = (int)n - (int)span > maxd ? (int)n - (int)span : maxd;
      // next value combination
      u32 j = 0;
      for (; j < U.k; j++) {
        if (!((mask >> j) & 1u)) continue;
        const u32 dj = ((odo >> (4 * j)) & 15u) + 1u;
        odo &= ~(15u << (4 * j));
        if (dj < T.keys[unit_mkey(U, j)].nvals && dj < 16u) { odo |= dj << (4 * j); break; }
      }
      if (j == U.k) break;
    }
  }
  U.R = R; U.ml = ml; U.mnl = mnl; U.spos = spos; U.sneg = sneg; U.maxd = maxd; U.ok = ok;
}

// Next unit at or after p (p advances past it).  Returns false at the end of the word.
// cbuf: a cluster's statistics come from the target -2 enumeration, which also leaves its
// choices in cbuf[a * cstride] (k_keyspace_cplx: the build pass then needs no enumeration
// of its own for that cluster); nullptr: statistics only.
template <class W>
A5X_HD bool next_unit(const W& wd, u32 L, u32& p, const Tab& T, Unit& U, u64* cbuf = nullptr, u32 cstride = 1) {
  for (; p < L; p++) {
    u32 e = p, nmatch = 0, k0 = 0;
    U.m0 = 0; U.m1 = 0;
    U.ok = true;
    // matches at p, then at every position inside the growing span
    for (u32 q = p; q < e || q == p; q++) {
      const u32 b = wd.at(q);
      const u32 ks = T.bucket[b], ke = T.bucket[b + 1];
      for (u32 kk = ks; kk < ke; kk++) {
        const A5xKey key = T.keys[kk];
        if (q + key.klen > L || !key_match_w(wd, q, key, T)) continue;
        if (nmatch < FW_UMAXM && q - p < 64 && kk < 1024) {
          const u64 f = (u64)(((q - p) << 10) | kk) << (16 * (nmatch & 3));
          if (nmatch < 4) U.m0 |= f; else U.m1 |= f;
        } else
          U.ok = false;
        if (nmatch == 0) k0 = kk;
        nmatch++;
        e = umax32(e, q + key.klen);
      }
      if (q == p && nmatch == 0) break;
    }
    if (nmatch == 0) continue;
    U.s = p; U.e = e; U.nm = nmatch;
    if (nmatch == 1) {
      const A5xKey key = T.keys[k0];
      U.key = k0; U.k = 0; U.cb = key.choice_base;
      U.R = key.nvals + 1u; U.ml = key.maxclen; U.mnl = key.minclen;
      U.spos = key.sum_dpos; U.sneg = key.sum_dneg; U.maxd = key.maxdelta;
      U.ok = true;
    } else {
      U.key = ~0u; U.k = nmatch;
      if (U.ok) cluster_choices(wd, U, T, cbuf ? -2 : -1, cbuf, nullptr, cstride);
    }
    p = e;
    return true;
  }
  return false;
}

// bytes and length of choice a of a unit
template <class W>
A5X_HD u64 unit_choice(const W& wd, const Unit& U, const Tab& T, u32 a, u32& len) {
  if (U.k == 0) {  // (entries hold <= FW_PLEN = 7 bytes: longer choices never get here)
    const u64 e = T.cval[U.cb + a];
    len = (u32)(e >> 56);
    return e & FW_M56;
  }
  Unit V = U;
  u64 v = 0;
  len = 0;
  cluster_choices(wd, V, T, (int)a, &v, &len);
  return v;
}

// unit_choice with a cluster's choices already enumerated into cb (stride cs)
template <class W>
A5X_HD u64 unit_choice_b(const W& wd, const Unit& U, const Tab& T, u32 a, u32& len, const u64* cb, u32 cs) {
  if (U.k == 0) return unit_choice(wd, U, T, a, len);
  const u64 e = cb[a * cs];
  len = (u32)(e >> 56);
  return e & FW_M56;
}

// ---------------------------------------------------------------------------
// piece plan -> record
// ---------------------------------------------------------------------------
struct Plan {
  u32 np, ng, ne, lconst, maxl, minl;
  u32 nbig, bstarts, bent;  // big pieces, their first small pieces (3 bits each), big entries
  u32 bRp;                  // R - 1 of big pieces 0..3 (6 bits each)
  bool ok;
};

// Record sinks.  gld/gst(ne, a): entry a of the open group (R <= FW_UMAXR entries, built in
// place while units merge into it; ne = the entries closed so far); ent(i, v): final entry i; desc(i, v): piece i.
// cbuf / cstride: where a cluster unit's choices are enumerated once (BUILD only).
struct NullSink {
  A5X_HD u64* cbuf() const { return nullptr; }
  A5X_HD u32 cstride() const { return 1; }
  A5X_HD u64 gld(u32, u32) const { return 0; }
  A5X_HD void gst(u32, u32, u64) {}
  A5X_HD void ent(u32, u64) {}
  A5X_HD void desc(u32, u64) {}
};
struct ArraySink {  // host replay / tests: rec[0..] as laid out in HBM
  u64* rec;
  u32 np;
  u64 g[FW_UMAXR], c[FW_UMAXR];
  A5X_HD u64* cbuf() { return c; }
  A5X_HD u32 cstride() const { return 1; }
  A5X_HD u64 gld(u32, u32 a) const { return g[a]; }
  A5X_HD void gst(u32, u32 a, u64 v) { g[a] = v; }
  A5X_HD void ent(u32 i, u64 v) { rec[1 + np + i] = v; }
  A5X_HD void desc(u32 i, u64 v) { rec[1 + i] = v; }
};

#ifndef PL_SPLIT_CAP
#define PL_SPLIT_CAP 4   // groups of <= this many entries merge read-all-then-write-all (registers); larger
                         // ones in place (k_keyspace_thread's 8-entry groups: C3 keyspace 2.19 vs 2.25 ms at 8,
                         // profiles/r06u_ab_vwords_fixed_width_c5.txt)
#endif


// Cut a unit-radix word into pieces (see the record format above), one unit at a
// time (unit() in word order, then finish()).  BUILD: also write the entries and
// piece descriptors through the sink (the header is the caller's: fr_hdr of P).
// Shared by the unit walk (plan_word) and the position-synchronous keyspace kernel.
template <bool BUILD, class W, class S, u32 CAP = FW_UMAXR>
struct Planner {
  const W& wd;
  const Tab& T;
  S& sk;
  Plan P;
  bool open;                    // a group piece is being built
  u32 bR, bl, bspan;            // the big piece being filled
  u32 cR, cmax, cmin, cpi, prev;
  // Balanced big pieces (BUILD walks): a second grouping of the same small pieces with
  // R per big piece capped at acap (0: none).  The greedy grouping fills every big piece
  // up to FB_RMAX combinations, e.g. R 4 4 4 3 -> 64 + 3 = 67 entries; capped near
  // P^(1 / nbig) the same two pieces are 16 + 12 = 28 entries.  k_expand_fast's windows
  // are bounded by their big entries, so fewer entries = more words and candidates per
  // window setup.  pick_balanced() takes it when it has as many big pieces as the greedy.
  u32 acap, aR, al, aspan;
  Plan A;
  // first word byte of pieces 0..7 (7 bits each; k_keyspace_vsub's patched sub-words --
  // dead code for every other user)
  u64 pst;

  A5X_HD Planner(const W& w, const Tab& t, S& s, u32 balanced_cap = 0) : wd(w), T(t), sk(s) {
    P.np = 0; P.ng = 0; P.ne = 0; P.lconst = 0; P.maxl = 0; P.minl = 0; P.ok = true;
    P.nbig = 0; P.bstarts = 0; P.bent = 0; P.bRp = 0;
    open = false; bR = 1; bl = 0; bspan = 0; cR = 1; cmax = 0; cmin = 0; cpi = 0; prev = 0; pst = 0;
    acap = balanced_cap; aR = 1; al = 0; aspan = 0;
    A.nbig = 0; A.bstarts = 0; A.bent = 0; A.bRp = 0;
  }
  static A5X_HD void big_join(Plan& Q, u32& qR, u32& ql, u32& qspan, u32 cap, u32 R, u32 maxlen, u32 pi) {
    if (Q.nbig && ql + maxlen <= FB_PLEN && qR * R <= cap && qspan < FB_SPAN) {
      Q.bent += qR * R - qR;
      qR *= R; ql += maxlen; qspan++;
    } else {
      if (Q.nbig >= 1 && Q.nbig <= 3) Q.bstarts |= (pi & 7u) << (3 * (Q.nbig - 1));
      Q.nbig++;
      Q.bent += R;
      qR = R; ql = maxlen; qspan = 1;
    }
    if (Q.nbig <= FB_NMAX) {
      const u32 sh = 6u * (Q.nbig - 1u);
      Q.bRp = (Q.bRp & ~(63u << sh)) | (((qR - 1u) & 63u) << sh);
    }
  }
  A5X_HD void big_add(u32 R, u32 maxlen, u32 pi) {  // small piece pi (in order) joins a big piece
    big_join(P, bR, bl, bspan, FB_RMAX, R, maxlen, pi);
    if (acap) big_join(A, aR, al, aspan, acap, R, maxlen, pi);
  }
  A5X_HD void pick_balanced() {
    if (acap && A.nbig == P.nbig && A.bent < P.bent) {
      P.bstarts = A.bstarts; P.bRp = A.bRp; P.bent = A.bent;
    }
  }
  A5X_HD void close_group() {
    if constexpr (BUILD) {
      for (u32 a = 0; a < cR; a++)
        if (a < cR) sk.ent(P.ne + a, sk.gld(P.ne, a));
      sk.desc(cpi, fr_desc(cR, P.ne));
    }
    big_add(cR, cmax, cpi);
    P.ne += cR; P.ng++; P.maxl += cmax; P.minl += cmin;
    open = false;
  }
  A5X_HD void piece_at(u32 pi, u32 off) {
    if (pi < 8) pst |= (u64)(off & 127u) << (7 * pi);
  }
  A5X_HD void literal(u32 off, u32 n, bool nl_last) {  // one literal piece of n bytes
    piece_at(P.np, off);
    if constexpr (BUILD) {
      const u32 nb = nl_last ? n - 1 : n;
      u64 v = nb ? wd.ld(off, nb) : 0ull;
      if (nl_last) v |= 10ull << (8 * nb);
      sk.ent(P.ne, v | fw_meta(n, 1));
      sk.desc(P.np, fr_desc(1, P.ne));
    }
    big_add(1, n, P.np);
    P.ne++; P.np++; P.lconst += n; P.maxl += n; P.minl += n;
  }
  // have_choices: the cluster's choices are already in the sink's cbuf (next_unit with cbuf)
  A5X_HD void unit(const Unit& U, bool have_choices = false) {
    if (!P.ok) return;
    const u32 Ru = U.R, ml = U.ml, run = U.s - prev;
    if (!U.ok || ml > FW_PLEN || Ru > CAP || Ru < 2) { P.ok = false; return; }
    u64* cb = nullptr;
    u32 cs = 1;
    if constexpr (BUILD) {
      if (U.k) {  // cluster: all choices once (unit_choice would re-enumerate per entry)
        cb = sk.cbuf(); cs = sk.cstride();
        if (!have_choices) {
          Unit V = U;
          cluster_choices(wd, V, T, -2, cb, nullptr, cs);
        }
      }
    }
    if (open && cmax + run + ml <= FW_PLEN && cR * Ru <= CAP) {
      // merge: entry a1 + cR * a2 = old[a1] ++ run ++ choice a2 (descending: in place;
      // fixed trip count so lanes of a wave stay together)
      const u32 nR = cR * Ru;
      if constexpr (BUILD && CAP <= PL_SPLIT_CAP) {
        // small groups: every old entry and choice read first (one round trip, nothing
        // written yet), then every new entry written -- no read waits behind a write
        const u64 rb = run ? wd.ld(prev, run) : 0ull;
        const u32 inv = (256u + cR - 1u) / cR;  // t / cR = (t * inv) >> 8 for t < 16
        u64 ov[CAP], cv[CAP];
        u32 cl[CAP];
#pragma unroll
        for (u32 t = 0; t < CAP; t++) {
          const u32 a2 = (t * inv) >> 8, a1 = t - a2 * cR;
          cl[t] = 0;
          ov[t] = t < nR ? sk.gld(P.ne, a1) : 0ull;
          cv[t] = t < nR ? unit_choice_b(wd, U, T, a2, cl[t], cb, cs) : 0ull;
        }
#pragma unroll
        for (u32 t = 0; t < CAP; t++) {
          if (t < nR) {
            const u32 ol = fw_len(ov[t]);
            const u64 v = (ov[t] & FW_M56) | (rb << (8 * ol)) | (cv[t] << (8 * (ol + run)));
            sk.gst(P.ne, t, (v & FW_M56) | fw_meta(ol + run + cl[t], nR));
          }
        }
      } else if constexpr (BUILD) {
        const u64 rb = run ? wd.ld(prev, run) : 0ull;
        const u32 inv = (256u + cR - 1u) / cR;  // t / cR = (t * inv) >> 8 for t < 16
        for (int t = nR - 1; t >= 0; t--) {
          if ((u32)t >= nR) continue;
          const u32 a2 = ((u32)t * inv) >> 8, a1 = (u32)t - a2 * cR;
          u32 cl = 0;
          const u64 cv = unit_choice_b(wd, U, T, a2, cl, cb, cs);
          const u64 old = sk.gld(P.ne, a1);
          const u32 ol = fw_len(old);
          const u64 v = (old & FW_M56) | (rb << (8 * ol)) | (cv << (8 * (ol + run)));
          sk.gst(P.ne, (u32)t, (v & FW_M56) | fw_meta(ol + run + cl, nR));
        }
      }
      cR = nR; cmax += run + ml; cmin += run + U.mnl;
    } else {
      if (open) close_group();
      u32 off = prev, rem = run;
      while (rem + ml > FW_PLEN) {  // literal run that does not fit with the unit
        const u32 n = umin32(FW_PLEN, rem);
        literal(off, n, false);
        off += n; rem -= n;
      }
      open = true; cR = Ru; cmax = rem + ml; cmin = rem + U.mnl; cpi = P.np;
      piece_at(cpi, off);
      P.np++;
      if constexpr (BUILD && CAP <= PL_SPLIT_CAP) {  // (read every choice, then write)
        const u64 rb = rem ? wd.ld(off, rem) : 0ull;
        u64 cv[CAP];
        u32 cl[CAP];
#pragma unroll
        for (u32 a = 0; a < CAP; a++) {
          cl[a] = 0;
          cv[a] = a < Ru ? unit_choice_b(wd, U, T, a, cl[a], cb, cs) : 0ull;
        }
#pragma unroll
        for (u32 a = 0; a < CAP; a++)
          if (a < Ru) sk.gst(P.ne, a, ((rb | (cv[a] << (8 * rem))) & FW_M56) | fw_meta(rem + cl[a], Ru));
      } else if constexpr (BUILD) {
        const u64 rb = rem ? wd.ld(off, rem) : 0ull;
        for (u32 a = 0; a < Ru; a++) {
          if (a >= Ru) continue;
          u32 cl = 0;
          const u64 cv = unit_choice_b(wd, U, T, a, cl, cb, cs);
          const u64 v = rb | (cv << (8 * rem));
          sk.gst(P.ne, a, (v & FW_M56) | fw_meta(rem + cl, Ru));
        }
      }
    }
    prev = U.e;
  }
  A5X_HD void finish(u32 L) {  // tail bytes + '\n'
    if (!P.ok) return;
    const u32 run = L - prev, tl = run + 1;
    if (open && cmax + tl <= FW_PLEN) {
      if constexpr (BUILD) {
        const u64 tb = (run ? wd.ld(prev, run) : 0ull) | (10ull << (8 * run));
        for (u32 a = 0; a < cR; a++) {
          if (a >= cR) continue;
          const u64 old = sk.gld(P.ne, a);
          const u32 ol = fw_len(old);
          sk.gst(P.ne, a, ((old | (tb << (8 * ol))) & FW_M56) | fw_meta(ol + tl, cR));
        }
      }
      cmax += tl; cmin += tl;
      close_group();
    } else {
      if (open) close_group();
      u32 off = prev, rem = tl;
      while (rem) {
        const u32 n = umin32(FW_PLEN, rem);
        literal(off, n, n == rem);
        off += n; rem -= n;
      }
    }
  }
};

// The count pass of k_keyspace_cplx's lean path, and through CutPlanner (below, which adds the
// group descriptors) of k_keyspace_thread: Planner<false> reduced to what the class decision
// (classify_finish: ok, np, ne, maxl, minl, nbig, bent) and the FAST flag fields (np, ng,
// ne) read.  No piece starts, literal bytes, big-piece starts or packed R, no balanced
// grouping; a run of literal pieces is accounted in closed form (nothing is stored per
// literal).  Same cuts as Planner: a5x_debug_plan_sizes / tests/test_plan_count_mode.py
// compare the two, and the build pass checks np / ng / ne against it per word.
template <u32 CAP = FW_UMAXR>
struct CountPlanner {
  static_assert(2 * FW_PLEN <= FB_PLEN && 3 * FW_PLEN > FB_PLEN && FB_SPAN >= 3 && FB_RMAX >= 1,
                "lit_full: two full literal pieces fill a big piece");
  // The two flags of the walk are kept as numbers, not bools: a bool that lives across the
  // divergent branches of the position loop is a lane mask that every join has to merge.
  Plan P;             // lconst, bstarts, bRp stay 0; ok is set by finish()
  u32 refused;        // units that do not fit a piece (Planner: P.ok = false)
  u32 bR, bl, bspan;  // the big piece being filled
  u32 cR, cmax, cmin, prev;  // cR = 0: no open group

  A5X_HD CountPlanner() {
    P.np = 0; P.ng = 0; P.ne = 0; P.lconst = 0; P.maxl = 0; P.minl = 0; P.ok = true;
    P.nbig = 0; P.bstarts = 0; P.bent = 0; P.bRp = 0;
    refused = 0; bR = 1; bl = 0; bspan = 0; cR = 0; cmax = 0; cmin = 0; prev = 0;
  }
  // Planner::big_join without the header fields, for a small piece that exists when c
  A5X_HD void big(u32 R, u32 maxlen, bool c = true) {
    const bool join = P.nbig && bl + maxlen <= FB_PLEN && bR * R <= FB_RMAX && bspan < FB_SPAN;
    const u32 nR = join ? bR * R : R;
    P.bent += c ? (join ? nR - bR : R) : 0u;
    P.nbig += c && !join ? 1u : 0u;
    bR = c ? nR : bR; bl = c ? (join ? bl + maxlen : maxlen) : bl; bspan = c ? (join ? bspan + 1u : 1u) : bspan;
  }
  // m literal pieces of FW_PLEN bytes (R = 1).  At most two join the open big piece (the
  // second needs bl <= FB_PLEN - 2 FW_PLEN before the first); the rest open big pieces in
  // pairs: FW_PLEN, 2 FW_PLEN <= FB_PLEN < 3 FW_PLEN.
  A5X_HD void lit_full(u32 m) {
#pragma unroll
    for (u32 t = 0; t < 2; t++) {
      const bool j = m && P.nbig && bl + FW_PLEN <= FB_PLEN && bR <= FB_RMAX && bspan < FB_SPAN;
      bl += j ? FW_PLEN : 0u; bspan += j ? 1u : 0u; m -= j ? 1u : 0u;
    }
    const u32 nb = (m + 1u) >> 1;
    P.nbig += nb; P.bent += nb;
    bR = m ? 1u : bR;
    bl = m ? ((m & 1u) ? FW_PLEN : 2u * FW_PLEN) : bl;
    bspan = m ? 2u - (m & 1u) : bspan;
  }
  // the literal pieces of Planner's splitting loops: m full ones, then one of r bytes (r > 0)
  A5X_HD void lits(u32 m, u32 r) {
    const u32 k = m + (r ? 1u : 0u), nb = m * FW_PLEN + r;
    P.np += k; P.ne += k; P.maxl += nb; P.minl += nb;
    lit_full(m);
    big(1, r, r != 0);
  }
  A5X_HD void close_group(bool c = true) {
    big(cR, cmax, c);
    P.ne += c ? cR : 0u; P.ng += c ? 1u : 0u; P.maxl += c ? cmax : 0u; P.minl += c ? cmin : 0u;
    cR = c ? 0u : cR;
  }
  // Straight-line (selects, no branches): the lanes of a wave are at different units, so a
  // branchy version runs every path anyway and pays for merging the lane masks of its
  // flags at every join.  After a refused unit the other fields are not meaningful (Planner
  // stops there; nothing reads them).
  A5X_HD void unit(const Unit& U) {
    const u32 Ru = U.R, ml = U.ml, run = U.s - prev;
    refused += U.ok && ml <= FW_PLEN && Ru <= CAP && Ru >= 2 ? 0u : 1u;
    const bool open = cR != 0, merge = open && cmax + run + ml <= FW_PLEN && cR * Ru <= CAP;
    close_group(open && !merge);
    // Planner: while (rem + ml > FW_PLEN) literal(min(FW_PLEN, rem)) -- full pieces while
    // rem >= FW_PLEN (ml = 0: while rem > FW_PLEN), then the rest when it does not fit with
    // the unit (then rest > 0, as ml <= FW_PLEN)
    const bool split = !merge && run + ml > FW_PLEN;
    const u32 m = split ? (run - (ml ? 0u : 1u)) / FW_PLEN : 0u, rest = run - m * FW_PLEN;
    const bool part = split && rest + ml > FW_PLEN;
    lits(m, part ? rest : 0u);
    const u32 rem = part ? 0u : rest;
    cR = merge ? cR * Ru : Ru;
    cmax = merge ? cmax + run + ml : rem + ml;
    cmin = merge ? cmin + run + U.mnl : rem + U.mnl;
    P.np += merge ? 0u : 1u;
    prev = U.e;
  }
  A5X_HD void finish(u32 L) {  // tail bytes + '\n'
    P.ok = refused == 0;
    if (!P.ok) return;
    const u32 tl = L - prev + 1;
    if (cR && cmax + tl <= FW_PLEN) {
      cmax += tl; cmin += tl;
      close_group();
    } else {
      if (cR) close_group();
      lits(tl / FW_PLEN, tl % FW_PLEN);
    }
  }
};

// fr_magic for the R of an 8-entry group, without the 32-bit division
A5X_HD u32 fr_magic8(u32 R) {
  u32 m = 0u;
  m = R == 2 ? 0x80000000u : m; m = R == 3 ? 0x55555556u : m; m = R == 4 ? 0x40000000u : m;
  m = R == 5 ? 0x33333334u : m; m = R == 6 ? 0x2AAAAAABu : m; m = R == 7 ? 0x24924925u : m;
  m = R == 8 ? 0x20000000u : m;
  return m;
}

// The build pass of k_keyspace_thread for words of lone units that come from a unit log
// (LG: ul(i) = unit i as q << 10 | key): Planner<true, ., ., CAP> with the construction of a
// group's entries taken out of the unit step.  Planner rewrites every entry of the open group
// at every merge, through the sink's group buffer; but a closed group's entries are a function
// of where its bytes start, its member units (<= 3: every R >= 2, CAP <= 8) and whether the
// tail joined it.  unit() / finish() only decide -- the same cuts as Planner, straight-line
// as in CountPlanner, with the header fields of big_join -- and leave one descriptor per group
// in the sink's group buffer (gst(0, g, .), g < 8: a FAST word has <= FW_PMAX pieces):
//   off | first unit << 7 | members << 15 | tail << 17 | first entry << 18 (10 bits) |
//   (R - 1) of members 0..2 << 30 (3 bits each; 0 past the last member) | piece << 39
// (the fields hold any word of <= 127 bytes with <= 8 groups, FAST or not: the host check)
// CutPlanner, which leaves the same descriptors from the count pass, adds what place_cuts
// needs to put the literal pieces and the header together without the units:
//   the byte where the last member ends << 46 (7 bits) | the longest entry's bytes << 53 (3 bits)
// build_group(g, L) then writes the group's entries and piece descriptor once, from
// registers.  Literal pieces are written where they are cut, as Planner::literal does.
// a5x_debug_piece_build / tests/test_plan_piece_build.py compare the records of the two.
template <class W, class S, class LG, u32 CAP = 8>
struct PieceBuilder {
  static_assert(CAP <= 8, "<= 3 members of R >= 2, 3-bit R - 1 fields, fr_magic8");
  const W& wd;
  const Tab& T;
  S& sk;
  const LG& ul;
  Plan P;             // lconst, minl stay 0
  u32 bR, bl, bspan;  // the big piece being filled
  u32 cR, cmax, prev; // cR = 0: no open group
  u32 nu;             // units taken (the log index of the next)
  u64 gd;             // the open group's descriptor
  u32 tj, mis;        // place_cuts: the last group took the tail; groups not where their descriptors say

  A5X_HD PieceBuilder(const W& w, const Tab& t, S& s, const LG& lg) : wd(w), T(t), sk(s), ul(lg) {
    P.np = 0; P.ng = 0; P.ne = 0; P.lconst = 0; P.maxl = 0; P.minl = 0; P.ok = true;
    P.nbig = 0; P.bstarts = 0; P.bent = 0; P.bRp = 0;
    bR = 1; bl = 0; bspan = 0; cR = 0; cmax = 0; prev = 0; nu = 0; gd = 0; tj = 0; mis = 0;
  }
  // Planner::big_join (FB_RMAX) for a small piece pi that exists when c
  A5X_HD void big(u32 R, u32 maxlen, u32 pi, bool c) {
    const bool join = P.nbig && bl + maxlen <= FB_PLEN && bR * R <= FB_RMAX && bspan < FB_SPAN;
    const bool fresh = c && !join;
    const u32 nR = join ? bR * R : R;
    P.bstarts |= fresh && P.nbig >= 1 && P.nbig <= 3 ? (pi & 7u) << ((3u * (P.nbig - 1u)) & 31u) : 0u;
    P.nbig += fresh ? 1u : 0u;
    P.bent += c ? (join ? nR - bR : R) : 0u;
    bR = c ? nR : bR; bl = c ? (join ? bl + maxlen : maxlen) : bl; bspan = c ? (join ? bspan + 1u : 1u) : bspan;
    const u32 sh = (6u * (P.nbig - 1u)) & 31u;
    P.bRp = c && P.nbig >= 1 && P.nbig <= FB_NMAX ? (P.bRp & ~(63u << sh)) | (((bR - 1u) & 63u) << sh) : P.bRp;
  }
  A5X_HD void literal(u32 off, u32 n, bool nl_last) {  // Planner::literal
    const u32 nb = nl_last ? n - 1 : n;
    u64 v = nb ? wd.ld(off, nb) : 0ull;
    if (nl_last) v |= 10ull << (8 * nb);
    sk.ent(P.ne, v | fw_meta(n, 1));
    sk.desc(P.np, fr_desc(1, P.ne));
    big(1, n, P.np, true);
    P.ne++; P.np++; P.maxl += n;
  }
  A5X_HD void close_group(bool c, bool tail) {
    if (c) sk.gst(0, P.ng & 7u, gd | ((u64)tail << 17));
    big(cR, cmax, (u32)(gd >> 39) & 127u, c);
    P.ne += c ? cR : 0u; P.ng += c ? 1u : 0u; P.maxl += c ? cmax : 0u;
    cR = c ? 0u : cR;
  }
  A5X_HD void unit(const Unit& U) {
    if (!P.ok) return;
    const u32 Ru = U.R, ml = U.ml, run = U.s - prev;
    if (!U.ok || ml > FW_PLEN || Ru > CAP || Ru < 2) { P.ok = false; return; }
    const bool open = cR != 0, merge = open && cmax + run + ml <= FW_PLEN && cR * Ru <= CAP;
    close_group(open && !merge, false);
    u32 off = prev, rem = run;
    while (!merge && rem + ml > FW_PLEN) {  // literal run that does not fit with the unit
      const u32 n = umin32(FW_PLEN, rem);
      literal(off, n, false);
      off += n; rem -= n;
    }
    const u32 nm = (u32)(gd >> 15) & 3u;  // members of the open group
    const u64 fresh = (u64)(off & 127u) | ((u64)(nu & 255u) << 7) | (1ull << 15) | ((u64)(P.ne & 1023u) << 18) |
                      ((u64)(Ru - 1u) << 30) | ((u64)(P.np & 127u) << 39);
    gd = merge ? (gd + (1ull << 15)) | ((u64)(Ru - 1u) << (30u + 3u * nm)) : fresh;
    cR = merge ? cR * Ru : Ru;
    cmax = merge ? cmax + run + ml : rem + ml;
    P.np += merge ? 0u : 1u;
    prev = U.e;
    nu++;
  }
  A5X_HD void finish(u32 L) {  // tail bytes + '\n'
    if (!P.ok) return;
    const u32 tl = L - prev + 1;
    const bool open = cR != 0, tm = open && cmax + tl <= FW_PLEN;
    cmax += tm ? tl : 0u;
    close_group(open, tm);
    u32 off = prev, rem = tm ? 0u : tl;
    while (rem) {
      const u32 n = umin32(FW_PLEN, rem);
      literal(off, n, n == rem);
      off += n; rem -= n;
    }
  }
  // The build pass from the descriptors that the count pass left (CutPlanner below: unit() /
  // finish() above are not run, the cuts are made once).  place_cuts(g), g = 0, 1, ... in
  // order: the literal pieces between the end of group g - 1 (the word's start) and group g's
  // first byte -- full FW_PLEN pieces, then the rest, as the splitting loop of unit() cuts
  // them -- and group g itself into the plan: its piece and entries are counted, its big
  // piece joined (R the product of its members', its longest entry from the descriptor).
  // build_group(g, L) writes the group as before.  place_tail(L) after the last group: the
  // tail's literal pieces ('\n' last) when no group took the tail.  P then holds what
  // unit() / finish() leave (np, ng, ne, maxl and the header's nbig, bstarts, bRp), and mis
  // counts the groups whose descriptor names another piece or first entry than the pieces
  // placed before it give.
  A5X_HD void place_cuts(u32 g) {
    const u64 d = sk.gld(0, g & 7u);
    const u32 off = (u32)d & 127u;
    for (u32 o = prev; o < off;) {
      const u32 n = umin32(FW_PLEN, off - o);
      literal(o, n, false);
      o += n;
    }
    const u32 R = (((u32)(d >> 30) & 7u) + 1u) * (((u32)(d >> 33) & 7u) + 1u) * (((u32)(d >> 36) & 7u) + 1u);
    const u32 cm = (u32)(d >> 53) & 7u;
    mis += ((u32)(d >> 39) & 127u) != P.np || ((u32)(d >> 18) & 1023u) != P.ne ? 1u : 0u;
    big(R, cm, P.np, true);
    P.ne += R; P.ng++; P.np++; P.maxl += cm;
    prev = (u32)(d >> 46) & 127u;
    tj = (u32)(d >> 17) & 1u;
  }
  A5X_HD void place_tail(u32 L) {
    u32 off = prev, rem = tj ? 0u : L - prev + 1u;
    while (rem) {
      const u32 n = umin32(FW_PLEN, rem);
      literal(off, n, n == rem);
      off += n; rem -= n;
    }
  }
  // Entries and piece descriptor of group g (< P.ng, < 8).  Entry a = the lead run, then for
  // each member in order its choice d_j and the bytes after it (the run to the next member;
  // after the last one the tail and '\n' when they joined), d_j the mixed-radix digits of a
  // over the members' R, first member least significant (Planner's a1 + cR * a2).  A group
  // is <= FW_PLEN bytes in every entry, so no shift below reaches 64 bits.
  A5X_HD void build_group(u32 g, u32 L) {
    const u64 d = sk.gld(0, g & 7u);
    const u32 off = (u32)d & 127u, i0 = (u32)(d >> 7) & 255u, nm = (u32)(d >> 15) & 3u;
    const u32 ebase = (u32)(d >> 18) & 1023u, pi = (u32)(d >> 39) & 127u;
    const bool tail = (d >> 17) & 1u;
    u32 R[3], cb[3], pl[3];
    u64 pv[3];
    u32 at = off, ll = 0;  // the byte after the last member; the lead run's length
    u64 lv = 0;
    // the group's source bytes, read once: runs and keys are <= FW_PLEN bytes together (a key
    // is no longer than its unit's longest choice, which the piece limit counts)
    const u64 src = wd.ld(off, umin32(FW_PLEN, L - off));
#pragma unroll
    for (u32 j = 0; j < 3; j++) {
      R[j] = ((u32)(d >> (30u + 3u * j)) & 7u) + 1u;
      cb[j] = 0; pl[j] = 0; pv[j] = 0;
      if (j < nm) {
        const u32 e = ul(i0 + j), q = e >> 10;
        const A5xKey& key = T.keys[e & 1023u];
        cb[j] = key.choice_base;
        const u32 n = q - at;  // the run before the member: the lead, or after member j - 1
        const u64 v = keep_bytes64(src >> (8 * (at - off)), n);
        if (j == 0) { lv = v; ll = n; }
        if (j == 1) { pv[0] = v; pl[0] = n; }
        if (j == 2) { pv[1] = v; pl[1] = n; }
        at = q + key.klen;
      }
    }
    if (tail) {
      const u32 n = L - at;
      const u64 v = keep_bytes64(src >> (8 * (at - off)), n) | (10ull << (8 * n));
#pragma unroll
      for (u32 j = 0; j < 3; j++)
        if (j + 1 == nm) { pv[j] = v; pl[j] = n + 1u; }
    }
    // Entry a = d0 + R0 (d1 + R1 d2): the bytes after member 0's choice depend on (d1, d2)
    // alone, so they are put together once per (d1, d2) (<= 4: R0 >= 2) and each of the R0
    // entries that share them costs one choice read and two appends.
    const u32 cRg = R[0] * R[1] * R[2], nsuf = R[1] * R[2];
    u32 d1 = 0, d2 = 0;
    for (u32 s = 0; s < nsuf; s++) {
      u64 sv = pv[0];
      u32 sn = pl[0];
      if (nm > 1) {
        const u64 c = T.cval[cb[1] + d1];
        sv |= (c & FW_M56) << (8 * sn);
        sn += (u32)(c >> 56);
        sv |= pv[1] << (8 * sn);
        sn += pl[1];
      }
      if (nm > 2) {
        const u64 c = T.cval[cb[2] + d2];
        sv |= (c & FW_M56) << (8 * sn);
        sn += (u32)(c >> 56);
        sv |= pv[2] << (8 * sn);
        sn += pl[2];
      }
      const u32 eb = ebase + R[0] * s;
      for (u32 a = 0; a < R[0]; a++) {  // (a plain loop: unrolled 8 times with guards it measured 20 us slower)
        const u64 c = T.cval[cb[0] + a];
        const u32 n = ll + (u32)(c >> 56);
        const u64 v = lv | ((c & FW_M56) << (8 * ll)) | (sv << (8 * n));
        sk.ent(eb + a, (v & FW_M56) | fw_meta(n + sn, cRg));
      }
      d1++;
      const bool w1 = d1 == R[1];
      d1 = w1 ? 0u : d1; d2 += w1 ? 1u : 0u;
    }
    sk.desc(pi, (u64)fr_magic8(cRg) | ((u64)(ebase & 255u) << 32) | ((u64)(cRg - 1u) << 40));
  }
};

// The count pass of k_keyspace_thread that keeps its cuts: CountPlanner (the same P and
// refused count, field by field) which also leaves the descriptor of every group it closes
// in the sink's group buffer (gst(0, g & 7, .): PieceBuilder's descriptor with the two
// fields place_cuts reads), so that the build pass makes no cut of its own.  Straight-line
// as CountPlanner::unit is; nothing is stored per unit or per literal, one store per group.
// After a refused unit, or past 8 groups, the descriptors are not meaningful (the word is
// not FAST and nothing reads them); the stores stay in the lane's 8 slots.
// a5x_debug_cut_once / tests/test_plan_cut_once.py compare it with CountPlanner, and the
// record built from its descriptors with Planner<true, ., ., 8>'s.
template <class S, u32 CAP = 8>
struct CutPlanner : CountPlanner<CAP> {
  static_assert(CAP <= 8, "3-bit R - 1 fields, <= 3 members");
  typedef CountPlanner<CAP> B;
  S& sk;
  u64 gd;  // the open group's descriptor
  u32 nu;  // units taken (the log index of the next)

  A5X_HD explicit CutPlanner(S& s) : sk(s), gd(0), nu(0) {}
  A5X_HD void close_cut(bool c, bool tail) {
    if (c) sk.gst(0, this->P.ng & 7u, gd | ((u64)tail << 17) | ((u64)(this->cmax & 7u) << 53));
    B::close_group(c);
  }
  A5X_HD void unit(const Unit& U) {  // CountPlanner::unit, with the descriptor
    const u32 Ru = U.R, ml = U.ml, run = U.s - this->prev;
    this->refused += U.ok && ml <= FW_PLEN && Ru <= CAP && Ru >= 2 ? 0u : 1u;
    const bool open = this->cR != 0, merge = open && this->cmax + run + ml <= FW_PLEN && this->cR * Ru <= CAP;
    close_cut(open && !merge, false);
    const bool split = !merge && run + ml > FW_PLEN;
    const u32 m = split ? (run - (ml ? 0u : 1u)) / FW_PLEN : 0u, rest = run - m * FW_PLEN;
    const bool part = split && rest + ml > FW_PLEN;
    this->lits(m, part ? rest : 0u);
    const u32 rem = part ? 0u : rest;
    const u32 nm = (u32)(gd >> 15) & 3u;  // members of the open group
    const u32 r1 = (Ru - 1u) & 7u;
    const u64 fresh = (u64)((U.s - rem) & 127u) | ((u64)(nu & 255u) << 7) | (1ull << 15) |
                      ((u64)(this->P.ne & 1023u) << 18) | ((u64)r1 << 30) | ((u64)(this->P.np & 127u) << 39);
    gd = (merge ? ((gd & ~(127ull << 46)) + (1ull << 15)) | ((u64)r1 << (30u + 3u * nm)) : fresh) |
         ((u64)(U.e & 127u) << 46);
    this->cR = merge ? this->cR * Ru : Ru;
    this->cmax = merge ? this->cmax + run + ml : rem + ml;
    this->cmin = merge ? this->cmin + run + U.mnl : rem + U.mnl;
    this->P.np += merge ? 0u : 1u;
    this->prev = U.e;
    nu++;
  }
  A5X_HD void finish(u32 L) {  // tail bytes + '\n'
    this->P.ok = this->refused == 0;
    if (!this->P.ok) return;
    const u32 tl = L - this->prev + 1;
    if (this->cR && this->cmax + tl <= FW_PLEN) {
      this->cmax += tl; this->cmin += tl;
      close_cut(true, true);
    } else {
      if (this->cR) close_cut(true, false);
      this->lits(tl / FW_PLEN, tl % FW_PLEN);
    }
  }
};

template <bool BUILD, class W, class S>
A5X_HD Plan plan_word(const W& wd, u32 L, const Tab& T, S& sk, u32 balanced_cap = 0) {
  Planner<BUILD, W, S> pl(wd, T, sk, balanced_cap);
  u32 p = 0;
  Unit U;
  while (pl.P.ok && next_unit(wd, L, p, T, U)) pl.unit(U);
  pl.finish(L);
  pl.pick_balanced();
  return pl.P;
}

// The units of one next_unit walk, kept so that the build pass of k_keyspace_cplx does
// not walk the word again.  Per lane, in registers (the kernel's LDS is at its
// residency limit; at 2 waves per SIMD it has registers to spare): UC_UNITS units of 16
// bits, s << 10 | key for a lone match (lone_unit rebuilds the rest), s << 10 | UC_CL for
// a cluster, whose matches and cluster_choices statistics are kept for the first
// UC_CLUSTERS clusters.  A word that does not fit (full) takes the two-walk path.
#define UC_UNITS 8
#define UC_CLUSTERS 2
#define UC_CL 1023u
A5X_HD void lone_unit(const Tab& T, u32 s, u32 k, Unit& U);
struct UnitCache {
  u64 ul0, ul1;                // units 0-3 / 4-7
  u64 m0[UC_CLUSTERS], m1[UC_CLUSTERS];
  u64 st[UC_CLUSTERS];         // span | k << 8 | R << 12 | ml << 20 | mnl << 24 | spos << 28 | sneg << 36 | (maxd + 128) << 48
  u32 n, nc;
  u32 res;                     // the unit whose choices the cluster buffer holds (~0u: none)
  bool full;
  A5X_HD UnitCache() {
    ul0 = 0; ul1 = 0; n = 0; nc = 0; res = ~0u; full = false;
    for (u32 j = 0; j < UC_CLUSTERS; j++) { m0[j] = 0; m1[j] = 0; st[j] = 0; }
  }
  A5X_HD void push(const Unit& U, bool enumerated) {
    if (full) return;
    const u32 span = U.e - U.s;
    // (an ok cluster: R <= FW_UMAXR choices of <= FW_PLEN bytes, <= FW_UMAXM matches)
    const bool fits = n < UC_UNITS && U.s < 64u && U.ok &&
                      (U.k ? nc < UC_CLUSTERS && span < 128u && U.spos < 256u && U.sneg < 4096u : U.key < UC_CL);
    if (!fits) { full = true; return; }
    const u64 f = (u64)((U.s << 10) | (U.k ? UC_CL : U.key)) << (16 * (n & 3u));
    if (n < 4) ul0 |= f; else ul1 |= f;
    if (U.k) {
      const u64 s = (u64)span | ((u64)U.k << 8) | ((u64)U.R << 12) | ((u64)U.ml << 20) | ((u64)U.mnl << 24) |
                    ((u64)U.spos << 28) | ((u64)U.sneg << 36) | ((u64)(u32)(U.maxd + 128) << 48);
#pragma unroll
      for (u32 j = 0; j < UC_CLUSTERS; j++)
        if (j == nc) { m0[j] = U.m0; m1[j] = U.m1; st[j] = s; }
      nc++;
      if (enumerated) res = n;
    }
    n++;
  }
  // unit i (in order, i = 0 .. n - 1; ci = the clusters before it, advanced here)
  A5X_HD void get(const Tab& T, u32 i, u32& ci, Unit& U) const {
    const u32 e = (u32)((i < 4 ? ul0 : ul1) >> (16 * (i & 3u))) & 0xFFFFu;
    const u32 s = e >> 10, key = e & 1023u;
    if (key != UC_CL) { lone_unit(T, s, key, U); return; }
    u64 a = 0, b = 0, c = 0;
#pragma unroll
    for (u32 j = 0; j < UC_CLUSTERS; j++)
      if (j == ci) { a = m0[j]; b = m1[j]; c = st[j]; }
    ci++;
    U.s = s; U.e = s + ((u32)c & 255u);
    U.k = (u32)(c >> 8) & 15u; U.nm = U.k; U.key = ~0u; U.cb = 0;
    U.R = (u32)(c >> 12) & 255u; U.ml = (u32)(c >> 20) & 15u; U.mnl = (u32)(c >> 24) & 15u;
    U.spos = (u32)(c >> 28) & 255u; U.sneg = (u32)(c >> 36) & 4095u; U.maxd = (int)((u32)(c >> 48) & 255u) - 128;
    U.m0 = a; U.m1 = b; U.ok = true;
  }
};

// plan_word<true> from the cached units of a walk (uc.full: not for this word).  A cluster
// whose choices the walk left in the sink's cbuf (uc.res) is not enumerated again; any
// other cluster's enumeration overwrites that buffer.
template <class W, class S>
A5X_HD Plan plan_word_cached(const W& wd, u32 L, const Tab& T, S& sk, const UnitCache& uc, u32 balanced_cap = 0) {
  Planner<true, W, S> pl(wd, T, sk, balanced_cap);
  u32 ci = 0, res = uc.res;
  for (u32 i = 0; i < uc.n && pl.P.ok; i++) {
    Unit U;
    uc.get(T, i, ci, U);
    const bool have = U.k && i == res;
    if (U.k && !have) res = ~0u;
    pl.unit(U, have);
  }
  pl.finish(L);
  pl.pick_balanced();
  return pl.P;
}

// The balanced grouping's cap for a FAST word of P = prod R = count + 1: the fewest big
// pieces nb with FB_RMAX^nb >= P, then about P^(1 / nb) with slack for the
// discreteness of the small pieces' R (slack8 in 1/8 units; 0: no balanced grouping).
#ifndef FB_BAL_SLACK8
#define FB_BAL_SLACK8 0  // off: measured on C3 (A/B, one box) the balanced grouping left the
                         // expansion at 8.78-8.80 ms and cost the keyspace 0.54 ms (3.14 -> 3.68)
#endif
// PieceBuilder (k_keyspace_thread's replayed words) keeps the greedy grouping only, while the
// fused walk, k_keyspace_cplx and the host replay call pick_balanced(): a build with the
// balanced grouping on would give the same word other big pieces by the path it takes.
static_assert(FB_BAL_SLACK8 == 0, "PieceBuilder does not track the balanced big-piece grouping");
A5X_HD u32 fb_balanced_cap(u64 P, u32 slack8 = FB_BAL_SLACK8) {
  if (!slack8 || P <= FB_RMAX) return 0;
  u32 nb = 1;
  for (u64 x = FB_RMAX; x < P && nb < FB_NMAX; nb++) x *= FB_RMAX;
  u32 r = 2;
  while (r < FB_RMAX) {
    u64 x = 1;
    for (u32 i = 0; i < nb && x < P; i++) x *= r;
    if (x >= P) break;
    r++;
  }
  const u32 c = (r * slack8 + 7u) / 8u;
  return c < r ? r : (c > FB_RMAX ? FB_RMAX : c);
}

// The unit of a lone match of key k at position s (next_unit's single-match case).
A5X_HD void lone_unit(const Tab& T, u32 s, u32 k, Unit& U) {
  const A5xKey key = T.keys[k];
  U.s = s; U.e = s + key.klen; U.nm = 1;
  U.key = k; U.k = 0; U.m0 = 0; U.m1 = 0; U.cb = key.choice_base;
  U.R = key.nvals + 1u; U.ml = key.maxclen; U.mnl = key.minclen;
  U.spos = key.sum_dpos; U.sneg = key.sum_dneg; U.maxd = key.maxdelta;
  U.ok = true;
}

// ---------------------------------------------------------------------------
// keyspace of one word by the unit closed form (k_keyspace_thread)
// ---------------------------------------------------------------------------
struct WordClass {
  u64 count, bytes;
  u32 flags;       // A5X_WF_* (+ FAST fields) or A5X_WF_DEFER
  bool ovf;        // count/bytes overflow u64
  bool clusters;   // the word has overlapping-key units (the slow path needs the DP)
};

// Closed-form keyspace accumulated unit by unit (P = product of R,
// bytes = (P - 1)(L + 1) + signed length deltas), plus the word-shape facts the
// class decision needs.
struct CountAcc {
  u64 P, Dp, Dn;
  u32 nmatch, nunits, maxl;
  bool bin, clusters, ok, ovf;
};
A5X_HD void count_init(CountAcc& A, u32 L) {
  A.P = 1; A.Dp = 0; A.Dn = 0; A.nmatch = 0; A.nunits = 0; A.maxl = L + 1;
  A.bin = true; A.clusters = false; A.ok = true; A.ovf = false;
}
A5X_HD void count_unit(CountAcc& A, const Unit& U) {
  A.nunits++;
  A.nmatch += U.nm;
  if (U.k) {
    A.clusters = true;
    if (!U.ok) A.ok = false;
  }
  const u64 R = U.R;
  // sum over the unit's choices of (|choice| - span), split by sign
  A.Dp = add_ovf(mul_ovf(A.Dp, R, A.ovf), mul_ovf(A.P, U.spos, A.ovf), A.ovf);
  A.Dn = add_ovf(mul_ovf(A.Dn, R, A.ovf), mul_ovf(A.P, U.sneg, A.ovf), A.ovf);
  A.P = mul_ovf(A.P, R, A.ovf);
  if (U.k || U.R != 2) A.bin = false;
  if (U.maxd > 0) A.maxl += (u32)U.maxd;
}

// The class decision from the accumulated units and the piece plan.  ringmax: the
// slow kernel's per-wave ring (a radix word's longest candidate must fit).
A5X_HD WordClass classify_finish(const CountAcc& A, const Plan& PL, u32 L, int mn, int mx, u32 ringmax) {
  WordClass C;
  C.count = 0; C.bytes = 0; C.flags = 0; C.ovf = false; C.clusters = A.clusters;
  if (A.ok && A.nunits == 0) {
    C.flags = A5X_WF_RADIX | A5X_WF_FAST;
    return C;
  }
  const bool freew = (mn <= 1) && ((i64)A.nmatch <= (i64)mx);
  if (!A.ok || !freew || A.ovf || A.P > (1ull << 32) || A.maxl > ringmax) {
    C.flags = A5X_WF_DEFER;
    return C;
  }
  bool o2 = false;
  const u64 cnt = A.P - 1;
  u64 byt = add_ovf(mul_ovf(cnt, (u64)L + 1, o2), A.Dp, o2);
  if (byt < A.Dn) o2 = true;
  byt -= A.Dn;
  if (o2) {
    C.flags = A5X_WF_ERR_OVF;
    C.ovf = true;
    return C;
  }
  C.count = cnt; C.bytes = byt;
  // minl >= 3: a candidate completes the dword that holds its first byte (see
  // fb_put); maxl bounds the per-round ring use
  const bool fast = PL.ok && PL.np <= FW_PMAX && PL.ne <= 255 && 1 + PL.np + PL.ne <= FW_RMAX &&
                    PL.maxl <= FW_MAXL && PL.minl >= 3 && A.P <= FW_PMAX_CNT && PL.nbig <= FB_NMAX &&
                    PL.bent <= FB_EMAX;
  if (fast) {
    C.flags = (A.clusters ? 0u : (A5X_WF_RADIX | (A.bin ? A5X_WF_BIN : 0u))) | A5X_WF_FAST | (PL.ng << 10) |
              (PL.ne << 16) | (PL.np << 24);
  } else {
    // the slow kernel re-derives the word (radix or DP walk); clusters need its DP
    C.flags = A.clusters ? 0u : (A5X_WF_RADIX | (A.bin ? A5X_WF_BIN : 0u));
  }
  return C;
}

// Host check of PieceBuilder against Planner<true, ., ., 8> on one word (a5x_debug_piece_build,
// tools/piece_build_selftest.cpp): wd = the word's L <= 127 bytes; nothing past them is read
// (GWord::at / ld take the bytes they are asked for, and both planners ask inside the word: the
// self-test passes exact-size blocks under AddressSanitizer).  out[0] = PB_EQUAL / PB_DIFFERENT / PB_NA (a cluster, a key index >= 1024, or a unit
// the 8-entry group refuses: then both planners must refuse, else PB_DIFFERENT) / PB_NOTFAST
// (not FAST and more than 8 groups: the kernel never builds it and the group list does not
// hold it; any other word is compared, FAST or not); out[1..8] = units, np, ng, ne, most
// members in a group, groups the tail joined, literal pieces (of the builder's plan; the
// tests' coverage counters), the word is FAST.
enum { PB_EQUAL = 0, PB_DIFFERENT = 1, PB_NA = 2, PB_NOTFAST = 3 };
struct ULogArr {
  const u32* p;
  A5X_HD u32 operator()(u32 i) const { return p[i]; }
};
inline void piece_build_compare(const uint8_t* wd, u32 L, const Tab& T, uint32_t* out) {
  constexpr u32 NREC = 1 + 128 + 128 * 8 + 128 + 16;  // (np <= 128, ne <= 8 per byte, of any word of <= 127 bytes)
  static_assert(NREC >= 1 + 128 + 1023 + 8, "the builder's masked entry indices stay inside");
  for (int j = 0; j < 9; j++) out[j] = 0;
  GWord gw;
  gw.p = wd;
  u32 log[128], nu = 0, p = 0;
  bool na = false;
  CountAcc A;
  count_init(A, L);
  CountPlanner<8> cp;
  Unit U;
  while (next_unit(gw, L, p, T, U)) {
    if (U.k || !U.ok || U.key >= 1024u || nu >= 128u) { na = true; break; }
    log[nu++] = (U.s << 10) | U.key;
    count_unit(A, U);
    cp.unit(U);
  }
  out[0] = PB_NA; out[1] = nu;
  if (na) return;
  cp.finish(L);
  u64 ra[NREC], rb[NREC];
  for (u32 i = 0; i < NREC; i++) ra[i] = rb[i] = 0;
  ArraySink sa, sb;
  sa.rec = ra; sa.np = cp.P.ok ? cp.P.np : 128u;
  sb.rec = rb; sb.np = sa.np;
  for (u32 i = 0; i < FW_UMAXR; i++) sa.g[i] = sa.c[i] = sb.g[i] = sb.c[i] = 0;
  Planner<true, GWord, ArraySink, 8> pa(gw, T, sa);
  ULogArr lg;
  lg.p = log;
  PieceBuilder<GWord, ArraySink, ULogArr, 8> pb(gw, T, sb, lg);
  for (u32 i = 0; i < nu; i++) {
    lone_unit(T, log[i] >> 10, log[i] & 1023u, U);
    pa.unit(U);
    pb.unit(U);
  }
  pa.finish(L);
  pb.finish(L);
  if (!pa.P.ok || !pb.P.ok) {
    out[0] = !pa.P.ok && !pb.P.ok && !cp.P.ok ? PB_NA : PB_DIFFERENT;
    return;
  }
  out[2] = pb.P.np; out[3] = pb.P.ng; out[4] = pb.P.ne; out[7] = pb.P.np - pb.P.ng;
  const WordClass C = classify_finish(A, cp.P, L, 0, 1 << 30, A5X_RING_A - 16);
  out[8] = (C.flags & A5X_WF_FAST) && !(C.flags & A5X_WF_DEFER) ? 1u : 0u;
  if (pb.P.ng > 8u) {
    out[0] = out[8] ? PB_DIFFERENT : PB_NOTFAST;  // (a FAST word has <= FW_PMAX pieces)
    return;
  }
  for (u32 g = 0; g < pb.P.ng; g++) {
    const u64 d = sb.gld(0, g);
    out[5] = umax32(out[5], (u32)(d >> 15) & 3u);
    out[6] += (u32)(d >> 17) & 1u;
    pb.build_group(g, L);
  }
  ra[0] = fr_hdr(pa.P.np, pa.P.ng, pa.P.ne, pa.P.maxl, pa.P.nbig, pa.P.bstarts, pa.P.bRp);
  rb[0] = fr_hdr(pb.P.np, pb.P.ng, pb.P.ne, pb.P.maxl, pb.P.nbig, pb.P.bstarts, pb.P.bRp);
  bool eq = pa.P.bent == pb.P.bent && pa.P.np == cp.P.np && pa.P.ne == cp.P.ne && pa.P.ng == cp.P.ng;
  for (u32 i = 0; i < NREC; i++) eq = eq && ra[i] == rb[i];
  out[0] = eq ? PB_EQUAL : PB_DIFFERENT;
}

// Host check of the cut-once path of k_keyspace_thread on one word (a5x_debug_cut_once,
// tools/cut_once_selftest.cpp): the count pass with CutPlanner, then the record from its
// descriptors alone (place_cuts / build_group / place_tail), against CountPlanner<8> and
// Planner<true, ., ., 8>.  wd and the result codes as for piece_build_compare.
//   out[0..8]    as piece_build_compare (np, ng, ne, members, tails, literals of the new
//                path's plan; FAST by CountPlanner and classify_finish alone)
//   out[9]       u64 of the record (1 + np + ne) when compared, else 0
//   out[10..18]  CutPlanner:   ok np ng ne maxl minl nbig bent refused
//   out[19..27]  CountPlanner: the same
//   out[28]      groups of the reference planner (Planner<true, ., ., 8>)
// rnew / rref (CO_NREC u64 each, may be null): the two records, zero past their ends.
#define CO_NREC (1 + 128 + 128 * 8 + 128 + 16)
#define CO_NOUT 29
inline void cut_once_compare(const uint8_t* wd, u32 L, const Tab& T, uint32_t* out, u64* rnew, u64* rref) {
  static_assert(CO_NREC >= 1 + 128 + 1023 + 8, "the builder's masked entry indices stay inside");
  for (int j = 0; j < CO_NOUT; j++) out[j] = 0;
  u64 ra[CO_NREC], rb[CO_NREC];
  for (u32 i = 0; i < CO_NREC; i++) ra[i] = rb[i] = 0;
  auto give = [&]() {
    for (u32 i = 0; i < CO_NREC; i++) {
      if (rref) rref[i] = ra[i];
      if (rnew) rnew[i] = rb[i];
    }
  };
  give();
  GWord gw;
  gw.p = wd;
  u32 log[128], nu = 0, p = 0;
  bool na = false;
  CountAcc A;
  count_init(A, L);
  ArraySink sa, sb;
  sa.rec = ra; sb.rec = rb; sa.np = sb.np = 128u;
  for (u32 i = 0; i < FW_UMAXR; i++) sa.g[i] = sa.c[i] = sb.g[i] = sb.c[i] = 0;
  CountPlanner<8> cp;
  CutPlanner<ArraySink, 8> ct(sb);
  Unit U;
  while (next_unit(gw, L, p, T, U)) {
    if (U.k || !U.ok || U.key >= 1024u || nu >= 128u) { na = true; break; }
    log[nu++] = (U.s << 10) | U.key;
    count_unit(A, U);
    cp.unit(U);
    ct.unit(U);
  }
  out[0] = PB_NA; out[1] = nu;
  if (na) return;
  cp.finish(L);
  ct.finish(L);
  const Plan* pp[2] = {&ct.P, &cp.P};
  for (int k = 0; k < 2; k++) {
    uint32_t* o = out + 10 + 9 * k;
    const Plan& Q = *pp[k];
    o[0] = Q.ok; o[1] = Q.np; o[2] = Q.ng; o[3] = Q.ne; o[4] = Q.maxl; o[5] = Q.minl; o[6] = Q.nbig; o[7] = Q.bent;
    o[8] = k ? cp.refused : ct.refused;
  }
  bool same = true;  // (after a refused unit only ok and the refused count mean anything)
  for (int j = 0; j < 9; j++) same = same && (out[10 + j] == out[19 + j] || (!cp.P.ok && j >= 1 && j <= 7));
  sa.np = sb.np = cp.P.ok ? cp.P.np : 128u;
  Planner<true, GWord, ArraySink, 8> pa(gw, T, sa);
  for (u32 i = 0; i < nu; i++) {
    lone_unit(T, log[i] >> 10, log[i] & 1023u, U);
    pa.unit(U);
  }
  pa.finish(L);
  out[28] = pa.P.ok ? pa.P.ng : 0u;
  if (!pa.P.ok || !cp.P.ok) {
    out[0] = !pa.P.ok && !cp.P.ok && same ? PB_NA : PB_DIFFERENT;
    return;
  }
  const WordClass C = classify_finish(A, cp.P, L, 0, 1 << 30, A5X_RING_A - 16);
  out[8] = (C.flags & A5X_WF_FAST) && !(C.flags & A5X_WF_DEFER) ? 1u : 0u;
  out[2] = ct.P.np; out[3] = ct.P.ng; out[4] = ct.P.ne; out[7] = ct.P.np - ct.P.ng;
  if (cp.P.ng > 8u || ct.P.ng > 8u) {
    out[0] = out[8] || !same ? PB_DIFFERENT : PB_NOTFAST;  // (a FAST word has <= FW_PMAX pieces)
    return;
  }
  ULogArr lg;
  lg.p = log;
  PieceBuilder<GWord, ArraySink, ULogArr, 8> pb(gw, T, sb, lg);
  for (u32 g = 0; g < ct.P.ng; g++) {
    const u64 d = sb.gld(0, g);
    out[5] = umax32(out[5], (u32)(d >> 15) & 3u);
    out[6] += (u32)(d >> 17) & 1u;
    pb.place_cuts(g);
    pb.build_group(g, L);
  }
  pb.place_tail(L);
  ra[0] = fr_hdr(pa.P.np, pa.P.ng, pa.P.ne, pa.P.maxl, pa.P.nbig, pa.P.bstarts, pa.P.bRp);
  rb[0] = fr_hdr(pb.P.np, pb.P.ng, pb.P.ne, pb.P.maxl, pb.P.nbig, pb.P.bstarts, pb.P.bRp);
  out[9] = 1u + pa.P.np + pa.P.ne;
  // what was placed against the count pass, as the kernel checks it
  bool eq = same && pb.mis == 0 && pb.P.np == cp.P.np && pb.P.ne == cp.P.ne && pb.P.ng == cp.P.ng &&
            pb.P.nbig == cp.P.nbig && pb.P.bent == cp.P.bent && pb.P.maxl == cp.P.maxl && pa.P.bent == cp.P.bent;
  for (u32 i = 0; i < CO_NREC; i++) eq = eq && ra[i] == rb[i];
  give();
  out[0] = eq ? PB_EQUAL : PB_DIFFERENT;
}

// One walk over the units: counts and the piece plan (count mode) together.  uc: the
// units are kept for plan_word_cached; cbuf: see next_unit.
template <class W>
A5X_HD WordClass classify_word(const W& wd, u32 L, const Tab& T, int mn, int mx, u32 ringmax, UnitCache* uc = nullptr,
                               u64* cbuf = nullptr, u32 cstride = 1) {
  if (mx < 1 || L == 0) {  // processWord emits nothing
    WordClass C;
    C.count = 0; C.bytes = 0; C.ovf = false; C.clusters = false;
    C.flags = A5X_WF_RADIX | A5X_WF_FAST;
    return C;
  }
  CountAcc A;
  count_init(A, L);
  NullSink ns;
  Planner<false, W, NullSink> pl(wd, T, ns);
  u32 p = 0;
  Unit U;
  while (next_unit(wd, L, p, T, U, cbuf, cstride)) {
    count_unit(A, U);
    if (!A.ok) break;
    pl.unit(U);
    if (uc) uc->push(U, cbuf != nullptr);
  }
  pl.finish(L);
  return classify_finish(A, pl.P, L, mn, mx, ringmax);
}

// ---------------------------------------------------------------------------
// k_keyspace_cplx's lean path: what k_keyspace_thread does for words of lone units
// (detection by the kmatch records, CountPlanner, a record built per piece), with clusters.
// A word the limits below do not hold (why != 0) takes the generic path (ks_word_once:
// next_unit, Planner); the decision is the word's own.
// ---------------------------------------------------------------------------
#ifndef CL_ABL
#define CL_ABL 0    // timing ablation (variant builds only, wrong output): 1 no cluster enumeration in the count pass
#endif
#define CL_ULOG 16  // logged units per word
#define CL_NCL 2    // clusters per word
#define CL_LMAX 36  // word bytes (k_keyspace_cplx's LDS slot)
enum {
  CL_WHY_LONGKEY = 1,   // a key longer than 4 bytes at a position it fits
  CL_WHY_UNITS = 2,     // more than CL_ULOG units
  CL_WHY_POS = 4,       // a unit at byte 64 or later
  CL_WHY_KEY = 8,       // a key index >= 1024 (or a table of more than 65536 choices)
  CL_WHY_CLUSTER = 16,  // a cluster that is not ok (FW_UMAXM matches, FW_UMAXR choices of <= FW_PLEN bytes)
  CL_WHY_NCL = 32,      // more than CL_NCL clusters
  CL_WHY_SLOT = 64      // a word longer than CL_LMAX
};

// The units of a word: entry i = s << 10 | key (lone match) or s << 10 | span (cluster, bit i of
// cmask), 16 bits each in ul[i / 4]; the matches (Unit::m0 / m1) and k | R << 4 | ml << 12 of
// the clusters.  Registers: every index below is resolved by selects.
struct CplxLog {
  u64 ul0, ul1, ul2, ul3;
  u64 m0[CL_NCL], m1[CL_NCL];
  u32 st[CL_NCL];
  u32 n, nc, cmask, why;
  A5X_HD CplxLog() {
    n = 0; nc = 0; cmask = 0; why = 0;
    ul0 = 0; ul1 = 0; ul2 = 0; ul3 = 0;
    for (u32 j = 0; j < CL_NCL; j++) { m0[j] = 0; m1[j] = 0; st[j] = 0; }
  }
  A5X_HD u32 operator()(u32 i) const {
    // (masks, not selects: a select between the four is folded into one read at a selected
    // address, and a log read that way lives in scratch memory)
    const u32 j = i >> 2;
    const u64 v = (ul0 & (0ull - (u64)(j == 0))) | (ul1 & (0ull - (u64)(j == 1))) | (ul2 & (0ull - (u64)(j == 2))) |
                  (ul3 & (0ull - (u64)(j == 3)));
    return (u32)(v >> (16u * (i & 3u))) & 0xFFFFu;
  }
  A5X_HD void put(u32 i, u32 e) {
    const u64 f = (u64)(e & 0xFFFFu) << (16u * (i & 3u));
    const u32 j = i >> 2;
    ul0 |= j == 0 ? f : 0ull; ul1 |= j == 1 ? f : 0ull; ul2 |= j == 2 ? f : 0ull; ul3 |= j == 3 ? f : 0ull;
  }
  A5X_HD bool is_cluster(u32 i) const { return (cmask >> i) & 1u; }
  A5X_HD u32 cluster_of(u32 i) const { return (u32)__builtin_popcount(cmask & ((1u << i) - 1u)); }
  // unit i, a cluster (ordinal ci) with the statistics the planners' cuts read (R, ml); the
  // count pass takes the rest from cluster_choices
  A5X_HD void get(const Tab& T, u32 i, Unit& U) const {
    const u32 e = (*this)(i), s = e >> 10;
    if (!is_cluster(i)) { lone_unit(T, s, e & 1023u, U); return; }
    const u32 ci = cluster_of(i);
    u64 a = 0, b = 0;
    u32 c = 0;
#pragma unroll
    for (u32 j = 0; j < CL_NCL; j++)
      if (j == ci) { a = m0[j]; b = m1[j]; c = st[j]; }
    U.s = s; U.e = s + (e & 1023u);
    U.k = c & 15u; U.nm = U.k; U.key = ~0u; U.cb = 0;
    U.R = (c >> 4) & 255u; U.ml = (c >> 12) & 15u; U.mnl = 0; U.spos = 0; U.sneg = 0; U.maxd = 0;
    U.m0 = a; U.m1 = b; U.ok = true;
  }
  A5X_HD void set_stats(u32 ci, const Unit& U) {
#pragma unroll
    for (u32 j = 0; j < CL_NCL; j++)
      if (j == ci) st[j] = (U.k & 15u) | ((U.R & 255u) << 4) | ((U.ml & 15u) << 12);
  }
};

// cluster_choices(target -2) for the lean path: the same choices in the same order with the
// same statistics.  cluster_choices reads the key record of every match again for every subset
// and every choice (its validity loop, its byte loop, its odometer) and copies the span byte by
// byte, each a dependent LDS round trip: on C3 that enumeration was two thirds of
// k_keyspace_cplx's time.  Here the matches' facts are read once into byte fields (start and
// end inside the span, value count, the earlier matches each one overlaps), a subset is tested
// with those masks, and a choice is put together from <= 7-byte reads of the span and the
// table's cval records.  Needs choice indices below 65536 (CplxDetect checks the table).
template <class W>
A5X_HD void cluster_enum(const W& wd, Unit& U, const Tab& T, u64* content, u32 cstride) {
  const u32 span = U.e - U.s, k = U.k;
  u64 PS = 0, PE = 0, NV = 0, CF = 0, CB0 = 0, CB1 = 0;
  for (u32 j = 0; j < k && j < FW_UMAXM; j++) {
    const A5xKey& key = T.keys[unit_mkey(U, j)];
    const u32 ps = unit_mpos(U, j) - U.s, pe = ps + key.klen;
    u32 cf = 0;
    for (u32 i = 0; i < j; i++) cf |= ((u32)(PE >> (8 * i)) & 255u) > ps ? 1u << i : 0u;
    PS |= (u64)(ps & 255u) << (8 * j); PE |= (u64)(pe & 255u) << (8 * j);
    NV |= (u64)umin32(key.nvals, 255u) << (8 * j); CF |= (u64)cf << (8 * j);
    const u64 cb = (u64)(key.choice_base & 0xFFFFu) << (16 * (j & 3u));
    if (j < 4) CB0 |= cb; else CB1 |= cb;
  }
  u32 R = 0, ml = 0, mnl = 0xffffffffu, spos = 0, sneg = 0;
  int maxd = -(int)span;
  bool ok = U.ok;
  for (u32 mask = 0; mask < (1u << k) && ok; mask++) {
    u32 bad = 0;  // chosen matches that overlap an earlier chosen one
    for (u32 m = mask; m; m &= m - 1u) bad |= (u32)(CF >> (8 * (u32)__builtin_ctz(m))) & mask;
    if (bad & 255u) continue;
    u32 odo = 0;
    while (true) {
      u64 v = 0;
      u32 n = 0, cur = 0;
      for (u32 m = mask; m; m &= m - 1u) {
        const u32 j = (u32)__builtin_ctz(m), pj = (u32)(PS >> (8 * j)) & 255u;
        if (pj > cur) {
          if (n < 8) v |= wd.ld(U.s + cur, umin32(pj - cur, 7u)) << (8 * n);
          n += pj - cur;
        }
        const u32 ci = ((u32)((j < 4 ? CB0 : CB1) >> (16 * (j & 3u))) & 0xFFFFu) + 1u + ((odo >> (4 * j)) & 15u);
        const u32 cl = T.ch[ci].len;
        if (n < 8) v |= (T.cval[ci] & FW_M56) << (8 * n);
        n += cl;
        cur = (u32)(PE >> (8 * j)) & 255u;
      }
      if (span > cur) {
        if (n < 8) v |= wd.ld(U.s + cur, umin32(span - cur, 7u)) << (8 * n);
        n += span - cur;
      }
      if (n > FW_PLEN || R >= FW_UMAXR) { ok = false; break; }
      content[R * cstride] = keep_bytes64(v, n) | ((u64)n << 56);
      R++;
      ml = umax32(ml, n);
      mnl = umin32(mnl, n);
      if (n > span) spos += n - span; else sneg += span - n;
      maxd = (int)n - (int)span > maxd ? (int)n - (int)span : maxd;
      bool more = false;  // next value combination, the first chosen match fastest
      for (u32 m = mask; m && !more; m &= m - 1u) {
        const u32 j = (u32)__builtin_ctz(m), dj = ((odo >> (4 * j)) & 15u) + 1u;
        odo &= ~(15u << (4 * j));
        if (dj < ((u32)(NV >> (8 * j)) & 255u) && dj < 16u) { odo |= dj << (4 * j); more = true; }
      }
      if (!more) break;
    }
  }
  U.R = R; U.ml = ml; U.mnl = mnl; U.spos = spos; U.sneg = sneg; U.maxd = maxd; U.ok = ok;
}

// next_unit's grouping of the matches, position by position: at(q) takes the matches that start
// at q, in key order (the bucket's); a match inside the open unit's span joins it and grows it,
// any other closes it and opens the next.  finish() closes the last.
template <class W>
struct CplxDetect {
  const W& wd;
  const Tab& T;
  CplxLog& lg;
  u32 L;
  u32 us, ue, unm, k0;
  u64 um0, um1;
  A5X_HD CplxDetect(const W& w, u32 l, const Tab& t, CplxLog& g) : wd(w), T(t), lg(g), L(l) {
    us = 0; ue = 0; unm = 0; k0 = 0; um0 = 0; um1 = 0;
    if (L > CL_LMAX) lg.why |= CL_WHY_SLOT;
    if (T.hdr->nchoices > 65536u) lg.why |= CL_WHY_KEY;  // (cluster_enum's 16-bit choice indices)
  }
  A5X_HD void close() {
    if (!unm) return;
    const bool isc = unm > 1;
    if (lg.n >= CL_ULOG) lg.why |= CL_WHY_UNITS;
    if (us >= 64u) lg.why |= CL_WHY_POS;
    if (isc && lg.nc >= CL_NCL) lg.why |= CL_WHY_NCL;
    if (isc && unm > FW_UMAXM) lg.why |= CL_WHY_CLUSTER;
    if (lg.n < CL_ULOG) {
      lg.put(lg.n, ((us & 63u) << 10) | ((isc ? ue - us : k0) & 1023u));
      if (isc) {
        lg.cmask |= 1u << lg.n;
#pragma unroll
        for (u32 j = 0; j < CL_NCL; j++)
          if (j == lg.nc) { lg.m0[j] = um0; lg.m1[j] = um1; lg.st[j] = umin32(unm, 15u); }
        lg.nc++;
      }
      lg.n++;
    }
    unm = 0;
  }
  A5X_HD void match(u32 q, u32 kk, u32 kl) {
    if (kk >= 1024u) lg.why |= CL_WHY_KEY;
    if (unm && q < ue) {
      if (unm < FW_UMAXM && q - us < 64u) {
        const u64 f = (u64)(((q - us) << 10) | (kk & 1023u)) << (16u * (unm & 3u));
        if (unm < 4) um0 |= f; else um1 |= f;
      } else
        lg.why |= CL_WHY_CLUSTER;
      unm++;
      ue = umax32(ue, q + kl);
    } else {
      close();
      us = q; ue = q + kl; unm = 1; k0 = kk;
      um0 = kk & 1023u; um1 = 0;
    }
  }
  A5X_HD void at(u32 q) {
    const u32 w4 = (u32)wd.ld(q, umin32(4u, L - q));
    const u32 bk = T.bucket2[w4 & 255u];
    for (u32 kk = bk & 0xFFFFu; kk < (bk >> 16); kk++) {
      const u64 km = T.kmatch[kk];
      const u32 kl = (u32)(km >> 32) & 0xFFFFu;
      if (q + kl > L) continue;
      if (kl > 4) { lg.why |= CL_WHY_LONGKEY; continue; }
      const u32 m = kl >= 4 ? 0xFFFFFFFFu : ((1u << (8 * kl)) - 1u);
      if ((w4 & m) == (u32)km) match(q, kk, kl);
    }
  }
  A5X_HD void finish() { close(); }
};

// PieceBuilder for the units of a CplxLog: groups of <= FW_UMAXR entries (Planner's CAP of
// k_keyspace_cplx), so <= 4 members of R >= 2 with 4-bit R - 1 fields, and a member's choice d
// is T.cval[cb + d] (lone match) or the cluster's enumerated choice d (the same format:
// bytes | len << 56).  The cluster last enumerated stays in the sink's cbuf (res = its
// ordinal, ~0u: none); build_group enumerates a cluster that is not there again.  A group
// of two clusters (R1 R2 <= FW_UMAXR: each has <= 8 choices) keeps its first in rows 8..15
// of the sink's group buffer, whose rows 0..7 are the group descriptors:
//   off | first unit << 7 (5 bits) | members << 12 (3) | tail << 15 | first entry << 16 (10) |
//   (R - 1) of members 0..3 << 26 (4 bits each) | piece << 42
// Only FAST words are built (<= FW_PMAX pieces, <= 255 entries).
template <class W, class S>
struct CplxBuilder {
  const W& wd;
  const Tab& T;
  S& sk;
  const CplxLog& ul;
  Plan P;             // lconst, minl stay 0
  u32 bR, bl, bspan;  // the big piece being filled
  u32 cR, cmax, prev; // cR = 0: no open group
  u32 nu;             // units taken
  u32 res;            // the cluster in the sink's cbuf
  u64 gd;             // the open group's descriptor

  A5X_HD CplxBuilder(const W& w, const Tab& t, S& s, const CplxLog& lg, u32 resident)
      : wd(w), T(t), sk(s), ul(lg) {
    P.np = 0; P.ng = 0; P.ne = 0; P.lconst = 0; P.maxl = 0; P.minl = 0; P.ok = true;
    P.nbig = 0; P.bstarts = 0; P.bent = 0; P.bRp = 0;
    bR = 1; bl = 0; bspan = 0; cR = 0; cmax = 0; prev = 0; nu = 0; gd = 0; res = resident;
  }
  // Planner::big_join (FB_RMAX) for a small piece pi that exists when c (PieceBuilder::big)
  A5X_HD void big(u32 R, u32 maxlen, u32 pi, bool c) {
    const bool join = P.nbig && bl + maxlen <= FB_PLEN && bR * R <= FB_RMAX && bspan < FB_SPAN;
    const bool fresh = c && !join;
    const u32 nR = join ? bR * R : R;
    P.bstarts |= fresh && P.nbig >= 1 && P.nbig <= 3 ? (pi & 7u) << ((3u * (P.nbig - 1u)) & 31u) : 0u;
    P.nbig += fresh ? 1u : 0u;
    P.bent += c ? (join ? nR - bR : R) : 0u;
    bR = c ? nR : bR; bl = c ? (join ? bl + maxlen : maxlen) : bl; bspan = c ? (join ? bspan + 1u : 1u) : bspan;
    const u32 sh = (6u * (P.nbig - 1u)) & 31u;
    P.bRp = c && P.nbig >= 1 && P.nbig <= FB_NMAX ? (P.bRp & ~(63u << sh)) | (((bR - 1u) & 63u) << sh) : P.bRp;
  }
  A5X_HD void literal(u32 off, u32 n, bool nl_last) {  // Planner::literal
    const u32 nb = nl_last ? n - 1 : n;
    u64 v = nb ? wd.ld(off, nb) : 0ull;
    if (nl_last) v |= 10ull << (8 * nb);
    sk.ent(P.ne, v | fw_meta(n, 1));
    sk.desc(P.np, fr_desc(1, P.ne));
    big(1, n, P.np, true);
    P.ne++; P.np++; P.maxl += n;
  }
  A5X_HD void close_group(bool c, bool tail) {
    if (c) sk.gst(0, P.ng & 7u, gd | ((u64)tail << 15));
    big(cR, cmax, (u32)(gd >> 42) & 127u, c);
    P.ne += c ? cR : 0u; P.ng += c ? 1u : 0u; P.maxl += c ? cmax : 0u;
    cR = c ? 0u : cR;
  }
  A5X_HD void unit(const Unit& U) {
    if (!P.ok) return;
    const u32 Ru = U.R, ml = U.ml, run = U.s - prev;
    if (!U.ok || ml > FW_PLEN || Ru > FW_UMAXR || Ru < 2) { P.ok = false; return; }
    const bool open = cR != 0, merge = open && cmax + run + ml <= FW_PLEN && cR * Ru <= FW_UMAXR;
    close_group(open && !merge, false);
    u32 off = prev, rem = run;
    while (!merge && rem + ml > FW_PLEN) {  // literal run that does not fit with the unit
      const u32 n = umin32(FW_PLEN, rem);
      literal(off, n, false);
      off += n; rem -= n;
    }
    const u32 nm = (u32)(gd >> 12) & 7u;  // members of the open group
    const u64 fresh = (u64)(off & 127u) | ((u64)(nu & 31u) << 7) | (1ull << 12) | ((u64)(P.ne & 1023u) << 16) |
                      ((u64)(Ru - 1u) << 26) | ((u64)(P.np & 127u) << 42);
    gd = merge ? (gd + (1ull << 12)) | ((u64)(Ru - 1u) << (26u + 4u * nm)) : fresh;
    cR = merge ? cR * Ru : Ru;
    cmax = merge ? cmax + run + ml : rem + ml;
    P.np += merge ? 0u : 1u;
    prev = U.e;
    nu++;
  }
  A5X_HD void finish(u32 L) {  // tail bytes + '\n'
    if (!P.ok) return;
    const u32 tl = L - prev + 1;
    const bool open = cR != 0, tm = open && cmax + tl <= FW_PLEN;
    cmax += tm ? tl : 0u;
    close_group(open, tm);
    u32 off = prev, rem = tm ? 0u : tl;
    while (rem) {
      const u32 n = umin32(FW_PLEN, rem);
      literal(off, n, n == rem);
      off += n; rem -= n;
    }
  }
  // Entries and piece descriptor of group g (< P.ng, < 8): entry a = the lead run, then for each
  // member its choice d_j and the bytes after it (PieceBuilder::build_group, <= 4 members).
  A5X_HD void build_group(u32 g, u32 L) {
    const u64 d = sk.gld(0, g & 7u);
    const u32 off = (u32)d & 127u, i0 = (u32)(d >> 7) & 31u, nm = (u32)(d >> 12) & 7u;
    const u32 ebase = (u32)(d >> 16) & 1023u, pi = (u32)(d >> 42) & 127u;
    const bool tail = (d >> 15) & 1u;
    const u32 cs = sk.cstride();
    u64* const cmain = sk.cbuf();
    u64* const calt = sk.g + 8u * cs;
    u32 R[4], pl[4];
    u64 pv[4];
    const u64* cp[4];
    u32 cst[4];
    u32 at = off, ll = 0, ncl = 0;
    u64 lv = 0;
    const u64 src = wd.ld(off, umin32(FW_PLEN, L - off));
    for (u32 j = 0; j < nm && j < 4; j++) ncl += ul.is_cluster(i0 + j) ? 1u : 0u;
    // the group's clusters into their buffers (a loop of its own, not unrolled: one enumeration
    // in the code); alt = the first cluster of a group of two
    u32 seen = 0;
    for (u32 j = 0; j < nm && j < 4; j++) {
      const u32 i = i0 + j;
      if (!ul.is_cluster(i)) continue;
      const u32 ci = ul.cluster_of(i);
      const bool alt = ncl > 1 && seen == 0;
      if (alt || res != ci) {
        Unit V;
        ul.get(T, i, V);
        cluster_enum(wd, V, T, alt ? calt : cmain, cs);
        if (!alt) res = ci;
      }
      seen++;
    }
    seen = 0;
#pragma unroll
    for (u32 j = 0; j < 4; j++) {
      R[j] = ((u32)(d >> (26u + 4u * j)) & 15u) + 1u;
      pl[j] = 0; pv[j] = 0; cp[j] = T.cval; cst[j] = 1;
      if (j < nm) {
        const u32 i = i0 + j, e = ul(i), q = e >> 10;
        u32 end;
        if (ul.is_cluster(i)) {
          cp[j] = ncl > 1 && seen == 0 ? calt : cmain; cst[j] = cs;
          end = q + (e & 1023u);
          seen++;
        } else {
          const A5xKey& key = T.keys[e & 1023u];
          cp[j] = T.cval + key.choice_base;
          end = q + key.klen;
        }
        const u32 n = q - at;  // the run before the member
        const u64 v = keep_bytes64(src >> (8 * (at - off)), n);
        if (j == 0) { lv = v; ll = n; }
#pragma unroll
        for (u32 t = 1; t < 4; t++)
          if (j == t) { pv[t - 1] = v; pl[t - 1] = n; }
        at = end;
      }
    }
    if (tail) {
      const u32 n = L - at;
      const u64 v = keep_bytes64(src >> (8 * (at - off)), n) | (10ull << (8 * n));
#pragma unroll
      for (u32 j = 0; j < 4; j++)
        if (j + 1 == nm) { pv[j] = v; pl[j] = n + 1u; }
    }
    const u32 cRg = R[0] * R[1] * R[2] * R[3];
    u32 dg[4] = {0, 0, 0, 0};
    for (u32 a = 0; a < cRg; a++) {
      u64 v = lv;
      u32 n = ll;
#pragma unroll
      for (u32 j = 0; j < 4; j++) {
        if (j < nm) {
          const u64 c = cp[j][dg[j] * cst[j]];
          v |= (c & FW_M56) << (8 * n);
          n += (u32)(c >> 56);
          v |= pv[j] << (8 * (n & 7u));
          n += pl[j];
        }
      }
      sk.ent(ebase + a, (v & FW_M56) | fw_meta(n, cRg));
      bool carry = true;  // the digits of a + 1, member 0 least significant
#pragma unroll
      for (u32 j = 0; j < 4; j++) {
        dg[j] += carry ? 1u : 0u;
        carry = dg[j] == R[j];
        dg[j] = carry ? 0u : dg[j];
      }
    }
    sk.desc(pi, fr_desc(cRg, ebase));
  }
};

// One complex word by the lean path: detection, the count pass by unit index (every cluster
// enumerated once, the last one left in the sink's cbuf), the class (classify_word's), and for
// a FAST word with candidates and a record slot (fits) its record through sk (sk.np is set
// here).  Returns why: nonzero = the word is not the lean path's, nothing of C / f is valid and
// nothing was written.  f = the flags as ks_word_once maps them; built: a record was written
// (rec0 = its header); bad: the build disagrees with the count pass.
template <class W, class S>
A5X_HD u32 cplx_word_lean(const W& wd, u32 L, const Tab& T, int mn, int mx, u32 ringmax, bool fits, S& sk,
                          WordClass& C, u32& f, bool& built, u64& rec0, bool& bad, CplxLog* keep = nullptr) {
  built = false; bad = false; rec0 = 0; f = 0;
  CplxLog lg;
  if (mx < 1 || L == 0) {  // processWord emits nothing (classify_word)
    C.count = 0; C.bytes = 0; C.ovf = false; C.clusters = false;
    C.flags = A5X_WF_RADIX | A5X_WF_FAST;
    f = C.flags;
    return L > CL_LMAX ? (u32)CL_WHY_SLOT : 0u;
  }
  CplxDetect<W> det(wd, L, T, lg);
  for (u32 q = 0; q < L; q++) det.at(q);  // (a word past CL_LMAX: the host check's, for its other reasons)
  det.finish();
  if (lg.why) return lg.why;
  CountAcc A;
  count_init(A, L);
  CountPlanner<FW_UMAXR> cp;
  u32 res = ~0u;
  for (u32 u = 0; u < lg.n; u++) {
    Unit U;
    lg.get(T, u, U);
    if (U.k) {
#if CL_ABL & 1
      U.R = 5; U.ml = 2; U.mnl = 1; U.spos = 0; U.sneg = 0; U.maxd = 0;
#else
      cluster_enum(wd, U, T, sk.cbuf(), sk.cstride());
#endif
      res = lg.cluster_of(u);
      lg.set_stats(res, U);
      if (!U.ok) { lg.why |= CL_WHY_CLUSTER; break; }
    }
    count_unit(A, U);
    cp.unit(U);
  }
  if (lg.why) return lg.why;
  cp.finish(L);
  C = classify_finish(A, cp.P, L, mn, mx, ringmax);
  f = C.flags;
  if ((f & A5X_WF_DEFER) || !(f & (A5X_WF_FAST | A5X_WF_RADIX | A5X_WF_ERR_OVF))) f = A5X_WF_DEFER;
  if (!((f & A5X_WF_FAST) && C.count > 0 && fits)) return 0;
  sk.np = ff_np(f);
  CplxBuilder<W, S> pb(wd, T, sk, lg, res);
  for (u32 u = 0; u < lg.n; u++) {
    Unit U;
    lg.get(T, u, U);
    pb.unit(U);
  }
  pb.finish(L);
  const Plan& P = pb.P;
  bad = !P.ok || P.ng != ff_ng(f) || P.ne != ff_ne(f) || P.np != ff_np(f) || P.ng > 8u;
  if (!bad)
    for (u32 g = 0; g < P.ng; g++) pb.build_group(g, L);
  rec0 = fr_hdr(P.np, P.ng, P.ne, P.maxl, P.nbig, P.bstarts, P.bRp);
  built = true;
  if (keep) *keep = lg;  // (the host check's coverage counters)
  return 0;
}

// Host check of the lean path against the generic one (ks_word_once's steps) on one word of
// <= 127 bytes (a5x_debug_cplx_build, tools/cplx_build_selftest.cpp).  out[0] = 1 when the two
// agree (flags, count, bytes, the record and its big entries) or the word falls back, out[1] =
// why (0: the lean path takes the word), out[2] = flags, out[3] = a record was built, out[4..5] =
// count, out[6..7] = bytes, and of a built record out[8] = units, out[9] = clusters | a group
// holds two of them << 8, out[10] = groups, out[11] = most members in a group.
inline void cplx_build_compare(const uint8_t* wd, u32 L, const Tab& T, int mn, int mx, uint32_t* out) {
  constexpr u32 NREC = 2048;
  for (int j = 0; j < 12; j++) out[j] = 0;
  GWord gw;
  gw.p = wd;
  // the generic path
  u64 ra[NREC], rb[NREC];
  for (u32 i = 0; i < NREC; i++) ra[i] = rb[i] = 0;
  ArraySink sa, sb;
  sa.rec = ra; sa.np = 0; sb.rec = rb; sb.np = 0;
  for (u32 i = 0; i < FW_UMAXR; i++) sa.g[i] = sa.c[i] = sb.g[i] = sb.c[i] = 0;
  WordClass CA;
  CA.count = 0; CA.bytes = 0; CA.flags = 0; CA.ovf = false; CA.clusters = false;
  u32 fa;
  bool builta = false;
  u32 benta = 0;
  if (L > A5X_LMAX_A && mx >= 1) {
    fa = A5X_WF_DEFER;
  } else {
    UnitCache uc;
    CA = classify_word(gw, L, T, mn, mx, A5X_RING_A - 16, &uc, sa.c, 1);
    fa = CA.flags;
    if ((fa & A5X_WF_DEFER) || !(fa & (A5X_WF_FAST | A5X_WF_RADIX | A5X_WF_ERR_OVF))) fa = A5X_WF_DEFER;
    if ((fa & A5X_WF_FAST) && CA.count > 0) {
      sa.np = ff_np(fa);
      const Plan P = uc.full ? plan_word<true>(gw, L, T, sa, fb_balanced_cap(CA.count + 1))
                             : plan_word_cached(gw, L, T, sa, uc, fb_balanced_cap(CA.count + 1));
      ra[0] = fr_hdr(P.np, P.ng, P.ne, P.maxl, P.nbig, P.bstarts, P.bRp);
      benta = P.bent;
      builta = true;
    }
  }
  // the lean path (a second group buffer: rows 8..15 take a cluster)
  WordClass CB;
  CB.count = 0; CB.bytes = 0; CB.flags = 0; CB.ovf = false; CB.clusters = false;
  u32 fb = 0;
  bool builtb = false, bad = false;
  u64 rec0 = 0;
  CplxLog lg;
  const u32 why = cplx_word_lean(gw, L, T, mn, mx, A5X_RING_A - 16, true, sb, CB, fb, builtb, rec0, bad, &lg);
  out[1] = why;
  if (why) {
    out[0] = 1; out[2] = fa; out[3] = builta ? 1u : 0u;
    out[4] = (u32)CA.count; out[5] = (u32)(CA.count >> 32); out[6] = (u32)CA.bytes; out[7] = (u32)(CA.bytes >> 32);
    return;
  }
  rb[0] = rec0;
  const bool defer = (fb & A5X_WF_DEFER) != 0;  // (the kernel stores count = bytes = 0 for a deferred word)
  bool eq = fa == fb && builta == builtb && !bad && (defer || (CA.count == CB.count && CA.bytes == CB.bytes)) &&
            CA.ovf == CB.ovf;
  if (!defer && (fb & A5X_WF_FAST) && CB.count > 0) eq = eq && CA.clusters == CB.clusters;
  for (u32 i = 0; i < NREC; i++) eq = eq && ra[i] == rb[i];
  out[0] = eq ? 1u : 0u;
  out[2] = fb; out[3] = builtb ? 1u : 0u;
  out[4] = (u32)CB.count; out[5] = (u32)(CB.count >> 32); out[6] = (u32)CB.bytes; out[7] = (u32)(CB.bytes >> 32);
  (void)benta;
  if (builtb) {
    out[8] = lg.n; out[9] = lg.nc; out[10] = frh_ng(rb[0]);
    for (u32 g = 0; g < frh_ng(rb[0]) && g < 8u; g++) {
      const u32 i0 = (u32)(sb.g[g] >> 7) & 31u, nm = (u32)(sb.g[g] >> 12) & 7u;
      out[11] = umax32(out[11], nm);
      u32 ncl = 0;
      for (u32 j = 0; j < nm; j++) ncl += lg.is_cluster(i0 + j) ? 1u : 0u;
      if (ncl > 1) out[9] |= 256u;
    }
  }
}

// ---------------------------------------------------------------------------
// k_expand_fast, per candidate (host replay in a5x_debug_plan_word)
// ---------------------------------------------------------------------------
// pass 1 over the window records wrec: word with its np piece descriptors at
// wrec[ga, ga + np) and entries from wrec[wbe]; n = rank in the word + 1.  Each
// piece takes its digit of n and selects its entry e[i].  NPM >= np fixed
// iterations (so the descriptor and entry loads are issued back to back): pieces
// past np select the empty entry wrec[FX_ZSLOT].  Returns the candidate's length
// including '\n'.
template <int NPM>
A5X_HD u32 fw_pass1(const u64* wrec, u32 ga, u32 np, u32 wbe, u32 n, u64* e) {
  u64 G[NPM];
#pragma unroll
  for (int i = 0; i < NPM; i++) G[i] = wrec[ga + i];  // past np: whatever follows (unused)
  u32 idx[NPM];
#pragma unroll
  for (int i = 0; i < NPM; i++) {
    const u32 ghi = (u32)(G[i] >> 32);
    u32 q = (u32)(((u64)n * (u32)G[i]) >> 32);
    q += n & (u32)((int)ghi >> 31);  // R = 1: q = n
    const u32 d = n - q * (((ghi >> 8) & 31u) + 1u);
    n = q;
    idx[i] = (u32)i < np ? wbe + (ghi & 255u) + d : (u32)FX_ZSLOT;
  }
  u32 len = 0;
#pragma unroll
  for (int i = 0; i < NPM; i++) {
    e[i] = wrec[idx[i]];
    len += (u32)(e[i] >> 56) & 7u;
  }
  return len;
}

// pass 2: the candidate's pieces e[0, NPM) appended to the output as whole,
// aligned dwords of a ring, with plain stores and no atomics.  Byte o (ring
// offset) is the candidate's first; acc holds the o & 3 bytes before it: the
// previous candidate's tail for a round's first lane (the carry), zeros otherwise.
// Dword ownership: the dword holding byte o belongs to the PREVIOUS candidate
// unless acc is the carry (has_prev = false): it is returned in *head (zeros below
// o) for the previous lane to merge into its last partial dword, which it writes.
// Requires every candidate to complete that dword (len >= 3, FAST minl).  Stores
// that are not due go to ring[trash] (a per-lane scratch dword): no branches.
// Returns the ring dword of the unfinished last dword; *acc_io / *n_io = its
// bytes / count.
template <int NPM>
A5X_HD u32 fw_pass2(const u64* e, u32 o, u32* ring, u32 trash, bool has_prev, u32* acc_io, u32* n_io, u32* head) {
  u32 acc = *acc_io, n = o & 3u, D = o >> 2;
  bool hp = has_prev && n != 0;
  u32 hd = 0;
#pragma unroll
  for (int i = 0; i < NPM; i++) {
    const u32 ehi = (u32)(e[i] >> 32);
    const u32 t = n + ((ehi >> 24) & 7u);
    const u32 chi = ehi & 0xFFFFFFu;
    const u64 lo = ((((u64)chi << 32) | (u32)e[i]) << (8u * n)) | acc;
    // bytes 8, 9 (only needed when t >= 8, i.e. n >= 1): chi >> (32 - 8n)
#ifdef __HIP_DEVICE_COMPILE__
    const u32 hi = __builtin_amdgcn_alignbyte(0u, chi, 0u - n);
#else
    const u32 hi = (u32)((((u64)chi << 32) >> (32u - 8u * (n & 3u))) >> 32);
#endif
    const bool c4 = t >= 4u, c8 = t >= 8u;
    ring[(c4 && !hp) ? D : trash] = (u32)lo;
    ring[c8 ? D + 1u : trash] = (u32)(lo >> 32);
    hd = (c4 && hp) ? (u32)lo : hd;
    hp = hp && !c4;
    acc = c8 ? hi : (c4 ? (u32)(lo >> 32) : (u32)lo);
    D += t >> 2;
    n = t & 3u;
  }
  *acc_io = acc;
  *n_io = n;
  *head = hd;
  return D;
}

// ---------------------------------------------------------------------------
// Big pieces (k_expand_fast): the small pieces [bstart(b), bstart(b+1)) of a
// word combined into one <= FB_PLEN-byte piece with R_b = product of their R
// combinations (R_b <= FB_RMAX), stored as 16-B entries: bytes 0-14 content (zero
// past the length), byte 15 = length.  Combination c of big piece b is the
// mixed-radix digit vector of its small pieces (first small piece least
// significant), so the big pieces are digits of n in the same order.
// ---------------------------------------------------------------------------
A5X_HD u32 fb_perm(u32 hi, u32 lo, u32 sel) {  // v_perm_b32 for selectors with bytes < 8
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const u64 v = ((u64)hi << 32) | lo;
  u32 r = 0;
  for (u32 i = 0; i < 4; i++) r |= (u32)((v >> (8 * ((sel >> (8 * i)) & 7u))) & 255u) << (8 * i);
  return r;
#endif
}

// R of big piece b of the word whose record is at wrec[wrb] (header h)
A5X_HD u32 fb_R(const u64* wrec, u32 wrb, u64 h, u32 b) {
  const u32 nb = frh_nbig(h), np = frh_np(h);
  if (b >= nb) return 1;
  const u32 s0 = frh_bstart(h, b), s1 = b + 1 < nb ? frh_bstart(h, b + 1) : np;
  u32 R = 1;
  for (u32 i = s0; i < s1 && i < FW_PMAX; i++) R *= frd_R(wrec[wrb + 1 + i]);
  return R;
}

// entry c of big piece b (x, y, z, w = bytes 0-3, 4-7, 8-11, 12-14 + length)
A5X_HD void fb_entry(const u64* wrec, u32 wrb, u32 b, u32 c, u32 out[4], u32 zslot = FX_ZSLOT) {
  const u64 h = wrec[wrb];
  const u32 nb = frh_nbig(h), np = frh_np(h);
  const u32 sp0 = frh_bstart(h, b), sp1 = b + 1 < nb ? frh_bstart(h, b + 1) : np;
  const u32 wbe = wrb + 1 + np;
  u64 lo64 = 0, hi64 = 0;
  u32 off = 0;
#pragma unroll
  for (u32 i = 0; i < FB_SPAN; i++) {
    const bool valid = sp0 + i < sp1;
    const u64 G = wrec[valid ? wrb + 1 + sp0 + i : zslot];
    const u32 ghi = (u32)(G >> 32);
    u32 q = (u32)(((u64)c * (u32)G) >> 32);
    q += c & (u32)((int)ghi >> 31);  // R = 1: q = c
    const u32 d = c - q * (((ghi >> 8) & 31u) + 1u);
    c = q;
    const u64 ev = wrec[valid ? wbe + (ghi & 255u) + d : zslot];
    const u64 cv = ev & FW_M56;
    if (off < 8) {
      lo64 |= cv << (8 * off);
      if (off) hi64 |= cv >> (64 - 8 * off);
    } else {
      hi64 |= cv << (8 * (off - 8));
    }
    off += fw_len(ev);
  }
  out[0] = (u32)lo64; out[1] = (u32)(lo64 >> 32); out[2] = (u32)hi64;
  out[3] = ((u32)(hi64 >> 32) & 0xFFFFFFu) | (off << 24);
}

// One big piece appended to a candidate's output as whole, aligned dwords of a
// ring: entry e (e[3] byte 3 = length) after the n pending bytes held in the TOP n
// bytes of pv; complete dwords go to ring[D ..].  Dword ownership: the dword
// holding a candidate's first byte belongs to the PREVIOUS candidate unless the
// pending bytes are the carry; while hp is set, the first complete dword is kept in
// hd (zeros below the candidate's first byte) for the previous lane to merge into
// its last partial dword.  Stores that are not due go to ring[T + k] (the lane's 4
// trash dwords): no branches.  acc = the unfinished dword (bottom-aligned n bytes).
A5X_HD void fb_put(const u32 e[4], u32& pv, u32& n, u32& D, bool& hp, u32& hd, u32& acc, u32* ring, u32 T) {
  const u32 sel = (u32)(0x0706050403020100ull >> (32u - 8u * n));  // bytes 4-n .. 7-n of {s_k, s_k-1}
  const u32 s3 = e[3] & 0xFFFFFFu;
  const u32 w0 = fb_perm(e[0], pv, sel);
  const u32 w1 = fb_perm(e[1], e[0], sel);
  const u32 w2 = fb_perm(e[2], e[1], sel);
  const u32 w3 = fb_perm(s3, e[2], sel);
  const u32 w4 = fb_perm(0u, s3, sel);
  const u32 t = n + (e[3] >> 24);
  const bool m1 = t >= 4u, m2 = t >= 8u, m3 = t >= 12u, m4 = t >= 16u;
  ring[(m1 && !hp) ? D : T] = w0;
  ring[(m2 ? D : T) + 1u] = w1;
  ring[(m3 ? D : T) + 2u] = w2;
  ring[(m4 ? D : T) + 3u] = w3;
  hd = (m1 && hp) ? w0 : hd;
  hp = hp && !m1;
  u32 x = m1 ? w1 : w0;
  x = m2 ? w2 : x;
  x = m3 ? w3 : x;
  x = m4 ? w4 : x;
  acc = x;
  n = t & 3u;
  pv = acc << ((32u - 8u * n) & 31u);
  D += t >> 2;
}
