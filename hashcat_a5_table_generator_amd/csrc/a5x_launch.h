// a5x_launch.h -- host-side launch interface of a5x_kernels.hip (internal to liba5x).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "a5x.h"

struct A5xKsLaunch {
  const uint8_t* table;
  uint32_t table_bytes;
  const uint8_t* words;
  const uint64_t* woff;
  uint64_t nw;
  int mn, mx;
  uint64_t* count;
  uint64_t* bytes;
  uint32_t* flags;
  uint32_t* defer_list;
  uint32_t* defer_n;
  uint32_t* nbig;
  uint32_t* nslow;
  uint32_t* big_list;   // nw entries each
  uint32_t* slow_list;
  uint32_t* err;
  uint32_t defer_blocks;
  uint64_t* rec;   // FAST plan records (tile regions of FW_TILE_REC u64, then complex slots)
  uint32_t* roff;  // per-word record offsets
  uint32_t* cplx_list;  // words for the general (per-lane walk) keyspace pass
  uint32_t* cplx_n;
  uint32_t cplx_cap;    // record slots of FW_RMAX u64 from rec + cplx_base
  uint64_t cplx_base;
  uint32_t* glob_list;  // words beyond the pass-B LDS budget (k_keyspace_wave appends)
  uint32_t* glob_n;
  uint8_t* gscr;        // pass G scratch: gslots x a5x_gslot_bytes() (ring zeroed)
  uint32_t gslots;
  int rmode;            // 1 / 2 / 3: -r / -s / -s -r FAST probe (k_keyspace_thread, mode_unit, then
                        // k_keyspace_rprobe over the words a tile could not decide: cplx_list,
                        // records in cplx slots); the other words are listed in defer_list / defer_n
  uint32_t rcmin;       // -r: max(min, 0)
  uint64_t* rnseg;      // -r: per FAST word, ceil(count / rseg) mode-engine items
  uint64_t rseg;
  // -s / -s -r virtual words (k_keyspace_vsub over defer_list): the words it leaves to the
  // mode engine, per word sub-words - 1 and record u64, the sub-word records (bump area)
  uint32_t* vout_list;
  uint32_t* vout_n;
  uint64_t* vn;
  uint64_t* vrsz;
  uint64_t* vrec;
  uint64_t* vrec_n;
  uint64_t vrec_cap;
  uint16_t* vocc;  // per word 16 u16: k_keyspace_thread's occurrence rows for k_keyspace_vsub (null: none)
  uint32_t* vlong_list;  // k_keyspace_vsub: words the small-slot pass hands to the large one (null: large only)
  uint32_t* vlong_n;
  uint32_t* hiflag;      // zeroed u32: k_keyspace_thread walks UTF-8 words by lead bytes (null: by bytes)
  uint32_t small_stage;  // k_keyspace_thread<false>'s small word stage (a5x_keyspace_small_stage; 0: the large one only)
  uint32_t* tspan;       // zeroed u32: the batch's largest tile span, which picks the stage (null: the large one only)
  uint32_t* stage_used;  // u32: the stage of the k_keyspace_thread launch that did the work (null: not reported)
  uint32_t* nrefit;      // zeroed u32: k_keyspace_thread counts the words it walked with the fused psk_walk (null: no count)
  uint32_t* ncplx_lean;  // two zeroed u32: k_keyspace_cplx counts the words of its lean and of its generic path (null: no count)
};

// the virtual word list of a batch with virtual words (k_vwords_fill)
struct A5xVwLaunch {
  const uint32_t* flags;
  const uint64_t* cand_off;
  const uint64_t* byte_off;  // null: no layout (fused digest)
  const uint32_t* roff;
  const uint64_t* rec;
  const uint64_t* vrec;
  const uint64_t* vpre;
  const uint64_t* vrpre;
  uint64_t nw;
  uint64_t* vcand_off;
  uint64_t* vbyte_off;
  uint32_t* vflags;
  uint32_t* vroff;
  uint32_t* vmap;
  uint32_t* vobase;
  uint64_t* vrec2;
  // fixed-width virtual words (A5X_WF_VFIX): their sub-words' records are written here from the
  // descriptors k_keyspace_vsub left
  const uint8_t* table;
  uint32_t table_bytes;
  int rmode;
  uint32_t rcmin;
  const uint8_t* words;
  const uint64_t* woff;
};
size_t a5x_keyspace_vsub_lds(uint32_t table_bytes);
hipError_t a5x_launch_vsub(const A5xKsLaunch& L, hipStream_t st);
hipError_t a5x_launch_vwords_sizes(const uint32_t* flags, const uint64_t* cand_off, uint64_t nw, uint64_t* vn,
                                   uint64_t* vrsz, hipStream_t st);
hipError_t a5x_launch_vwords_fill(const A5xVwLaunch& L, hipStream_t st);

struct A5xHitRaw;
struct A5xExpLaunch {
  const uint8_t* table;
  uint32_t table_bytes;
  const uint8_t* words;
  const uint64_t* woff;
  uint64_t nw;
  const uint64_t* cand_off;
  const uint64_t* byte_off;
  const uint32_t* flags;
  const uint32_t* chunk_w0;
  const uint64_t* segs;    // k_expand_slow / k_expand_b items (a5x_launch_segments)
  const uint32_t* nsegs;   // device count of segs
  uint64_t nsegs_bound;    // host bound on *nsegs
  uint64_t cand_begin, cand_end;
  uint64_t CH;
  uint64_t SEG;  // candidates per slow / BIG segment
  uint8_t* out;
  uint64_t out_base;
  uint64_t out_cap;
  int mn, mx;
  uint32_t* err;
  uint64_t* dbg;
  uint32_t waves_per_block;       // k_expand_slow
  uint32_t waves_per_block_fast;  // k_expand_fast (one wave per chunk; 1 measured fastest)
  const uint64_t* rec;
  const uint32_t* roff;
  uint64_t rec_n;   // u64 in rec
  // fused digest (kinds 3, 5): target set + hit buffer (see A5xDigLaunch)
  const uint32_t* dg_bitmap;
  uint32_t dg_bm_mask, dg_has_zero, dg_hit_cap;
  const uint4* dg_table;
  uint64_t dg_tmask;
  A5xHitRaw* dg_hits;
  uint32_t* dg_nhits;
  // pass G (words beyond the pass-B LDS budget): HBM scratch slots, one per wave
  uint8_t* gscr;
  uint32_t gslots;
  // the virtual word list (-s / -s -r batches with virtual words): entry -> word and its
  // first candidate in the word, for the fused digest's hit records (null: words)
  const uint32_t* vmap;
  const uint32_t* vobase;
};

hipError_t a5x_set_kernel_attrs();
// pass G: bytes per scratch slot (ring of A5X_RING_G bytes, then the word's WaveLds)
uint64_t a5x_gslot_bytes();
// k_keyspace_g over the words k_keyspace_wave listed (grid = gslots)
hipError_t a5x_launch_keyspace_g(const A5xKsLaunch& L, hipStream_t st);
int a5x_read_stamps(unsigned long long* out16, int reset);
hipError_t a5x_launch_keyspace(const A5xKsLaunch& L, hipStream_t st);
size_t a5x_keyspace_wave_lds(uint32_t table_bytes);
size_t a5x_keyspace_thread_lds(uint32_t table_bytes, uint32_t stage);
uint32_t a5x_keyspace_small_stage(uint32_t table_bytes);  // 0: not offered for this table
size_t a5x_keyspace_rprobe_lds(uint32_t table_bytes);
uint64_t a5x_scan_tmp_elems(uint64_t n);
hipError_t a5x_launch_scan(const uint64_t* ca, const uint64_t* cb, uint64_t n, uint64_t* outa, uint64_t* outb,
                           uint64_t* tmp, uint32_t* err, hipStream_t st);
hipError_t a5x_launch_plan(const uint64_t* cand_off, uint64_t nw, uint64_t CH, uint32_t* chunk_w0, hipStream_t st);
// (word, segment) items of the listed words' candidates in [cb, ce), CH per segment
hipError_t a5x_launch_segments(const uint32_t* list, const uint32_t* list_n, uint32_t n_bound,
                               const uint64_t* cand_off, uint64_t cb, uint64_t ce, uint64_t CH, uint64_t* segs,
                               uint32_t* nsegs, hipStream_t st);
size_t a5x_expand_lds(uint32_t table_bytes, int kind, uint32_t waves);
// kind 0: k_expand_fast, 1: k_expand_slow, 2: k_expand_b (pass B), 3: k_expand_fast_md5,
// 4: k_expand_g (pass G: the GLOB words of the BIG segment list), 5: k_expand_fast_ntlm
hipError_t a5x_launch_expand(const A5xExpLaunch& L, int kind, hipStream_t st);
hipError_t a5x_launch_locate(const A5xExpLaunch& L, const uint64_t* cands, uint32_t n, uint64_t* out_bytes,
                             hipStream_t st);
hipError_t a5x_launch_word_of(const uint64_t* cand_off, uint64_t nw, const uint64_t* g, uint32_t nt, uint64_t* word,
                              uint64_t* ciw, hipStream_t st);
hipError_t a5x_launch_digest(const uint8_t* out, const uint64_t* byte_off, uint64_t out_base, uint64_t nw,
                             uint64_t* dig, hipStream_t st);

// ---- -r / -s / -s -r engines (a5x_modes.hip) --------------------------------
struct A5xModeLaunch {
  const uint8_t* mtab;  // A5xMHdr blob (a5x_format.h)
  uint32_t mtab_bytes;
  const uint8_t* words;
  const uint64_t* woff;
  uint64_t nw;
  int mode, mn, mx;
  uint64_t SEG;          // candidates per item
  uint64_t* count;       // k_mode_count outputs: per-word count, items, flags
  uint64_t* nseg;
  uint32_t* flags;
  const uint64_t* cand_off;  // exclusive scans (n+1)
  const uint64_t* seg_off;
  const uint32_t* item_w;    // item -> word
  uint64_t nitems;
  uint64_t item_begin, item_end;
  uint64_t* seg_bytes;       // length pass output (per item)
  uint8_t* item_fl;          // per item: which layout expands it (set by the length pass)
  uint64_t* wbytes;          // per word: closed-form output bytes of single-item positional words (~0: none)
  const uint64_t* seg_boff;  // exclusive scan of seg_bytes (nitems+1)
  uint64_t cand_begin, cand_end;
  uint8_t* out;
  uint64_t out_base, out_cap;
  uint32_t* err;
  // mode pass G: words longer than A5X_M_LMAX (flag A5X_WF_GLOB), listed by k_mode_count,
  // run by one wave per HBM scratch slot (gslots x a5x_mode_gslot_bytes(); gscr null: none)
  uint32_t* glob_list;
  uint32_t* glob_n;
  uint8_t* gscr;
  uint32_t gslots;
  // -r FAST words (flags & A5X_WF_FAST, set by the k_keyspace_thread -r probe): counted
  // there, their items sized L + 1 per candidate and expanded by k_expand_fast
  int rfast;
  // -s / -s -r lane-per-word keyspace (k_mode_count_thread): the words it leaves to the
  // wave kernel k_mode_count (cl_list null: k_mode_count takes every word)
  uint32_t* cl_list;
  uint32_t* cl_n;
  const uint32_t* in_list;  // k_mode_count_thread's words (null: all; else the probe's list)
  const uint32_t* in_n;
  const uint64_t* rec;      // FAST plan records / offsets (k_mode_locate inside -s FAST words)
  const uint32_t* roff;
  // virtual words (flags & A5X_WF_VIRT; k_mode_locate): the virtual word list
  const uint64_t* vpre;
  const uint64_t* vcand_off;
  const uint64_t* vbyte_off;
  const uint32_t* vroff;
  const uint64_t* vrec;
  // fused digest (op 2): every candidate hashed where it is built and probed against the
  // target set; hits as (word, candidate in word) -- see A5xDigLaunch
  int dg_algo;
  const uint32_t* dg_bitmap;
  uint32_t dg_bm_mask, dg_has_zero, dg_hit_cap;
  const uint4* dg_table;
  uint64_t dg_tmask;
  struct A5xHitRaw* dg_hits;
  uint32_t* dg_nhits;
  uint32_t grid_cap;  // item kernels: workgroups at most (0: M_GRID_MAX); a few mode words among many
                      // FAST ones are filtered by a small grid beside k_expand_fast
};
size_t a5x_mode_lds(uint32_t mtab_bytes);
uint64_t a5x_mode_gslot_bytes();
hipError_t a5x_launch_mode_count(const A5xModeLaunch& L, hipStream_t st);
// -s / -s -r: radix positional words counted lane per word; the others listed for
// a5x_launch_mode_count (which then runs over L.cl_list)
hipError_t a5x_launch_mode_count_thread(const A5xModeLaunch& L, hipStream_t st);
hipError_t a5x_launch_mode_count_g(const A5xModeLaunch& L, hipStream_t st);
// op 0: per-item output bytes (seg_bytes); op 1: expand items [item_begin, item_end);
// op 2: fused digest of items [item_begin, item_end) (no length pass needed before it)
hipError_t a5x_launch_mode_items(const A5xModeLaunch& L, int op, hipStream_t st);
// out[3q..3q+2] = {item, index in item, byte offset} of global candidate cands[q]
hipError_t a5x_launch_mode_locate(const A5xModeLaunch& L, const uint64_t* cands, uint32_t n, uint64_t* out,
                                  hipStream_t st);
hipError_t a5x_launch_mode_wordbytes(const uint64_t* seg_off, const uint64_t* seg_boff, uint64_t nw,
                                     uint64_t* byte_off, uint64_t* bytes, hipStream_t st);

// ---- fused digest + lookup (a5x_digest.hip) ----------------------------------
struct A5xHitRaw {  // (block, ordinal) until k_hits_resolve, then (word, candidate in word)
  uint64_t blk;
  uint64_t idx;
  uint32_t d[4];
};
struct A5xDigLaunch {
  const uint8_t* out;  // "cand\n" stream, 16-B aligned, starts at a candidate
  uint64_t nbytes;
  int algo;            // A5X_ALGO_*
  const uint32_t* bitmap;
  uint32_t bm_mask;    // prefilter index mask: 2^k - 1 for a 2^k-bit bitmap (k <= 32)
  const uint4* table;  // open addressing, all-zero = empty; the first 16 digest bytes
  uint64_t tmask;
  uint32_t has_zero_target;
  A5xHitRaw* hits;
  uint32_t* nhits;
  uint32_t hit_cap;
  uint64_t* blk_cnt;        // op 1 output (per 2 KiB block line starts)
  const uint64_t* blk_pre;  // op 2 / resolve input (exclusive scan of blk_cnt)
  uint8_t* dig_out;         // op 2 output: a5x_digest_size(algo) bytes per candidate
  uint32_t* err;
  // wide algorithms (tail words: SHA-1 1, SHA-224 3, SHA-256 4, SHA-384 8, SHA-512 12): the
  // digest words past the first four of every table slot, the tails of the targets whose
  // first 16 bytes are zero (has_zero_target), and per hit the tail that matched, in hit
  // order at a stride of a5x_hit_tail_stride(algo) words: 4 for SHA-1 / SHA-256, 12 for
  // SHA-224 / SHA-384 / SHA-512 (words past the algorithm's tail are zero); the nested
  // algorithms go by their outer digest's width (a5x_algo_words)
  const uint32_t* tails;
  const uint32_t* ztails;
  uint32_t nztails;
  uint32_t* hit_tail;
};
// Kind and width of an algorithm value.  Every place that used to compare A5X_ALGO_* values
// numerically asks these instead: the nested values (16..22) sort after SHA-512 whatever
// their width.
// a digest of the hex text of another digest (a5x_nest.h), 16 to 32 bytes wide
constexpr bool a5x_algo_nested(int algo) { return algo >= A5X_ALGO_MD5_MD5 && algo <= A5X_ALGO_SHA256_MD5; }
// 32-bit words of the digest (0: not an algorithm)
constexpr uint32_t a5x_algo_words(int algo) {
  return algo == A5X_ALGO_MD5 || algo == A5X_ALGO_NTLM ? 4u
       : algo == A5X_ALGO_SHA1 ? 5u : algo == A5X_ALGO_SHA224 ? 7u : algo == A5X_ALGO_SHA256 ? 8u
       : algo == A5X_ALGO_SHA384 ? 12u : algo == A5X_ALGO_SHA512 ? 16u
       : algo == A5X_ALGO_MD5_MD5 || algo == A5X_ALGO_MD5_MD5_MD5 || algo == A5X_ALGO_MD5_MD5UP ||
         algo == A5X_ALGO_MD5_SHA1 ? 4u
       : algo == A5X_ALGO_SHA1_SHA1 || algo == A5X_ALGO_SHA1_MD5 ? 5u : algo == A5X_ALGO_SHA256_MD5 ? 8u
       : algo >= A5X_ALGO_MD5_MD5_SALT && algo <= A5X_ALGO_MD5_MD5SALT_MD5 ? 4u    // salted nested, MD5 outside
       : algo >= A5X_ALGO_SHA1_SHA1_SALT && algo <= A5X_ALGO_SHA1_MD5_SALT ? 5u       // SHA-1 outside
       : algo == A5X_ALGO_HMAC_MD5_KEY_PASS || algo == A5X_ALGO_HMAC_MD5_KEY_SALT ? 4u  // HMAC: the hash's width
       : algo == A5X_ALGO_HMAC_SHA1_KEY_PASS || algo == A5X_ALGO_HMAC_SHA1_KEY_SALT ? 5u
       : algo == A5X_ALGO_HMAC_SHA256_KEY_PASS || algo == A5X_ALGO_HMAC_SHA256_KEY_SALT ? 8u
       : algo == A5X_ALGO_HMAC_SHA512_KEY_PASS || algo == A5X_ALGO_HMAC_SHA512_KEY_SALT ? 16u
       : algo >= A5X_ALGO_PBKDF2_HMAC_MD5 && algo <= A5X_ALGO_PBKDF2_HMAC_SHA512 ? 4u : 0u;  // PBKDF2: the compared 16 bytes
}
// wider than the 16 bytes a table slot and a hit hold: tails compared and recorded
constexpr bool a5x_algo_wide(int algo) { return a5x_algo_words(algo) > 4u; }
// words of a hit's tail record, by digest width: 5 and 8 words (SHA-1, SHA-256 and the nested
// forms with such an outer digest) 4; 7, 12 and 16 words (SHA-224 / SHA-384 / SHA-512) 12;
// unused for a 4-word digest
constexpr uint32_t a5x_hit_tail_stride(int algo) {
  return a5x_algo_words(algo) == 7u || a5x_algo_words(algo) > 8u ? 12u : 4u;
}
size_t a5x_digest_lds(int algo);
uint64_t a5x_digest_blocks(uint64_t nbytes, int algo);  // 2 KiB (NTLM) / 4 KiB (MD5, SHA-*) blocks
hipError_t a5x_launch_digest_stream(const A5xDigLaunch& L, int op, uint32_t grid, hipStream_t st);
// hybrid fused digest: list the candidate-bearing non-FAST words (n: device counter),
// then gather them into a sub-batch (lens != null: their lengths; else the bytes at sub_off)
hipError_t a5x_launch_nonfast_list(const uint32_t* flags, const uint64_t* cand_off, uint64_t nw, uint64_t cb,
                                   uint64_t ce, uint32_t* list, uint32_t* n, hipStream_t st);
hipError_t a5x_launch_gather_words(const uint8_t* words, const uint64_t* woff, const uint32_t* idx, uint32_t m,
                                   uint64_t* lens, const uint64_t* sub_off, uint8_t* out, hipStream_t st);
hipError_t a5x_launch_hits_resolve(A5xHitRaw* hits, uint32_t n, const uint64_t* blk_pre, uint64_t cand_base,
                                   const uint64_t* cand_off, uint64_t nw, hipStream_t st);

// ---- rules in the digest + lookup stage (a5x_rules.hip) -----------------------
struct A5xRuleLaunch {
  A5xDigLaunch d;                // the stream, target set and hit buffer, as k_digest_stream (blocks of 4 KiB)
  const uint32_t* rules;         // nrules x A5X_RULE_STRIDE u32: function count, then the encoded functions
  uint32_t nrules;
  uint32_t* hit_rule;            // op 0: the rule index of hit h, beside d.hits
  unsigned long long* rejected;  // += lines longer than A5X_RULE_LMAX (hashed under no rule)
};
// LDS of a workgroup and 4 KiB blocks of a stream, for this route and the salted one (a5x_stream.h)
size_t a5x_stream_lds();
uint64_t a5x_stream_blocks(uint64_t nbytes);
// op 0: hash + probe every (line, rule); op 1: line starts per block (d.blk_cnt); op 2: every
// digest to d.dig_out at index line * nrules + rule (a rejected line's are zero)
// (cus: the device's compute units; the grid is cus x the workgroups a CU holds at once)
hipError_t a5x_launch_rules_stream(const A5xRuleLaunch& L, int op, uint32_t cus, hipStream_t st);

// ---- salted target lists in the digest + lookup stage (a5x_salt.hip) -----------
struct A5xSaltLaunch {
  A5xDigLaunch d;               // the stream, target set (keyed on the masked digests) and hit buffer (blocks of 4 KiB)
  const uint32_t* salts;        // nsalts records of A5X_SALT_STRIDE u32 (a5x_salt.h), sorted by salt length
  uint32_t nsalts;
  int order;                    // A5X_SALT_ORDER_PASS_SALT / A5X_SALT_ORDER_SALT_PASS
  uint32_t* hit_salt;           // op 0: the public salt index of hit h, beside d.hits
  unsigned long long* skipped;  // += (line, salt) pairs whose message would exceed A5X_RULE_LMAX (not hashed)
};
// op 0: hash + probe every (line, salt); op 1: line starts per block (d.blk_cnt); op 2: every
// digest to d.dig_out at index line * nsalts + public salt index (a skipped pair's is zero)
// (cus: the device's compute units; the grid is cus x the workgroups a CU holds at once)
hipError_t a5x_launch_salt_stream(const A5xSaltLaunch& L, int op, uint32_t cus, hipStream_t st);

// ---- salted nested target lists (a5x_salt_nest.hip) ----------------------------
// The same launch for a set of one of the algorithms 32..38 (L.d.algo): L.salts holds records of
// A5X_SNEST_STRIDE u32 built for that algorithm (a5x_salt_nest.h), L.order its own placement.
// The ops are a5x_launch_salt_stream's; a pair is skipped only for a line over A5X_RULE_LMAX.
hipError_t a5x_launch_salt_nest_stream(const A5xSaltLaunch& L, int op, uint32_t cus, hipStream_t st);

// ---- HMAC target lists (a5x_hmac.hip) -------------------------------------------
// The same launch for a set of one of the algorithms 48..55 (L.d.algo): L.salts holds records of
// A5X_HMAC_STRIDE u32 built for that algorithm (a5x_hmac.h), L.order 0 for key = pass, 1 for key
// = salt.  The ops are a5x_launch_salt_stream's; a pair is skipped only for a line over
// A5X_RULE_LMAX.
hipError_t a5x_launch_hmac_stream(const A5xSaltLaunch& L, int op, uint32_t cus, hipStream_t st);

// ---- iterated target lists: PBKDF2 (a5x_pbkdf2.hip) -----------------------------
// One pass of an iterated set (s.d.algo 72..75): the candidates of the stream blocks [b0, b1) under
// the salt records [s0, s1) of s.salts (A5X_PBKDF2_STRIDE u32 each, a5x_pbkdf2.h).  The pair of the
// pass's line `ord` (counted from block b0: s.d.blk_pre) and record s0 + r has slot r * np + ord of
// the pass's `pairs` = (s1 - s0) * np slots (np: a multiple of 64 that holds the pass's lines, so a
// wave of the flat kernels has one record); word k of slot p is state[k * pairs + p], the words
// as Pbkdf2Cfg::STATE_WORDS lists them.  Word 1 (the ordinal in the block) is ~0 for a slot with
// no pair: the caller sets all of them so before init.
struct A5xPbkdf2Launch {
  A5xSaltLaunch s;   // the stream, the target set, the hit buffer, the records, hit_salt, skipped
  uint32_t* state;
  uint64_t pairs;
  uint32_t np;
  uint64_t b0, b1;
  uint32_t s0, s1;
  uint32_t k0, k1;   // loop: iterations [k0, k1) (iteration j makes U_{j+1}; 1 <= k0), clipped to the pair's own count
};
// op 0: key states and U1 of every pair of the pass into state, += skipped pairs; op 1: line
// starts per block (s.d.blk_cnt, all blocks of the stream)
hipError_t a5x_launch_pbkdf2_init(const A5xPbkdf2Launch& L, int op, uint32_t cus, hipStream_t st);
hipError_t a5x_launch_pbkdf2_loop(const A5xPbkdf2Launch& L, hipStream_t st);
// op 0: t under the salt's mask probed, hits recorded with their index; op 2: the 16 bytes of
// every pair to s.d.dig_out at index line * s.nsalts + public index
hipError_t a5x_launch_pbkdf2_compare(const A5xPbkdf2Launch& L, int op, hipStream_t st);
