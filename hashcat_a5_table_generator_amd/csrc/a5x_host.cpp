// a5x_host.cpp -- host side of liba5x: the C ABI declared in include/a5x.h.
//
//   * substitution tables: Go-exact parser (readSubstitutionTable, main.go:108-144;
//     decodeHexNotation, main.go:147-162) and the -t merge (main.go:40-50), then
//     compiled into the flat LDS-resident device table of a5x_format.h;
//   * dictionary splitting with bufio.ScanLines semantics (main.go:72-74);
//   * the per-batch device pipeline (keyspace -> scans -> plan -> expand) on one
//     HIP stream, replacing the goroutine-per-word dispatch and the single
//     channel writer of main.go:58-98;
//   * host-buffer convenience calls (a5x_keyspace, a5x_expand) that stage words
//     into HBM and stream the expanded bytes back to a sink.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <unordered_map>
#include <memory>
#include <vector>

#include "a5x.h"
#include "a5x_format.h"
#include "a5x_plan.h"
#include "a5x_gosem.h"
#include "a5x_launch.h"
#include "a5x_md.h"
#include "a5x_nest.h"
#include "a5x_rules.h"
#include "a5x_salt.h"
#include "a5x_hmac.h"
#include "a5x_pbkdf2.h"
#include "a5x_salt_nest.h"
#include "a5x_sha.h"

namespace {

// ---------------------------------------------------------------------------
// the merged map[string][]string (keys in first-appearance order)
// ---------------------------------------------------------------------------
struct Table {
  std::vector<std::string> keys;
  std::vector<std::vector<std::string>> vals;
  std::unordered_map<std::string, uint32_t> index;

  void add(const std::string& k, const std::string& v) {
    auto it = index.find(k);
    uint32_t i;
    if (it == index.end()) {
      i = (uint32_t)keys.size();
      index.emplace(k, i);
      keys.push_back(k);
      vals.emplace_back();
    } else {
      i = it->second;
    }
    vals[i].push_back(v);
  }
  void clear() { keys.clear(); vals.clear(); index.clear(); }
  size_t nvals() const {
    size_t n = 0;
    for (auto& v : vals) n += v.size();
    return n;
  }
};

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
};

// The device scalar block a5x_ctx::d_scalars, in u32 words; h_scalars is its pinned host image
// (read_scalars).  The keyspace passes clear all of it, [0, S_COUNT).
enum Slot : uint32_t {
  S_DEFER_N = 0,     // default keyspace: words k_keyspace_thread defers to the wave kernel
  S_NBIG = 1,        // default keyspace: BIG words (big_list)
  S_ERR = 2,         // the error word of every kernel (decode_dev_err)
  S_NSLOW = 3,       // default keyspace: slow words (slow_list)
  S_CPLX_N = 4,      // default keyspace: complex words (cplx), against the record slots offered
  S_SLOW_SEGS = 5,   // job_launch: the range's slow segment items
  S_BIG_SEGS = 6,    //   and its BIG ones (the two are cleared together)
  S_GLOB_N = 7,      // both engines: pass G words (glob)
  // Two uses that never overlap in time: k_hibytes sets the flag and k_keyspace_thread reads it
  // inside one a5x_launch_keyspace, and nothing reads it afterwards; every digest route clears
  // the word before each of its launches (hits_run), behind the keyspace on the same stream.
  S_HIFLAG = 8,      // keyspace: the batch has bytes >= 0x80
  S_NHITS = 8,       // digest routes: hits found by one launch, beyond the hit buffer's room too
  // Again two: the virtual-word split runs in the -s / -s -r keyspace only, the hybrid gathers
  // its sub-batch in default mode only, after the keyspace, and clears the word first.
  S_VLONG_N = 9,     // -s / -s -r keyspace: words k_keyspace_vsub leaves to its large stage (m_cl2)
  S_NONFAST_N = 9,   // fused default route: candidate-bearing words the fused kernel skipped (hy_list)
  S_VREC_N = 10,     // -s / -s -r keyspace: sub-word record u64 needed, one u64 in [10, 11]
  S_PROBE_N = 12,    // -r / -s keyspace: words the FAST probe leaves to the mode engine (m_cl);
                     //   without the probe, k_mode_count_thread's left-over list
  S_MCT_N = 13,      // -s / -s -r keyspace: k_mode_count_thread's left-over list behind the probe (m_cl2)
  S_ROV_N = 14,      // -r / -s keyspace: words a tile could not decide, against the overflow slots offered
  S_VOUT_N = 15,     // -s / -s -r keyspace: words the split leaves to the mode engine (m_vl)
  S_GUARD = 16,      // the bounds guard's record, 8 u64 in [16, 31] (decode_dev_err)
  S_REFIT = 32,      // keyspace words walked twice (a5x_debug_keyspace_refit)
  S_TSPAN = 33,      // largest tile span of the batch (k_tile_span)
  S_STAGE = 34,      // word stage the keyspace pass used (a5x_debug_keyspace_stage)
  S_CPLX_LEAN = 35,  // k_keyspace_cplx: words of the lean path, of the generic one, [35, 36] (a5x_debug_keyspace_cplx_lean)
  S_COUNT = 37,      // device words in use
  H_RANGE_ERR = 38,  // host image only: a5x_expand_range's error word per output buffer, [38, 39]
  S_ALLOC = 64       // words allocated, device and host
};
static_assert(S_COUNT <= H_RANGE_ERR && H_RANGE_ERR + 2 <= S_ALLOC, "the scalar block holds every slot");

// a5x_ctx::h_totals (pinned u64): the scan totals read back
enum Total : uint32_t {
  T_CANDS = 0,   // the batch's candidates
  T_BYTES = 1,   // its output bytes; -r / -s keyspace: its mode items, then its bytes
  T_LINES = 2,   // stream_count_lines: the stream's lines
  T_VWORDS = 3,  // build_virtual: sub-words added to the word list
  T_VREC = 4,    //   and their record u64
  T_ALLOC = 8
};

}  // namespace

struct a5x_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::string devname;
  int cus = 0;

  Table table;
  bool table_dirty = true;
  std::vector<uint8_t> blob;
  uint8_t* d_table = nullptr;
  size_t d_table_cap = 0;
  uint32_t table_bytes = 0;
  // -r / -s / -s -r engines (a5x_modes.hip): sorted mode table + per-item state
  bool mtable_dirty = true;
  std::vector<uint8_t> mblob;
  uint8_t* d_mtab = nullptr;
  size_t d_mtab_cap = 0;
  uint32_t mtab_bytes = 0;
  DevBuf<uint64_t> m_nseg, m_seg_off, m_seg_bytes, m_seg_boff, m_tmp;
  DevBuf<uint8_t> m_item_fl;  // per item: the layout that expands it (a5x_modes.hip m_item)
  DevBuf<uint32_t> m_item_w;
  uint64_t m_items = 0;
  uint64_t m_nglob = 0;       // mode pass G words of the current batch (their list: glob)
  // hybrid fused digest: the non-FAST words of a batch gathered into a sub-batch
  DevBuf<uint32_t> hy_list;
  DevBuf<uint64_t> hy_lens, hy_off;
  DevBuf<uint8_t> hy_words;
  uint8_t* mgscr = nullptr;   // mode pass G scratch: A5X_G_SLOTS x a5x_mode_gslot_bytes(), on first use
  uint64_t mseg = 4096;  // candidates per mode-engine item (C5 -r: most words one item, sized by k_mode_count)
  uint64_t rov_need = 0;  // -r/-s FAST probe: overflow slots a previous batch needed (k_keyspace_rprobe)
  uint64_t cplx_need = 0;  // default mode: complex-word record slots a previous batch needed
  // -s / -s -r virtual words (k_keyspace_vsub, k_vwords_fill): the words left to the mode
  // engine, per-word sub-word counts / record sizes and their scans, the sub-word records,
  // and the virtual word list k_expand_fast runs on
  DevBuf<uint32_t> m_vl;
  DevBuf<uint64_t> vn, vrsz, vpre, vrpre, vrec, vrec2, vcand_off, vbyte_off;
  DevBuf<uint16_t> vocc;  // per word 16 u16: occurrence rows (k_keyspace_thread -> k_keyspace_vsub)
  DevBuf<uint32_t> vflags, vroff, vmap, vobase;
  uint64_t vrec_need = 0;  // sub-word record u64 a previous batch needed
  // fused digest + lookup (a5x_digest.hip)
  int t_algo = -1;
  uint64_t n_targets = 0;
  uint32_t t_bm_log2 = 0, t_has_zero = 0;
  uint64_t t_tmask = 0;
  DevBuf<uint32_t> t_bitmap;
  DevBuf<uint4> t_table;
  DevBuf<uint8_t> dg_scratch;
  DevBuf<uint64_t> dg_blk_cnt, dg_blk_pre, dg_cand_off, dg_byte_off;
  DevBuf<A5xHitRaw> dg_hits;
  // wide algorithms (SHA-1 and the SHA-2 family): t_tw tail words per digest past the first
  // four -- per table slot (t_tails), of the zero-prefix targets (t_ztails), per device hit
  // (dg_hit_tail, a5x_hit_tail_stride words each); the sorted unique digests on the host (a5x_hit_digest),
  // whether two of them share their first 16 bytes, and for such prefixes the tails the
  // latest expand_digest call's hits matched, keyed by (word, cand)
  uint32_t t_tw = 0, t_nz = 0;
  DevBuf<uint32_t> t_tails, t_ztails, dg_hit_tail;
  std::vector<uint8_t> t_full;
  bool t_shared_prefix = false;
  std::map<std::pair<uint64_t, uint64_t>, std::array<uint32_t, 12>> t_hit_tails;
  hipEvent_t dev_ev[2] = {nullptr, nullptr};
  // rules (a5x_rules.hip): the accepted rules as a table of A5X_RULE_STRIDE u32 each (host
  // copy + device copy), and of the latest digest call: each copied hit's rule, the lines
  // rejected as longer than A5X_RULE_LMAX, the hashes computed
  std::vector<uint32_t> r_rules;
  uint32_t n_rules = 0;
  DevBuf<uint32_t> r_table, dg_hit_rule;
  DevBuf<unsigned long long> r_counter;
  std::vector<uint32_t> r_hit_rule;
  uint64_t r_rejected = 0, r_hashed = 0;
  // salted target lists (a5x_salt.hip): the set's order, its distinct salts in first-
  // appearance order (bytes + n + 1 offsets), the salt records sorted by length (host copy +
  // device copy), and of the latest digest call: each copied hit's salt index, the (candidate,
  // salt) pairs hashed and skipped.  The pair counter on the device is r_counter: a context
  // holds rules or salts, never both.
  bool salted = false;
  int s_order = 0;
  std::vector<uint8_t> s_bytes;
  std::vector<uint64_t> s_off;
  std::vector<uint32_t> s_recs;
  uint32_t n_salts = 0;
  DevBuf<uint32_t> s_table, dg_hit_salt;
  std::vector<uint32_t> s_hit_salt;
  uint64_t s_hashed = 0, s_skipped = 0;
  // iterated target lists (a5x_pbkdf2.hip): a salted set of order 0 whose "salts" are distinct
  // (salt, iterations) pairs -- the count of each, per target its index, the whole key the list
  // gave and its line (a5x_load_pbkdf2_hashes; empty: none), the targets of each (index, first 16
  // bytes).  The pairs' state buffer; the budgets of a pass and of a loop launch (0: the defaults,
  // a5x_debug_iter_budget) and the latest call's loop launches.
  std::vector<uint32_t> it_iters, it_tidx;
  std::vector<std::vector<uint8_t>> it_keys;
  std::vector<std::string> it_lines;
  std::map<std::pair<uint32_t, std::array<uint8_t, 16>>, std::vector<uint64_t>> it_by_key;
  DevBuf<uint32_t> it_state;
  uint64_t it_slots = 0, it_pair_iters = 0, it_launches = 0;

  DevBuf<uint64_t> count, bytes, cand_off, byte_off, scan_tmp, locate;
  DevBuf<uint32_t> flags, defer, chunk_w0, slow_list, big_list, roff, cplx;
  DevBuf<uint64_t> segs;  // slow / BIG segment items
  DevBuf<uint32_t> glob;  // pass G word list (words beyond the pass-B LDS budget)
  DevBuf<uint32_t> m_cl, m_cl2;  // mode-engine word lists (FAST probe -> k_mode_count_thread -> k_mode_count)
  uint8_t* gscr = nullptr;  // pass G scratch: A5X_G_SLOTS x a5x_gslot_bytes(), allocated on first use
  DevBuf<uint64_t> rec;  // FAST plan records (keyspace tiles of FW_TILE_REC u64)
  bool ks_large_only = false;  // a5x_debug_keyspace_large_stage: the small word stage is not offered
  uint64_t flags_nw = 0;       // words whose flags the last keyspace pass wrote (a5x_debug_word_flags)
  uint32_t* d_scalars = nullptr;  // S_ALLOC words, indexed by Slot
  uint32_t* h_scalars = nullptr;  // pinned, its host image
  uint64_t* h_totals = nullptr;   // pinned, T_ALLOC u64 indexed by Total

  // host-API staging: words, and the double-buffered output stream of a5x_expand
  // (two HBM range buffers, two pinned host buffers, a copy stream; main.go:58-68)
  DevBuf<uint8_t> s_words, s_out[2];
  DevBuf<uint64_t> s_woff;
  uint8_t* h_out[2] = {nullptr, nullptr};
  size_t h_out_cap = 0;
  hipStream_t cstream = nullptr;
  hipEvent_t ev_exp[2] = {nullptr, nullptr}, ev_cpy[2] = {nullptr, nullptr};
  DevBuf<uint64_t> loc_q, loc_r;  // range-boundary queries / results (job_locate)

  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // side stream: the per-word kernels (k_expand_slow / k_expand_b) of a range run beside
  // k_expand_fast (disjoint output bytes), joined back before the range completes
  hipStream_t sstream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  uint64_t seg = 512;         // candidates per per-word-path segment (a radix round there costs ~64x a FAST one;
                              // C3 A/B: 512 / 256 -1 %, 4096 +8 %, 16384 +44 % -- the slow words run beside k_expand_fast)
  uint64_t chunk = 16384;     // candidates per expand wave (round-5 A/B, profiles/r05c_ab_chunk_16k.txt:
                              // C3 expansion 8.49-8.53 vs 8.62-8.76 ms at 8192, 8.56 at 32768)
  uint32_t waves_per_block = 4;
  uint32_t waves_per_block_fast = 1;
};

namespace {

int fail(a5x_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return code;
}

#define HIPCHK(c, x)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) return fail((c), A5X_E_HIP, "%s failed: %s", #x, hipGetErrorString(e_)); \
  } while (0)

template <typename T>
int grow(a5x_ctx* c, DevBuf<T>& b, size_t n) {
  if (n <= b.cap) return A5X_OK;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  size_t want = n + n / 8 + 64;
  hipError_t e = hipMalloc((void**)&b.p, want * sizeof(T));
  if (e != hipSuccess) {
    b.p = nullptr;
    return fail(c, A5X_E_NOMEM, "hipMalloc(%zu bytes) failed: %s", want * sizeof(T), hipGetErrorString(e));
  }
  b.cap = want;
  return A5X_OK;
}

template <typename T>
void release(DevBuf<T>& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

// Device slots [0, last] into h_scalars, behind the stream's work: valid once the caller has
// synchronised the stream.
hipError_t read_scalars(a5x_ctx* c, hipStream_t st, Slot last) {
  return hipMemcpyAsync(c->h_scalars, c->d_scalars, (last + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
}

// readSubstitutionTable on one file's bytes, merged into t (main.go:108-144 + 40-50)
int parse_table_into(a5x_ctx* c, Table& t, const uint8_t* d, size_t n) {
  using namespace a5x::gosem;
  Table ft;  // the file's own map, then appended per key like main.go:47-49
  size_t pos = 0;
  const uint8_t* line;
  size_t len;
  int r;
  while ((r = scan_line(d, n, &pos, &line, &len)) == 1) {
    const uint8_t* s = line;
    size_t m = len;
    trim_space(&s, &m);
    if (m == 0 || s[0] == '#') continue;
    const uint8_t* eq = (const uint8_t*)memchr(s, '=', m);
    if (!eq) continue;
    std::string k, v;
    const size_t kn = (size_t)(eq - s);
    if (!decode_hex_notation(s, kn, &k)) {
      fprintf(stderr, "Error decoding hex notation in key: %.*s\n", (int)m, (const char*)s);
      continue;
    }
    if (!decode_hex_notation(eq + 1, m - kn - 1, &v)) {
      fprintf(stderr, "Error decoding hex notation in value: %.*s\n", (int)m, (const char*)s);
      continue;
    }
    ft.add(k, v);
  }
  if (r < 0) return fail(c, A5X_E_TOOLONG, "bufio.Scanner: token too long");
  for (size_t i = 0; i < ft.keys.size(); i++)
    for (auto& v : ft.vals[i]) t.add(ft.keys[i], v);
  return A5X_OK;
}

// Compile the map into the device table blob of a5x_format.h.
// Static per-key facts of the -s / -s -r positional engines (k_mode_count_thread, the
// -s / -s -r FAST probe of k_keyspace_thread): bit 0 / 1 = the key passes m_pos_setup's
// positional checks in -s / -s -r for ANY word (one codepoint, ASCII if one byte; <= 14
// values (-s) or subs[0] (-s -r) of <= 15 valid UTF-8 bytes containing no key at all -- a
// superset of "no later pattern"); bits 8-19 / 20-31 = sum over those values of
// (len - klen) + 2048.
uint32_t key_pos_facts(const Table& t, const std::string& k, const std::vector<std::string>& vs) {
  if (t.keys.size() > 1024) return 0;  // (the containment test is O(keys^2))
  auto valid_utf8 = [](const std::string& v) {
    for (size_t i = 0; i < v.size();) {
      int sz = 0;
      const int r = a5x::gosem::decode_rune((const uint8_t*)v.data() + i, v.size() - i, &sz);
      if (r == a5x::gosem::kRuneError && sz == 1) return false;
      i += (size_t)sz;
    }
    return true;
  };
  auto has_key = [&](const std::string& v) {
    for (const std::string& kj : t.keys)
      if (!kj.empty() && v.find(kj) != std::string::npos) return true;
    return false;
  };
  int sz = 0;
  const int r0 = k.empty() ? 0 : a5x::gosem::decode_rune((const uint8_t*)k.data(), k.size(), &sz);
  const bool cp = k.size() >= 1 && k.size() <= 4 && sz == (int)k.size() && !(r0 == a5x::gosem::kRuneError && sz == 1) &&
                  !(sz == 1 && (uint8_t)k[0] >= 0x80);
  auto vok = [&](const std::string& v) { return v.size() <= 15 && valid_utf8(v) && !has_key(v); };
  bool ok2 = cp && vs.size() <= 14, ok3 = cp;
  int d2 = 0, d3 = 0;
  for (size_t v = 0; v < vs.size(); v++) {
    const bool o = vok(vs[v]);
    ok2 = ok2 && o;
    if (v == 0) { ok3 = ok3 && o; d3 = (int)vs[0].size() - (int)k.size(); }
    d2 += (int)vs[v].size() - (int)k.size();
  }
  return (ok2 ? 1u : 0u) | (ok3 ? 2u : 0u) | ((uint32_t)(d2 + 2048) & 0xFFFu) << 8 | ((uint32_t)(d3 + 2048) & 0xFFFu) << 20;
}

int compile_table(a5x_ctx* c) {
  const Table& t = c->table;
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < t.keys.size(); i++)
    if (!t.keys[i].empty()) order.push_back(i);
  // bucket by first byte, longest key first inside a bucket
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const uint8_t fa = (uint8_t)t.keys[a][0], fb = (uint8_t)t.keys[b][0];
    if (fa != fb) return fa < fb;
    return t.keys[a].size() > t.keys[b].size();
  });
  if (order.size() > 65535) return fail(c, A5X_E_UNSUPPORTED, "table has %zu keys (max 65535)", order.size());
  std::vector<uint16_t> bucket(257, 0);
  for (uint32_t i : order) bucket[(uint8_t)t.keys[i][0] + 1]++;
  for (int b = 0; b < 256; b++) bucket[b + 1] += bucket[b];

  std::vector<A5xKey> keys;
  std::vector<A5xChoice> ch;
  std::vector<uint8_t> blob;
  uint32_t max_klen = 0, max_vlen = 0;
  auto add_choice = [&](const std::string& s) -> int {
    A5xChoice x;
    memset(&x, 0, sizeof x);
    if (s.size() > 65535) return -1;
    x.len = (uint16_t)s.size();
    for (size_t i = 0; i < s.size() && i < 4; i++) x.first4 |= (uint32_t)(uint8_t)s[i] << (8 * i);
    if (blob.size() + s.size() > 65535) return -1;
    x.blob_off = (uint16_t)blob.size();
    blob.insert(blob.end(), s.begin(), s.end());
    ch.push_back(x);
    return 0;
  };
  for (uint32_t i : order) {
    const std::string& k = t.keys[i];
    const auto& vs = t.vals[i];
    if (k.size() > 65535 || vs.size() > 65535)
      return fail(c, A5X_E_UNSUPPORTED, "table key/value list too large for the device table");
    A5xKey key;
    memset(&key, 0, sizeof key);
    key.pad0 = (uint16_t)(key_pos_facts(t, k, vs) & 3u);  // -s / -s -r FAST probe (r_unit)
    key.klen = (uint16_t)k.size();
    key.nvals = (uint16_t)vs.size();
    key.choice_base = (uint32_t)ch.size();
    int maxd = -65536;
    if (add_choice(k)) return fail(c, A5X_E_UNSUPPORTED, "device table blob exceeds 64 KiB");
    for (auto& v : vs) {
      if (add_choice(v)) return fail(c, A5X_E_UNSUPPORTED, "device table blob exceeds 64 KiB");
      key.sumlen += (uint32_t)v.size();
      maxd = std::max(maxd, (int)v.size() - (int)k.size());
      max_vlen = std::max(max_vlen, (uint32_t)v.size());
    }
    key.maxdelta = (int16_t)std::max(-32768, std::min(32767, maxd));
    {
      size_t mc = k.size();
      for (auto& v : vs) mc = std::max(mc, v.size());
      key.maxclen = (uint16_t)std::min<size_t>(mc, 65535);
    }
    for (auto& v : vs) {
      const long d = (long)v.size() - (long)k.size();
      if (d > 0) key.sum_dpos += (uint32_t)d; else key.sum_dneg += (uint32_t)(-d);
    }
    {
      size_t mn = k.size();
      for (auto& v : vs) mn = std::min(mn, v.size());
      key.minclen = (uint16_t)std::min<size_t>(mn, 65535);
    }
    max_klen = std::max(max_klen, (uint32_t)k.size());
    keys.push_back(key);
  }
  auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  A5xTableHdr h;
  memset(&h, 0, sizeof h);
  h.magic = A5X_TABLE_MAGIC;
  h.nkeys = (uint32_t)keys.size();
  h.nchoices = (uint32_t)ch.size();
  h.off_bucket = sizeof(A5xTableHdr);
  h.off_keys = (uint32_t)al16(h.off_bucket + 257 * sizeof(uint16_t));
  h.off_choices = (uint32_t)al16(h.off_keys + keys.size() * sizeof(A5xKey));
  h.off_kmatch = (uint32_t)al16(h.off_choices + ch.size() * sizeof(A5xChoice));
  h.off_bucket2 = (uint32_t)al16(h.off_kmatch + std::max<size_t>(keys.size(), 1) * 8);
  h.off_cval = (uint32_t)al16(h.off_bucket2 + 256 * 4);
  h.off_blob = (uint32_t)al16(h.off_cval + std::max<size_t>(ch.size(), 1) * 8);
  h.blob_bytes = (uint32_t)blob.size();
  h.total_bytes = (uint32_t)al16(h.off_blob + blob.size() + 8);  // 8 B tail for 4-byte reads
  h.max_klen = max_klen;
  h.max_vlen = max_vlen;
  h.has_empty_key = t.index.count(std::string()) ? 1u : 0u;
  for (int b = 0; b < 256; b++) h.max_bucket = std::max<uint32_t>(h.max_bucket, bucket[b + 1] - bucket[b]);
  h.lead_only = 1;
  for (int b = 0x80; b < 0xC0; b++) h.lead_only = bucket[b + 1] > bucket[b] ? 0u : h.lead_only;
  if (h.total_bytes > A5X_TABLE_LDS_MAX)
    return fail(c, A5X_E_UNSUPPORTED, "device table is %u bytes (LDS staging max %u)", h.total_bytes,
                (unsigned)A5X_TABLE_LDS_MAX);
  c->blob.assign(h.total_bytes, 0);
  memcpy(c->blob.data(), &h, sizeof h);
  memcpy(c->blob.data() + h.off_bucket, bucket.data(), 257 * sizeof(uint16_t));
  if (!keys.empty()) memcpy(c->blob.data() + h.off_keys, keys.data(), keys.size() * sizeof(A5xKey));
  if (!ch.empty()) memcpy(c->blob.data() + h.off_choices, ch.data(), ch.size() * sizeof(A5xChoice));
  if (!blob.empty()) memcpy(c->blob.data() + h.off_blob, blob.data(), blob.size());
  // the walk's compact views (k_keyspace_thread psk_walk): one read per byte, one per key
  for (size_t k = 0; k < keys.size(); k++) {
    const uint64_t km = (uint64_t)ch[keys[k].choice_base].first4 | ((uint64_t)keys[k].klen << 32);
    memcpy(c->blob.data() + h.off_kmatch + 8 * k, &km, 8);
  }
  for (int b = 0; b < 256; b++) {
    const uint32_t v = (uint32_t)bucket[b] | ((uint32_t)bucket[b + 1] << 16);
    memcpy(c->blob.data() + h.off_bucket2 + 4 * b, &v, 4);
  }
  for (size_t i = 0; i < ch.size(); i++) {  // the planner's choice bytes, one read each
    uint64_t v = 0;
    for (uint32_t k = 0; k < ch[i].len && k < 7; k++) v |= (uint64_t)blob[ch[i].blob_off + k] << (8 * k);
    v |= (uint64_t)std::min<uint32_t>(ch[i].len, 255) << 56;
    memcpy(c->blob.data() + h.off_cval + 8 * i, &v, 8);
  }
  c->table_bytes = h.total_bytes;
  return A5X_OK;
}

// the compiled table's keys all start on UTF-8 lead (or ASCII) bytes (A5xTableHdr::lead_only)
bool table_lead_only(const a5x_ctx* c) {
  return c->blob.size() >= sizeof(A5xTableHdr) && ((const A5xTableHdr*)c->blob.data())->lead_only != 0 &&
         !getenv("A5X_NO_UTF_WALK");
}

int upload_table(a5x_ctx* c) {
  if (c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (c->table.keys.empty()) return fail(c, A5X_E_NOTABLE, "no substitution table loaded");
  if (!c->table_dirty) return A5X_OK;
  int rc = compile_table(c);
  if (rc) return rc;
  if (c->d_table_cap < c->blob.size()) {
    if (c->d_table) (void)hipFree(c->d_table);
    c->d_table = nullptr;
    HIPCHK(c, hipMalloc((void**)&c->d_table, c->blob.size()));
    c->d_table_cap = c->blob.size();
  }
  HIPCHK(c, hipMemcpyAsync(c->d_table, c->blob.data(), c->blob.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->table_dirty = false;
  return A5X_OK;
}

int check_mode(a5x_ctx* c, int mode) {
  if (mode < 0 || mode > 3) return fail(c, A5X_E_ARG, "bad mode %d", mode);
  return A5X_OK;
}

int decode_dev_err(a5x_ctx* c, uint32_t e) {
  if (!e) return A5X_OK;
  if (e & 32u) {
    uint64_t d[8] = {0};
    (void)hipMemcpy(d, c->d_scalars + S_GUARD, sizeof d, hipMemcpyDeviceToHost);
    return fail(c, A5X_E_HIP,
                "device bounds guard tripped: code %llu ctx {%llu, %llu, %llu, %llu} block %llu thread %llu",
                (unsigned long long)d[0], (unsigned long long)d[1], (unsigned long long)d[2],
                (unsigned long long)d[3], (unsigned long long)d[4], (unsigned long long)d[5],
                (unsigned long long)d[6]);
  }
  if (e & 128u)
    return fail(c, A5X_E_BOUNDS,
                "panic: runtime error: slice bounds out of range (processWordReverse, main.go:255: a negative "
                "actualStart from the running offset)");
  if (e & 64u)
    return fail(c, A5X_E_UNSUPPORTED,
                "a word exceeds the -r/-s engine limits (length <= %d B, <= %d patterns/positions, DP <= %d "
                "entries, <= %d keys)", A5X_M_LMAX, A5X_M_NMAX, A5X_M_DPMAX, A5X_MTAB_KEYS_MAX);
  if (e & 256u)
    return fail(c, A5X_E_UNSUPPORTED, "a -r/-s candidate is longer than %d bytes (device limit)", A5X_M_CBUF - 1);
  if (e & 2u) return fail(c, A5X_E_OVERFLOW, "a word's keyspace overflows 64 bits");
  if (e & 16u) return fail(c, A5X_E_OVERFLOW, "batch keyspace overflows 64 bits");
  if (e & 4u)
    return fail(c, A5X_E_UNSUPPORTED,
                "a word with candidates exceeds the device limits (length %d B, %d matches, min(max,matches) "
                "<= 63 substitutions unless the window is free, DP (events+1) x (min(max,matches)+1) <= %u, "
                "candidates <= %u B)", A5X_LMAX_G, A5X_MLMAX_G, (unsigned)A5X_DPENT_G, (unsigned)A5X_RING_G - 16u);
  return fail(c, A5X_E_HIP, "device consistency error 0x%x", e);
}

// words with overlapping keys (or other irregular shapes) whose FAST records go to
// fixed slots after the tile regions: this many slots at first (a batch with more complex
// words grows them and runs its keyspace again, run_keyspace)
uint32_t ks_cplx_cap(uint64_t nw) { return (uint32_t)std::min<uint64_t>(nw / 16 + 1024, 1u << 22); }

struct Batch {  // device-side per-batch state after keyspace
  uint64_t total_cands = 0, total_bytes = 0;
  uint32_t nbig = 0, nslow = 0;
  uint32_t nglob = 0;  // pass G words (on the BIG list, expanded by k_expand_g)
  bool rfast = false;  // -r / -s / -s -r: FAST words probed by k_keyspace_thread (k_expand_fast)
  uint64_t nmode = 0;  // -r / -s / -s -r: words left to the mode engine (0: no mode-item launch)
  bool virt = false;   // -s / -s -r: virtual words present; k_expand_fast runs on the virtual list
  uint64_t nv = 0;     // its entries
  const uint64_t* cand_off = nullptr;
  const uint64_t* byte_off = nullptr;
};

// Exclusive scans of the per-word a and b (n entries) into pa and pb, their totals into
// h_totals[T_CANDS] / [T_BYTES], device slots [0, last] into h_scalars; synchronises.
int scan_totals(a5x_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* pa, uint64_t* pb, Slot last,
                hipStream_t st) {
  HIPCHK(c, a5x_launch_scan(a, b, n, pa, pb, c->scan_tmp.p, c->d_scalars + S_ERR, st));
  HIPCHK(c, hipMemcpyAsync(c->h_totals + T_CANDS, pa + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(c->h_totals + T_BYTES, pb + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, read_scalars(c, st, last));
  HIPCHK(c, hipStreamSynchronize(st));
  return A5X_OK;
}

// Diagnostics of a keyspace error: the first offending word, appended to the error text
// (with_flags: the default engine's text, which shows the word's flags too).
void name_offending_word(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, bool with_flags) {
  std::vector<uint32_t> fl(nw);
  std::vector<uint64_t> wo(nw + 1);
  if (!nw || hipMemcpy(fl.data(), c->flags.p, nw * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(wo.data(), d_woff, (nw + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return;
  for (uint64_t i = 0; i < nw; i++)
    if (fl[i] & (A5X_WF_ERR_BIG | A5X_WF_ERR_OVF)) {
      std::string w((size_t)(wo[i + 1] - wo[i]), '\0');
      (void)hipMemcpy(&w[0], d_words + wo[i], w.size(), hipMemcpyDeviceToHost);
      char tail[160];
      if (with_flags)
        snprintf(tail, sizeof tail, " [word %llu len %zu flags 0x%08x: %.40s]", (unsigned long long)i, w.size(),
                 fl[i], w.c_str());
      else
        snprintf(tail, sizeof tail, " [word %llu len %zu: %.40s]", (unsigned long long)i, w.size(), w.c_str());
      c->err += tail;
      return;
    }
}

// keyspace -> flags, per-word counts/bytes, exclusive scans (synchronises once)
int run_keyspace(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mn, int mx,
                 uint64_t* d_cand_off, uint64_t* d_byte_off, hipStream_t st, Batch* B, bool timed) {
  int rc;
  if ((rc = upload_table(c))) return rc;
  if (nw > 0xffffffffull) return fail(c, A5X_E_ARG, "batch of %llu words (max 2^32-1)", (unsigned long long)nw);
  // FAST record slots of the complex words (k_keyspace_cplx): enough for every one of them,
  // so whether a word is FAST (and how its candidates are numbered) never depends on how
  // many complex words share its batch; u32 record offsets bound the whole record area
  const uint64_t ccap = std::min<uint64_t>(nw + 1, std::max<uint64_t>(ks_cplx_cap(nw), c->cplx_need));
  if (((nw + FW_TILE - 1) / FW_TILE) * (uint64_t)FW_TILE_REC + ccap * FW_RMAX > 0xffffffffull)
    return fail(c, A5X_E_ARG, "batch of %llu words is too large for one call (FAST record index; split it)",
                (unsigned long long)nw);
  if ((rc = grow(c, c->count, nw + 1)) || (rc = grow(c, c->bytes, nw + 1)) || (rc = grow(c, c->flags, nw + 1)) ||
      (rc = grow(c, c->defer, nw + 1)) || (rc = grow(c, c->scan_tmp, a5x_scan_tmp_elems(nw + 1) + 16)) ||
      (rc = grow(c, c->roff, nw + 1)) || (rc = grow(c, c->cplx, nw + 1)) ||
      (rc = grow(c, c->slow_list, nw + 1)) || (rc = grow(c, c->big_list, nw + 1)) || (rc = grow(c, c->glob, nw + 1)) ||
      (rc = grow(c, c->rec, ((nw + FW_TILE - 1) / FW_TILE) * (uint64_t)FW_TILE_REC + ccap * FW_RMAX + 2)))
    return rc;
  c->flags_nw = nw;
  if (!d_cand_off) {
    if ((rc = grow(c, c->cand_off, nw + 1))) return rc;
    d_cand_off = c->cand_off.p;
  }
  if (!d_byte_off) {
    if ((rc = grow(c, c->byte_off, nw + 1))) return rc;
    d_byte_off = c->byte_off.p;
  }
  if (timed) HIPCHK(c, hipEventRecord(c->ev[0], st));
  HIPCHK(c, hipMemsetAsync(c->d_scalars, 0, S_COUNT * sizeof(uint32_t), st));
  A5xKsLaunch K;
  memset(&K, 0, sizeof K);
  if (nw > 0) {
    K.table = c->d_table; K.table_bytes = c->table_bytes; K.words = d_words; K.woff = d_woff; K.nw = nw;
    K.mn = mn; K.mx = mx; K.count = c->count.p; K.bytes = c->bytes.p; K.flags = c->flags.p;
    K.defer_list = c->defer.p; K.defer_n = c->d_scalars + S_DEFER_N; K.nbig = c->d_scalars + S_NBIG;
    K.err = c->d_scalars + S_ERR;
    K.hiflag = table_lead_only(c) ? c->d_scalars + S_HIFLAG : nullptr;
    K.nrefit = c->d_scalars + S_REFIT;
    K.ncplx_lean = c->d_scalars + S_CPLX_LEAN;
    K.small_stage = c->ks_large_only ? 0u : a5x_keyspace_small_stage(c->table_bytes);
    K.tspan = c->d_scalars + S_TSPAN; K.stage_used = c->d_scalars + S_STAGE;
    K.nslow = c->d_scalars + S_NSLOW;
    K.slow_list = c->slow_list.p; K.big_list = c->big_list.p;
    K.rec = c->rec.p; K.roff = c->roff.p;
    K.cplx_list = c->cplx.p; K.cplx_n = c->d_scalars + S_CPLX_N; K.cplx_cap = (uint32_t)ccap;
    K.cplx_base = ((nw + FW_TILE - 1) / FW_TILE) * (uint64_t)FW_TILE_REC;
    K.defer_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nw, (uint64_t)c->cus * 4));
    K.glob_list = c->glob.p; K.glob_n = c->d_scalars + S_GLOB_N;
    HIPCHK(c, a5x_launch_keyspace(K, st));
    if ((rc = scan_totals(c, c->count.p, c->bytes.p, nw, d_cand_off, d_byte_off, S_GLOB_N, st))) return rc;
  } else {
    HIPCHK(c, hipMemsetAsync(d_cand_off, 0, 8, st));
    HIPCHK(c, hipMemsetAsync(d_byte_off, 0, 8, st));
    c->h_totals[T_CANDS] = c->h_totals[T_BYTES] = 0;
    HIPCHK(c, read_scalars(c, st, S_GLOB_N));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  if (nw > 0 && c->h_scalars[S_CPLX_N] > ccap) {
    // more complex words than record slots: room for all of them, and the keyspace again
    c->cplx_need = c->h_scalars[S_CPLX_N];
    return run_keyspace(c, d_words, d_woff, nw, mn, mx, d_cand_off, d_byte_off, st, B, timed);
  }
  if (nw > 0 && c->h_scalars[S_ERR] == 0 && c->h_scalars[S_GLOB_N] > 0) {
    // pass G: words beyond the pass-B LDS budget are sized in HBM scratch slots (their
    // counts were 0 in the first scan), then the scan runs again
    if (!c->gscr) {
      const size_t gb = (size_t)A5X_G_SLOTS * a5x_gslot_bytes();
      HIPCHK(c, hipMalloc((void**)&c->gscr, gb));
      HIPCHK(c, hipMemsetAsync(c->gscr, 0, gb, st));  // the rings start (and stay) zero
    }
    K.gscr = c->gscr; K.gslots = A5X_G_SLOTS;
    HIPCHK(c, a5x_launch_keyspace_g(K, st));
    if ((rc = scan_totals(c, c->count.p, c->bytes.p, nw, d_cand_off, d_byte_off, S_GLOB_N, st))) return rc;
  }
  if ((rc = decode_dev_err(c, c->h_scalars[S_ERR]))) {
    name_offending_word(c, d_words, d_woff, nw, true);
    return rc;
  }
  B->total_cands = nw ? c->h_totals[T_CANDS] : 0;
  B->total_bytes = nw ? c->h_totals[T_BYTES] : 0;
  B->nbig = c->h_scalars[S_NBIG];
  B->nslow = c->h_scalars[S_NSLOW];
  B->nglob = nw ? c->h_scalars[S_GLOB_N] : 0;
  B->cand_off = d_cand_off;
  B->byte_off = d_byte_off;
  return A5X_OK;
}

A5xExpLaunch exp_launch(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mn, int mx,
                        const Batch& B) {
  A5xExpLaunch E;
  memset(&E, 0, sizeof E);
  E.table = c->d_table; E.table_bytes = c->table_bytes; E.words = d_words; E.woff = d_woff; E.nw = nw;
  E.cand_off = B.cand_off; E.byte_off = B.byte_off; E.flags = c->flags.p; E.chunk_w0 = c->chunk_w0.p;
  E.CH = c->chunk; E.SEG = c->seg; E.mn = mn; E.mx = mx; E.err = c->d_scalars + S_ERR;
  E.dbg = (uint64_t*)(c->d_scalars + S_GUARD);
  E.waves_per_block = c->waves_per_block;
  E.waves_per_block_fast = c->waves_per_block_fast;
  E.rec = c->rec.p; E.roff = c->roff.p; E.rec_n = c->rec.cap;
  if (B.nglob) { E.gscr = c->gscr; E.gslots = A5X_G_SLOTS; }
  return E;
}


// ---------------------------------------------------------------------------
// -r / -s / -s -r engines (a5x_modes.hip)
// ---------------------------------------------------------------------------

// The sorted mode table of a5x_format.h (keys in Go sort.Strings order, main.go:327).
int compile_mtable(a5x_ctx* c) {
  const Table& t = c->table;
  std::vector<uint32_t> order(t.keys.size());
  for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return t.keys[a] < t.keys[b]; });
  if (order.size() > A5X_MTAB_KEYS_MAX)
    return fail(c, A5X_E_UNSUPPORTED, "table has %zu keys (-r/-s device engines: max %d)", order.size(),
                A5X_MTAB_KEYS_MAX);
  std::vector<A5xMKey> keys;
  std::vector<A5xMVal> vals;
  std::vector<uint8_t> blob;
  std::vector<uint16_t> bucket(257, 0);
  uint32_t has_empty = 0;
  for (uint32_t i : order) {
    const std::string& k = t.keys[i];
    if (k.empty()) has_empty = 1;  // sorts first: key 0
    else bucket[(uint8_t)k[0] + 1]++;
    A5xMKey K;
    memset(&K, 0, sizeof K);
    if (k.size() > 65535 || t.vals[i].size() > 65535) return fail(c, A5X_E_UNSUPPORTED, "table key too large");
    K.key_off = (uint32_t)blob.size();
    K.klen = (uint16_t)k.size();
    K.nvals = (uint16_t)t.vals[i].size();
    K.val_base = (uint32_t)vals.size();
    blob.insert(blob.end(), k.begin(), k.end());
    for (auto& v : t.vals[i]) {
      A5xMVal V;
      V.off = (uint32_t)blob.size();
      V.len = (uint32_t)v.size();
      blob.insert(blob.end(), v.begin(), v.end());
      vals.push_back(V);
    }
    keys.push_back(K);
  }
  // static per-key facts (key_pos_facts) for the lane-per-word -s / -s -r keyspace
  for (size_t i = 0; i < order.size(); i++)
    keys[i].pad = key_pos_facts(t, t.keys[order[i]], t.vals[order[i]]);
  bucket[0] = (uint16_t)has_empty;
  for (int b = 0; b < 256; b++) bucket[b + 1] += bucket[b];
  auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  A5xMHdr h;
  memset(&h, 0, sizeof h);
  h.magic = A5X_MTAB_MAGIC;
  h.nkeys = (uint32_t)keys.size();
  h.nvals = (uint32_t)vals.size();
  h.has_empty = has_empty;
  h.off_bucket = sizeof(A5xMHdr);
  h.off_keys = (uint32_t)al16(h.off_bucket + 257 * sizeof(uint16_t));
  h.off_vals = (uint32_t)al16(h.off_keys + keys.size() * sizeof(A5xMKey));
  h.off_blob = (uint32_t)al16(h.off_vals + vals.size() * sizeof(A5xMVal));
  const size_t total = al16(h.off_blob + blob.size() + 8);
  if (total > A5X_MTAB_LDS_MAX)
    return fail(c, A5X_E_UNSUPPORTED, "mode table is %zu bytes (-r/-s LDS staging max %d)", total,
                A5X_MTAB_LDS_MAX);
  h.total_bytes = (uint32_t)total;
  c->mblob.assign(total, 0);
  memcpy(c->mblob.data(), &h, sizeof h);
  memcpy(c->mblob.data() + h.off_bucket, bucket.data(), 257 * sizeof(uint16_t));
  if (!keys.empty()) memcpy(c->mblob.data() + h.off_keys, keys.data(), keys.size() * sizeof(A5xMKey));
  if (!vals.empty()) memcpy(c->mblob.data() + h.off_vals, vals.data(), vals.size() * sizeof(A5xMVal));
  if (!blob.empty()) memcpy(c->mblob.data() + h.off_blob, blob.data(), blob.size());
  c->mtab_bytes = (uint32_t)total;
  return A5X_OK;
}

int upload_mtable(a5x_ctx* c) {
  if (c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (c->table.keys.empty()) return fail(c, A5X_E_NOTABLE, "no substitution table loaded");
  if (!c->mtable_dirty) return A5X_OK;
  int rc = compile_mtable(c);
  if (rc) return rc;
  if (c->d_mtab_cap < c->mblob.size()) {
    if (c->d_mtab) (void)hipFree(c->d_mtab);
    c->d_mtab = nullptr;
    HIPCHK(c, hipMalloc((void**)&c->d_mtab, c->mblob.size()));
    c->d_mtab_cap = c->mblob.size();
  }
  HIPCHK(c, hipMemcpyAsync(c->d_mtab, c->mblob.data(), c->mblob.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->mtable_dirty = false;
  return A5X_OK;
}

A5xModeLaunch mode_launch(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode,
                          int mn, int mx, bool rfast = false, bool virt = false) {
  A5xModeLaunch M;
  memset(&M, 0, sizeof M);
  M.rfast = rfast ? 1 : 0;
  if (rfast) { M.rec = c->rec.p; M.roff = c->roff.p; }
  if (virt) {
    M.vpre = c->vpre.p; M.vcand_off = c->vcand_off.p; M.vbyte_off = c->vbyte_off.p;
    M.vroff = c->vroff.p; M.vrec = c->vrec2.p;
  }
  M.mtab = c->d_mtab; M.mtab_bytes = c->mtab_bytes; M.words = d_words; M.woff = d_woff; M.nw = nw;
  M.mode = mode; M.mn = mn; M.mx = mx; M.SEG = c->mseg;
  M.count = c->count.p; M.nseg = c->m_nseg.p; M.flags = c->flags.p;
  M.wbytes = c->bytes.p;  // (scratch until k_mode_wordbytes writes the per-word bytes)
  M.seg_off = c->m_seg_off.p; M.item_w = c->m_item_w.p; M.nitems = c->m_items;
  M.seg_bytes = c->m_seg_bytes.p; M.seg_boff = c->m_seg_boff.p; M.item_fl = c->m_item_fl.p;
  M.cand_begin = 0; M.cand_end = ~0ull;
  M.err = c->d_scalars + S_ERR;
  M.glob_list = c->glob.p; M.glob_n = c->d_scalars + S_GLOB_N;
  if (c->m_nglob) { M.gscr = c->mgscr; M.gslots = A5X_G_SLOTS; }
  return M;
}

// The virtual word list of a -s / -s -r batch with virtual words (k_keyspace_vsub): every
// word one entry, a virtual word one per sub-word, records in list order (copied, or written
// from a fixed-width word's descriptor); the chunk -> first entry map of k_expand_fast over it.
// byte_off null: no output layout (fused digest).  Synchronises once.
int build_virtual(a5x_ctx* c, uint64_t nw, const uint8_t* d_words, const uint64_t* d_woff, int mode, int mn,
                  const uint64_t* d_cand_off, const uint64_t* d_byte_off, hipStream_t st, Batch* B) {
  int rc;
  if ((rc = grow(c, c->vpre, nw + 1)) || (rc = grow(c, c->vrpre, nw + 1))) return rc;
  HIPCHK(c, a5x_launch_vwords_sizes(c->flags.p, d_cand_off, nw, c->vn.p, c->vrsz.p, st));
  HIPCHK(c, a5x_launch_scan(c->vn.p, c->vrsz.p, nw, c->vpre.p, c->vrpre.p, c->scan_tmp.p, c->d_scalars + S_ERR, st));
  HIPCHK(c, hipMemcpyAsync(c->h_totals + T_VWORDS, c->vpre.p + nw, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(c->h_totals + T_VREC, c->vrpre.p + nw, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const uint64_t nv = nw + c->h_totals[T_VWORDS], nrec = c->h_totals[T_VREC];
  if (nv > 0xffffffffull || nrec + 4 > 0xffffffffull)
    return fail(c, A5X_E_ARG, "batch of %llu words is too large for one -s call (virtual word list)",
                (unsigned long long)nw);
  if ((rc = grow(c, c->vcand_off, nv + 1)) || (rc = grow(c, c->vbyte_off, nv + 1)) ||
      (rc = grow(c, c->vflags, nv + 1)) || (rc = grow(c, c->vroff, nv + 1)) || (rc = grow(c, c->vmap, nv + 1)) ||
      (rc = grow(c, c->vobase, nv + 1)) || (rc = grow(c, c->vrec2, nrec + 4)))
    return rc;
  A5xVwLaunch V;
  V.flags = c->flags.p; V.cand_off = d_cand_off; V.byte_off = d_byte_off; V.roff = c->roff.p; V.rec = c->rec.p;
  V.vrec = c->vrec.p; V.vpre = c->vpre.p; V.vrpre = c->vrpre.p; V.nw = nw;
  V.vcand_off = c->vcand_off.p; V.vbyte_off = c->vbyte_off.p; V.vflags = c->vflags.p; V.vroff = c->vroff.p;
  V.vmap = c->vmap.p; V.vobase = c->vobase.p; V.vrec2 = c->vrec2.p;
  V.table = c->d_table; V.table_bytes = c->table_bytes; V.rmode = mode; V.rcmin = mn > 0 ? 1u : 0u;
  V.words = d_words; V.woff = d_woff;
  HIPCHK(c, a5x_launch_vwords_fill(V, st));
  if (B->total_cands) {
    const uint64_t nchunks = (B->total_cands + c->chunk - 1) / c->chunk;
    if ((rc = grow(c, c->chunk_w0, nchunks + 1))) return rc;
    HIPCHK(c, a5x_launch_plan(c->vcand_off.p, nv, c->chunk, c->chunk_w0.p, st));
  }
  B->virt = true;
  B->nv = nv;
  return A5X_OK;
}

// k_expand_fast over a -r / -s / -s -r batch's FAST words (the virtual word list when the
// batch has virtual words)
A5xExpLaunch exp_launch_mode(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mn, int mx,
                             const Batch& B) {
  A5xExpLaunch E = exp_launch(c, d_words, d_woff, nw, mn, mx, B);
  if (B.virt) {
    E.nw = B.nv; E.cand_off = c->vcand_off.p; E.byte_off = c->vbyte_off.p; E.flags = c->vflags.p;
    E.roff = c->vroff.p; E.rec = c->vrec2.p; E.rec_n = c->vrec2.cap; E.vmap = c->vmap.p; E.vobase = c->vobase.p;
  }
  return E;
}

// Keyspace of the -r / -s / -s -r engines: per-word counts (DP), items of mseg
// candidates, a length pass over every item (output bytes are not closed-form under
// sequential strings.ReplaceAll), and the scans.  Synchronises twice.
// lengths = false (the fused digest): counts and items only -- no length pass, no
// output layout (B->total_bytes = 0).
int run_keyspace_mode(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode, int mn,
                      int mx, uint64_t* d_cand_off, uint64_t* d_byte_off, hipStream_t st, Batch* B, bool timed,
                      bool lengths = true) {
  int rc;
  if ((rc = upload_mtable(c))) return rc;
  if (nw > 0xffffffffull) return fail(c, A5X_E_ARG, "batch of %llu words (max 2^32-1)", (unsigned long long)nw);
  // -r with min < 0: the subCount loop (main.go:238) reaches k = min < 0 whenever it runs
  // at all (min(max, n) >= min, i.e. max >= min), and generateCombinations(n, k < 0)
  // recurses until the goroutine stack overflows (main.go:263-281), which kills the
  // reference process on the first word.
  if (mode == A5X_MODE_REVERSE && mn < 0 && mx >= mn && nw > 0)
    return fail(c, A5X_E_BOUNDS,
                "fatal error: stack overflow (generateCombinations with k < 0, main.go:273; --table-min %d)", mn);
  if ((rc = grow(c, c->count, nw + 1)) || (rc = grow(c, c->bytes, nw + 1)) || (rc = grow(c, c->flags, nw + 1)) ||
      (rc = grow(c, c->m_nseg, nw + 1)) || (rc = grow(c, c->m_seg_off, nw + 1)) ||
      (rc = grow(c, c->glob, nw + 1)) || (rc = grow(c, c->scan_tmp, a5x_scan_tmp_elems(nw + 1) + 16)))
    return rc;
  c->m_nglob = 0;
  c->flags_nw = nw;
  if (!d_cand_off) {
    if ((rc = grow(c, c->cand_off, nw + 1))) return rc;
    d_cand_off = c->cand_off.p;
  }
  if (!d_byte_off) {
    if ((rc = grow(c, c->byte_off, nw + 1))) return rc;
    d_byte_off = c->byte_off.p;
  }
  if (timed) HIPCHK(c, hipEventRecord(c->ev[0], st));
  HIPCHK(c, hipMemsetAsync(c->d_scalars, 0, S_COUNT * sizeof(uint32_t), st));
  B->cand_off = d_cand_off;
  B->byte_off = d_byte_off;
  B->nbig = B->nslow = 0;
  B->rfast = false;
  B->virt = false;
  B->nv = 0;
  if (nw == 0) {
    HIPCHK(c, hipMemsetAsync(d_cand_off, 0, 8, st));
    HIPCHK(c, hipMemsetAsync(d_byte_off, 0, 8, st));
    HIPCHK(c, hipStreamSynchronize(st));
    B->total_cands = B->total_bytes = 0;
    c->m_items = 0;
    return A5X_OK;
  }
  // FAST probe (a5x_kernels.hip mode_unit): -r words with pairwise disjoint positions whose
  // subs[0] keep the key lengths, -s / -s -r words whose every pattern occurs once and is
  // statically positional, go to the FAST path: the default keyspace kernel plans them
  // (count, bytes, record; flags & A5X_WF_FAST), the mode-engine kernels skip them, and
  // k_expand_fast (k_expand_fast_md5 / _ntlm in the fused digest) writes them beside the
  // mode engine's items -- every path numbers a word's candidates the same way.  The other
  // words are listed for the mode engine.  (An empty key makes "" a pattern of every -s word.)
  const bool has_empty = ((const A5xMHdr*)c->mblob.data())->has_empty != 0;
  bool rfast = mx >= 1 && mn <= 1 && !getenv("A5X_NO_RFAST") &&
               (mode == A5X_MODE_REVERSE || ((mode == A5X_MODE_SUBALL || mode == A5X_MODE_SUBALL_REVERSE) && !has_empty));
  if (rfast && upload_table(c) != A5X_OK) {  // (a table the default engine refuses: mode engine only)
    rfast = false;
    c->err.clear();
  }
  B->rfast = rfast;
  // -s / -s -r: radix positional words counted lane per word (k_mode_count_thread) over the
  // words the probe left; the wave kernel k_mode_count only for the words it lists
  const bool mct = (mode == A5X_MODE_SUBALL || mode == A5X_MODE_SUBALL_REVERSE) && mx >= 0 && !has_empty &&
                   !getenv("A5X_NO_MCT");
  if ((rfast || mct) && ((rc = grow(c, c->m_cl, nw + 1)) || (rc = grow(c, c->m_cl2, nw + 1)))) return rc;
  // -s / -s -r words the probe refused for repeated patterns: split into FAST sub-words
  // (k_keyspace_vsub) before the mode engine counts the rest
  const bool vsub = rfast && mct && mode != A5X_MODE_REVERSE && !getenv("A5X_NO_VSUB");
  const uint64_t vcap = std::min<uint64_t>(0xfffffff0ull, std::max<uint64_t>(nw * 64 + 4096, c->vrec_need));
  if (vsub && ((rc = grow(c, c->m_vl, nw + 1)) || (rc = grow(c, c->vn, nw + 1)) || (rc = grow(c, c->vrsz, nw + 1)) ||
               (rc = grow(c, c->vrec, vcap + 2)) || (rc = grow(c, c->vocc, 16 * (nw + 1)))))
    return rc;
  // (the probe's overflow slots: words a keyspace tile could not decide, k_keyspace_rprobe)
  const uint64_t rtiles = ((nw + FW_TILE - 1) / FW_TILE) * (uint64_t)FW_TILE_REC;
  const uint64_t rcap = std::min<uint64_t>(nw, std::max<uint64_t>(ks_cplx_cap(nw), c->rov_need));
  if (rfast) {
    if (rtiles + rcap * FW_RMAX > 0xffffffffull)  // (u32 record offsets)
      return fail(c, A5X_E_ARG, "batch of %llu words is too large for one -r/-s call (FAST record index)",
                  (unsigned long long)nw);
    if ((rc = grow(c, c->roff, nw + 1)) || (rc = grow(c, c->cplx, nw + 1)) ||
        (rc = grow(c, c->rec, rtiles + rcap * FW_RMAX + 2)))
      return rc;
    A5xKsLaunch K;
    memset(&K, 0, sizeof K);
    K.table = c->d_table; K.table_bytes = c->table_bytes; K.words = d_words; K.woff = d_woff; K.nw = nw;
    K.mn = mn; K.mx = mx; K.count = c->count.p; K.bytes = c->bytes.p; K.flags = c->flags.p;
    K.err = c->d_scalars + S_ERR; K.rec = c->rec.p; K.roff = c->roff.p;
    K.rmode = mode; K.rcmin = mn > 0 ? 1u : 0u; K.rnseg = c->m_nseg.p; K.rseg = c->mseg;
    K.defer_list = c->m_cl.p; K.defer_n = c->d_scalars + S_PROBE_N;
    K.cplx_list = c->cplx.p; K.cplx_n = c->d_scalars + S_ROV_N; K.cplx_cap = (uint32_t)rcap; K.cplx_base = rtiles;
    K.defer_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nw + 255) / 256, (uint64_t)c->cus * 2));
    K.vocc = vsub ? c->vocc.p : nullptr;
    K.hiflag = table_lead_only(c) ? c->d_scalars + S_HIFLAG : nullptr;
    K.nrefit = c->d_scalars + S_REFIT;
    K.small_stage = c->ks_large_only ? 0u : a5x_keyspace_small_stage(c->table_bytes);
    K.tspan = c->d_scalars + S_TSPAN; K.stage_used = c->d_scalars + S_STAGE;
    HIPCHK(c, a5x_launch_keyspace(K, st));
    if (vsub) {
      K.vout_list = c->m_vl.p; K.vout_n = c->d_scalars + S_VOUT_N;
      K.vn = c->vn.p; K.vrsz = c->vrsz.p; K.vrec = c->vrec.p;
      K.vrec_n = (uint64_t*)(c->d_scalars + S_VREC_N); K.vrec_cap = vcap;
      if (!getenv("A5X_VSUB_LARGE_ONLY")) {  // (m_cl2 is free until k_mode_count_thread below)
        K.vlong_list = c->m_cl2.p; K.vlong_n = c->d_scalars + S_VLONG_N;
      }
      HIPCHK(c, a5x_launch_vsub(K, st));
    }
  }
  A5xModeLaunch M = mode_launch(c, d_words, d_woff, nw, mode, mn, mx, rfast);
  if (mct) {
    M.in_list = vsub ? c->m_vl.p : rfast ? c->m_cl.p : nullptr;
    M.in_n = vsub ? c->d_scalars + S_VOUT_N : rfast ? c->d_scalars + S_PROBE_N : nullptr;
    M.cl_list = rfast ? c->m_cl2.p : c->m_cl.p;
    M.cl_n = c->d_scalars + (rfast ? S_MCT_N : S_PROBE_N);
    HIPCHK(c, a5x_launch_mode_count_thread(M, st));
  } else if (rfast) {  // k_mode_count only over the words the probe left to the mode engine
    M.cl_list = c->m_cl.p;
    M.cl_n = c->d_scalars + S_PROBE_N;
  }
  HIPCHK(c, a5x_launch_mode_count(M, st));
  if ((rc = scan_totals(c, c->count.p, c->m_nseg.p, nw, d_cand_off, c->m_seg_off.p, S_VOUT_N, st))) return rc;
  if (rfast && c->h_scalars[S_ROV_N] > rcap) {
    // more undecided words than overflow slots: grow to fit them all and run again (the
    // undecided tail was left uncounted, so nothing of this pass is used)
    c->rov_need = c->h_scalars[S_ROV_N];
    return run_keyspace_mode(c, d_words, d_woff, nw, mode, mn, mx, d_cand_off, d_byte_off, st, B, timed, lengths);
  }
  uint64_t vused = 0;
  if (vsub) memcpy(&vused, c->h_scalars + S_VREC_N, 8);
  if (vsub && vused > vcap) {
    // more sub-word records than room: grow to fit them all and run again (words past
    // the room were left undecided)
    if (vused > 0xfffffff0ull)
      return fail(c, A5X_E_ARG, "batch of %llu words is too large for one -s call (sub-word records)",
                  (unsigned long long)nw);
    c->vrec_need = vused;
    return run_keyspace_mode(c, d_words, d_woff, nw, mode, mn, mx, d_cand_off, d_byte_off, st, B, timed, lengths);
  }
  B->nmode = vsub ? c->h_scalars[S_VOUT_N] : rfast ? c->h_scalars[S_PROBE_N] : nw;
  if (vsub && getenv("A5X_VSUB_DEBUG")) {  // (diagnostics: what the split leaves to the mode engine)
    fprintf(stderr, "[vsub] words %llu probe-left %u split-left %u vrec %llu\n", (unsigned long long)nw,
            c->h_scalars[S_PROBE_N], c->h_scalars[S_VOUT_N], (unsigned long long)vused);
    const uint32_t k = std::min<uint32_t>(c->h_scalars[S_VOUT_N], 24);
    std::vector<uint32_t> li(k);
    std::vector<uint64_t> wo(nw + 1);
    if (k && hipMemcpy(li.data(), c->m_vl.p, 4 * k, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(wo.data(), d_woff, 8 * (nw + 1), hipMemcpyDeviceToHost) == hipSuccess)
      for (uint32_t x : li) {
        std::string s((size_t)(wo[x + 1] - wo[x]), '\0');
        (void)hipMemcpy(&s[0], d_words + wo[x], s.size(), hipMemcpyDeviceToHost);
        fprintf(stderr, "[vsub]   left: %s\n", s.c_str());
      }
  }
  if (c->h_scalars[S_ERR] == 0 && c->h_scalars[S_GLOB_N] > 0) {
    // mode pass G: words longer than the LDS engines take are counted in HBM scratch
    // slots (their counts were 0 in the first scan), then the scan runs again
    if (!c->mgscr) {
      HIPCHK(c, hipMalloc((void**)&c->mgscr, (size_t)A5X_G_SLOTS * a5x_mode_gslot_bytes()));
    }
    c->m_nglob = c->h_scalars[S_GLOB_N];
    M = mode_launch(c, d_words, d_woff, nw, mode, mn, mx, rfast);
    HIPCHK(c, a5x_launch_mode_count_g(M, st));
    if ((rc = scan_totals(c, c->count.p, c->m_nseg.p, nw, d_cand_off, c->m_seg_off.p, S_GLOB_N, st))) return rc;
  }
  if ((rc = decode_dev_err(c, c->h_scalars[S_ERR]))) {
    name_offending_word(c, d_words, d_woff, nw, false);
    return rc;
  }
  B->total_cands = c->h_totals[T_CANDS];
  const uint64_t items = c->h_totals[T_BYTES];
  c->m_items = items;
  if ((rc = grow(c, c->m_item_w, items + 1)) || (rc = grow(c, c->m_seg_bytes, items + 1)) ||
      (rc = grow(c, c->m_item_fl, items + 1)) ||
      (rc = grow(c, c->m_seg_boff, items + 1)) || (rc = grow(c, c->m_tmp, items + 1)) ||
      (rc = grow(c, c->scan_tmp, a5x_scan_tmp_elems(items + 1) + 16)))
    return rc;
  M = mode_launch(c, d_words, d_woff, nw, mode, mn, mx, rfast);
  M.cand_off = d_cand_off;
  M.item_begin = 0;
  M.item_end = items;
  if (rfast && B->total_cands) {  // chunk -> first word map for k_expand_fast
    const uint64_t nchunks = (B->total_cands + c->chunk - 1) / c->chunk;
    if ((rc = grow(c, c->chunk_w0, nchunks + 1))) return rc;
    HIPCHK(c, a5x_launch_plan(d_cand_off, nw, c->chunk, c->chunk_w0.p, st));
  }
  if (items) HIPCHK(c, a5x_launch_plan(c->m_seg_off.p, nw, 1, c->m_item_w.p, st));
  if (!lengths) {
    HIPCHK(c, read_scalars(c, st, S_ERR));
    HIPCHK(c, hipStreamSynchronize(st));
    if ((rc = decode_dev_err(c, c->h_scalars[S_ERR]))) return rc;
    B->total_bytes = 0;
    return vused ? build_virtual(c, nw, d_words, d_woff, mode, mn, d_cand_off, nullptr, st, B) : A5X_OK;
  }
  if (items) HIPCHK(c, a5x_launch_mode_items(M, 0, st));
  if (items)
    HIPCHK(c, a5x_launch_scan(c->m_seg_bytes.p, c->m_seg_bytes.p, items, c->m_seg_boff.p, c->m_tmp.p,
                              c->scan_tmp.p, c->d_scalars + S_ERR, st));
  else
    HIPCHK(c, hipMemsetAsync(c->m_seg_boff.p, 0, 8, st));
  HIPCHK(c, a5x_launch_mode_wordbytes(c->m_seg_off.p, c->m_seg_boff.p, nw, d_byte_off, c->bytes.p, st));
  HIPCHK(c, hipMemcpyAsync(c->h_totals + T_BYTES, d_byte_off + nw, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, read_scalars(c, st, S_ERR));
  HIPCHK(c, hipStreamSynchronize(st));
  if ((rc = decode_dev_err(c, c->h_scalars[S_ERR]))) return rc;
  B->total_bytes = c->h_totals[T_BYTES];
  return vused ? build_virtual(c, nw, d_words, d_woff, mode, mn, d_cand_off, d_byte_off, st, B) : A5X_OK;
}

// ---------------------------------------------------------------------------
// Batch jobs: the keyspace runs once per batch (job_prepare), then any number of
// candidate ranges are located and expanded against it (job_locate, job_launch).
// ---------------------------------------------------------------------------
struct Job {  // (opened as Job J{words, offsets, nw, mode, mn, mx, stream})
  const uint8_t* w = nullptr;
  const uint64_t* wo = nullptr;
  uint64_t nw = 0;
  int mode = 0, mn = 0, mx = 0;
  hipStream_t st = nullptr;
  bool lengths = true;  // -r / -s engines: output layout wanted (false: the fused digest)
  Batch B;
};

// [cb, ce) global candidates <-> output bytes [b0, b1); -r/-s engines: items [i0, i1)
struct Range {
  uint64_t cb, ce, b0, b1, i0, i1;
};

int job_prepare(a5x_ctx* c, Job& J, uint64_t* d_cand_off, uint64_t* d_byte_off, bool timed) {
  int rc;
  if (J.mode != A5X_MODE_DEFAULT)
    return run_keyspace_mode(c, J.w, J.wo, J.nw, J.mode, J.mn, J.mx, d_cand_off, d_byte_off, J.st, &J.B, timed,
                             J.lengths);
  if ((rc = run_keyspace(c, J.w, J.wo, J.nw, J.mn, J.mx, d_cand_off, d_byte_off, J.st, &J.B, timed))) return rc;
  if (J.B.total_cands) {  // chunk -> first word map, consumed by every range's k_expand_fast
    const uint64_t nchunks = (J.B.total_cands + c->chunk - 1) / c->chunk;
    if ((rc = grow(c, c->chunk_w0, nchunks + 1))) return rc;
    HIPCHK(c, a5x_launch_plan(J.B.cand_off, J.nw, c->chunk, c->chunk_w0.p, J.st));
  }
  return A5X_OK;
}

int job_check(a5x_ctx* c, const Job& J) {
  HIPCHK(c, read_scalars(c, J.st, S_ERR));
  HIPCHK(c, hipStreamSynchronize(J.st));
  return decode_dev_err(c, c->h_scalars[S_ERR]);
}

// Output byte (and -r/-s item) positions of global candidate indices q[0..n) (sorted or
// not); synchronises.  res[3 i] = byte offset, [3 i + 1] = item, [3 i + 2] = index in item.
int job_locate(a5x_ctx* c, const Job& J, const std::vector<uint64_t>& q, std::vector<uint64_t>& res) {
  int rc;
  const uint32_t n = (uint32_t)q.size();
  res.assign(3 * (size_t)n, 0);
  if (!n) return A5X_OK;
  if ((rc = grow(c, c->loc_q, n)) || (rc = grow(c, c->loc_r, 3 * (size_t)n))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->loc_q.p, q.data(), 8 * (size_t)n, hipMemcpyHostToDevice, J.st));
  if (J.mode != A5X_MODE_DEFAULT) {
    A5xModeLaunch M = mode_launch(c, J.w, J.wo, J.nw, J.mode, J.mn, J.mx, J.B.rfast, J.B.virt);
    M.cand_off = J.B.cand_off;
    HIPCHK(c, a5x_launch_mode_locate(M, c->loc_q.p, n, c->loc_r.p, J.st));
    std::vector<uint64_t> t(3 * (size_t)n);
    HIPCHK(c, hipMemcpyAsync(t.data(), c->loc_r.p, 24 * (size_t)n, hipMemcpyDeviceToHost, J.st));
    if ((rc = job_check(c, J))) return rc;
    for (uint32_t i = 0; i < n; i++) {
      res[3 * i] = t[3 * i + 2];
      res[3 * i + 1] = t[3 * i];
      res[3 * i + 2] = t[3 * i + 1];
    }
    return A5X_OK;
  }
  A5xExpLaunch E = exp_launch(c, J.w, J.wo, J.nw, J.mn, J.mx, J.B);
  HIPCHK(c, a5x_launch_locate(E, c->loc_q.p, n, c->loc_r.p, J.st));
  std::vector<uint64_t> t(n);
  HIPCHK(c, hipMemcpyAsync(t.data(), c->loc_r.p, 8 * (size_t)n, hipMemcpyDeviceToHost, J.st));
  if ((rc = job_check(c, J))) return rc;
  for (uint32_t i = 0; i < n; i++) res[3 * i] = t[i];
  return A5X_OK;
}

// the range [cb, ce) from job_locate's answers for cb (lb) and ce (le)
Range range_of(uint64_t cb, uint64_t ce, const uint64_t* lb, const uint64_t* le) {
  return Range{cb, ce, lb[0], le[0], lb[1], le[1] + (le[2] ? 1 : 0)};
}

// Cut [0, total) into ranges of at most cap output bytes: candidate boundaries spaced for
// ~3/4 cap each, located in one call; ranges that still exceed cap are halved.
// (cb, ce: only the candidates [cb, ce) of the batch, cut into ranges the same way)
int plan_ranges(a5x_ctx* c, const Job& J, uint64_t cap, std::vector<Range>& out, uint64_t cb = 0,
                uint64_t ce = ~0ull) {
  out.clear();
  const uint64_t T = J.B.total_cands, TB = J.B.total_bytes;
  ce = std::min(ce, T);
  if (cb >= ce) return A5X_OK;
  int rc;
  uint64_t RB = TB;  // the bytes of [cb, ce)
  std::vector<uint64_t> ends;
  if (cb != 0 || ce != T) {
    if ((rc = job_locate(c, J, {cb, ce}, ends))) return rc;
    RB = ends[3] - ends[0];
  }
  if (RB <= cap) {
    if (cb == 0 && ce == T) out.push_back(Range{0, T, 0, TB, 0, J.mode != A5X_MODE_DEFAULT ? c->m_items : 0});
    else out.push_back(range_of(cb, ce, &ends[0], &ends[3]));
    return A5X_OK;
  }
  const uint64_t K = std::max<uint64_t>(2, (RB + cap * 3 / 4 - 1) / std::max<uint64_t>(1, cap * 3 / 4));
  std::vector<uint64_t> q(K + 1), res;
  for (uint64_t k = 0; k <= K; k++) q[k] = cb + (uint64_t)((unsigned __int128)(ce - cb) * k / K);
  if ((rc = job_locate(c, J, q, res))) return rc;
  std::vector<Range> work;
  for (uint64_t k = 0; k < K; k++)
    if (q[k + 1] > q[k]) work.push_back(range_of(q[k], q[k + 1], &res[3 * k], &res[3 * (k + 1)]));
  // halve oversize ranges until every range fits
  for (int pass = 0; pass < 64; pass++) {
    std::vector<uint64_t> mid;
    for (auto& R : work)
      if (R.b1 - R.b0 > cap) {
        if (R.ce - R.cb == 1)
          return fail(c, A5X_E_CAPACITY, "one candidate needs %llu bytes, the range buffer has %llu",
                      (unsigned long long)(R.b1 - R.b0), (unsigned long long)cap);
        mid.push_back(R.cb + (R.ce - R.cb) / 2);
      }
    if (mid.empty()) break;
    std::vector<uint64_t> mres;
    if ((rc = job_locate(c, J, mid, mres))) return rc;
    std::vector<Range> next;
    size_t m = 0;
    for (auto& R : work) {
      if (R.b1 - R.b0 > cap) {
        const uint64_t lb[3] = {R.b0, R.i0, 0};
        const uint64_t* lm = &mres[3 * m];
        const uint64_t le[3] = {R.b1, R.i1, 0};
        next.push_back(range_of(R.cb, mid[m], lb, lm));
        Range H = range_of(mid[m], R.ce, lm, le);
        H.i0 = lm[1];  // the half starts inside item lm[1]
        next.push_back(H);
        m++;
      } else {
        next.push_back(R);
      }
    }
    work.swap(next);
  }
  out.swap(work);
  return A5X_OK;
}

// The side stream picks up behind the work queued on st so far (stream and events made on
// first use); side_join: st goes on behind the side stream's work.
int side_fork(a5x_ctx* c, hipStream_t st) {
  if (!c->sstream) HIPCHK(c, hipStreamCreateWithFlags(&c->sstream, hipStreamNonBlocking));
  if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  if (!c->ev_join) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->ev_fork, st));
  HIPCHK(c, hipStreamWaitEvent(c->sstream, c->ev_fork, 0));
  return A5X_OK;
}

int side_join(a5x_ctx* c, hipStream_t st) {
  HIPCHK(c, hipEventRecord(c->ev_join, c->sstream));
  HIPCHK(c, hipStreamWaitEvent(st, c->ev_join, 0));
  return A5X_OK;
}

// a located range and its output buffer into an expansion or mode-engine launch
template <class L>
void range_into(L& X, const Range& R, uint8_t* d_out, uint64_t out_cap) {
  X.cand_begin = R.cb;
  X.cand_end = R.ce;
  X.out = d_out;
  X.out_base = R.b0;
  X.out_cap = out_cap;
}

// Launch the expansion of one located range into d_out (asynchronous on J.st).
int job_launch(a5x_ctx* c, const Job& J, const Range& R, uint8_t* d_out, uint64_t out_cap) {
  int rc;
  if (R.ce <= R.cb) return A5X_OK;
  if (R.b1 - R.b0 > out_cap || (!d_out && R.b1 > R.b0))
    return fail(c, A5X_E_CAPACITY, "output needs %llu bytes, buffer has %llu", (unsigned long long)(R.b1 - R.b0),
                (unsigned long long)out_cap);
  if (J.mode != A5X_MODE_DEFAULT) {
    A5xModeLaunch M = mode_launch(c, J.w, J.wo, J.nw, J.mode, J.mn, J.mx, J.B.rfast);
    M.cand_off = J.B.cand_off;
    M.item_begin = R.i0;
    M.item_end = R.i1;
    range_into(M, R, d_out, out_cap);
    if (!J.B.rfast) {
      HIPCHK(c, a5x_launch_mode_items(M, 1, J.st));
      return A5X_OK;
    }
    // -r FAST words: k_expand_fast on the job stream, the mode engine's items (disjoint
    // output bytes) on the side stream, joined before the range completes
    if ((rc = side_fork(c, J.st))) return rc;
    // a few mode words among many FAST ones: a small grid filters the items beside k_expand_fast
    // instead of one workgroup per 64 items (C5 -s A/B, profiles/r05g_ab_mode_items_grid_c5.txt)
    M.grid_cap = J.B.nmode * 8 < J.nw ? 2048u : 0u;
    if (J.B.nmode) HIPCHK(c, a5x_launch_mode_items(M, 1, c->sstream));  // (every word FAST: none)
    A5xExpLaunch E = exp_launch_mode(c, J.w, J.wo, J.nw, J.mn, J.mx, J.B);
    range_into(E, R, d_out, out_cap);
    HIPCHK(c, a5x_launch_expand(E, 0, J.st));
    return side_join(c, J.st);
  }
  const Batch& B = J.B;
  A5xExpLaunch E = exp_launch(c, J.w, J.wo, J.nw, J.mn, J.mx, B);
  range_into(E, R, d_out, out_cap);
  // slow / BIG words: (word, SEG-candidate segment) items, slow from segs[0], BIG
  // from segs[sbound]; a word adds at most ceil(range / SEG) + 1 segments
  const uint64_t rng_segs = (R.ce - R.cb) / c->seg + 1;
  const uint64_t sbound = B.nslow ? B.nslow + rng_segs : 0;
  const uint64_t bbound = B.nbig ? B.nbig + rng_segs : 0;
  if (sbound + bbound > 0xffffffffull)
    return fail(c, A5X_E_CAPACITY, "call range needs more than 2^32 slow-path segments (lower A5X_CHUNK range)");
  if (B.nslow || B.nbig) {
    if ((rc = grow(c, c->segs, sbound + bbound + 1))) return rc;
    static_assert(S_BIG_SEGS == S_SLOW_SEGS + 1, "one clear for both segment counts");
    HIPCHK(c, hipMemsetAsync(c->d_scalars + S_SLOW_SEGS, 0, 2 * sizeof(uint32_t), J.st));
  }
  if (B.nslow)
    HIPCHK(c, a5x_launch_segments(c->slow_list.p, c->d_scalars + S_NSLOW, B.nslow, B.cand_off, R.cb, R.ce, c->seg,
                                  c->segs.p, c->d_scalars + S_SLOW_SEGS, J.st));
  if (B.nbig)
    HIPCHK(c, a5x_launch_segments(c->big_list.p, c->d_scalars + S_NBIG, B.nbig, B.cand_off, R.cb, R.ce, c->seg,
                                  c->segs.p + sbound, c->d_scalars + S_BIG_SEGS, J.st));
  const bool forked = B.nslow || B.nbig;
  if (forked && (rc = side_fork(c, J.st))) return rc;
  if (B.nslow) {
    E.segs = c->segs.p; E.nsegs = c->d_scalars + S_SLOW_SEGS; E.nsegs_bound = sbound;
    HIPCHK(c, a5x_launch_expand(E, 1, c->sstream));
  }
  if (B.nbig) {
    E.segs = c->segs.p + sbound; E.nsegs = c->d_scalars + S_BIG_SEGS; E.nsegs_bound = bbound;
    HIPCHK(c, a5x_launch_expand(E, 2, c->sstream));
    if (B.nglob) HIPCHK(c, a5x_launch_expand(E, 4, c->sstream));  // pass G words of the same list
  }
  HIPCHK(c, a5x_launch_expand(E, 0, J.st));
  return forked ? side_join(c, J.st) : A5X_OK;
}

// ---------------------------------------------------------------------------
// fused digest + lookup (a5x_digest.hip)
// ---------------------------------------------------------------------------
inline uint64_t tgt_slot(const uint32_t* d, uint64_t tmask) {
  const uint64_t h = ((uint64_t)d[1] | ((uint64_t)d[2] << 32)) * 0x9E3779B97F4A7C15ull;  // == probe()
  return (h >> 20) & tmask;
}

A5xDigLaunch dig_launch(a5x_ctx* c) {
  A5xDigLaunch D;
  memset(&D, 0, sizeof D);
  D.algo = c->t_algo < 0 ? A5X_ALGO_MD5 : c->t_algo;
  D.bitmap = c->t_bitmap.p;
  D.bm_mask = c->t_bm_log2 >= 32 ? 0xffffffffu : (uint32_t)((1ull << c->t_bm_log2) - 1);
  D.table = c->t_table.p; D.tmask = c->t_tmask; D.has_zero_target = c->t_has_zero;
  D.err = c->d_scalars + S_ERR;
  if (c->t_tw) {
    D.tails = c->t_tails.p; D.ztails = c->t_ztails.p; D.nztails = c->t_nz;
  }
  return D;
}

// digest bytes per algorithm (a5x_digest_size), 0: not an algorithm
inline uint32_t algo_size(int algo) { return 4u * a5x_algo_words(algo); }  // (4, 8, 9..15 and 23..31 are unassigned)
// no salted mode: NTLM and the nested algorithms
inline bool algo_unsalted(int algo) { return algo == A5X_ALGO_NTLM || a5x_algo_nested(algo); }
// the salted nested algorithms 32..38 (a5x_salt_nest.h) and the HMAC algorithms 48..55 (a5x_hmac.h):
// salted sets only, each with its own salt order and its own salt records; the PBKDF2 algorithms
// 72..75 (a5x_pbkdf2.h) likewise, as iterated sets (a5x_set_iterated_targets), order 0
inline bool algo_salted_only(int algo) { return a5x_algo_salt_nested(algo) || a5x_algo_hmac(algo) || a5x_algo_pbkdf2(algo); }
// that order (a5x_algo_salt_order); -1: not such an algorithm
inline int salted_only_order(int algo) {
  return a5x_algo_pbkdf2(algo) ? A5X_SALT_ORDER_PASS_SALT : a5x_algo_hmac(algo) ? hmac_order(algo) : snest_order(algo);
}
// u32 per record of a salted set's device salt table, by the set's kind
inline uint32_t salt_stride(int algo) {
  return a5x_algo_hmac(algo) ? A5X_HMAC_STRIDE : a5x_algo_salt_nested(algo) ? A5X_SNEST_STRIDE : A5X_SALT_STRIDE;
}
// the stream kernel of a salted set, by the algorithm its salt records were built for
inline hipError_t launch_salted(int rec_algo, const A5xSaltLaunch& SL, int op, uint32_t cus, hipStream_t st) {
  return a5x_algo_pbkdf2(rec_algo) ? hipErrorInvalidValue  // (an iterated set has no stream kernel: iter_stream)
       : a5x_algo_hmac(rec_algo) ? a5x_launch_hmac_stream(SL, op, cus, st)
       : a5x_algo_salt_nested(rec_algo) ? a5x_launch_salt_nest_stream(SL, op, cus, st)
                                        : a5x_launch_salt_stream(SL, op, cus, st);
}
// the fused expansion kernel that hashes a narrow plain algorithm (a5x_launch_expand's kind):
// k_expand_fast_md5 / k_expand_fast_ntlm; -1: none (wide and nested sets never get here,
// expand_digest sends them to the two-pass route)
inline int fused_kind(int algo) { return algo == A5X_ALGO_MD5 ? 3 : algo == A5X_ALGO_NTLM ? 5 : -1; }

// the context's sorted unique wide digests, in place
template <size_t W>
void sort_unique_digests(std::vector<uint8_t>& v) {
  struct E { uint8_t b[W]; };
  E* p = (E*)v.data();
  const size_t n = v.size() / W;
  std::sort(p, p + n, [](const E& x, const E& y) { return memcmp(x.b, y.b, W) < 0; });
  E* e = std::unique(p, p + n, [](const E& x, const E& y) { return memcmp(x.b, y.b, W) == 0; });
  v.resize((size_t)(e - p) * W);
}

// The target set as a5x_set_targets uploads it, built on the host from n digests of W
// bytes: the prefilter bitmap, the open-addressing table of the first 16 bytes, the tail
// words per slot and of the zero-prefix targets (wide digests), and the sorted unique
// digests a5x_hit_digest answers from.
struct TargetSet {
  uint32_t bm_log2 = 0, has_zero = 0;
  uint64_t tmask = 0;
  std::vector<uint32_t> bm, tails, ztails;
  std::vector<uint4> tab;
  std::vector<uint8_t> full;
  bool shared = false;  // two digests share their first 16 bytes
};
// (full_src: the digests the host copy is made of when dig holds masked keys, a5x_set_salted_targets)
void build_target_set(uint32_t W, const uint8_t* dig, uint64_t n, TargetSet& T, const uint8_t* full_src = nullptr) {
  // prefilter: >= 64 bits per target (false-positive rate <= 1/64), table: load <= 1/2
  uint32_t bm_log2 = 16;
  const uint32_t TW = W / 4 - 4;  // tail words
  while (bm_log2 < 32 && (1ull << bm_log2) < n * 64) bm_log2++;
  // (test hook: force the prefilter size, e.g. the 2^32-bit filter of > 2^26 targets)
  if (const char* e = getenv("A5X_TARGET_BM_LOG2")) bm_log2 = std::max(16u, std::min(32u, (uint32_t)atoi(e)));
  uint64_t tsz = 16;
  while (tsz < 2 * n) tsz <<= 1;
  std::vector<uint32_t>& bm = T.bm;
  std::vector<uint4>& tab = T.tab;
  bm.assign((1ull << bm_log2) / 32, 0);
  tab.resize(tsz);
  memset(tab.data(), 0, tsz * sizeof(uint4));
  // wide digests: the words past the first four, per slot; the zero-prefix targets' tails
  std::vector<uint32_t>&tails = T.tails, &ztails = T.ztails;
  tails.assign(TW ? tsz * TW : 0, 0);
  ztails.clear();
  uint32_t has_zero = 0;
  const uint64_t tmask = tsz - 1;
  for (uint64_t i = 0; i < n; i++) {
    uint32_t d[16];
    memcpy(d, dig + (uint64_t)W * i, W);
    if ((d[0] | d[1] | d[2] | d[3]) == 0) {
      has_zero = 1;
      ztails.insert(ztails.end(), d + 4, d + 4 + TW);
      continue;
    }
    const uint32_t bi = d[0] & (uint32_t)((1ull << bm_log2) - 1);
    const uint64_t m = md_bloom_bits(d[3]);  // (a5x_md.h md_prefilter: the 64-bit word of bi, two bits from word 3)
    bm[(bi >> 6) * 2] |= (uint32_t)m;
    bm[(bi >> 6) * 2 + 1] |= (uint32_t)(m >> 32);
    for (uint64_t slot = tgt_slot(d, tmask);; slot = (slot + 1) & tmask) {
      uint4& e = tab[slot];
      if (e.x == d[0] && e.y == d[1] && e.z == d[2] && e.w == d[3] &&
          (!TW || memcmp(&tails[slot * TW], d + 4, 4 * TW) == 0))
        break;  // duplicate (an equal prefix with another tail takes a slot of its own)
      if ((e.x | e.y | e.z | e.w) == 0) {
        e = make_uint4(d[0], d[1], d[2], d[3]);
        if (TW) memcpy(&tails[slot * TW], d + 4, 4 * TW);
        break;
      }
    }
  }
  // the host copy a5x_hit_digest answers from (wide algorithms only)
  std::vector<uint8_t>& full = T.full;
  full.clear();
  bool shared = false;
  if (TW) {
    const uint8_t* fs = full_src ? full_src : dig;
    full.assign(fs, fs + (uint64_t)W * n);
    switch (W) {
      case 20: sort_unique_digests<20>(full); break;
      case 28: sort_unique_digests<28>(full); break;
      case 32: sort_unique_digests<32>(full); break;
      case 48: sort_unique_digests<48>(full); break;
      default: sort_unique_digests<64>(full); break;
    }
    for (size_t i = 1; i < full.size() / W && !shared; i++)
      shared = memcmp(&full[(i - 1) * W], &full[i * W], 16) == 0;
  }
  T.bm_log2 = bm_log2;
  T.has_zero = has_zero;
  T.tmask = tmask;
  T.shared = shared;
}

// The full digest of a hit (a5x_hit_digest): narrow algorithms, the hit's own bytes; wide
// ones, the target with the hit's first 16 bytes -- and where several targets share them,
// the one whose tail the latest expand_digest call recorded for the hit's (word, cand).
int hit_full_digest(a5x_ctx* c, const a5x_hit* h, uint8_t* out) {
  const uint32_t W = algo_size(c->t_algo);
  if (W == 16) {
    memcpy(out, h->digest, 16);
    return A5X_OK;
  }
  const size_t n = c->t_full.size() / W;
  const uint8_t* base = c->t_full.data();
  size_t lo = 0, hi = n;  // first digest with prefix >= the hit's
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (memcmp(base + mid * W, h->digest, 16) < 0) lo = mid + 1; else hi = mid;
  }
  size_t e = lo;
  while (e < n && memcmp(base + e * W, h->digest, 16) == 0) e++;
  if (e == lo) return fail(c, A5X_E_ARG, "no target with the hit's first 16 digest bytes");
  if (e - lo > 1) {
    const auto it = c->t_hit_tails.find(std::make_pair(h->word, h->cand));
    if (it == c->t_hit_tails.end())
      return fail(c, A5X_E_ARG, "%zu targets share the hit's first 16 digest bytes and the hit is not one of the latest call's",
                  e - lo);
    for (; lo < e; lo++)
      if (memcmp(base + lo * W + 16, it->second.data(), W - 16) == 0) break;
    if (lo == e) return fail(c, A5X_E_ARG, "no target with the hit's digest");
  }
  memcpy(out, base + lo * W, W);
  return A5X_OK;
}

uint32_t dig_grid(a5x_ctx* c) { return (uint32_t)std::max(1, c->cus) * 8u; }

// the per-block arrays of a stream of nblk blocks (dg_blk_cnt, dg_blk_pre) and their scan's scratch
int grow_blocks(a5x_ctx* c, uint64_t nblk) {
  int rc;
  if ((rc = grow(c, c->dg_blk_cnt, nblk + 1)) || (rc = grow(c, c->dg_blk_pre, nblk + 1)) ||
      (rc = grow(c, c->scan_tmp, a5x_scan_tmp_elems(nblk + 1) + 16)))
    return rc;
  return A5X_OK;
}

// Line starts per stream block and their exclusive scan (dg_blk_pre, nblk + 1 entries), for any
// of the three stream kernels: launch_op1() runs the route's op 1 into dg_blk_cnt, which is
// grown here first.  lines (null: not wanted): the stream's line count, read back.
template <class F>
int stream_count_lines(a5x_ctx* c, F launch_op1, uint64_t nblk, hipStream_t st, uint64_t* lines) {
  int rc;
  if ((rc = grow_blocks(c, nblk))) return rc;
  HIPCHK(c, launch_op1());
  HIPCHK(c, a5x_launch_scan(c->dg_blk_cnt.p, c->dg_blk_cnt.p, nblk, c->dg_blk_pre.p, c->dg_blk_pre.p, c->scan_tmp.p,
                            c->d_scalars + S_ERR, st));
  if (lines) {
    HIPCHK(c, hipMemcpyAsync(c->h_totals + T_LINES, c->dg_blk_pre.p + nblk, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *lines = c->h_totals[T_LINES];
  }
  return A5X_OK;
}

// the plain route's: D.blk_cnt / D.blk_pre set for op 2 and the hit resolve
int dig_block_prefix(a5x_ctx* c, A5xDigLaunch& D, hipStream_t st, uint64_t* total_lines) {
  auto op1 = [&] {
    D.blk_cnt = c->dg_blk_cnt.p;
    return a5x_launch_digest_stream(D, 1, dig_grid(c), st);
  };
  const int rc = stream_count_lines(c, op1, a5x_digest_blocks(D.nbytes, D.algo), st, total_lines);
  D.blk_pre = c->dg_blk_pre.p;
  return rc;
}

// a5x_digest_lines_rules_device / a5x_digest_lines_salted_device behind their argument checks:
// op 1, the capacity check for per_line digests a line, op 2, and the route's device counter
// (r_counter, grown by the caller) read back into *counter.  Q holds the route's own fields,
// Q.d is filled here; launch(op) runs the route's kernel on Q.
template <class L, class F>
int digest_lines_multi(a5x_ctx* c, L& Q, F launch, int algo, const uint8_t* d_lines, uint64_t nbytes, uint8_t* d_dig,
                       uint64_t cap, uint32_t per_line, const char* unit, uint64_t* n_lines, hipStream_t st,
                       uint64_t* lines, unsigned long long* counter) {
  int rc;
  HIPCHK(c, hipMemsetAsync(c->d_scalars, 0, S_GUARD * sizeof(uint32_t), st));  // the counters before the guard record
  HIPCHK(c, hipMemsetAsync(c->r_counter.p, 0, 8, st));
  Q.d = dig_launch(c);
  Q.d.algo = algo;
  Q.d.out = d_lines;
  Q.d.nbytes = nbytes;
  auto op1 = [&] {
    Q.d.blk_cnt = c->dg_blk_cnt.p;
    return launch(1);
  };
  if ((rc = stream_count_lines(c, op1, a5x_stream_blocks(nbytes), st, lines))) return rc;
  if (n_lines) *n_lines = *lines;
  if (*lines > cap / per_line || !d_dig)
    return fail(c, A5X_E_CAPACITY, "%llu lines x %u %s, digest buffer has room for %llu", (unsigned long long)*lines,
                per_line, unit, (unsigned long long)cap);
  Q.d.blk_cnt = nullptr;
  Q.d.blk_pre = c->dg_blk_pre.p;
  Q.d.dig_out = d_dig;
  HIPCHK(c, launch(2));
  HIPCHK(c, read_scalars(c, st, S_ERR));
  HIPCHK(c, hipMemcpyAsync(counter, c->r_counter.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return A5X_OK;
}

static_assert(sizeof(a5x_hit) == sizeof(A5xHitRaw), "resolved device hits are copied out as a5x_hit");

// The item range [*i0, *i1) of the -r / -s engines holding candidates [cb, ce) (ce <= the
// batch's count, cb < ce): the words of cb and ce - 1 from k_word_of, their first items.
int mode_item_bounds(a5x_ctx* c, const Job& J, uint64_t cb, uint64_t ce, uint64_t* i0, uint64_t* i1) {
  int rc;
  if ((rc = grow(c, c->loc_q, 2)) || (rc = grow(c, c->loc_r, 4))) return rc;
  const uint64_t q[2] = {cb, ce - 1};
  HIPCHK(c, hipMemcpyAsync(c->loc_q.p, q, 16, hipMemcpyHostToDevice, J.st));
  HIPCHK(c, a5x_launch_word_of(J.B.cand_off, J.nw, c->loc_q.p, 2, c->loc_r.p, c->loc_r.p + 2, J.st));
  uint64_t wc[4], so[2];
  HIPCHK(c, hipMemcpyAsync(wc, c->loc_r.p, 32, hipMemcpyDeviceToHost, J.st));
  HIPCHK(c, hipStreamSynchronize(J.st));
  for (int k = 0; k < 2; k++) {
    if (wc[k] >= J.nw) return fail(c, A5X_E_ARG, "candidate %llu past the batch", (unsigned long long)q[k]);
    HIPCHK(c, hipMemcpyAsync(&so[k], c->m_seg_off.p + wc[k], 8, hipMemcpyDeviceToHost, J.st));
  }
  HIPCHK(c, hipStreamSynchronize(J.st));
  *i0 = so[0] + wc[2] / c->mseg;
  *i1 = so[1] + wc[3] / c->mseg + 1;
  return A5X_OK;
}

// ---------------------------------------------------------------------------
// The digest routes.  expand_digest prepares the batch and picks one of three: the fused
// -r / -s / -s -r route, the fused default route (with its hybrid sub-batch), the two-pass
// range loop.  They share the hit buffer (HitBuf, hits_run), the target-set fields of their
// launches (target_fields_into) and the way a call ends (digest_finish).
// ---------------------------------------------------------------------------

// One expand_digest call behind its keyspace: the candidates [rb, re) of the job's batch
// (clipped to it) and what the caller gave for the answer.
struct DigestCall {
  uint64_t rb, re;
  uint64_t scratch_bytes;
  a5x_hit* hits;
  uint64_t hit_cap;
  uint64_t* n_hits;
  a5x_stats* stats;
  uint64_t count() const { return re - rb; }  // the candidates this call digests
};

int expand_digest(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode, int mn, int mx,
                  uint64_t rb, uint64_t re, uint64_t scratch_bytes, a5x_hit* hits, uint64_t hit_cap,
                  uint64_t* n_hits, a5x_stats* stats, hipStream_t st, bool allow_fused, uint64_t trim = 0);

// The device hit buffer of one digest call: dg_hits, and on the two-pass route the arrays that
// hold one record per hit beside it.  A launch counts every hit in S_NHITS and stores the
// first n of them.
struct HitBuf {
  uint64_t n = 0;                    // entries
  uint32_t tail_words = 0;           // two-pass, wide set: dg_hit_tail words per entry (0: no tails)
  DevBuf<uint32_t>* side = nullptr;  // two-pass, rules / salts: dg_hit_rule / dg_hit_salt, one index per entry
  bool flags_full = false;           // two-pass: the stream kernels flag a full buffer in S_ERR (STREAM_ERR_HITCAP)
};

int hits_resize(a5x_ctx* c, HitBuf& H, uint64_t n) {
  int rc;
  if ((rc = grow(c, c->dg_hits, n))) return rc;
  if (H.tail_words && (rc = grow(c, c->dg_hit_tail, (uint64_t)H.tail_words * n))) return rc;
  if (H.side && (rc = grow(c, *H.side, n))) return rc;
  H.n = n;
  return A5X_OK;
}

// the buffer's first size: the caller's, between 1024 and 2^20 entries
int hits_open(a5x_ctx* c, HitBuf& H, uint64_t hit_cap) {
  return hits_resize(c, H, std::max<uint64_t>(1024, std::min<uint64_t>(hit_cap, 1u << 20)));
}

// Runs run() until its hits fit the buffer.  Each turn clears S_NHITS, then run() queues the
// route's launch, brings the scalars back ([0, S_NHITS] at least), synchronises and checks the
// error word; *nh is the launch's hit count.  With more hits than entries, regrow(*nh) is the
// route's rule: the size to run again with, or one no larger than the buffer to stop.
template <class Run, class Regrow>
int hits_run(a5x_ctx* c, hipStream_t st, HitBuf& H, uint64_t* nh, Run run, Regrow regrow) {
  int rc;
  for (;;) {
    HIPCHK(c, hipMemsetAsync(c->d_scalars + S_NHITS, 0, sizeof(uint32_t), st));
    if ((rc = run())) return rc;
    *nh = c->h_scalars[S_NHITS];
    const uint64_t n = *nh > H.n ? regrow(*nh) : 0;
    if (n <= H.n) return A5X_OK;
    if ((rc = hits_resize(c, H, n))) return rc;
    if (H.flags_full) HIPCHK(c, hipMemsetAsync(c->d_scalars + S_ERR, 0, sizeof(uint32_t), st));
  }
}

// the target set and the hit buffer into the dg_* fields of an expansion or mode-engine launch
template <class L>
void target_fields_into(a5x_ctx* c, L& X, const HitBuf& H) {
  const A5xDigLaunch D = dig_launch(c);
  X.dg_bitmap = D.bitmap; X.dg_bm_mask = D.bm_mask; X.dg_has_zero = D.has_zero_target;
  X.dg_table = D.table; X.dg_tmask = D.tmask;
  X.dg_hits = c->dg_hits.p; X.dg_hit_cap = (uint32_t)H.n; X.dg_nhits = c->d_scalars + S_NHITS;
}

// The hits of a fused route: launch(H) queues the route's kernels between ev[1] and ev[2], as
// often as hits_run asks.  The fused kernels write (word, candidate) hits and never flag a
// full buffer, so the error word is checked whole, and a second run has room for every hit the
// caller takes: min(found, hit_cap), which stops once the buffer has hit_cap entries.
// *ms: the last run's time; *take: the hits copied to the caller, the first of *nh found.
template <class Launch>
int fused_hits(a5x_ctx* c, hipStream_t st, const DigestCall& Q, Launch launch, uint64_t* nh, uint64_t* take,
               float* ms) {
  int rc;
  HitBuf H;
  if ((rc = hits_open(c, H, Q.hit_cap))) return rc;
  auto run = [&]() -> int {
    int rc;
    if ((rc = launch(H))) return rc;
    HIPCHK(c, read_scalars(c, st, S_NHITS));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev[1], c->ev[2]));
    return decode_dev_err(c, c->h_scalars[S_ERR]);
  };
  if ((rc = hits_run(c, st, H, nh, run, [&](uint64_t found) { return std::min(found, Q.hit_cap); }))) return rc;
  *take = std::min(std::min(*nh, H.n), Q.hit_cap);
  if (*take) {
    HIPCHK(c, hipMemcpyAsync(Q.hits, c->dg_hits.p, *take * sizeof(a5x_hit), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  return A5X_OK;
}

a5x_stats digest_stats(const Job& J, const DigestCall& Q) {
  a5x_stats s;
  memset(&s, 0, sizeof s);
  s.words = J.nw;
  s.candidates = Q.count();
  return s;
}

// how every route ends: the hit count, the stats, and A5X_E_CAPACITY for hits the caller's buffer had no room for
int digest_finish(a5x_ctx* c, const DigestCall& Q, uint64_t found, const a5x_stats& total) {
  if (Q.n_hits) *Q.n_hits = found;
  if (Q.stats) *Q.stats = total;
  if (found > Q.hit_cap)
    return fail(c, A5X_E_CAPACITY, "%llu hits, buffer has %llu", (unsigned long long)found,
                (unsigned long long)Q.hit_cap);
  return A5X_OK;
}

// Fused -r / -s / -s -r route: every item's candidates hashed where the engine builds them
// (positional ring or byte-builder buffer), the FAST words' in k_expand_fast_md5 / _ntlm's
// ring; hits as (word, candidate) directly.  No output layout, so stats.bytes stays 0.
int digest_fused_modes(a5x_ctx* c, const Job& J, const DigestCall& Q) {
  int rc;
  const uint64_t tc = Q.count();
  uint64_t it0 = 0, it1 = c->m_items;  // the items holding [rb, re)
  const bool whole = Q.rb == 0 && Q.re == J.B.total_cands;
  if (!whole && tc && (rc = mode_item_bounds(c, J, Q.rb, Q.re, &it0, &it1))) return rc;
  auto launch = [&](const HitBuf& H) -> int {
    A5xModeLaunch M = mode_launch(c, J.w, J.wo, J.nw, J.mode, J.mn, J.mx, J.B.rfast);
    M.cand_off = J.B.cand_off;
    M.item_begin = it0;
    M.item_end = tc ? it1 : it0;
    M.cand_begin = Q.rb;
    M.cand_end = Q.re;
    M.dg_algo = c->t_algo;
    target_fields_into(c, M, H);
    HIPCHK(c, hipEventRecord(c->ev[1], J.st));
    M.grid_cap = J.B.nmode * 8 < J.nw ? 2048u : 0u;  // (as in job_launch)
    if (J.B.nmode && tc) HIPCHK(c, a5x_launch_mode_items(M, 2, J.st));
    if (J.B.rfast && tc) {
      A5xExpLaunch E = exp_launch_mode(c, J.w, J.wo, J.nw, J.mn, J.mx, J.B);
      E.cand_begin = Q.rb;
      E.cand_end = Q.re;
      target_fields_into(c, E, H);
      HIPCHK(c, a5x_launch_expand(E, fused_kind(c->t_algo), J.st));
    }
    HIPCHK(c, hipEventRecord(c->ev[2], J.st));
    return A5X_OK;
  };
  uint64_t nh = 0, take = 0;
  float ms = 0, ms_ks = 0;
  if ((rc = fused_hits(c, J.st, Q, launch, &nh, &take, &ms))) return rc;
  HIPCHK(c, hipEventElapsedTime(&ms_ks, c->ev[0], c->ev[1]));
  a5x_stats total = digest_stats(J, Q);
  total.expand_launches = 1;
  total.ms_keyspace = ms_ks;
  total.ms_expand = ms;  // build + digest + lookup, fused
  total.ms_total = ms_ks + ms;
  return digest_finish(c, Q, nh, total);
}

// The hybrid's sub-batch: the candidate-bearing words the fused kernel skipped (slow / BIG /
// pass G), in batch order, as a compact batch in the context's hybrid buffers (sized with
// grow(): no per-call allocation), through the two-pass route; its hits land behind the *take
// the caller already has, their word indices mapped back to the batch.
// Host memory touched with device-produced values: idx[] (sized by the device count m, itself
// bounded by nw) and the caller's hits[take, take + got) with got <= room.
int digest_hybrid_rest(a5x_ctx* c, const Job& J, const DigestCall& Q, uint64_t* take, uint64_t* nh, float* ms_sub) {
  int rc;
  const uint64_t nw = J.nw;
  if ((rc = grow(c, c->hy_list, std::max<uint64_t>(1, nw)))) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_scalars + S_NONFAST_N, 0, sizeof(uint32_t), J.st));
  HIPCHK(c, a5x_launch_nonfast_list(c->flags.p, J.B.cand_off, nw, Q.rb, Q.re, c->hy_list.p,
                                    c->d_scalars + S_NONFAST_N, J.st));
  HIPCHK(c, hipMemcpyAsync(c->h_scalars + S_NONFAST_N, c->d_scalars + S_NONFAST_N, sizeof(uint32_t),
                           hipMemcpyDeviceToHost, J.st));
  HIPCHK(c, hipStreamSynchronize(J.st));
  const uint32_t m = c->h_scalars[S_NONFAST_N];
  if (m > nw) return fail(c, A5X_E_HIP, "non-FAST word list of %u words in a batch of %llu", m, (unsigned long long)nw);
  std::vector<uint32_t> idx(m);
  std::vector<uint64_t> off((size_t)m + 1, 0);
  if ((rc = grow(c, c->hy_lens, (size_t)m + 1)) || (rc = grow(c, c->hy_off, (size_t)m + 1))) return rc;
  if (m) {
    HIPCHK(c, hipMemcpyAsync(idx.data(), c->hy_list.p, (size_t)m * 4, hipMemcpyDeviceToHost, J.st));
    HIPCHK(c, hipStreamSynchronize(J.st));
    std::sort(idx.begin(), idx.end());
    HIPCHK(c, hipMemcpyAsync(c->hy_list.p, idx.data(), (size_t)m * 4, hipMemcpyHostToDevice, J.st));
    HIPCHK(c, a5x_launch_gather_words(J.w, J.wo, c->hy_list.p, m, c->hy_lens.p, nullptr, nullptr, J.st));
    HIPCHK(c, hipMemcpyAsync(off.data() + 1, c->hy_lens.p, (size_t)m * 8, hipMemcpyDeviceToHost, J.st));
    HIPCHK(c, hipStreamSynchronize(J.st));
    for (uint32_t k = 0; k < m; k++) off[k + 1] += off[k];
  }
  if ((rc = grow(c, c->hy_words, off[m] + 16))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->hy_off.p, off.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, J.st));
  HIPCHK(c, hipMemsetAsync(c->hy_words.p, 0, off[m] + 16, J.st));
  HIPCHK(c, a5x_launch_gather_words(J.w, J.wo, c->hy_list.p, m, nullptr, c->hy_off.p, c->hy_words.p, J.st));
  // A word cut by [rb, re) (the first / last listed): only its part inside the range --
  // the sub-batch range drops the candidates before rb and after re.
  uint64_t sb = 0, se_cut = 0;
  if (m && !(Q.rb == 0 && Q.re == J.B.total_cands)) {
    uint64_t c0 = 0, c1 = 0;
    HIPCHK(c, hipMemcpyAsync(&c0, J.B.cand_off + idx[0], 8, hipMemcpyDeviceToHost, J.st));
    HIPCHK(c, hipMemcpyAsync(&c1, J.B.cand_off + idx[m - 1] + 1, 8, hipMemcpyDeviceToHost, J.st));
    HIPCHK(c, hipStreamSynchronize(J.st));
    sb = Q.rb > c0 ? Q.rb - c0 : 0;
    se_cut = c1 > Q.re ? c1 - Q.re : 0;
  }
  const uint64_t room = Q.hit_cap > *take ? Q.hit_cap - *take : 0;
  uint64_t nh2 = 0;
  a5x_stats st2;
  memset(&st2, 0, sizeof st2);
  // (allow_fused false: these words are exactly the ones the fused kernel skips)
  rc = expand_digest(c, c->hy_words.p, c->hy_off.p, m, J.mode, J.mn, J.mx, sb, ~0ull, Q.scratch_bytes,
                     room ? Q.hits + *take : nullptr, room, &nh2, &st2, J.st, false, se_cut);
  if (rc && rc != A5X_E_CAPACITY) return rc;
  const uint64_t got = std::min(nh2, room);
  for (uint64_t i = *take; i < *take + got; i++) {
    if (Q.hits[i].word >= m)
      return fail(c, A5X_E_HIP, "sub-batch hit word %llu of %u", (unsigned long long)Q.hits[i].word, m);
    Q.hits[i].word = idx[Q.hits[i].word];
  }
  *take += got;
  *nh += nh2;
  *ms_sub = st2.ms_total;
  return A5X_OK;
}

// Fused default route: k_expand_fast_md5 / k_expand_fast_ntlm hash each FAST word's candidates
// in the LDS ring where they are built -- no HBM scratch, no second pass, hits already
// (word, candidate).  The other candidate-bearing words follow as the hybrid's sub-batch.
int digest_fused_default(a5x_ctx* c, const Job& J, const DigestCall& Q) {
  int rc;
  auto launch = [&](const HitBuf& H) -> int {
    A5xExpLaunch E = exp_launch(c, J.w, J.wo, J.nw, J.mn, J.mx, J.B);
    E.cand_begin = Q.rb;
    E.cand_end = Q.re;
    target_fields_into(c, E, H);
    HIPCHK(c, hipEventRecord(c->ev[1], J.st));
    HIPCHK(c, a5x_launch_expand(E, fused_kind(c->t_algo), J.st));
    HIPCHK(c, hipEventRecord(c->ev[2], J.st));
    return A5X_OK;
  };
  uint64_t nh = 0, take = 0;
  float ms = 0, ms_ks = 0, ms_sub = 0;
  if ((rc = fused_hits(c, J.st, Q, launch, &nh, &take, &ms))) return rc;
  HIPCHK(c, hipEventElapsedTime(&ms_ks, c->ev[0], c->ev[1]));  // this batch's keyspace, before the sub-batch reuses the events
  if ((J.B.nslow || J.B.nbig || J.B.nglob) && (rc = digest_hybrid_rest(c, J, Q, &take, &nh, &ms_sub))) return rc;
  a5x_stats total = digest_stats(J, Q);
  total.bytes = J.B.total_bytes;
  total.expand_launches = 1;
  total.ms_keyspace = ms_ks;
  total.ms_expand = ms + ms_sub;  // expansion + digest + lookup: fused (+ the two-pass sub-batch)
  total.ms_total = ms_ks + ms + ms_sub;
  return digest_finish(c, Q, nh, total);
}


// ---- iterated sets (a5x_pbkdf2.hip) --------------------------------------------------------
// The defaults of a pass and of a loop launch.  IT_SLOTS pair slots: at 55 state words a pair
// (SHA-512) 220 MiB of state, and more than five rounds of the 196608 lanes the device holds.
// IT_PAIR_ITERS pair-iterations bound the time of one loop launch (DESIGN "Iterated target
// lists" has the measured times).
constexpr uint64_t IT_SLOTS = 1ull << 20;
constexpr uint64_t IT_PAIR_ITERS = 1ull << 30;

// The passes of a stream whose line starts are counted and scanned (L.s.d.blk_pre = dg_blk_pre,
// nblk + 1 entries): blocks are taken while their lines, rounded up to a wave, fit the pass's
// slots under every salt record; a run of blocks that does not -- at the least one block, so a
// pass may exceed a budget smaller than a block's lines under one record -- is taken under a
// slice of the records at a time.  Per pass: init, the loop launches of at most slice =
// max(1, B / pairs) iterations up to the largest count of the pass's records, then per_pass(L)
// (the compare step, as often as it likes: the iterations never run again).
template <class PerPass>
int iter_stream(a5x_ctx* c, A5xPbkdf2Launch& L, uint64_t nblk, hipStream_t st, PerPass per_pass) {
  int rc;
  const uint32_t S = c->n_salts, sw = pbkdf2_state_words(c->t_algo);
  const uint64_t P = c->it_slots ? c->it_slots : IT_SLOTS, B = c->it_pair_iters ? c->it_pair_iters : IT_PAIR_ITERS;
  const uint32_t cus = (uint32_t)std::max(1, c->cus);
  std::vector<uint64_t> pre(nblk + 1);
  HIPCHK(c, hipMemcpyAsync(pre.data(), c->dg_blk_pre.p, (nblk + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  auto slots = [](uint64_t lines) { return (lines + 63) & ~63ull; };
  for (uint64_t b0 = 0; b0 < nblk;) {
    uint64_t b1 = b0 + 1;
    while (b1 < nblk && slots(pre[b1 + 1] - pre[b0]) * S <= P) b1++;
    const uint64_t lines = pre[b1] - pre[b0];
    if (lines > 0xffffffc0ull) return fail(c, A5X_E_UNSUPPORTED, "more lines in a pass than slots can be numbered");
    const uint32_t np = (uint32_t)slots(lines);
    const uint32_t ns = np ? (uint32_t)std::min<uint64_t>(S, std::max<uint64_t>(1, P / np)) : S;
    for (uint32_t s0 = 0; lines && s0 < S; s0 += ns) {
      L.b0 = b0; L.b1 = b1; L.np = np;
      L.s0 = s0; L.s1 = std::min(S, s0 + ns);
      L.pairs = (uint64_t)(L.s1 - L.s0) * np;
      if ((rc = grow(c, c->it_state, L.pairs * sw))) return rc;
      L.state = c->it_state.p;
      HIPCHK(c, hipMemsetAsync(L.state + L.pairs, 0xff, L.pairs * 4, st));  // word 1 of every slot: no pair yet
      HIPCHK(c, a5x_launch_pbkdf2_init(L, 0, cus, st));
      uint32_t cmax = 1;
      for (uint32_t k = L.s0; k < L.s1; k++)
        cmax = std::max(cmax, c->s_recs[(size_t)k * A5X_PBKDF2_STRIDE + A5X_PBKDF2_R_ITERS]);
      const uint64_t slice = std::max<uint64_t>(1, B / L.pairs);
      for (uint64_t k0 = 1; k0 < cmax; k0 += slice) {
        L.k0 = (uint32_t)k0;
        L.k1 = (uint32_t)std::min<uint64_t>(cmax, k0 + slice);
        HIPCHK(c, a5x_launch_pbkdf2_loop(L, st));
        c->it_launches++;
      }
      if ((rc = per_pass(L))) return rc;
    }
    b0 = b1;
  }
  return A5X_OK;
}

// Two-pass route, the range loop: each range of at most scratch_bytes is expanded into HBM
// scratch (job_launch), then a stream kernel hashes its lines -- k_digest_stream, with rules
// k_rules_stream, with a salted set k_salt_stream.  Hits are (block, ordinal) until
// k_hits_resolve.  A range's candidates stay in scratch, so a range with more hits than the
// device buffer is digested again with room for all of them -- unless the caller's buffer is
// full already, when only the count matters.
int digest_two_pass(a5x_ctx* c, const Job& J, const DigestCall& Q) {
  int rc;
  const bool wide = c->t_tw != 0, ruled = c->n_rules != 0, salted = c->salted;
  const bool iterated = salted && a5x_algo_pbkdf2(c->t_algo);  // passes of pairs instead of one stream launch
  const uint64_t nw = J.nw, hit_cap = Q.hit_cap;
  a5x_hit* const hits = Q.hits;
  uint64_t cap = Q.scratch_bytes ? Q.scratch_bytes : ((uint64_t)2 << 30);
  cap = std::max<uint64_t>(4096, std::min<uint64_t>(cap, J.B.total_bytes + 64));
  std::vector<Range> ranges;
  if ((rc = plan_ranges(c, J, cap, ranges, Q.rb, Q.re))) return rc;
  if ((rc = grow(c, c->dg_scratch, cap + 64))) return rc;
  // The set's kind, chosen here once: the tail words the kernels record per hit, the rule / salt
  // index of every hit (device array beside the hit buffer, and the context's copy), and below
  // the launch of the kind's op 0 kernel
  const uint32_t HT = a5x_hit_tail_stride(c->t_algo);
  DevBuf<uint32_t>* const side = ruled ? &c->dg_hit_rule : salted ? &c->dg_hit_salt : nullptr;
  std::vector<uint32_t>& side_host = ruled ? c->r_hit_rule : c->s_hit_salt;
  HitBuf H;
  H.tail_words = wide ? HT : 0;
  H.side = side;
  H.flags_full = true;
  // (an iterated set: a pass's hits are few against its work and a second run costs only the
  // compare step, so its buffer starts at the floor whatever the caller's)
  if ((rc = iterated ? hits_resize(c, H, 1024) : hits_open(c, H, hit_cap))) return rc;
  if (side && (rc = grow(c, c->r_counter, 2))) return rc;
  auto launch_op0 = [&](const A5xDigLaunch& D) -> hipError_t {
    const uint32_t cus = (uint32_t)std::max(1, c->cus);
    if (ruled) {
      const A5xRuleLaunch RL = {D, c->r_table.p, c->n_rules, side->p, c->r_counter.p};
      return a5x_launch_rules_stream(RL, 0, cus, J.st);
    }
    if (salted) {  // (an empty salted set has no salt to hash under: no launch, no hit)
      const A5xSaltLaunch SL = {D, c->s_table.p, c->n_salts, c->s_order, side->p, c->r_counter.p};
      if (!c->n_salts) return hipSuccess;
      // (by the set's algorithm: its salt records are a5x_salt.h's, a5x_salt_nest.h's or a5x_hmac.h's)
      return launch_salted(c->t_algo, SL, 0, cus, J.st);
    }
    return a5x_launch_digest_stream(D, 0, dig_grid(c), J.st);
  };
  std::vector<uint32_t> htail;  // wide: the range's hit tails
  a5x_stats total = digest_stats(J, Q);
  total.bytes = J.B.total_bytes;
  uint64_t found = 0, copied = 0;
  float ms_exp = 0, ms_dig = 0, ms_ks = 0;
  HIPCHK(c, hipEventRecord(c->ev[3], J.st));  // the keyspace (and the range plan) ends here
  HIPCHK(c, hipEventSynchronize(c->ev[3]));
  HIPCHK(c, hipEventElapsedTime(&ms_ks, c->ev[0], c->ev[3]));
  for (const Range& R : ranges) {
    HIPCHK(c, hipEventRecord(c->ev[1], J.st));
    if ((rc = job_launch(c, J, R, c->dg_scratch.p, cap))) return rc;
    HIPCHK(c, hipEventRecord(c->ev[2], J.st));
    A5xDigLaunch D = dig_launch(c);
    D.out = c->dg_scratch.p;
    D.nbytes = R.b1 - R.b0;
    const uint64_t nblk = side ? a5x_stream_blocks(D.nbytes) : a5x_digest_blocks(D.nbytes, D.algo);
    if ((rc = grow_blocks(c, nblk))) return rc;
    D.blk_cnt = c->dg_blk_cnt.p;
    uint64_t nh = 0;
    unsigned long long rej = 0;  // ruled: the range's lines longer than A5X_RULE_LMAX; salted: its skipped pairs
    {
      float me = 0;  // the range's expansion, once (a second run below re-runs only the digest)
      HIPCHK(c, hipEventSynchronize(c->ev[2]));
      HIPCHK(c, hipEventElapsedTime(&me, c->ev[1], c->ev[2]));
      ms_exp += me;
    }
    auto digest = [&]() -> int {
      D.hits = c->dg_hits.p;
      D.hit_tail = wide ? c->dg_hit_tail.p : nullptr;
      D.hit_cap = (uint32_t)H.n;
      D.nhits = c->d_scalars + S_NHITS;
      if (side) HIPCHK(c, hipMemsetAsync(c->r_counter.p, 0, 8, J.st));
      HIPCHK(c, hipEventRecord(c->dev_ev[0], J.st));
      HIPCHK(c, launch_op0(D));
      HIPCHK(c, hipEventRecord(c->dev_ev[1], J.st));
      HIPCHK(c, read_scalars(c, J.st, S_NHITS));
      if (side) HIPCHK(c, hipMemcpyAsync(&rej, c->r_counter.p, 8, hipMemcpyDeviceToHost, J.st));
      HIPCHK(c, hipStreamSynchronize(J.st));
      float md = 0;
      HIPCHK(c, hipEventElapsedTime(&md, c->dev_ev[0], c->dev_ev[1]));
      ms_dig += md;
      return decode_dev_err(c, c->h_scalars[S_ERR] & ~(1u << 10));  // (STREAM_ERR_HITCAP is hits_run's business)
    };
    // the hits of one hits_run out of the device buffer: resolved to (word, candidate) and copied
    // to the caller behind those already there
    auto deliver = [&]() -> int {
      if (!nh) return A5X_OK;
      const uint64_t got = std::min<uint64_t>(nh, H.n);
      HIPCHK(c, a5x_launch_scan(c->dg_blk_cnt.p, c->dg_blk_cnt.p, nblk, c->dg_blk_pre.p, c->dg_blk_pre.p,
                                c->scan_tmp.p, c->d_scalars + S_ERR, J.st));
      HIPCHK(c, a5x_launch_hits_resolve(c->dg_hits.p, (uint32_t)got, c->dg_blk_pre.p, R.cb, c->dg_cand_off.p, nw,
                                        J.st));
      const uint64_t take = std::min(hit_cap - std::min(hit_cap, copied), got);
      if (take)
        HIPCHK(c, hipMemcpyAsync(hits + copied, c->dg_hits.p, take * sizeof(a5x_hit), hipMemcpyDeviceToHost, J.st));
      if (take && c->t_shared_prefix) {
        htail.resize(HT * take);
        HIPCHK(c, hipMemcpyAsync(htail.data(), c->dg_hit_tail.p, take * 4 * HT, hipMemcpyDeviceToHost, J.st));
      }
      if (take && side) {
        side_host.resize(copied + take);
        HIPCHK(c, hipMemcpyAsync(side_host.data() + copied, side->p, take * 4, hipMemcpyDeviceToHost, J.st));
      }
      HIPCHK(c, hipStreamSynchronize(J.st));
      if (take && c->t_shared_prefix)  // (which of the targets sharing a prefix each hit matched: a5x_hit_digest)
        for (uint64_t k = 0; k < take; k++) {
          std::array<uint32_t, 12>& t = c->t_hit_tails[std::make_pair(hits[copied + k].word, hits[copied + k].cand)];
          t.fill(0u);
          memcpy(t.data(), &htail[HT * k], 4 * HT);
        }
      copied += take;
      found += nh;
      return A5X_OK;
    };
    if (iterated && c->n_salts) {
      // An iterated set: the range's line starts first (every pass needs the blocks' ordinals),
      // then pass by pass init, the loop launches and the compare step.  Each pass's hits are
      // taken out of the one hit buffer before the next pass's go in; when the buffer was too
      // small, hits_run repeats the compare step alone.
      A5xPbkdf2Launch L;
      memset(&L, 0, sizeof L);
      L.s = {D, c->s_table.p, c->n_salts, c->s_order, side->p, c->r_counter.p};
      HIPCHK(c, hipMemsetAsync(c->r_counter.p, 0, 8, J.st));
      auto op1 = [&] {
        L.b0 = 0; L.b1 = nblk;
        return a5x_launch_pbkdf2_init(L, 1, (uint32_t)std::max(1, c->cus), J.st);
      };
      if ((rc = stream_count_lines(c, op1, nblk, J.st, nullptr))) return rc;
      L.s.d.blk_pre = c->dg_blk_pre.p;
      HIPCHK(c, hipEventRecord(c->dev_ev[0], J.st));
      rc = iter_stream(c, L, nblk, J.st, [&](A5xPbkdf2Launch& Lp) -> int {
        int rc2;
        auto compare = [&]() -> int {
          Lp.s.d.hits = c->dg_hits.p;
          Lp.s.d.hit_cap = (uint32_t)H.n;
          Lp.s.d.nhits = c->d_scalars + S_NHITS;
          Lp.s.hit_salt = side->p;
          HIPCHK(c, a5x_launch_pbkdf2_compare(Lp, 0, J.st));
          HIPCHK(c, read_scalars(c, J.st, S_NHITS));
          HIPCHK(c, hipStreamSynchronize(J.st));
          return decode_dev_err(c, c->h_scalars[S_ERR] & ~(1u << 10));
        };
        if ((rc2 = hits_run(c, J.st, H, &nh, compare, [&](uint64_t n) { return copied >= hit_cap ? 0 : n; }))) return rc2;
        return deliver();
      });
      if (rc) return rc;
      HIPCHK(c, hipEventRecord(c->dev_ev[1], J.st));
      HIPCHK(c, hipMemcpyAsync(&rej, c->r_counter.p, 8, hipMemcpyDeviceToHost, J.st));
      HIPCHK(c, hipStreamSynchronize(J.st));
      float md = 0;
      HIPCHK(c, hipEventElapsedTime(&md, c->dev_ev[0], c->dev_ev[1]));
      ms_dig += md;
      nh = 0;  // (delivered pass by pass)
    } else if ((rc = hits_run(c, J.st, H, &nh, digest, [&](uint64_t n) { return copied >= hit_cap ? 0 : n; }))) {
      return rc;
    }
    if (salted) {
      const uint64_t pairs = (R.ce - R.cb) * c->n_salts;
      if (rej > pairs) return fail(c, A5X_E_HIP, "more skipped pairs than the range has");
      c->s_skipped += rej;
      c->s_hashed += pairs - rej;
    }
    if (ruled) {
      if (rej > R.ce - R.cb) return fail(c, A5X_E_HIP, "more rejected lines than the range has candidates");
      c->r_rejected += rej;
      c->r_hashed += (R.ce - R.cb - rej) * c->n_rules;
    }
    if ((rc = deliver())) return rc;
    total.expand_launches += 1;
  }
  total.ms_keyspace = ms_ks;
  total.ms_expand = ms_exp;
  total.ms_total = total.ms_keyspace + ms_exp + ms_dig;
  total.words_slow = J.B.nslow;
  total.words_pass_b = J.B.nbig;
  return digest_finish(c, Q, found, total);
}

// Expansion + digest + lookup of the batch's candidates [rb, re) (clipped to the batch;
// [0, ~0) = all, less the last trim): hits as (word, candidate in word).  allow_fused: the
// caller's wish (A5X_NO_FUSED_DIGEST; the hybrid's sub-batch passes false).
int expand_digest(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode, int mn, int mx,
                  uint64_t rb, uint64_t re, uint64_t scratch_bytes, a5x_hit* hits, uint64_t hit_cap,
                  uint64_t* n_hits, a5x_stats* stats, hipStream_t st, bool allow_fused, uint64_t trim) {
  int rc;
  // what the latest call's hits left in the context: the tails of hits on a shared prefix (wide
  // sets), each hit's rule and the rule counts, each hit's salt and the pair counts
  if (c->t_tw) c->t_hit_tails.clear();
  c->r_hit_rule.clear();
  c->r_rejected = c->r_hashed = 0;
  c->s_hit_salt.clear();
  c->s_hashed = c->s_skipped = 0;
  c->it_launches = 0;
  // The fused kernels hash plain MD5 and NTLM only.  The two-pass range loop in every mode for:
  // a wide set (SHA-1 and the SHA-2 family); a nested one (a5x_nest.h -- an MD5-outer one is not
  // wide, and the fused kernels would hash it as plain MD5); rules loaded (k_rules_stream); a
  // salted set (k_salt_stream, or k_salt_nest_stream for a salted nested one, whose MD5-outer
  // forms are not wide either; a5x_set_rules / a5x_set_salted_targets refuse the two together)
  if (c->t_tw || a5x_algo_nested(c->t_algo) || fused_kind(c->t_algo) < 0 || c->n_rules || c->salted) allow_fused = false;
  Job J{d_words, d_woff, nw, mode, mn, mx, st};
  J.lengths = mode == A5X_MODE_DEFAULT || !allow_fused;  // the fused -r / -s digest needs no layout
  if ((rc = grow(c, c->dg_cand_off, nw + 1)) || (rc = grow(c, c->dg_byte_off, nw + 1))) return rc;
  if ((rc = job_prepare(c, J, c->dg_cand_off.p, c->dg_byte_off.p, true))) return rc;  // (records ev[0])
  const uint64_t tc_all = J.B.total_cands;
  re = std::min(re, tc_all - std::min(trim, tc_all));  // (trim: candidates dropped at the end)
  rb = std::min(rb, re);
  const DigestCall Q{rb, re, scratch_bytes, hits, hit_cap, n_hits, stats};
  if (allow_fused && mode != A5X_MODE_DEFAULT) return digest_fused_modes(c, J, Q);
  if (allow_fused && Q.count() > 0) return digest_fused_default(c, J, Q);
  return digest_two_pass(c, J, Q);
}

// host words and offsets of a batch into the context's staging buffers (s_words, s_woff), on its stream
int stage_words(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw) {
  int rc;
  const uint64_t wbytes = nw ? woff[nw] : 0;
  if ((rc = grow(c, c->s_words, wbytes + 16)) || (rc = grow(c, c->s_woff, nw + 1))) return rc;
  if (wbytes) HIPCHK(c, hipMemcpyAsync(c->s_words.p, words, wbytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->s_woff.p, woff, (nw + 1) * 8, hipMemcpyHostToDevice, c->stream));
  return A5X_OK;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int a5x_abi_version(void) { return A5X_ABI_VERSION; }

// Why the calling thread's last a5x_create failed (no context exists to carry
// a5x_last_error): the failing HIP call and hipGetErrorString, or the argument problem.
static thread_local std::string g_create_err;

static int create_fail(int rc, const char* call, hipError_t e, int device) {
  char buf[256];
  if (e != hipSuccess)
    snprintf(buf, sizeof buf, "a5x_create(device=%d): %s failed: %s (hipError_t %d)", device, call,
             hipGetErrorString(e), (int)e);
  else
    snprintf(buf, sizeof buf, "a5x_create(device=%d): %s", device, call);
  g_create_err = buf;
  return rc;
}

int a5x_create(int device, a5x_ctx** out) {
  g_create_err.clear();
  if (!out) return create_fail(A5X_E_ARG, "null output pointer", hipSuccess, device);
  *out = nullptr;
  if (device == -1) {  // host-only context: tables, splitting, export (no GPU needed)
    a5x_ctx* c = new a5x_ctx();
    c->device = -1;
    *out = c;
    return A5X_OK;
  }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return create_fail(A5X_E_HIP, "hipGetDeviceCount", e, device);
  if (n <= 0) return create_fail(A5X_E_HIP, "hipGetDeviceCount found no device", hipSuccess, device);
  if (device < 0 || device >= n) {
    char msg[96];
    snprintf(msg, sizeof msg, "device out of range (%d visible)", n);
    return create_fail(A5X_E_ARG, msg, hipSuccess, device);
  }
  a5x_ctx* c = new a5x_ctx();
  c->device = device;
  if ((e = hipSetDevice(device)) != hipSuccess) {
    delete c;
    return create_fail(A5X_E_HIP, "hipSetDevice", e, device);
  }
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
    delete c;
    return create_fail(A5X_E_HIP, "hipStreamCreateWithFlags", e, device);
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    c->devname = std::string(prop.name) + " (" + prop.gcnArchName + ")";
    c->cus = prop.multiProcessorCount;
  }
  if (c->cus <= 0) c->cus = 256;
  const char* what = nullptr;
  if ((e = hipMalloc((void**)&c->d_scalars, S_ALLOC * sizeof(uint32_t))) != hipSuccess) what = "hipMalloc";
  else if ((e = hipHostMalloc((void**)&c->h_scalars, S_ALLOC * sizeof(uint32_t), 0)) != hipSuccess) what = "hipHostMalloc";
  else if ((e = hipHostMalloc((void**)&c->h_totals, T_ALLOC * sizeof(uint64_t), 0)) != hipSuccess) what = "hipHostMalloc";
  else if ((e = a5x_set_kernel_attrs()) != hipSuccess) what = "hipFuncSetAttribute";
  for (int i = 0; i < 4 && !what; i++)
    if ((e = hipEventCreate(&c->ev[i])) != hipSuccess) what = "hipEventCreate";
  for (int i = 0; i < 2 && !what; i++)
    if ((e = hipEventCreate(&c->dev_ev[i])) != hipSuccess) what = "hipEventCreate";
  if (what) {
    a5x_destroy(c);
    return create_fail(A5X_E_HIP, what, e, device);
  }
  if (const char* e = getenv("A5X_CHUNK")) c->chunk = std::max<uint64_t>(64, strtoull(e, nullptr, 10));
  // (< 2^24: k_keyspace_vsub packs a sub-word count <= mseg into 24 bits)
  if (const char* e = getenv("A5X_MSEG")) c->mseg = std::min<uint64_t>((1u << 24) - 1, std::max<uint64_t>(1, strtoull(e, nullptr, 10)));
  if (const char* e = getenv("A5X_SEG")) c->seg = std::max<uint64_t>(64, strtoull(e, nullptr, 10));
  // (tuning knobs; a5x_launch_expand clamps each launch to the kernel's compiled launch bound)
  if (const char* e = getenv("A5X_WAVES")) c->waves_per_block = std::max(1u, std::min(16u, (unsigned)atoi(e)));
  if (const char* e = getenv("A5X_FAST_WAVES")) c->waves_per_block_fast = std::max(1u, std::min(16u, (unsigned)atoi(e)));
  *out = c;
  return A5X_OK;
}

void a5x_destroy(a5x_ctx* c) {
  if (!c) return;
  if (c->device < 0) { delete c; return; }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  release(c->count); release(c->bytes); release(c->cand_off); release(c->byte_off); release(c->scan_tmp);
  release(c->locate); release(c->flags); release(c->defer); release(c->chunk_w0); release(c->slow_list); release(c->big_list);
  release(c->segs);
  release(c->m_nseg); release(c->m_seg_off); release(c->m_seg_bytes); release(c->m_item_fl); release(c->m_seg_boff); release(c->m_tmp);
  release(c->m_item_w);
  release(c->t_bitmap); release(c->t_table); release(c->dg_scratch); release(c->dg_blk_cnt); release(c->dg_blk_pre);
  release(c->dg_cand_off); release(c->dg_byte_off); release(c->dg_hits);
  release(c->t_tails); release(c->t_ztails); release(c->dg_hit_tail);
  release(c->r_table); release(c->dg_hit_rule); release(c->r_counter);
  release(c->s_table); release(c->dg_hit_salt); release(c->it_state);
  release(c->hy_list); release(c->hy_lens); release(c->hy_off); release(c->hy_words);
  for (auto& e : c->dev_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->d_mtab) (void)hipFree(c->d_mtab);
  release(c->s_words); release(c->s_out[0]); release(c->s_out[1]); release(c->s_woff);
  release(c->loc_q); release(c->loc_r);
  for (auto& e : c->ev_exp)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->ev_cpy)
    if (e) (void)hipEventDestroy(e);
  if (c->cstream) (void)hipStreamDestroy(c->cstream);
  release(c->glob);
  release(c->m_vl); release(c->vn); release(c->vrsz); release(c->vpre); release(c->vrpre); release(c->vrec);
  release(c->vrec2); release(c->vcand_off); release(c->vbyte_off); release(c->vflags); release(c->vroff);
  release(c->vmap); release(c->vobase); release(c->vocc);
  if (c->mgscr) (void)hipFree(c->mgscr);
  if (c->gscr) (void)hipFree(c->gscr);
  if (c->sstream) (void)hipStreamSynchronize(c->sstream);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->sstream) (void)hipStreamDestroy(c->sstream);
  if (c->d_table) (void)hipFree(c->d_table);
  if (c->d_scalars) (void)hipFree(c->d_scalars);
  if (c->h_scalars) (void)hipHostFree(c->h_scalars);
  if (c->h_totals) (void)hipHostFree(c->h_totals);
  for (auto& h : c->h_out)
    if (h) (void)hipHostFree(h);
  for (auto& e : c->ev)
    if (e) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* a5x_last_error(const a5x_ctx* c) { return c ? c->err.c_str() : "null context"; }

const char* a5x_create_error(void) { return g_create_err.c_str(); }

int a5x_device_info(a5x_ctx* c, char* name, size_t cap, int* cu_count) {
  if (!c) return A5X_E_ARG;
  if (name && cap) {
    strncpy(name, c->devname.c_str(), cap - 1);
    name[cap - 1] = 0;
  }
  if (cu_count) *cu_count = c->cus;
  return A5X_OK;
}

int a5x_load_table_file(a5x_ctx* c, const char* path) {
  if (!c || !path) return A5X_E_ARG;
  FILE* f = fopen(path, "rb");
  if (!f) return fail(c, A5X_E_IO, "open %s: %s", path, strerror(errno));
  std::vector<uint8_t> d;
  uint8_t buf[65536];
  size_t r;
  while ((r = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + r);
  const bool err = ferror(f);
  fclose(f);
  if (err) return fail(c, A5X_E_IO, "read %s failed", path);
  return a5x_parse_table(c, d.data(), d.size());
}

int a5x_parse_table(a5x_ctx* c, const uint8_t* data, size_t len) {
  if (!c || (!data && len)) return A5X_E_ARG;
  Table t = c->table;
  int rc = parse_table_into(c, t, data, len);
  if (rc) return rc;
  c->table = std::move(t);
  c->table_dirty = true;
  c->mtable_dirty = true;
  return A5X_OK;
}

int a5x_set_table(a5x_ctx* c, const uint8_t* kb, const uint64_t* koff, uint32_t nk, const uint8_t* vb,
                  const uint64_t* voff, const uint32_t* vkey, uint32_t nv) {
  if (!c || (nk && !koff) || (nv && (!voff || !vkey))) return A5X_E_ARG;
  Table t;
  for (uint32_t i = 0; i < nk; i++) {
    if (koff[i + 1] < koff[i]) return fail(c, A5X_E_ARG, "key offsets not monotone");
    std::string k((const char*)kb + koff[i], (size_t)(koff[i + 1] - koff[i]));
    if (t.index.count(k)) return fail(c, A5X_E_ARG, "duplicate key %u", i);
    t.index.emplace(k, (uint32_t)t.keys.size());
    t.keys.push_back(k);
    t.vals.emplace_back();
  }
  for (uint32_t j = 0; j < nv; j++) {
    if (vkey[j] >= nk || voff[j + 1] < voff[j]) return fail(c, A5X_E_ARG, "bad value %u", j);
    t.vals[vkey[j]].emplace_back((const char*)vb + voff[j], (size_t)(voff[j + 1] - voff[j]));
  }
  c->table = std::move(t);
  c->table_dirty = true;
  c->mtable_dirty = true;
  return A5X_OK;
}

int a5x_clear_table(a5x_ctx* c) {
  if (!c) return A5X_E_ARG;
  c->table.clear();
  c->table_dirty = true;
  c->mtable_dirty = true;
  return A5X_OK;
}

int a5x_table_export(const a5x_ctx* c, uint32_t* n_keys, uint32_t* n_vals, uint64_t* key_bytes, uint64_t* val_bytes,
                     uint8_t* ko, uint64_t* koff, uint8_t* vo, uint64_t* voff, uint32_t* vkey) {
  if (!c) return A5X_E_ARG;
  const Table& t = c->table;
  uint64_t kbt = 0, vbt = 0, nv = 0;
  if (koff) koff[0] = 0;
  if (voff) voff[0] = 0;
  for (uint32_t i = 0; i < t.keys.size(); i++) {
    if (ko) memcpy(ko + kbt, t.keys[i].data(), t.keys[i].size());
    kbt += t.keys[i].size();
    if (koff) koff[i + 1] = kbt;
    for (auto& v : t.vals[i]) {
      if (vo) memcpy(vo + vbt, v.data(), v.size());
      vbt += v.size();
      if (vkey) vkey[nv] = i;
      nv++;
      if (voff) voff[nv] = vbt;
    }
  }
  if (n_keys) *n_keys = (uint32_t)t.keys.size();
  if (n_vals) *n_vals = (uint32_t)nv;
  if (key_bytes) *key_bytes = kbt;
  if (val_bytes) *val_bytes = vbt;
  return A5X_OK;
}

int a5x_split_words(const uint8_t* data, size_t len, uint8_t* words_out, uint64_t* off_out, uint64_t off_cap,
                    uint64_t* n_words) {
  if ((!data && len) || !n_words) return A5X_E_ARG;
  size_t pos = 0, wb = 0;
  uint64_t n = 0;
  const uint8_t* line;
  size_t l;
  if (off_out && off_cap) off_out[0] = 0;
  while (a5x::gosem::scan_line(data, len, &pos, &line, &l) == 1) {  // ErrTooLong: silently stop
    if (words_out) {
      if (!off_out || n + 1 >= off_cap) return A5X_E_ARG;
      memcpy(words_out + wb, line, l);
    }
    wb += l;
    n++;
    if (words_out) off_out[n] = wb;
  }
  *n_words = n;
  return A5X_OK;
}

int a5x_keyspace_device(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode, int mn,
                        int mx, uint64_t* d_cand_off, uint64_t* d_byte_off, uint64_t* tc, uint64_t* tb,
                        void* stream) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nw && (!d_words || !d_woff))) return A5X_E_ARG;
  int rc;
  if ((rc = check_mode(c, mode))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  Batch B;
  if (mode != A5X_MODE_DEFAULT)
    rc = run_keyspace_mode(c, d_words, d_woff, nw, mode, mn, mx, d_cand_off, d_byte_off, st, &B, false);
  else
    rc = run_keyspace(c, d_words, d_woff, nw, mn, mx, d_cand_off, d_byte_off, st, &B, false);
  if (rc) return rc;
  if (tc) *tc = B.total_cands;
  if (tb) *tb = B.total_bytes;
  return A5X_OK;
}

int a5x_expand_device(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode, int mn,
                      int mx, uint64_t cand_begin, uint64_t cand_end, uint8_t* d_out, uint64_t out_cap,
                      uint64_t* d_cand_off, uint64_t* d_byte_off, a5x_stats* stats, void* stream) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nw && (!d_words || !d_woff))) return A5X_E_ARG;
  int rc;
  if ((rc = check_mode(c, mode))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  Job J{d_words, d_woff, nw, mode, mn, mx, stream ? (hipStream_t)stream : c->stream};
  if ((rc = job_prepare(c, J, d_cand_off, d_byte_off, true))) return rc;
  const Batch& B = J.B;
  const uint64_t cb = std::min(cand_begin, B.total_cands);
  const uint64_t ce = std::min(cand_end, B.total_cands);
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->words = nw;
  }
  if (ce <= cb) return A5X_OK;
  Range R{cb, ce, 0, B.total_bytes, 0, mode != A5X_MODE_DEFAULT ? c->m_items : 0};
  if (cb > 0 || ce < B.total_cands) {
    std::vector<uint64_t> res;
    if ((rc = job_locate(c, J, {cb, ce}, res))) return rc;
    R = range_of(cb, ce, &res[0], &res[3]);
  }
  if (stats) {
    stats->candidates = ce - cb;
    stats->bytes = R.b1 - R.b0;
  }
  HIPCHK(c, hipEventRecord(c->ev[1], J.st));
  if ((rc = job_launch(c, J, R, d_out, out_cap))) return rc;
  HIPCHK(c, hipEventRecord(c->ev[2], J.st));
  if ((rc = job_check(c, J))) return rc;
  if (stats) {
    float a = 0, b = 0, t = 0;
    HIPCHK(c, hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
    HIPCHK(c, hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
    HIPCHK(c, hipEventElapsedTime(&t, c->ev[0], c->ev[2]));
    stats->ms_keyspace = a;
    stats->ms_expand = b;
    stats->ms_total = t;
    stats->words_pass_b = B.nbig;
    stats->expand_launches = mode != A5X_MODE_DEFAULT ? 1 : 1 + (B.nslow ? 1 : 0) + (B.nbig ? 1 : 0);
    stats->words_slow = B.nslow;
  }
  return A5X_OK;
}

int a5x_locate_device(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode, int mn,
                      int mx, const uint64_t* cands, uint64_t n, uint64_t* byte_off_out, void* stream) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nw && (!d_words || !d_woff)) || (n && (!cands || !byte_off_out))) return A5X_E_ARG;
  if (n > 0xffffffffull) return fail(c, A5X_E_ARG, "too many queries");
  int rc;
  if ((rc = check_mode(c, mode))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  Job J{d_words, d_woff, nw, mode, mn, mx, stream ? (hipStream_t)stream : c->stream};
  if ((rc = job_prepare(c, J, nullptr, nullptr, false))) return rc;
  std::vector<uint64_t> q(n), res;
  for (uint64_t i = 0; i < n; i++) q[i] = std::min(cands[i], J.B.total_cands);
  if ((rc = job_locate(c, J, q, res))) return rc;
  for (uint64_t i = 0; i < n; i++) byte_off_out[i] = res[3 * i];
  return A5X_OK;
}

int a5x_split_device(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode, int mn,
                     int mx, const uint64_t* targets, uint32_t nt, uint64_t* cand_out, uint64_t* word_out,
                     uint64_t* ciw_out, void* stream) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nw && (!d_words || !d_woff)) || (nt && (!targets || !cand_out || !word_out || !ciw_out)))
    return A5X_E_ARG;
  int rc;
  if ((rc = check_mode(c, mode))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  Job J{d_words, d_woff, nw, mode, mn, mx, stream ? (hipStream_t)stream : c->stream};
  if ((rc = job_prepare(c, J, nullptr, nullptr, false))) return rc;
  const uint64_t T = J.B.total_cands, TB = J.B.total_bytes;
  // lockstep binary searches: lo[i] < answer <= hi[i], byte(g) = first byte of candidate g
  std::vector<uint64_t> lo(nt), hi(nt), res;
  for (uint32_t i = 0; i < nt; i++) {
    if (targets[i] > TB) return fail(c, A5X_E_ARG, "byte target %llu past the batch's %llu bytes",
                                     (unsigned long long)targets[i], (unsigned long long)TB);
    lo[i] = ~0ull;  // "-1": byte(-1) < every target
    hi[i] = T;      // byte(T) = TB >= every target
  }
  for (int it = 0; it < 70; it++) {
    std::vector<uint64_t> q;
    std::vector<uint32_t> who;
    for (uint32_t i = 0; i < nt; i++)
      if (hi[i] - (lo[i] + 1) > 0) {  // candidates lo+1 .. hi-1 still open
        q.push_back(lo[i] + 1 + (hi[i] - lo[i] - 1) / 2);
        who.push_back(i);
      }
    if (q.empty()) break;
    if ((rc = job_locate(c, J, q, res))) return rc;
    for (size_t k = 0; k < q.size(); k++) {
      const uint32_t i = who[k];
      if (res[3 * k] >= targets[i]) hi[i] = q[k];
      else lo[i] = q[k];
    }
  }
  // the word of each split candidate and its index there: one device binary search per target
  if ((rc = grow(c, c->loc_q, nt)) || (rc = grow(c, c->loc_r, 2 * (size_t)nt))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->loc_q.p, hi.data(), 8 * (size_t)nt, hipMemcpyHostToDevice, J.st));
  HIPCHK(c, a5x_launch_word_of(J.B.cand_off, nw, c->loc_q.p, nt, c->loc_r.p, c->loc_r.p + nt, J.st));
  std::vector<uint64_t> wc(2 * (size_t)nt);
  HIPCHK(c, hipMemcpyAsync(wc.data(), c->loc_r.p, 16 * (size_t)nt, hipMemcpyDeviceToHost, J.st));
  if ((rc = job_check(c, J))) return rc;
  for (uint32_t i = 0; i < nt; i++) {
    cand_out[i] = hi[i];
    word_out[i] = wc[i];
    ciw_out[i] = wc[nt + i];
  }
  return A5X_OK;
}

int a5x_digest_device(a5x_ctx* c, const uint8_t* d_out, const uint64_t* d_byte_off, uint64_t out_base, uint64_t nw,
                      uint64_t* d_digest, void* stream) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nw && (!d_byte_off || !d_digest))) return A5X_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if (nw) HIPCHK(c, a5x_launch_digest(d_out, d_byte_off, out_base, nw, d_digest, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return A5X_OK;
}

int a5x_keyspace(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw, int mode, int mn, int mx,
                 uint64_t* out_count, uint64_t* out_bytes) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nw && (!words || !woff))) return A5X_E_ARG;
  int rc;
  if ((rc = check_mode(c, mode))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = stage_words(c, words, woff, nw))) return rc;
  Batch B;
  if (mode != A5X_MODE_DEFAULT)
    rc = run_keyspace_mode(c, c->s_words.p, c->s_woff.p, nw, mode, mn, mx, nullptr, nullptr, c->stream, &B, false);
  else
    rc = run_keyspace(c, c->s_words.p, c->s_woff.p, nw, mn, mx, nullptr, nullptr, c->stream, &B, false);
  if (rc) return rc;
  if (out_count && nw) HIPCHK(c, hipMemcpyAsync(out_count, c->count.p, nw * 8, hipMemcpyDeviceToHost, c->stream));
  if (out_bytes && nw) HIPCHK(c, hipMemcpyAsync(out_bytes, c->bytes.p, nw * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return A5X_OK;
}

// The stdout path's buffers: two HBM range buffers and two pinned host buffers of cap
// bytes, the copy stream and its events (a5x_expand; a5x_stream_reserve makes them ahead).
size_t stream_cap() {
  size_t cap = (size_t)1 << 27;
  if (const char* e = getenv("A5X_HOST_CHUNK_BYTES")) cap = std::max<size_t>(4096, strtoull(e, nullptr, 10));
  return cap;
}

int stream_buffers(a5x_ctx* c, size_t cap) {
  int rc;
  if ((rc = grow(c, c->s_out[0], cap)) || (rc = grow(c, c->s_out[1], cap))) return rc;
  if (c->h_out_cap < cap) {
    for (auto& h : c->h_out)
      if (h) (void)hipHostFree(h), h = nullptr;
    c->h_out_cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&c->h_out[0], cap, 0));
    HIPCHK(c, hipHostMalloc((void**)&c->h_out[1], cap, 0));
    c->h_out_cap = cap;
  }
  if (!c->cstream) HIPCHK(c, hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
  for (int i = 0; i < 2; i++) {
    if (!c->ev_exp[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_exp[i], hipEventDisableTiming));
    if (!c->ev_cpy[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_cpy[i], hipEventDisableTiming));
  }
  return A5X_OK;
}

int a5x_stream_reserve(a5x_ctx* c, uint64_t words, uint64_t word_bytes) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c) return A5X_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = stream_buffers(c, stream_cap()))) return rc;
  // the per-batch keyspace state of a batch of this size, and the staged words
  c->flags_nw = 0;  // (growing the flags array need not keep the last pass's)
  if ((rc = grow(c, c->s_words, word_bytes + 16)) || (rc = grow(c, c->s_woff, words + 1)) ||
      (rc = grow(c, c->count, words + 1)) || (rc = grow(c, c->bytes, words + 1)) ||
      (rc = grow(c, c->flags, words + 1)) || (rc = grow(c, c->defer, words + 1)) ||
      (rc = grow(c, c->roff, words + 1)) || (rc = grow(c, c->cplx, words + 1)) ||
      (rc = grow(c, c->slow_list, words + 1)) || (rc = grow(c, c->big_list, words + 1)) ||
      (rc = grow(c, c->glob, words + 1)) || (rc = grow(c, c->cand_off, words + 1)) ||
      (rc = grow(c, c->byte_off, words + 1)) ||
      (rc = grow(c, c->scan_tmp, a5x_scan_tmp_elems(words + 1) + 16)) ||
      (rc = grow(c, c->rec, ((words + FW_TILE - 1) / FW_TILE) * (uint64_t)FW_TILE_REC +
                                (uint64_t)ks_cplx_cap(words) * FW_RMAX + 2)))
    return rc;
  if ((rc = upload_table(c))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return A5X_OK;
}

// The stdout path (main.go:58-68): ranges of <= cap bytes expanded into two HBM buffers
// in turn; each range's D2H runs on a copy stream into a pinned buffer while the next
// range expands, and the sink consumes range k while range k + 1 is being copied.
int a5x_expand(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw, int mode, int mn, int mx,
               a5x_sink_fn sink, void* user, a5x_stats* stats) {
  return a5x_expand_range(c, words, woff, nw, mode, mn, mx, 0, ~0ull, sink, user, stats);
}

// a5x_expand over the batch's global candidates [cb, ce) only (the CLI's --skip / --limit
// resume cursor): the same keyspace, the ranges cut at the window's ends.
int a5x_expand_range(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw, int mode, int mn, int mx,
                     uint64_t cb, uint64_t ce, a5x_sink_fn sink, void* user, a5x_stats* stats) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || !sink || (nw && (!words || !woff))) return A5X_E_ARG;
  int rc;
  if ((rc = check_mode(c, mode))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = stage_words(c, words, woff, nw))) return rc;
  Job J{c->s_words.p, c->s_woff.p, nw, mode, mn, mx, c->stream};
  if ((rc = job_prepare(c, J, nullptr, nullptr, true))) return rc;
  const size_t cap = stream_cap();
  std::vector<Range> ranges;
  if ((rc = plan_ranges(c, J, cap, ranges, cb, ce))) return rc;
  if (!ranges.empty() && (rc = stream_buffers(c, cap))) return rc;
  // error word of each range, copied behind its launch (valid once its copy event fired)
  uint32_t* herr = c->h_scalars + H_RANGE_ERR;
  auto drain = [&](size_t k) -> int {  // range k has been copied: check it, hand it to the sink
    HIPCHK(c, hipEventSynchronize(c->ev_cpy[k & 1]));
    if (herr[k & 1]) return decode_dev_err(c, herr[k & 1]);
    const uint64_t nb = ranges[k].b1 - ranges[k].b0;
    if (nb && sink(user, c->h_out[k & 1], nb)) return fail(c, A5X_E_SINK, "sink returned non-zero");
    return A5X_OK;
  };
  HIPCHK(c, hipEventRecord(c->ev[1], J.st));
  for (size_t k = 0; k < ranges.size(); k++) {
    const int b = (int)(k & 1);
    if (k >= 2) HIPCHK(c, hipStreamWaitEvent(J.st, c->ev_cpy[b], 0));  // range k-2's copy left buffer b
    if ((rc = job_launch(c, J, ranges[k], c->s_out[b].p, cap))) return rc;
    HIPCHK(c, hipMemcpyAsync(herr + b, c->d_scalars + S_ERR, 4, hipMemcpyDeviceToHost, J.st));
    HIPCHK(c, hipEventRecord(c->ev_exp[b], J.st));
    HIPCHK(c, hipStreamWaitEvent(c->cstream, c->ev_exp[b], 0));
    HIPCHK(c, hipMemcpyAsync(c->h_out[b], c->s_out[b].p, ranges[k].b1 - ranges[k].b0, hipMemcpyDeviceToHost,
                             c->cstream));
    HIPCHK(c, hipEventRecord(c->ev_cpy[b], c->cstream));
    if (k >= 1 && (rc = drain(k - 1))) return rc;
  }
  if (!ranges.empty() && (rc = drain(ranges.size() - 1))) return rc;
  HIPCHK(c, hipEventRecord(c->ev[2], J.st));
  if ((rc = job_check(c, J))) return rc;
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->words = nw;
    stats->candidates = J.B.total_cands;  // (the whole batch; the window's: its ranges below)
    stats->bytes = J.B.total_bytes;
    if (cb != 0 || ce < J.B.total_cands) {
      stats->candidates = 0;
      stats->bytes = 0;
      for (const Range& R : ranges) stats->candidates += R.ce - R.cb, stats->bytes += R.b1 - R.b0;
    }
    float a = 0, t = 0;
    HIPCHK(c, hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
    HIPCHK(c, hipEventElapsedTime(&t, c->ev[0], c->ev[2]));
    stats->ms_keyspace = a;
    stats->ms_total = t;  // includes the D2H copies and the sink
    stats->ms_expand = t - a;
    stats->expand_launches = (uint32_t)ranges.size();
    stats->words_slow = J.B.nslow;
    stats->words_pass_b = J.B.nbig;
  }
  return A5X_OK;
}

// diagnostic builds only (-DA5X_STAMPS); A5X_E_UNSUPPORTED otherwise
int a5x_debug_stamps(unsigned long long* out16, int reset) {
  const int rc = a5x_read_stamps(out16, reset);
  return rc == 0 ? A5X_OK : (rc == -9 ? A5X_E_UNSUPPORTED : A5X_E_HIP);
}

int a5x_debug_keyspace_refit(a5x_ctx* c, uint64_t* out) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || !out) return A5X_E_ARG;
  uint32_t n = 0;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(&n, c->d_scalars + S_REFIT, 4, hipMemcpyDeviceToHost));
  *out = n;
  return A5X_OK;
}

int a5x_debug_keyspace_cplx_lean(a5x_ctx* c, uint64_t* out) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || !out) return A5X_E_ARG;
  uint32_t n[2] = {0, 0};
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(n, c->d_scalars + S_CPLX_LEAN, 8, hipMemcpyDeviceToHost));
  out[0] = n[0]; out[1] = n[1];
  return A5X_OK;
}

int a5x_debug_keyspace_small_stage(a5x_ctx* c, uint32_t* out) {
  if (!c || !out) return A5X_E_ARG;
  if (c->table.keys.empty()) return fail(c, A5X_E_NOTABLE, "no substitution table loaded");
  if (c->table_dirty || c->blob.empty()) {
    int rc = compile_table(c);
    if (rc) return rc;
  }
  *out = a5x_keyspace_small_stage(c->table_bytes);
  return A5X_OK;
}

int a5x_debug_keyspace_stage(a5x_ctx* c, uint32_t* out) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || !out) return A5X_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->d_scalars + S_STAGE, 4, hipMemcpyDeviceToHost));
  return A5X_OK;
}

int a5x_debug_word_flags(a5x_ctx* c, uint32_t* out, uint64_t n) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (!out && n)) return A5X_E_ARG;
  if (n > c->flags_nw)
    return fail(c, A5X_E_ARG, "flags of %llu words asked, the last keyspace pass had %llu", (unsigned long long)n,
                (unsigned long long)c->flags_nw);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n) HIPCHK(c, hipMemcpy(out, c->flags.p, n * 4, hipMemcpyDeviceToHost));
  return A5X_OK;
}

int a5x_debug_keyspace_large_stage(a5x_ctx* c, int on) {
  if (!c) return A5X_E_ARG;
  c->ks_large_only = on != 0;
  return A5X_OK;
}

int a5x_debug_plan_word(a5x_ctx* c, const uint8_t* word, size_t len, int mn, int mx, uint8_t* out, size_t cap,
                        uint64_t* info) {
  if (!c || !info || (!word && len) || (!out && cap)) return A5X_E_ARG;
  if (c->table.keys.empty()) return fail(c, A5X_E_NOTABLE, "no substitution table loaded");
  if (c->table_dirty || c->blob.empty()) {
    int rc = compile_table(c);
    if (rc) return rc;
  }
  info[0] = info[1] = info[2] = info[3] = 0;
  if (len > A5X_LMAX_A && mx >= 1) {
    info[2] = A5X_WF_DEFER;
    return A5X_OK;
  }
  std::vector<uint8_t> wb(word, word + len);
  wb.resize(len + 16, 0);
  GWord gw;
  gw.p = wb.data();
  const Tab T = tab_view(c->blob.data());
  const WordClass C = classify_word(gw, (u32)len, T, mn, mx, A5X_RING_A - 16);
  info[0] = C.count; info[1] = C.bytes; info[2] = C.flags;
  if (!(C.flags & A5X_WF_FAST) || C.count == 0) return A5X_OK;
  // the record exactly as k_keyspace_thread builds it, placed as a one-word window
  std::vector<u64> wrec(FX_WREC + FW_PMAX + 16, 0);
  ArraySink sk;
  sk.rec = wrec.data(); sk.np = ff_np(C.flags);
  // (diagnostics: A5X_BAL_SLACK8 overrides the balanced big-piece slack of the device
  // build, FB_BAL_SLACK8, for the window simulation in tools/window_sim.py)
  u32 slack = FB_BAL_SLACK8;
  if (const char* e = getenv("A5X_BAL_SLACK8")) slack = (u32)atoi(e);
  const Plan P = plan_word<true>(gw, (u32)len, T, sk, fb_balanced_cap(C.count + 1, slack));
  wrec[0] = fr_hdr(P.np, P.ng, P.ne, P.maxl, P.nbig, P.bstarts, P.bRp);
  wrec[FX_ZSLOT] = 0;
  if (!P.ok || P.ng != ff_ng(C.flags) || P.ne != ff_ne(C.flags) || P.np != ff_np(C.flags))
    return fail(c, A5X_E_BOUNDS, "piece plan disagrees with the keyspace fields");
  info[2] |= (uint64_t)P.nbig << 32 | (uint64_t)P.bent << 40;  // diagnostics: big pieces / entries
  if (!out) return A5X_OK;  // no out: classification and plan only
  // big pieces and their entries as the k_expand_fast window setup builds them
  u32 Rb[FB_NMAX], base[FB_NMAX], E = 0;
  std::vector<u32> be(4 * 256, 0);
  for (u32 b = 0; b < FB_NMAX; b++) {
    Rb[b] = fb_R(wrec.data(), 0, wrec[0], b);
    if (Rb[b] != frh_R(wrec[0], b)) return fail(c, A5X_E_BOUNDS, "header R of big piece %u: %u != %u", b, frh_R(wrec[0], b), Rb[b]);
    base[b] = E;
    if (b < P.nbig) E += Rb[b];
  }
  if (E != P.bent) return fail(c, A5X_E_BOUNDS, "big entries %u != plan %u", E, P.bent);
  for (u32 b = 0; b < P.nbig; b++)
    for (u32 cc = 0; cc < Rb[b]; cc++) fb_entry(wrec.data(), 0, b, cc, &be[4 * (base[b] + cc)]);
  // replay the rounds: lanes one after the other, passes 1-2 into a linear ring
  // with the head/carry hand-over and block moves exactly as the kernel does them
  if (C.bytes > cap) return fail(c, A5X_E_CAPACITY, "output buffer too small");
  const u32 RING = 2048;
  std::vector<u32> ring(RING / 4 + 4 * 64, 0xA5A5A5A5u);
  uint64_t pos = 0, B = 0;  // bytes produced / global byte of ring byte 0
  u32 carry = 0;
  const u32 nl = std::min<u32>(64, (RING - 32) / std::max<u32>(P.maxl, 1));
  auto flush = [&]() {
    const u32 nb = (u32)((pos - B) >> 4);
    if (!nb) return;
    for (uint64_t X = B; X < B + 16ull * nb; X++) out[X] = (uint8_t)(ring[(X - B) >> 2] >> (8 * ((X - B) & 3)));
    for (u32 k = 0; k < 4; k++) ring[k] = ring[4 * nb + k];
    B += 16ull * nb;
  };
  for (uint64_t rr = 0; rr < C.count; rr += nl) {
    const u32 nact = (u32)std::min<uint64_t>(nl, C.count - rr);
    u32 len[64], o[64], acc[64], pn[64], hd[64], D[64];
    u32 ent[64][FB_NMAX][4];
    u32 run = (u32)(pos - B);
    for (u32 l = 0; l < nact; l++) {
      u32 n = (u32)(rr + l + 1);
      len[l] = 0;
      for (u32 b = 0; b < FB_NMAX; b++) {
        const u32 q = Rb[b] > 1 ? (u32)(((u64)n * fr_magic(Rb[b])) >> 32) : n;
        const u32 d = n - q * Rb[b];
        n = q;
        for (u32 k = 0; k < 4; k++) ent[l][b][k] = b < P.nbig ? be[4 * (base[b] + d) + k] : 0u;
        len[l] += ent[l][b][3] >> 24;
      }
      o[l] = run;
      run += len[l];
    }
    for (u32 l = 0; l < nact; l++) {
      pn[l] = o[l] & 3u; D[l] = o[l] >> 2; acc[l] = 0; hd[l] = 0;
      u32 pv = l == 0 ? (carry << ((32u - 8u * pn[l]) & 31u)) : 0u;
      bool hp = l != 0 && pn[l] != 0;
      for (u32 b = 0; b < FB_NMAX; b++) fb_put(ent[l][b], pv, pn[l], D[l], hp, hd[l], acc[l], ring.data(), RING / 4 + 4 * l);
    }
    for (u32 l = 0; l < nact; l++)
      ring[(l + 1 < nact && pn[l]) ? D[l] : RING / 4 + 4 * l] = acc[l] | (l + 1 < nact ? hd[l + 1] : 0u);
    carry = acc[nact - 1];
    pos = B + run;
    flush();
  }
  if (pos & 3) ring[(u32)(pos - B) >> 2] = carry;
  flush();
  for (uint64_t X = B; X < pos; X++) out[X] = (uint8_t)(ring[(X - B) >> 2] >> (8 * ((X - B) & 3)));
  if (pos != C.bytes) return fail(c, A5X_E_BOUNDS, "replayed %llu bytes, keyspace says %llu",
                                  (unsigned long long)pos, (unsigned long long)C.bytes);
  info[3] = pos;
  return A5X_OK;
}

extern "C++" {
template <u32 CAP>
static void plan_sizes_rows(const GWord& gw, u32 L, const Tab& T, uint32_t* cnt, uint32_t* bld) {
  std::vector<u64> rec(1 + 128 + 64 * FW_UMAXR + 128, 0);  // (np, ne of any word of <= 64 bytes)
  ArraySink sk;
  sk.rec = rec.data(); sk.np = 128;
  CountPlanner<CAP> cp;
  Planner<true, GWord, ArraySink, CAP> pb(gw, T, sk);
  u32 p = 0;
  Unit U;
  while (next_unit(gw, L, p, T, U)) {
    cp.unit(U);
    pb.unit(U);
  }
  cp.finish(L);
  pb.finish(L);
  pb.pick_balanced();
  const Plan* P[2] = {&cp.P, &pb.P};
  uint32_t* o[2] = {cnt, bld};
  for (int k = 0; k < 2; k++) {
    const Plan& Q = *P[k];
    const uint32_t v[8] = {Q.ok ? 1u : 0u, Q.np, Q.ng, Q.ne, Q.maxl, Q.minl, Q.nbig, Q.bent};
    for (int j = 0; j < 8; j++) o[k][j] = v[j];
  }
}
}  // extern "C++"

int a5x_debug_plan_sizes(a5x_ctx* c, const uint8_t* word, size_t len, uint32_t* out) {
  if (!c || !out || (!word && len)) return A5X_E_ARG;
  if (len > A5X_LMAX_A) return fail(c, A5X_E_ARG, "word of %zu bytes (the planners take <= %d)", len, A5X_LMAX_A);
  if (c->table.keys.empty()) return fail(c, A5X_E_NOTABLE, "no substitution table loaded");
  if (c->table_dirty || c->blob.empty()) {
    int rc = compile_table(c);
    if (rc) return rc;
  }
  std::vector<uint8_t> wb(word, word + len);
  wb.resize(len + 16, 0);
  GWord gw;
  gw.p = wb.data();
  const Tab T = tab_view(c->blob.data());
  const u32 L = (u32)len;
  for (int j = 0; j < 40; j++) out[j] = 0;
  plan_sizes_rows<FW_UMAXR>(gw, L, T, out, out + 8);
  plan_sizes_rows<8>(gw, L, T, out + 16, out + 24);
  // k_keyspace_cplx's two paths: the record planned from the units of the classification
  // walk (cluster choices left in the sink by that walk) against plan_word's own walk
  std::vector<u64> ra(FX_WREC + FW_PMAX + 16, 0), rb(FX_WREC + FW_PMAX + 16, 0);
  ArraySink sa, sb;
  UnitCache uc;
  const WordClass C = classify_word(gw, L, T, 0, 15, A5X_RING_A - 16, &uc, sb.c, 1);
  if (!(C.flags & A5X_WF_FAST) || (C.flags & A5X_WF_DEFER) || C.count == 0) {
    out[32] = 3;
    return A5X_OK;
  }
  if (uc.full) {
    out[32] = 2;
    return A5X_OK;
  }
  sa.rec = ra.data(); sa.np = ff_np(C.flags);
  sb.rec = rb.data(); sb.np = ff_np(C.flags);
  const Plan PA = plan_word<true>(gw, L, T, sa, fb_balanced_cap(C.count + 1));
  const Plan PB = plan_word_cached(gw, L, T, sb, uc, fb_balanced_cap(C.count + 1));
  ra[0] = fr_hdr(PA.np, PA.ng, PA.ne, PA.maxl, PA.nbig, PA.bstarts, PA.bRp);
  rb[0] = fr_hdr(PB.np, PB.ng, PB.ne, PB.maxl, PB.nbig, PB.bstarts, PB.bRp);
  out[32] = PA.ok && PB.ok && PA.minl == PB.minl && PA.bent == PB.bent && ra == rb ? 1u : 0u;
  return A5X_OK;
}

int a5x_debug_piece_build(a5x_ctx* c, const uint8_t* word, size_t len, uint32_t* out) {
  if (!c || !out || (!word && len)) return A5X_E_ARG;
  if (len > 127) return fail(c, A5X_E_ARG, "word of %zu bytes (the piece builder's check takes <= 127)", len);
  if (c->table.keys.empty()) return fail(c, A5X_E_NOTABLE, "no substitution table loaded");
  if (c->table_dirty || c->blob.empty()) {
    int rc = compile_table(c);
    if (rc) return rc;
  }
  std::vector<uint8_t> wb(word, word + len);
  wb.resize(len + 16, 0);
  piece_build_compare(wb.data(), (u32)len, tab_view(c->blob.data()), out);
  return A5X_OK;
}

int a5x_debug_cut_once(a5x_ctx* c, const uint8_t* word, size_t len, uint32_t* out, uint64_t* rec_new, uint64_t* rec_ref) {
  static_assert(A5X_CUT_ONCE_OUT == CO_NOUT && A5X_CUT_ONCE_REC == CO_NREC, "a5x.h and a5x_plan.h");
  if (!c || !out || (!word && len)) return A5X_E_ARG;
  if (len > 127) return fail(c, A5X_E_ARG, "word of %zu bytes (the cut-once check takes <= 127)", len);
  if (c->table.keys.empty()) return fail(c, A5X_E_NOTABLE, "no substitution table loaded");
  if (c->table_dirty || c->blob.empty()) {
    int rc = compile_table(c);
    if (rc) return rc;
  }
  std::vector<uint8_t> wb(word, word + len);
  wb.resize(len + 16, 0);
  cut_once_compare(wb.data(), (u32)len, tab_view(c->blob.data()), out, rec_new, rec_ref);
  return A5X_OK;
}

int a5x_debug_cplx_build(a5x_ctx* c, const uint8_t* word, size_t len, int mn, int mx, uint32_t* out) {
  if (!c || !out || (!word && len)) return A5X_E_ARG;
  if (len > 127) return fail(c, A5X_E_ARG, "word of %zu bytes (the complex-word check takes <= 127)", len);
  if (c->table.keys.empty()) return fail(c, A5X_E_NOTABLE, "no substitution table loaded");
  if (c->table_dirty || c->blob.empty()) {
    int rc = compile_table(c);
    if (rc) return rc;
  }
  std::vector<uint8_t> wb(word, word + len);
  wb.resize(len + 16, 0);
  cplx_build_compare(wb.data(), (u32)len, tab_view(c->blob.data()), mn, mx, out);
  return A5X_OK;
}

// the context's salted state dropped: the target set (if any) is an unsalted one
static void clear_salts(a5x_ctx* c) {
  c->salted = false;
  c->n_salts = 0;
  c->s_bytes.clear();
  c->s_off.clear();
  c->s_recs.clear();
  c->s_hit_salt.clear();
  c->s_hashed = c->s_skipped = 0;
  c->it_iters.clear();
  c->it_tidx.clear();
  c->it_keys.clear();
  c->it_lines.clear();
  c->it_by_key.clear();
}

// the built target set into the context's device buffers (a5x_set_targets, a5x_set_salted_targets)
static int upload_target_set(a5x_ctx* c, int algo, uint64_t n, TargetSet& T) {
  const uint32_t TW = algo_size(algo) / 4 - 4;  // tail words
  int rc;
  if ((rc = grow(c, c->t_bitmap, T.bm.size())) || (rc = grow(c, c->t_table, T.tab.size()))) return rc;
  if (TW && ((rc = grow(c, c->t_tails, T.tails.size())) || (rc = grow(c, c->t_ztails, T.ztails.size() + 1)))) return rc;
  HIPCHK(c, hipMemcpy(c->t_bitmap.p, T.bm.data(), T.bm.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->t_table.p, T.tab.data(), T.tab.size() * sizeof(uint4), hipMemcpyHostToDevice));
  if (TW) HIPCHK(c, hipMemcpy(c->t_tails.p, T.tails.data(), T.tails.size() * 4, hipMemcpyHostToDevice));
  if (!T.ztails.empty())
    HIPCHK(c, hipMemcpy(c->t_ztails.p, T.ztails.data(), T.ztails.size() * 4, hipMemcpyHostToDevice));
  c->t_tw = TW;
  c->t_nz = TW ? (uint32_t)(T.ztails.size() / TW) : 0;
  c->t_full.swap(T.full);
  c->t_shared_prefix = T.shared;
  c->t_hit_tails.clear();
  c->t_algo = algo;
  c->n_targets = n;
  c->t_bm_log2 = T.bm_log2;
  c->t_tmask = T.tmask;
  c->t_has_zero = T.has_zero;
  return A5X_OK;
}

int a5x_set_targets(a5x_ctx* c, int algo, const uint8_t* dig, uint64_t n) {
  if (c && algo_salted_only(algo))
    return fail(c, A5X_E_ARG, "digest algorithm %d is salted only (a5x_set_salted_targets)", algo);
  if (c && c->device < 0) {
    clear_salts(c);  // (a host-only context keeps a salted set's host copy: dropped, as on a device context)
    return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  }
  if (!c || (n && !dig)) return A5X_E_ARG;
  const uint32_t W = algo_size(algo);  // digest bytes
  if (!W) return fail(c, A5X_E_ARG, "bad digest algorithm %d", algo);
  HIPCHK(c, hipSetDevice(c->device));
  TargetSet T;
  build_target_set(W, dig, n, T);
  const int rc = upload_target_set(c, algo, n, T);
  if (rc == A5X_OK) clear_salts(c);  // the set is unsalted again
  return rc;
}

// ---- salted target lists (a5x_salt.h, a5x_salt.hip) ------------------------------
int a5x_set_salted_targets(a5x_ctx* c, int algo, int order, const uint8_t* dig, uint64_t n, const uint8_t* salt_bytes,
                           const uint64_t* salt_off) {
  if (!c) return A5X_E_ARG;
  const uint32_t W = algo_size(algo);  // digest bytes
  if (!W || algo_unsalted(algo)) return fail(c, A5X_E_ARG, "no salted mode for digest algorithm %d", algo);
  if (a5x_algo_pbkdf2(algo)) return fail(c, A5X_E_ARG, "digest algorithm %d is iterated (a5x_set_iterated_targets)", algo);
  if (order != A5X_SALT_ORDER_PASS_SALT && order != A5X_SALT_ORDER_SALT_PASS)
    return fail(c, A5X_E_ARG, "salt order %d: 0 is pass.salt, 1 is salt.pass", order);
  if (algo_salted_only(algo) && order != salted_only_order(algo))
    return fail(c, A5X_E_ARG, "salt order %d: digest algorithm %d places its salt by order %d", order, algo, salted_only_order(algo));
  if (n && (!dig || !salt_off)) return fail(c, A5X_E_ARG, "null digests or salt offsets");
  for (uint64_t i = 0; i < n; i++) {
    if (salt_off[i + 1] < salt_off[i]) return fail(c, A5X_E_ARG, "salt offsets of target %llu decrease", (unsigned long long)i);
    if (salt_off[i + 1] - salt_off[i] > A5X_SALT_MAX)
      return fail(c, A5X_E_ARG, "salt of target %llu has %llu bytes, the limit is %u", (unsigned long long)i,
                  (unsigned long long)(salt_off[i + 1] - salt_off[i]), A5X_SALT_MAX);
    if (salt_off[i + 1] > salt_off[i] && !salt_bytes) return fail(c, A5X_E_ARG, "null salt bytes");
  }
  if (c->n_rules)
    return fail(c, A5X_E_UNSUPPORTED, "rules and salted targets together are not supported: %u rules are loaded (clear them first)",
                c->n_rules);
  // distinct salts, indexed by first appearance; every target's salt index
  std::unordered_map<std::string, uint32_t> index;
  std::vector<uint8_t> sb;
  std::vector<uint64_t> so(1, 0);
  std::vector<uint32_t> tidx(n);
  for (uint64_t i = 0; i < n; i++) {
    const size_t sl = (size_t)(salt_off[i + 1] - salt_off[i]);
    std::string s(sl ? (const char*)salt_bytes + salt_off[i] : "", sl);
    auto it = index.find(s);
    if (it == index.end()) {
      it = index.emplace(s, (uint32_t)(so.size() - 1)).first;
      sb.insert(sb.end(), s.begin(), s.end());
      so.push_back(sb.size());
    }
    tidx[i] = it->second;
  }
  const uint32_t S = (uint32_t)(so.size() - 1);
  // the device salt table: one record per salt, sorted by length (salt.pass copies the
  // candidate once per run of equal lengths), the public index kept in the record
  std::vector<uint32_t> ord(S);
  for (uint32_t i = 0; i < S; i++) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return so[x + 1] - so[x] < so[y + 1] - so[y]; });
  // (a salted nested set: the record layout of a5x_salt_nest.h, built for this algorithm -- the
  // padded outer message per salt, for 34 / 35 over the salt's own MD5 text; their effective
  // salts are all 32 bytes, so the order by the caller's lengths is an order by theirs too)
  // (an HMAC set: a5x_hmac.h's, the salt's padded message or its two key states)
  const bool snest = a5x_algo_salt_nested(algo), hmac = a5x_algo_hmac(algo);
  const uint32_t stride = salt_stride(algo);
  std::vector<uint32_t> recs((size_t)S * stride, 0u);
  for (uint32_t k = 0; k < S; k++) {
    uint32_t* r = &recs[(size_t)k * stride];
    const uint32_t i = ord[k], sl = (uint32_t)(so[i + 1] - so[i]);
    if (snest) {
      snest_record(algo, sb.data() + so[i], sl, i, r);
      continue;
    }
    if (hmac) {
      hmac_record(algo, sb.data() + so[i], sl, i, r);
      continue;
    }
    r[A5X_SALT_R_LEN] = sl;
    r[A5X_SALT_R_INDEX] = i;
    salt_mask(i, r + A5X_SALT_R_MASK);
    if (sl) memcpy(r + A5X_SALT_R_BYTES, sb.data() + so[i], sl);
  }
  if (c->device >= 0) {
    // the target set keyed on the masked digests: the first 16 bytes XOR the salt's mask
    std::vector<uint8_t> md(dig, dig + (size_t)W * n);
    for (uint64_t i = 0; i < n; i++) {
      uint32_t m[4], d[4];
      salt_mask(tidx[i], m);
      memcpy(d, &md[(size_t)W * i], 16);
      for (int k = 0; k < 4; k++) d[k] ^= m[k];
      memcpy(&md[(size_t)W * i], d, 16);
    }
    auto upload = [&]() -> int {
      int rc;
      HIPCHK(c, hipSetDevice(c->device));
      HIPCHK(c, hipStreamSynchronize(c->stream));  // (no kernel of an earlier call still reads the tables)
      TargetSet T;
      build_target_set(W, md.data(), n, T, dig);
      if ((rc = upload_target_set(c, algo, n, T))) return rc;
      if ((rc = grow(c, c->s_table, recs.size() + 1))) return rc;
      if (S) HIPCHK(c, hipMemcpy(c->s_table.p, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
      return A5X_OK;
    };
    const int rc = upload();
    if (rc) {  // a half-replaced set (masked table without its salts, or the reverse) is no set
      c->t_algo = -1;
      clear_salts(c);
      return rc;
    }
  } else {
    c->t_algo = algo;
    c->n_targets = n;
  }
  clear_salts(c);  // (an iterated set's own fields with them)
  c->salted = true;
  c->s_order = order;
  c->n_salts = S;
  c->s_bytes.swap(sb);
  c->s_off.swap(so);
  c->s_recs.swap(recs);
  return A5X_OK;
}

// ---- iterated target lists (a5x_pbkdf2.h, a5x_pbkdf2.hip) ------------------------
// a5x_set_iterated_targets; keys / lines: per target the whole key and the line of the list
// (null: the 16 bytes, no line)
static int set_iterated(a5x_ctx* c, int algo, const uint8_t* dig, uint64_t n, const uint8_t* salt_bytes,
                        const uint64_t* salt_off, const uint32_t* iters, std::vector<std::vector<uint8_t>>* keys,
                        std::vector<std::string>* lines) {
  if (!c) return A5X_E_ARG;
  if (!a5x_algo_pbkdf2(algo)) return fail(c, A5X_E_ARG, "digest algorithm %d is not an iterated one (72..75)", algo);
  if (n && (!dig || !salt_off || !iters)) return fail(c, A5X_E_ARG, "null digests, salt offsets or iteration counts");
  for (uint64_t i = 0; i < n; i++) {
    if (salt_off[i + 1] < salt_off[i]) return fail(c, A5X_E_ARG, "salt offsets of target %llu decrease", (unsigned long long)i);
    if (salt_off[i + 1] - salt_off[i] > A5X_SALT_MAX)
      return fail(c, A5X_E_ARG, "salt of target %llu has %llu bytes, the limit is %u", (unsigned long long)i,
                  (unsigned long long)(salt_off[i + 1] - salt_off[i]), A5X_SALT_MAX);
    if (salt_off[i + 1] > salt_off[i] && !salt_bytes) return fail(c, A5X_E_ARG, "null salt bytes");
    if (!iters[i]) return fail(c, A5X_E_ARG, "target %llu has an iteration count of 0", (unsigned long long)i);
  }
  if (c->n_rules)
    return fail(c, A5X_E_UNSUPPORTED, "rules and iterated targets together are not supported: %u rules are loaded (clear them first)",
                c->n_rules);
  // distinct (salt, iterations) pairs, indexed by first appearance; every target's index
  std::map<std::pair<std::string, uint32_t>, uint32_t> index;
  std::vector<uint8_t> sb;
  std::vector<uint64_t> so(1, 0);
  std::vector<uint32_t> tidx(n), its;
  for (uint64_t i = 0; i < n; i++) {
    const size_t sl = (size_t)(salt_off[i + 1] - salt_off[i]);
    std::string sk(sl ? (const char*)salt_bytes + salt_off[i] : "", sl);
    auto it = index.find(std::make_pair(sk, iters[i]));
    if (it == index.end()) {
      it = index.emplace(std::make_pair(sk, iters[i]), (uint32_t)its.size()).first;
      sb.insert(sb.end(), sk.begin(), sk.end());
      so.push_back(sb.size());
      its.push_back(iters[i]);
    }
    tidx[i] = it->second;
  }
  const uint32_t S = (uint32_t)its.size();
  // the device table: one record per pair, sorted by salt length as the other salt tables are
  std::vector<uint32_t> ord(S);
  for (uint32_t i = 0; i < S; i++) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return so[x + 1] - so[x] < so[y + 1] - so[y]; });
  std::vector<uint32_t> recs((size_t)S * A5X_PBKDF2_STRIDE, 0u);
  for (uint32_t k = 0; k < S; k++) {
    const uint32_t i = ord[k];
    pbkdf2_record(algo, sb.data() + so[i], (uint32_t)(so[i + 1] - so[i]), i, its[i], &recs[(size_t)k * A5X_PBKDF2_STRIDE]);
  }
  if (c->device >= 0) {
    std::vector<uint8_t> md(dig, dig + (size_t)16 * n);  // the first 16 bytes XOR the index's mask
    for (uint64_t i = 0; i < n; i++) {
      uint32_t m[4], d[4];
      salt_mask(tidx[i], m);
      memcpy(d, &md[(size_t)16 * i], 16);
      for (int k = 0; k < 4; k++) d[k] ^= m[k];
      memcpy(&md[(size_t)16 * i], d, 16);
    }
    auto upload = [&]() -> int {
      int rc;
      HIPCHK(c, hipSetDevice(c->device));
      HIPCHK(c, hipStreamSynchronize(c->stream));  // (no kernel of an earlier call still reads the tables)
      TargetSet T;
      build_target_set(16, md.data(), n, T, dig);
      if ((rc = upload_target_set(c, algo, n, T))) return rc;
      if ((rc = grow(c, c->s_table, recs.size() + 1))) return rc;
      if (S) HIPCHK(c, hipMemcpy(c->s_table.p, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
      return A5X_OK;
    };
    const int rc = upload();
    if (rc) {
      c->t_algo = -1;
      clear_salts(c);
      return rc;
    }
  } else {
    c->t_algo = algo;
    c->n_targets = n;
  }
  clear_salts(c);
  c->salted = true;
  c->s_order = A5X_SALT_ORDER_PASS_SALT;
  c->n_salts = S;
  c->s_bytes.swap(sb);
  c->s_off.swap(so);
  c->s_recs.swap(recs);
  c->it_iters.swap(its);
  c->it_keys.resize(n);
  for (uint64_t i = 0; i < n; i++) {
    if (keys) c->it_keys[i].swap((*keys)[i]);
    else c->it_keys[i].assign(dig + 16 * i, dig + 16 * i + 16);
    std::array<uint8_t, 16> k16;
    memcpy(k16.data(), dig + 16 * i, 16);
    c->it_by_key[std::make_pair(tidx[i], k16)].push_back(i);
  }
  if (lines) c->it_lines.swap(*lines);
  c->it_tidx.swap(tidx);
  return A5X_OK;
}

int a5x_set_iterated_targets(a5x_ctx* c, int algo, const uint8_t* dig, uint64_t n, const uint8_t* salt_bytes,
                             const uint64_t* salt_off, const uint32_t* iters) {
  return set_iterated(c, algo, dig, n, salt_bytes, salt_off, iters, nullptr, nullptr);
}

static const char* pbkdf2_name(int algo) {
  return algo == A5X_ALGO_PBKDF2_HMAC_MD5 ? "md5" : algo == A5X_ALGO_PBKDF2_HMAC_SHA1 ? "sha1"
       : algo == A5X_ALGO_PBKDF2_HMAC_SHA256 ? "sha256" : "sha512";
}
// standard base64 with padding; false: not such a text
static bool b64_decode(const uint8_t* p, size_t n, std::vector<uint8_t>& out) {
  out.clear();
  if (n % 4) return false;
  auto val = [](uint8_t ch) -> int {
    return ch >= 'A' && ch <= 'Z' ? ch - 'A' : ch >= 'a' && ch <= 'z' ? ch - 'a' + 26 : ch >= '0' && ch <= '9' ? ch - '0' + 52
         : ch == '+' ? 62 : ch == '/' ? 63 : -1;
  };
  for (size_t i = 0; i < n; i += 4) {
    int v[4], pad = 0;
    for (int k = 0; k < 4; k++) {
      if (p[i + k] == '=') {
        if (i + 4 != n || k < 2) return false;
        v[k] = 0;
        pad++;
      } else {
        if (pad) return false;  // a character behind padding
        if ((v[k] = val(p[i + k])) < 0) return false;
      }
    }
    const uint32_t w = (uint32_t)v[0] << 18 | (uint32_t)v[1] << 12 | (uint32_t)v[2] << 6 | (uint32_t)v[3];
    if ((pad == 1 && (w & 0xffu)) || (pad == 2 && (w & 0xffffu))) return false;  // (bits that decode to nothing)
    out.push_back((uint8_t)(w >> 16));
    if (pad < 2) out.push_back((uint8_t)(w >> 8));
    if (pad < 1) out.push_back((uint8_t)w);
  }
  return true;
}
static std::string b64_encode(const uint8_t* p, size_t n) {
  static const char* T = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string o;
  for (size_t i = 0; i < n; i += 3) {
    const uint32_t w = (uint32_t)p[i] << 16 | (i + 1 < n ? (uint32_t)p[i + 1] << 8 : 0u) | (i + 2 < n ? p[i + 2] : 0u);
    o += T[w >> 18];
    o += T[(w >> 12) & 63];
    o += i + 1 < n ? T[(w >> 6) & 63] : '=';
    o += i + 2 < n ? T[w & 63] : '=';
  }
  return o;
}

int a5x_load_pbkdf2_hashes(a5x_ctx* c, int algo, const uint8_t* text, size_t len, uint64_t* n_targets, uint64_t* n_salts,
                           uint64_t* n_skipped) {
  if (!c || (len && !text)) return A5X_E_ARG;
  if (!a5x_algo_pbkdf2(algo)) return fail(c, A5X_E_ARG, "digest algorithm %d is not an iterated one (72..75)", algo);
  const std::string name = pbkdf2_name(algo);
  std::vector<uint8_t> dig, sb, salt, key;
  std::vector<uint64_t> so(1, 0);
  std::vector<uint32_t> its;
  std::vector<std::vector<uint8_t>> keys;
  std::vector<std::string> lines;
  uint64_t bad = 0;
  for (size_t p = 0; p < len;) {
    size_t e = p;
    while (e < len && text[e] != '\n') e++;
    size_t n = e - p;
    const uint8_t* l = text + p;
    p = e + 1;
    if (n && l[n - 1] == '\r') n--;
    if (!n) continue;  // (an empty line is no target and no error)
    // name : iterations : base64(salt) : base64(dk) -- base64 has no ':', so exactly three of them
    size_t f[5] = {0, 0, 0, 0, n + 1};
    int nf = 1;
    for (size_t k = 0; k < n; k++)
      if (l[k] == ':') {
        if (nf < 4) f[nf] = k + 1;
        nf++;
      }
    bool ok = nf == 4 && std::string((const char*)l, f[1] - 1) == name;
    uint64_t it = 0;
    if (ok) {
      ok = f[2] - 1 > f[1] && f[2] - 1 - f[1] <= 10;
      for (size_t k = f[1]; ok && k < f[2] - 1; k++) {
        if (l[k] < '0' || l[k] > '9') ok = false;
        else it = it * 10 + (l[k] - '0');
      }
      if (it == 0 || it > 0xffffffffull) ok = false;
    }
    ok = ok && b64_decode(l + f[2], f[3] - 1 - f[2], salt) && salt.size() <= A5X_SALT_MAX;
    ok = ok && b64_decode(l + f[3], n - f[3], key) && key.size() >= A5X_PBKDF2_KEEP_BYTES;
    if (!ok) { bad++; continue; }
    dig.insert(dig.end(), key.begin(), key.begin() + 16);
    sb.insert(sb.end(), salt.begin(), salt.end());
    so.push_back(sb.size());
    its.push_back((uint32_t)it);
    keys.push_back(key);
    lines.emplace_back((const char*)l, n);
  }
  const uint64_t n = its.size();
  if (n_skipped) *n_skipped = bad;
  const int rc = set_iterated(c, algo, dig.data(), n, sb.data(), so.data(), its.data(), &keys, &lines);
  if (rc) return rc;
  if (n_targets) *n_targets = n;
  if (n_salts) *n_salts = c->n_salts;
  return A5X_OK;
}

int a5x_salt_iterations(a5x_ctx* c, uint32_t index, uint32_t* iters) {
  if (!c || !iters) return A5X_E_ARG;
  if (!c->salted || index >= c->it_iters.size())
    return fail(c, A5X_E_ARG, "index %u of %zu of an iterated set", index, c->it_iters.size());
  *iters = c->it_iters[index];
  return A5X_OK;
}

int a5x_debug_pbkdf2(int algo, const uint8_t* pass, size_t len, const uint8_t* salt, size_t slen, uint32_t iters,
                     uint8_t* out, size_t dklen) {
  if (!a5x_algo_pbkdf2(algo) || (!pass && len) || (!salt && slen) || slen > A5X_SALT_MAX || !iters || (!out && dklen))
    return A5X_E_ARG;
  if (len > A5X_RULE_LMAX) return A5X_E_UNSUPPORTED;
  ShaBytes src;
  src.p = pass;
  src.n = (uint32_t)len;
  return pbkdf2_host_any(algo, src, (uint32_t)len, salt, (uint32_t)slen, iters, out, dklen) ? A5X_OK : A5X_E_ARG;
}

int a5x_debug_iter_budget(a5x_ctx* c, uint64_t pair_slots, uint64_t pair_iterations, uint64_t* loop_launches) {
  if (!c) return A5X_E_ARG;
  c->it_slots = pair_slots;
  c->it_pair_iters = pair_iterations;
  if (loop_launches) *loop_launches = c->it_launches;
  return A5X_OK;
}

int a5x_load_salted_hashes(a5x_ctx* c, int algo, int order, const uint8_t* text, size_t len, int hex_salt,
                           uint64_t* n_targets, uint64_t* n_salts, uint64_t* n_skipped) {
  if (!c || (len && !text)) return A5X_E_ARG;
  const uint32_t W = algo_size(algo);
  if (!W || algo_unsalted(algo)) return fail(c, A5X_E_ARG, "no salted mode for digest algorithm %d", algo);
  if (a5x_algo_pbkdf2(algo)) return fail(c, A5X_E_ARG, "digest algorithm %d is iterated (a5x_load_pbkdf2_hashes)", algo);
  auto hexv = [](uint8_t ch) -> int {
    return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1;
  };
  std::vector<uint8_t> dig, sb;
  std::vector<uint64_t> so(1, 0);
  uint64_t bad = 0;
  for (size_t p = 0; p < len;) {
    size_t e = p;
    while (e < len && text[e] != '\n') e++;
    size_t n = e - p;
    const uint8_t* l = text + p;
    p = e + 1;
    if (n && l[n - 1] == '\r') n--;
    if (!n) continue;  // (an empty line is no target and no error)
    uint8_t d[64];
    bool ok = n > 2u * W && l[2u * W] == ':';  // the digest, then the first ':'
    for (uint32_t k = 0; ok && k < 2u * W; k++) {
      const int v = hexv(l[k]);
      if (v < 0) ok = false;
      else if (k & 1u) d[k / 2] |= (uint8_t)v;
      else d[k / 2] = (uint8_t)(v << 4);
    }
    const uint8_t* s = l + 2u * W + 1u;
    size_t sl = ok ? n - (2u * W + 1u) : 0;
    uint8_t raw[A5X_SALT_MAX];
    if (ok && hex_salt) {
      ok = (sl & 1u) == 0 && sl / 2 <= A5X_SALT_MAX;
      for (size_t k = 0; ok && k < sl; k += 2) {
        const int hi = hexv(s[k]), lo = hexv(s[k + 1]);
        if (hi < 0 || lo < 0) ok = false;
        else raw[k / 2] = (uint8_t)(hi << 4 | lo);
      }
      s = raw;
      sl /= 2;
    }
    if (ok && sl > A5X_SALT_MAX) ok = false;
    if (!ok) { bad++; continue; }
    dig.insert(dig.end(), d, d + W);
    sb.insert(sb.end(), s, s + sl);
    so.push_back(sb.size());
  }
  const uint64_t n = so.size() - 1;
  if (n_skipped) *n_skipped = bad;
  const int rc = a5x_set_salted_targets(c, algo, order, dig.data(), n, sb.data(), so.data());
  if (rc) return rc;
  if (n_targets) *n_targets = n;
  if (n_salts) *n_salts = c->n_salts;
  return A5X_OK;
}

int a5x_salt_count(const a5x_ctx* c) { return c ? (c->salted ? (int)c->n_salts : 0) : A5X_E_ARG; }

int a5x_salt_get(a5x_ctx* c, uint32_t index, uint8_t* out, size_t cap, size_t* out_len) {
  if (!c || !out_len) return A5X_E_ARG;
  if (!c->salted || index >= c->n_salts) return fail(c, A5X_E_ARG, "salt %u of %u", index, c->salted ? c->n_salts : 0u);
  const size_t sl = (size_t)(c->s_off[index + 1] - c->s_off[index]);
  *out_len = sl;
  if (!out) return A5X_OK;
  if (cap < sl) return fail(c, A5X_E_CAPACITY, "salt of %zu bytes, buffer has %zu", sl, cap);
  if (sl) memcpy(out, c->s_bytes.data() + c->s_off[index], sl);
  return A5X_OK;
}

int a5x_hit_salts(a5x_ctx* c, uint32_t* salt_out, uint64_t cap, uint64_t* n) {
  if (!c || !n) return A5X_E_ARG;
  *n = c->s_hit_salt.size();
  if (!salt_out) return A5X_OK;
  if (cap < c->s_hit_salt.size())
    return fail(c, A5X_E_CAPACITY, "%zu hit salts, buffer has %llu", c->s_hit_salt.size(), (unsigned long long)cap);
  if (!c->s_hit_salt.empty()) memcpy(salt_out, c->s_hit_salt.data(), c->s_hit_salt.size() * 4);
  return A5X_OK;
}

int a5x_salts_last(a5x_ctx* c, uint64_t* hashed, uint64_t* skipped) {
  if (!c) return A5X_E_ARG;
  if (hashed) *hashed = c->s_hashed;
  if (skipped) *skipped = c->s_skipped;
  return A5X_OK;
}

int a5x_digest_lines_salted_device(a5x_ctx* c, int algo, int order, const uint8_t* d_lines, uint64_t nbytes,
                                   uint8_t* d_dig, uint64_t cap, uint64_t* n_lines, void* stream) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nbytes && !d_lines)) return A5X_E_ARG;
  if (!algo_size(algo) || algo_unsalted(algo)) return fail(c, A5X_E_ARG, "no salted mode for digest algorithm %d", algo);
  if (order != A5X_SALT_ORDER_PASS_SALT && order != A5X_SALT_ORDER_SALT_PASS) return fail(c, A5X_E_ARG, "bad salt order %d", order);
  if (!c->salted || !c->n_salts) return fail(c, A5X_E_ARG, "no salted target set (a5x_set_salted_targets)");
  const bool own = algo_salted_only(algo);  // its own salt records: the set's algorithm only
  if (own && order != salted_only_order(algo))
    return fail(c, A5X_E_ARG, "salt order %d: digest algorithm %d places its salt by order %d", order, algo, salted_only_order(algo));
  if ((own || algo_salted_only(c->t_algo)) && algo != c->t_algo)
    return fail(c, A5X_E_ARG, "digest algorithm %d: the set's salt records are built for algorithm %d", algo, c->t_algo);
  if (((uintptr_t)d_lines & 15u) != 0) return fail(c, A5X_E_ARG, "d_lines must be 16-byte aligned");
  if (((uintptr_t)d_dig & 3u) != 0) return fail(c, A5X_E_ARG, "d_digests must be 4-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if (n_lines) *n_lines = 0;
  c->s_hashed = c->s_skipped = 0;
  c->s_hit_salt.clear();
  if (!nbytes) return A5X_OK;
  int rc;
  if ((rc = grow(c, c->r_counter, 2))) return rc;
  if (a5x_algo_pbkdf2(algo)) {
    // an iterated set: the passes of iter_stream, each ended by the compare step's op 2 twin
    const uint32_t S = c->n_salts;
    const uint64_t nblk = a5x_stream_blocks(nbytes);
    uint64_t lines = 0;
    unsigned long long skp = 0;
    c->it_launches = 0;
    HIPCHK(c, hipMemsetAsync(c->d_scalars, 0, S_GUARD * sizeof(uint32_t), st));
    HIPCHK(c, hipMemsetAsync(c->r_counter.p, 0, 8, st));
    A5xPbkdf2Launch L;
    memset(&L, 0, sizeof L);
    L.s.d = dig_launch(c);
    L.s.d.algo = algo;
    L.s.d.out = d_lines;
    L.s.d.nbytes = nbytes;
    L.s.salts = c->s_table.p;
    L.s.nsalts = S;
    L.s.order = order;
    L.s.skipped = c->r_counter.p;
    auto op1 = [&] {
      L.s.d.blk_cnt = c->dg_blk_cnt.p;
      L.b0 = 0; L.b1 = nblk;
      return a5x_launch_pbkdf2_init(L, 1, (uint32_t)std::max(1, c->cus), st);
    };
    if ((rc = stream_count_lines(c, op1, nblk, st, &lines))) return rc;
    if (n_lines) *n_lines = lines;
    if (lines > cap / S || !d_dig)
      return fail(c, A5X_E_CAPACITY, "%llu lines x %u salts, digest buffer has room for %llu", (unsigned long long)lines, S,
                  (unsigned long long)cap);
    L.s.d.blk_pre = c->dg_blk_pre.p;
    L.s.d.dig_out = d_dig;
    HIPCHK(c, hipMemsetAsync(d_dig, 0, lines * S * 16, st));  // a skipped pair's bytes
    if ((rc = iter_stream(c, L, nblk, st, [&](A5xPbkdf2Launch& Lp) -> int {
           HIPCHK(c, a5x_launch_pbkdf2_compare(Lp, 2, st));
           return A5X_OK;
         })))
      return rc;
    HIPCHK(c, read_scalars(c, st, S_ERR));
    HIPCHK(c, hipMemcpyAsync(&skp, c->r_counter.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (skp > lines * S) return fail(c, A5X_E_HIP, "more skipped pairs than pairs");
    c->s_skipped = skp;
    c->s_hashed = lines * S - skp;
    return decode_dev_err(c, c->h_scalars[S_ERR]);
  }
  A5xSaltLaunch SL;
  SL.salts = c->s_table.p;
  SL.nsalts = c->n_salts;
  SL.order = order;
  SL.hit_salt = nullptr;
  SL.skipped = c->r_counter.p;
  auto launch = [&](int op) {
    const uint32_t cus = (uint32_t)std::max(1, c->cus);
    return launch_salted(algo, SL, op, cus, st);
  };
  uint64_t lines = 0;
  unsigned long long skp = 0;
  if ((rc = digest_lines_multi(c, SL, launch, algo, d_lines, nbytes, d_dig, cap, c->n_salts, "salts", n_lines, st, &lines,
                               &skp)))
    return rc;
  if (skp > lines * c->n_salts) return fail(c, A5X_E_HIP, "more skipped pairs than pairs");
  c->s_skipped = skp;
  c->s_hashed = lines * c->n_salts - skp;
  return decode_dev_err(c, c->h_scalars[S_ERR]);
}

int a5x_debug_digest_salted(int algo, int order, const uint8_t* salt, size_t slen, const uint8_t* msg, size_t len,
                            uint8_t* out, size_t cap) {
  const uint32_t W = algo_size(algo);
  if (!W || algo_unsalted(algo) || (order != A5X_SALT_ORDER_PASS_SALT && order != A5X_SALT_ORDER_SALT_PASS) ||
      (!salt && slen) || (!msg && len) || !out || slen > A5X_SALT_MAX || a5x_algo_pbkdf2(algo))
    return A5X_E_ARG;
  if (algo_salted_only(algo) && order != salted_only_order(algo)) return A5X_E_ARG;
  if (cap < W) return A5X_E_CAPACITY;
  if (a5x_algo_hmac(algo)) {  // the host path of a5x_hmac.h: only a candidate over 128 bytes is skipped
    if (len > A5X_RULE_LMAX) return A5X_E_UNSUPPORTED;
    ShaBytes src;
    src.p = msg;
    src.n = (uint32_t)len;
    uint32_t d[16];
    if (!hmac_pair_host_any(algo, src, (uint32_t)len, salt, (uint32_t)slen, d)) return A5X_E_ARG;
    memcpy(out, d, W);
    return A5X_OK;
  }
  if (algo_salted_only(algo)) {  // the host path of a5x_salt_nest.h: only a candidate over 128 bytes is skipped
    if (len > A5X_RULE_LMAX) return A5X_E_UNSUPPORTED;
    ShaBytes src;
    src.p = msg;
    src.n = (uint32_t)len;
    uint32_t w[A5X_SNEST_PW], d[5];
    if (!snest_pair_host_any(algo, src, (uint32_t)len, salt, (uint32_t)slen, w, d)) return A5X_E_ARG;
    memcpy(out, d, W);
    return A5X_OK;
  }
  if (len > A5X_RULE_LMAX || !salt_fits((uint32_t)len, (uint32_t)slen)) return A5X_E_UNSUPPORTED;  // a skipped pair
  uint32_t rec[A5X_SALT_STRIDE] = {0}, w[A5X_RULE_NDW] = {0};
  rec[A5X_SALT_R_LEN] = (uint32_t)slen;
  if (slen) memcpy(rec + A5X_SALT_R_BYTES, salt, slen);
  SaltRec sr;
  sr.r = rec;
  SaltBuf b;
  b.w = w;
  SaltCandBytes cand;
  cand.p = msg;
  cand.n = (uint32_t)len;
  if (order == A5X_SALT_ORDER_PASS_SALT) {
    const uint32_t dirty = salt_copy_cand(b, cand, (uint32_t)len, 0u);
    salt_append(b, (uint32_t)len, dirty, sr, (uint32_t)slen);
  } else {
    salt_prefix_cand(b, cand, (uint32_t)len, (uint32_t)slen, 0u);
    salt_prefix_salt(b, sr, (uint32_t)slen);
  }
  const uint32_t L = (uint32_t)(len + slen);
  // (test hook: the zero-past-the-message invariant of a5x_salt.h holds after the placement)
  for (uint32_t i = L; i < 4u * A5X_RULE_NDW; i++)
    if (((const uint8_t*)w)[i]) return A5X_E_BOUNDS;
  uint32_t d[16];
  switch (algo) {
    case A5X_ALGO_MD5: md5_src_hd(b, L, d); break;
    case A5X_ALGO_SHA1: sha_digest<A5X_ALGO_SHA1>(b, L, d); break;
    case A5X_ALGO_SHA256: sha_digest<A5X_ALGO_SHA256>(b, L, d); break;
    case A5X_ALGO_SHA224: sha_digest<A5X_ALGO_SHA224>(b, L, d); break;
    case A5X_ALGO_SHA384: sha_digest<A5X_ALGO_SHA384>(b, L, d); break;
    default: sha_digest<A5X_ALGO_SHA512>(b, L, d); break;
  }
  memcpy(out, d, W);
  return A5X_OK;
}

int a5x_expand_digest_device(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode,
                             int mn, int mx, uint64_t scratch_bytes, a5x_hit* hits, uint64_t hit_cap,
                             uint64_t* n_hits, a5x_stats* stats, void* stream) {
  // (the whole batch is the range [0, ~0): the same checks, the same call)
  return a5x_expand_digest_range_device(c, d_words, d_woff, nw, mode, mn, mx, 0, ~0ull, scratch_bytes, hits, hit_cap,
                                        n_hits, stats, stream);
}

int a5x_expand_digest_range_device(a5x_ctx* c, const uint8_t* d_words, const uint64_t* d_woff, uint64_t nw, int mode,
                                   int mn, int mx, uint64_t cand_begin, uint64_t cand_end, uint64_t scratch_bytes,
                                   a5x_hit* hits, uint64_t hit_cap, uint64_t* n_hits, a5x_stats* stats, void* stream) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nw && (!d_words || !d_woff)) || (hit_cap && !hits) || cand_end < cand_begin) return A5X_E_ARG;
  if (c->t_algo < 0) return fail(c, A5X_E_ARG, "no target set (a5x_set_targets)");
  int rc;
  if ((rc = check_mode(c, mode))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const bool fused = !getenv("A5X_NO_FUSED_DIGEST");
  return expand_digest(c, d_words, d_woff, nw, mode, mn, mx, cand_begin, cand_end, scratch_bytes, hits, hit_cap,
                       n_hits, stats, stream ? (hipStream_t)stream : c->stream, fused);
}

int a5x_expand_digest(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw, int mode, int mn, int mx,
                      a5x_hit* hits, uint64_t hit_cap, uint64_t* n_hits, a5x_stats* stats) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nw && (!words || !woff))) return A5X_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = stage_words(c, words, woff, nw))) return rc;
  return a5x_expand_digest_device(c, c->s_words.p, c->s_woff.p, nw, mode, mn, mx, 0, hits, hit_cap, n_hits, stats,
                                  c->stream);
}

int a5x_digest_lines_device(a5x_ctx* c, int algo, const uint8_t* d_lines, uint64_t nbytes, uint8_t* d_dig,
                            uint64_t cap, uint64_t* n_lines, void* stream) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nbytes && !d_lines)) return A5X_E_ARG;
  if (!algo_size(algo)) return fail(c, A5X_E_ARG, "bad digest algorithm %d", algo);
  if (algo_salted_only(algo)) return fail(c, A5X_E_ARG, "digest algorithm %d is salted only (a5x_digest_lines_salted_device)", algo);
  if (((uintptr_t)d_lines & 15u) != 0) return fail(c, A5X_E_ARG, "d_lines must be 16-byte aligned");
  if (algo_size(algo) > 16 && ((uintptr_t)d_dig & 3u) != 0) return fail(c, A5X_E_ARG, "d_digests must be 4-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if (n_lines) *n_lines = 0;
  if (!nbytes) return A5X_OK;
  HIPCHK(c, hipMemsetAsync(c->d_scalars, 0, S_GUARD * sizeof(uint32_t), st));  // the counters before the guard record
  A5xDigLaunch D = dig_launch(c);
  D.algo = algo;
  D.out = d_lines;
  D.nbytes = nbytes;
  uint64_t lines = 0;
  int rc;
  if ((rc = dig_block_prefix(c, D, st, &lines))) return rc;
  if (n_lines) *n_lines = lines;
  if (lines > cap || !d_dig)
    return fail(c, A5X_E_CAPACITY, "%llu lines, digest buffer has room for %llu", (unsigned long long)lines,
                (unsigned long long)cap);
  D.dig_out = d_dig;
  HIPCHK(c, a5x_launch_digest_stream(D, 2, dig_grid(c), st));
  HIPCHK(c, read_scalars(c, st, S_ERR));
  HIPCHK(c, hipStreamSynchronize(st));
  return decode_dev_err(c, c->h_scalars[S_ERR]);
}

int a5x_digest_size(int algo) {
  const uint32_t w = algo_size(algo);
  return w ? (int)w : A5X_E_ARG;
}

int a5x_algo_salt_order(int algo) {
  const int o = salted_only_order(algo);
  return o < 0 ? A5X_E_ARG : o;
}

int a5x_hit_digest(a5x_ctx* c, const a5x_hit* hit, uint8_t* out, size_t cap, size_t* out_len) {
  if (!c || !hit || !out_len) return A5X_E_ARG;
  if (c->t_algo < 0) return fail(c, A5X_E_ARG, "no target set (a5x_set_targets)");
  const uint32_t W = algo_size(c->t_algo);
  *out_len = W;
  if (!out) return A5X_OK;
  if (cap < W) return fail(c, A5X_E_CAPACITY, "digest of %u bytes, buffer has %zu", W, cap);
  uint8_t d[64];
  const int rc = hit_full_digest(c, hit, d);
  if (rc) return rc;
  memcpy(out, d, W);
  return A5X_OK;
}

int a5x_debug_digest(int algo, const uint8_t* msg, size_t len, uint8_t* out, size_t cap) {
  // (MD5 and NTLM have no host core here: the kernels' are device code)
  if (algo == A5X_ALGO_MD5 || algo == A5X_ALGO_NTLM || !algo_size(algo) || (!msg && len) || !out || len > 0xffffff00u)
    return A5X_E_ARG;
  const uint32_t W = algo_size(algo);
  if (cap < W) return A5X_E_CAPACITY;
  ShaBytes src;
  src.p = msg;
  src.n = (uint32_t)len;
  uint32_t d[16];
  switch (algo) {
    case A5X_ALGO_SHA1: sha_digest<A5X_ALGO_SHA1>(src, (uint32_t)len, d); break;
    case A5X_ALGO_SHA256: sha_digest<A5X_ALGO_SHA256>(src, (uint32_t)len, d); break;
    case A5X_ALGO_SHA224: sha_digest<A5X_ALGO_SHA224>(src, (uint32_t)len, d); break;
    case A5X_ALGO_SHA384: sha_digest<A5X_ALGO_SHA384>(src, (uint32_t)len, d); break;
    case A5X_ALGO_SHA512: sha_digest<A5X_ALGO_SHA512>(src, (uint32_t)len, d); break;
    case A5X_ALGO_MD5_MD5: nest_digest<A5X_ALGO_MD5_MD5>(src, (uint32_t)len, d); break;
    case A5X_ALGO_MD5_MD5_MD5: nest_digest<A5X_ALGO_MD5_MD5_MD5>(src, (uint32_t)len, d); break;
    case A5X_ALGO_MD5_MD5UP: nest_digest<A5X_ALGO_MD5_MD5UP>(src, (uint32_t)len, d); break;
    case A5X_ALGO_MD5_SHA1: nest_digest<A5X_ALGO_MD5_SHA1>(src, (uint32_t)len, d); break;
    case A5X_ALGO_SHA1_SHA1: nest_digest<A5X_ALGO_SHA1_SHA1>(src, (uint32_t)len, d); break;
    case A5X_ALGO_SHA1_MD5: nest_digest<A5X_ALGO_SHA1_MD5>(src, (uint32_t)len, d); break;
    case A5X_ALGO_SHA256_MD5: nest_digest<A5X_ALGO_SHA256_MD5>(src, (uint32_t)len, d); break;
    default: return A5X_E_ARG;
  }
  memcpy(out, d, W);
  return A5X_OK;
}

int a5x_debug_target_set(uint32_t width, const uint8_t* dig, uint64_t n, uint64_t* info, uint32_t* table,
                         size_t table_cap, uint32_t* tails, size_t tails_cap, uint32_t* ztails, size_t ztails_cap,
                         uint32_t* bitmap, size_t bitmap_cap) {
  const bool known = width == 16 || width == 20 || width == 28 || width == 32 || width == 48 || width == 64;
  if (!known || (n && !dig) || !info) return A5X_E_ARG;
  TargetSet T;
  build_target_set(width, dig, n, T);
  info[0] = T.bm_log2;
  info[1] = T.tmask + 1;
  info[2] = T.has_zero;
  info[3] = T.shared ? 1 : 0;
  info[4] = T.tab.size() * 4;
  info[5] = T.tails.size();
  info[6] = T.ztails.size();
  info[7] = T.bm.size();
  if (!table && !tails && !ztails && !bitmap) return A5X_OK;  // the size query
  if (!table || !bitmap || (!tails && info[5]) || (!ztails && info[6])) return A5X_E_ARG;
  if (table_cap < info[4] || tails_cap < info[5] || ztails_cap < info[6] || bitmap_cap < info[7]) return A5X_E_CAPACITY;
  memcpy(table, T.tab.data(), T.tab.size() * sizeof(uint4));
  if (info[5]) memcpy(tails, T.tails.data(), T.tails.size() * 4);
  if (info[6]) memcpy(ztails, T.ztails.data(), T.ztails.size() * 4);
  memcpy(bitmap, T.bm.data(), T.bm.size() * 4);
  return A5X_OK;
}

int a5x_partition(const uint64_t* prefix, uint64_t n, uint32_t parts, uint64_t* split) {
  if (!prefix || !split || parts == 0) return A5X_E_ARG;
  const uint64_t total = prefix[n];
  split[0] = 0;
  for (uint32_t r = 1; r < parts; r++) {
    const unsigned __int128 target = (unsigned __int128)total * r / parts;
    // first word i whose start offset >= target
    uint64_t lo = split[r - 1], hi = n;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if ((unsigned __int128)prefix[mid] < target) lo = mid + 1; else hi = mid;
    }
    split[r] = lo;
  }
  split[parts] = n;
  return A5X_OK;
}

// ---- hashcat-style hit output (README.MD:74-106, :168) ------------
// hashcat's outfile auto-hex convention, restated (hashcat is not part of the
// reference): a plain is written as $HEX[lowercase hex] when it is not valid UTF-8
// (Go utf8.Valid rules), contains a control byte (< 0x20 or 0x7f, which would break
// the "hash:plain" line), or itself has the $HEX[...] form.
static bool plain_needs_hex(const uint8_t* p, size_t n) {
  if (n >= 6 && memcmp(p, "$HEX[", 5) == 0 && p[n - 1] == ']') return true;
  for (size_t i = 0; i < n;) {
    if (p[i] < 0x20 || p[i] == 0x7f) return true;
    int sz;
    const int r = a5x::gosem::decode_rune(p + i, n - i, &sz);
    if (r == a5x::gosem::kRuneError && sz == 1) return true;  // invalid byte (a literal U+FFFD has sz 3)
    i += (size_t)sz;
  }
  return false;
}

static void append_plain(std::string& o, const uint8_t* p, size_t n) {
  static const char* hx = "0123456789abcdef";
  if (!plain_needs_hex(p, n)) {
    o.append((const char*)p, n);
    return;
  }
  o += "$HEX[";
  for (size_t i = 0; i < n; i++) {
    o += hx[p[i] >> 4];
    o += hx[p[i] & 15];
  }
  o += ']';
}

int a5x_format_plain(const uint8_t* plain, size_t len, uint8_t* out, size_t cap, size_t* out_len) {
  if ((!plain && len) || !out_len) return A5X_E_ARG;
  std::string o;
  append_plain(o, plain, len);
  *out_len = o.size();
  if (!out || cap < o.size()) return out ? A5X_E_CAPACITY : A5X_OK;
  memcpy(out, o.data(), o.size());
  return A5X_OK;
}

// a5x_format_hits, and with hit_rule a5x_format_hits_rules: each regenerated plain goes
// through its hit's rule on the host (the interpreter the kernel ran); with hit_salt
// a5x_format_hits_salted: "hexdigest:salt:plain", the salt raw or (hex_salt) in hex
static int format_hits(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw, int mode, int mn, int mx,
                       const a5x_hit* hits, uint64_t n_hits, const uint32_t* hit_rule, a5x_sink_fn sink, void* user,
                       const uint32_t* hit_salt = nullptr, int hex_salt = 0, uint64_t* it_dropped = nullptr,
                       bool iterated = false) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || !sink || (n_hits && (!hits || !words || !woff))) return A5X_E_ARG;
  if (!n_hits) return A5X_OK;
  int rc;
  if ((rc = check_mode(c, mode))) return rc;
  // the digests to print: the hits' own 16 bytes, or the full-width digests of a wide target set
  const uint32_t dsz = c->t_tw ? algo_size(c->t_algo) : 16u;
  std::vector<uint8_t> full((size_t)dsz * n_hits);
  for (uint64_t h = 0; h < n_hits; h++) {
    if (!c->t_tw) memcpy(&full[(size_t)16 * h], hits[h].digest, 16);
    else if ((rc = hit_full_digest(c, &hits[h], &full[(size_t)dsz * h]))) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  // The hit words, once each, as a sub-batch; only the hit candidates themselves are
  // regenerated on the device (located, then expanded as single-candidate ranges, or
  // one range per run of nearby hits), never a hit word's whole keyspace: a word's
  // output may exceed host memory and 2^32 bytes.
  std::vector<uint64_t> uw(n_hits);
  for (uint64_t h = 0; h < n_hits; h++) {
    if (hits[h].word >= nw) return fail(c, A5X_E_ARG, "hit word index beyond the batch");
    uw[h] = hits[h].word;
  }
  std::sort(uw.begin(), uw.end());
  uw.erase(std::unique(uw.begin(), uw.end()), uw.end());
  std::vector<uint8_t> sb;
  std::vector<uint64_t> so(1, 0);
  for (uint64_t w : uw) {
    sb.insert(sb.end(), words + woff[w], words + woff[w + 1]);
    so.push_back(sb.size());
  }
  sb.resize(sb.size() + 16, 0);
  const uint64_t m = uw.size();
  if ((rc = grow(c, c->s_words, sb.size())) || (rc = grow(c, c->s_woff, m + 1))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->s_words.p, sb.data(), sb.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->s_woff.p, so.data(), (m + 1) * 8, hipMemcpyHostToDevice, c->stream));
  Job J{c->s_words.p, c->s_woff.p, m, mode, mn, mx, c->stream};
  if ((rc = job_prepare(c, J, nullptr, nullptr, false))) return rc;
  std::vector<uint64_t> coff(m + 1);
  HIPCHK(c, hipMemcpyAsync(coff.data(), J.B.cand_off, (m + 1) * 8, hipMemcpyDeviceToHost, J.st));
  HIPCHK(c, hipStreamSynchronize(J.st));
  // global candidate index (in the sub-batch) of every hit
  std::vector<uint64_t> g(n_hits);
  for (uint64_t h = 0; h < n_hits; h++) {
    const size_t k = (size_t)(std::lower_bound(uw.begin(), uw.end(), hits[h].word) - uw.begin());
    if (hits[h].cand >= coff[k + 1] - coff[k])
      return fail(c, A5X_E_ARG, "hit candidate index beyond its word's keyspace");
    g[h] = coff[k] + hits[h].cand;
  }
  std::vector<uint64_t> ug(g);
  std::sort(ug.begin(), ug.end());
  ug.erase(std::unique(ug.begin(), ug.end()), ug.end());
  // runs of hit candidates: a run spans at most 4096 candidates (its bytes are checked
  // after the locate: a run over 1 MiB is split into single-candidate ranges)
  struct Run { size_t a, b; };  // ug[a..b)
  std::vector<Run> runs;
  for (size_t i = 0; i < ug.size();) {
    size_t j = i + 1;
    while (j < ug.size() && ug[j] - ug[i] < 4096) j++;
    runs.push_back({i, j});
    i = j;
  }
  std::vector<uint64_t> q;
  for (auto& r : runs) { q.push_back(ug[r.a]); q.push_back(ug[r.b - 1] + 1); }
  std::vector<uint64_t> loc;
  if ((rc = job_locate(c, J, q, loc))) return rc;
  std::vector<Range> ranges;  // one per run, or per candidate of an oversize run
  std::vector<std::pair<size_t, size_t>> rcand;  // ug[first, last) covered by each range
  std::vector<uint64_t> q2;
  std::vector<size_t> split_runs;
  for (size_t r = 0; r < runs.size(); r++) {
    const uint64_t* lb = &loc[3 * (2 * r)];
    const uint64_t* le = &loc[3 * (2 * r + 1)];
    if (le[0] - lb[0] <= (1u << 20) || runs[r].b - runs[r].a == 1) {
      ranges.push_back(range_of(ug[runs[r].a], ug[runs[r].b - 1] + 1, lb, le));
      rcand.push_back({runs[r].a, runs[r].b});
    } else {
      split_runs.push_back(r);
      for (size_t i = runs[r].a; i < runs[r].b; i++) { q2.push_back(ug[i]); q2.push_back(ug[i] + 1); }
    }
  }
  if (!q2.empty()) {
    std::vector<uint64_t> loc2;
    if ((rc = job_locate(c, J, q2, loc2))) return rc;
    size_t t = 0;
    for (size_t r : split_runs)
      for (size_t i = runs[r].a; i < runs[r].b; i++, t++) {
        ranges.push_back(range_of(ug[i], ug[i] + 1, &loc2[3 * (2 * t)], &loc2[3 * (2 * t + 1)]));
        rcand.push_back({i, i + 1});
      }
  }
  // expand every range into the staging buffer and cut out the hit candidates
  std::vector<std::string> plain(ug.size());
  std::vector<uint8_t> hb;
  for (size_t r = 0; r < ranges.size(); r++) {
    const Range& R = ranges[r];
    const uint64_t nb = R.b1 - R.b0;
    if ((rc = grow(c, c->s_out[0], nb + 64))) return rc;
    if ((rc = job_launch(c, J, R, c->s_out[0].p, nb + 64))) return rc;
    hb.resize(nb);
    HIPCHK(c, hipMemcpyAsync(hb.data(), c->s_out[0].p, nb, hipMemcpyDeviceToHost, J.st));
    if ((rc = job_check(c, J))) return rc;
    // the range's lines are candidates R.cb, R.cb + 1, ... in order
    size_t want = rcand[r].first;
    uint64_t cand = R.cb, p0 = 0;
    for (uint64_t x = 0; x < nb && want < rcand[r].second; x++) {
      if (hb[x] != '\n') continue;
      if (cand == ug[want]) plain[want++].assign((const char*)hb.data() + p0, (size_t)(x - p0));
      cand++;
      p0 = x + 1;
    }
    if (want != rcand[r].second) return fail(c, A5X_E_HIP, "hit candidates not found in their located range");
  }
  static const char* hx = "0123456789abcdef";
  std::string o;
  for (uint64_t h = 0; iterated && h < n_hits; h++) {
    // An iterated set: the targets registered with the hit's index and 16 bytes; for each the
    // whole key derived again by the host path and compared with every byte the list gave.
    const size_t k = (size_t)(std::lower_bound(ug.begin(), ug.end(), g[h]) - ug.begin());
    if (!c->salted || !a5x_algo_pbkdf2(c->t_algo) || hit_salt[h] >= c->n_salts)
      return fail(c, A5X_E_ARG, "hit index %u of %u in an iterated set", hit_salt[h], c->salted ? c->n_salts : 0u);
    if (plain[k].size() > A5X_RULE_LMAX) return fail(c, A5X_E_ARG, "hit candidate longer than 128 bytes");
    std::array<uint8_t, 16> k16;
    memcpy(k16.data(), hits[h].digest, 16);
    auto it = c->it_by_key.find(std::make_pair(hit_salt[h], k16));
    bool any = false;
    if (it != c->it_by_key.end()) {
      const uint32_t si = hit_salt[h];
      const uint8_t* salt = c->s_bytes.data() + c->s_off[si];
      const uint32_t slen = (uint32_t)(c->s_off[si + 1] - c->s_off[si]);
      ShaBytes src;
      src.p = (const uint8_t*)plain[k].data();
      src.n = (uint32_t)plain[k].size();
      size_t longest = 0;
      for (uint64_t t : it->second) longest = std::max(longest, c->it_keys[t].size());
      std::vector<uint8_t> dk(longest);
      pbkdf2_host_any(c->t_algo, src, src.n, salt, slen, c->it_iters[si], dk.data(), longest);
      for (uint64_t t : it->second) {
        const std::vector<uint8_t>& key = c->it_keys[t];
        if (memcmp(dk.data(), key.data(), key.size()) != 0) continue;
        any = true;
        if (!c->it_lines.empty()) o += c->it_lines[t];
        else
          o += std::string(pbkdf2_name(c->t_algo)) + ":" + std::to_string(c->it_iters[si]) + ":" + b64_encode(salt, slen) +
               ":" + b64_encode(key.data(), key.size());
        o += ':';
        append_plain(o, (const uint8_t*)plain[k].data(), plain[k].size());
        o += '\n';
      }
    }
    if (!any && it_dropped) ++*it_dropped;
    if (o.size() >= (1u << 20) || (h + 1 == n_hits && !o.empty())) {
      if (sink(user, (const uint8_t*)o.data(), o.size())) return fail(c, A5X_E_SINK, "sink returned non-zero");
      o.clear();
    }
  }
  for (uint64_t h = 0; !iterated && h < n_hits; h++) {
    const size_t k = (size_t)(std::lower_bound(ug.begin(), ug.end(), g[h]) - ug.begin());
    for (uint32_t i = 0; i < dsz; i++) {
      o += hx[full[(size_t)dsz * h + i] >> 4];
      o += hx[full[(size_t)dsz * h + i] & 15];
    }
    o += ':';
    if (hit_salt) {
      if (!c->salted || hit_salt[h] >= c->n_salts)
        return fail(c, A5X_E_ARG, "hit salt %u of %u in the set", hit_salt[h], c->salted ? c->n_salts : 0u);
      for (uint64_t i = c->s_off[hit_salt[h]]; i < c->s_off[hit_salt[h] + 1]; i++) {
        if (hex_salt) { o += hx[c->s_bytes[i] >> 4]; o += hx[c->s_bytes[i] & 15]; }
        else o += (char)c->s_bytes[i];
      }
      o += ':';
    }
    if (hit_rule) {
      if (hit_rule[h] >= c->n_rules) return fail(c, A5X_E_ARG, "hit rule %u of %u loaded", hit_rule[h], c->n_rules);
      if (plain[k].size() > A5X_RULE_LMAX) return fail(c, A5X_E_ARG, "hit candidate longer than the rule limit");
      RuleFlat b;
      memset(&b, 0, sizeof b);
      memcpy(b.w, plain[k].data(), plain[k].size());
      const uint32_t* ops = &c->r_rules[(size_t)hit_rule[h] * A5X_RULE_STRIDE];
      const uint32_t L = rule_apply(b, (uint32_t)plain[k].size(), ops + 1, ops[0]);
      append_plain(o, (const uint8_t*)b.w, L);
    } else {
      append_plain(o, (const uint8_t*)plain[k].data(), plain[k].size());
    }
    o += '\n';
    if (o.size() >= (1u << 20) || h + 1 == n_hits) {
      if (sink(user, (const uint8_t*)o.data(), o.size())) return fail(c, A5X_E_SINK, "sink returned non-zero");
      o.clear();
    }
  }
  return A5X_OK;
}

int a5x_format_hits(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw, int mode, int mn, int mx,
                    const a5x_hit* hits, uint64_t n_hits, a5x_sink_fn sink, void* user) {
  return format_hits(c, words, woff, nw, mode, mn, mx, hits, n_hits, nullptr, sink, user);
}

int a5x_format_hits_rules(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw, int mode, int mn,
                          int mx, const a5x_hit* hits, uint64_t n_hits, const uint32_t* hit_rule, a5x_sink_fn sink,
                          void* user) {
  if (c && n_hits && !hit_rule) return fail(c, A5X_E_ARG, "no rule indices");
  return format_hits(c, words, woff, nw, mode, mn, mx, hits, n_hits, hit_rule, sink, user);
}

int a5x_format_hits_salted(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw, int mode, int mn,
                           int mx, const a5x_hit* hits, uint64_t n_hits, const uint32_t* hit_salt, int hex_salt,
                           a5x_sink_fn sink, void* user) {
  if (c && n_hits && !hit_salt) return fail(c, A5X_E_ARG, "no salt indices");
  return format_hits(c, words, woff, nw, mode, mn, mx, hits, n_hits, nullptr, sink, user, hit_salt, hex_salt);
}

int a5x_format_hits_iterated(a5x_ctx* c, const uint8_t* words, const uint64_t* woff, uint64_t nw, int mode, int mn,
                             int mx, const a5x_hit* hits, uint64_t n_hits, const uint32_t* hit_salt, uint64_t* n_dropped,
                             a5x_sink_fn sink, void* user) {
  if (n_dropped) *n_dropped = 0;
  if (c && n_hits && !hit_salt) return fail(c, A5X_E_ARG, "no salt indices");
  if (c && !(c->salted && a5x_algo_pbkdf2(c->t_algo))) return fail(c, A5X_E_ARG, "the target set is not an iterated one");
  return format_hits(c, words, woff, nw, mode, mn, mx, hits, n_hits, nullptr, sink, user, hit_salt, 0, n_dropped, true);
}

// ---- rules (a5x_rules.h, a5x_rules.hip) -----------------------------------------
int a5x_set_rules(a5x_ctx* c, const uint8_t* text, size_t len, uint32_t* n_rules, uint32_t* n_skipped) {
  if (!c || (len && !text)) return A5X_E_ARG;
  std::vector<uint32_t> tab;
  uint32_t nr = 0, ns = 0;
  for (size_t p = 0; p < len;) {
    size_t e = p;
    while (e < len && text[e] != '\n') e++;
    uint32_t ops[A5X_RULE_OPS_MAX], nops = 0;
    const int k = rule_parse_line(text + p, e - p, ops, &nops);
    if (k == RULE_LINE_SKIPPED) ns++;
    if (k == RULE_LINE_OK) {
      tab.resize((size_t)(nr + 1) * A5X_RULE_STRIDE, 0u);
      tab[(size_t)nr * A5X_RULE_STRIDE] = nops;
      memcpy(&tab[(size_t)nr * A5X_RULE_STRIDE + 1], ops, nops * sizeof(uint32_t));
      nr++;
    }
    p = e + 1;
  }
  if (nr && c->salted)
    return fail(c, A5X_E_UNSUPPORTED, "rules and salted targets together are not supported: the target set is salted (%u salts)",
                c->n_salts);
  if (c->device >= 0 && nr) {
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (no kernel of an earlier call still reads the table)
    if ((rc = grow(c, c->r_table, tab.size()))) return rc;
    HIPCHK(c, hipMemcpy(c->r_table.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  }
  c->r_rules.swap(tab);
  c->n_rules = nr;
  c->r_hit_rule.clear();
  if (n_rules) *n_rules = nr;
  if (n_skipped) *n_skipped = ns;
  return A5X_OK;
}

int a5x_load_rules_file(a5x_ctx* c, const char* path, uint32_t* n_rules, uint32_t* n_skipped) {
  if (!c || !path) return A5X_E_ARG;
  FILE* f = fopen(path, "rb");
  if (!f) return fail(c, A5X_E_IO, "open %s: %s", path, strerror(errno));
  std::vector<uint8_t> d;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) return fail(c, A5X_E_IO, "read %s failed", path);
  return a5x_set_rules(c, d.data(), d.size(), n_rules, n_skipped);
}

int a5x_rule_count(const a5x_ctx* c) { return c ? (int)c->n_rules : A5X_E_ARG; }

int a5x_hit_rules(a5x_ctx* c, uint32_t* rule_out, uint64_t cap, uint64_t* n) {
  if (!c || !n) return A5X_E_ARG;
  *n = c->r_hit_rule.size();
  if (!rule_out) return A5X_OK;
  if (cap < c->r_hit_rule.size())
    return fail(c, A5X_E_CAPACITY, "%zu hit rules, buffer has %llu", c->r_hit_rule.size(), (unsigned long long)cap);
  if (!c->r_hit_rule.empty()) memcpy(rule_out, c->r_hit_rule.data(), c->r_hit_rule.size() * 4);
  return A5X_OK;
}

int a5x_rules_last(a5x_ctx* c, uint64_t* hashed, uint64_t* rejected) {
  if (!c) return A5X_E_ARG;
  if (hashed) *hashed = c->r_hashed;
  if (rejected) *rejected = c->r_rejected;
  return A5X_OK;
}

int a5x_digest_lines_rules_device(a5x_ctx* c, int algo, const uint8_t* d_lines, uint64_t nbytes, uint8_t* d_dig,
                                  uint64_t cap, uint64_t* n_lines, void* stream) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || (nbytes && !d_lines)) return A5X_E_ARG;
  if (!algo_size(algo)) return fail(c, A5X_E_ARG, "bad digest algorithm %d", algo);
  if (algo_salted_only(algo)) return fail(c, A5X_E_ARG, "digest algorithm %d is salted only: no rules on it", algo);
  if (!c->n_rules) return fail(c, A5X_E_ARG, "no rules loaded (a5x_set_rules)");
  if (((uintptr_t)d_lines & 15u) != 0) return fail(c, A5X_E_ARG, "d_lines must be 16-byte aligned");
  if (((uintptr_t)d_dig & 3u) != 0) return fail(c, A5X_E_ARG, "d_digests must be 4-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if (n_lines) *n_lines = 0;
  c->r_rejected = c->r_hashed = 0;
  c->r_hit_rule.clear();
  if (!nbytes) return A5X_OK;
  int rc;
  if ((rc = grow(c, c->r_counter, 2))) return rc;
  A5xRuleLaunch RL;
  RL.rules = c->r_table.p;
  RL.nrules = c->n_rules;
  RL.hit_rule = nullptr;
  RL.rejected = c->r_counter.p;
  auto launch = [&](int op) { return a5x_launch_rules_stream(RL, op, (uint32_t)std::max(1, c->cus), st); };
  uint64_t lines = 0;
  unsigned long long rej = 0;
  if ((rc = digest_lines_multi(c, RL, launch, algo, d_lines, nbytes, d_dig, cap, c->n_rules, "rules", n_lines, st, &lines,
                               &rej)))
    return rc;
  if (rej > lines) return fail(c, A5X_E_HIP, "more rejected lines than lines");
  c->r_rejected = rej;
  c->r_hashed = (lines - rej) * c->n_rules;
  return decode_dev_err(c, c->h_scalars[S_ERR]);
}

int a5x_debug_apply_rule(const uint8_t* rule, size_t rule_len, const uint8_t* word, size_t len, uint8_t* out,
                         size_t cap, size_t* out_len) {
  if ((!rule && rule_len) || (!word && len) || !out_len || len > A5X_RULE_LMAX) return A5X_E_ARG;
  uint32_t ops[A5X_RULE_OPS_MAX], nops = 0;
  if (rule_parse_line(rule, rule_len, ops, &nops) != RULE_LINE_OK) return A5X_E_ARG;
  RuleFlat b;
  memset(&b, 0, sizeof b);
  if (len) memcpy(b.w, word, len);
  const uint32_t L = rule_apply(b, (uint32_t)len, ops, nops);
  // (test hook: the zero-past-the-word invariant of a5x_rules.h holds after every rule)
  for (uint32_t i = L; i < 4u * A5X_RULE_NDW; i++)
    if (((const uint8_t*)b.w)[i]) return A5X_E_BOUNDS;
  *out_len = L;
  if (!out) return A5X_OK;
  if (cap < L) return A5X_E_CAPACITY;
  memcpy(out, b.w, L);
  return A5X_OK;
}

int a5x_dev_alloc(a5x_ctx* c, void** p, size_t bytes) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c || !p) return A5X_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  hipError_t e = hipMalloc(p, bytes ? bytes : 16);
  if (e != hipSuccess) return fail(c, A5X_E_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
  return A5X_OK;
}
int a5x_dev_free(a5x_ctx* c, void* p) {
  if (!c) return A5X_E_ARG;
  if (p) HIPCHK(c, hipFree(p));
  return A5X_OK;
}
int a5x_memcpy_h2d(a5x_ctx* c, void* dst, const void* src, size_t bytes) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c) return A5X_E_ARG;
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return A5X_OK;
}
int a5x_memcpy_d2h(a5x_ctx* c, void* dst, const void* src, size_t bytes) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c) return A5X_E_ARG;
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return A5X_OK;
}
int a5x_synchronize(a5x_ctx* c) {
  if (c && c->device < 0) return fail(c, A5X_E_HIP, "host-only context (device -1) cannot run kernels");
  if (!c) return A5X_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return A5X_OK;
}

}  // extern "C"
