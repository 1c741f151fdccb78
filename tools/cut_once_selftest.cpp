// cut_once_selftest.cpp -- stand-alone host check of the cut-once path of k_keyspace_thread
// (csrc/a5x_plan.h: CutPlanner in the count pass, then PieceBuilder::place_cuts / build_group /
// place_tail from its group descriptors) against CountPlanner<8> and Planner<true, ., ., 8>,
// for sanitizer builds:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I hashcat_a5_table_generator_amd/csrc tools/cut_once_selftest.cpp \
//       -o cut_once_selftest && ./cut_once_selftest
//
// Tables whose keys cannot overlap (distinct one-byte keys and 2-4 byte keys over letters of
// their own, R = 2..8, values of 0..7 bytes), compiled here into the device-table layout of
// a5x_format.h in an exact-size heap block; more than a million words of 0..127 bytes with
// 0..16 units, each in an exact-size heap block (the planners read a word through
// GWord::at / ld only, which never pass its end).  Every word must compare equal
// (cut_once_compare: the count-pass fields and every u64 of the record), or be a word of more
// than 8 groups that is not FAST; the same family as tests/test_plan_cut_once.py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#include "a5x_plan.h"

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  uint32_t below(uint32_t n) { return next() % n; }
  bool chance(uint32_t pct) { return below(100) < pct; }
};

struct KeyDef {
  std::string k;
  std::vector<std::string> vs;
};

// the device table of keys with distinct first bytes (a bucket holds at most one key)
static std::unique_ptr<uint8_t[]> compile(std::vector<KeyDef> ks, size_t* bytes) {
  std::sort(ks.begin(), ks.end(), [](const KeyDef& a, const KeyDef& b) { return (uint8_t)a.k[0] < (uint8_t)b.k[0]; });
  std::vector<uint16_t> bucket(257, 0);
  for (auto& k : ks) bucket[(uint8_t)k.k[0] + 1]++;
  for (int b = 0; b < 256; b++) bucket[b + 1] += bucket[b];
  std::vector<A5xKey> keys;
  std::vector<A5xChoice> ch;
  std::vector<uint8_t> blob;
  auto add_choice = [&](const std::string& s) {
    A5xChoice x;
    memset(&x, 0, sizeof x);
    x.len = (uint16_t)s.size();
    for (size_t i = 0; i < s.size() && i < 4; i++) x.first4 |= (uint32_t)(uint8_t)s[i] << (8 * i);
    x.blob_off = (uint16_t)blob.size();
    blob.insert(blob.end(), s.begin(), s.end());
    ch.push_back(x);
  };
  for (auto& d : ks) {
    A5xKey key;
    memset(&key, 0, sizeof key);
    key.klen = (uint16_t)d.k.size();
    key.nvals = (uint16_t)d.vs.size();
    key.choice_base = (uint32_t)ch.size();
    add_choice(d.k);
    size_t mc = d.k.size(), mn = d.k.size();
    int maxd = -65536;
    for (auto& v : d.vs) {
      add_choice(v);
      key.sumlen += (uint32_t)v.size();
      mc = std::max(mc, v.size());
      mn = std::min(mn, v.size());
      const int dl = (int)v.size() - (int)d.k.size();
      maxd = std::max(maxd, dl);
      if (dl > 0) key.sum_dpos += (uint32_t)dl; else key.sum_dneg += (uint32_t)(-dl);
    }
    key.maxdelta = (int16_t)maxd;
    key.maxclen = (uint16_t)mc;
    key.minclen = (uint16_t)mn;
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
  h.off_bucket2 = (uint32_t)al16(h.off_kmatch + keys.size() * 8);
  h.off_cval = (uint32_t)al16(h.off_bucket2 + 256 * 4);
  h.off_blob = (uint32_t)al16(h.off_cval + ch.size() * 8);
  h.blob_bytes = (uint32_t)blob.size();
  h.total_bytes = (uint32_t)al16(h.off_blob + blob.size());
  h.max_bucket = 1;
  h.lead_only = 1;
  std::unique_ptr<uint8_t[]> out(new uint8_t[h.total_bytes]);
  memset(out.get(), 0, h.total_bytes);
  memcpy(out.get(), &h, sizeof h);
  memcpy(out.get() + h.off_bucket, bucket.data(), 257 * sizeof(uint16_t));
  memcpy(out.get() + h.off_keys, keys.data(), keys.size() * sizeof(A5xKey));
  memcpy(out.get() + h.off_choices, ch.data(), ch.size() * sizeof(A5xChoice));
  if (!blob.empty()) memcpy(out.get() + h.off_blob, blob.data(), blob.size());
  for (size_t k = 0; k < keys.size(); k++) {
    const uint64_t km = (uint64_t)ch[keys[k].choice_base].first4 | ((uint64_t)keys[k].klen << 32);
    memcpy(out.get() + h.off_kmatch + 8 * k, &km, 8);
  }
  for (int b = 0; b < 256; b++) {
    const uint32_t v = (uint32_t)bucket[b] | ((uint32_t)bucket[b + 1] << 16);
    memcpy(out.get() + h.off_bucket2 + 4 * b, &v, 4);
  }
  for (size_t i = 0; i < ch.size(); i++) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < ch[i].len && k < 7; k++) v |= (uint64_t)blob[ch[i].blob_off + k] << (8 * k);
    v |= (uint64_t)ch[i].len << 56;
    memcpy(out.get() + h.off_cval + 8 * i, &v, 8);
  }
  *bytes = h.total_bytes;
  return out;
}

static const char* SINGLE = "abcdefghijklmn";
static const char* MULTI[] = {"PQ", "RS", "TUV", "WXYZ", "ABC", "DE"};
static const char* FILLER = ".,_-+~";

static std::string digits(Rng& r, uint32_t n) {
  std::string s;
  for (uint32_t i = 0; i < n; i++) s += (char)('0' + r.below(10));
  return s;
}
static std::string fill(Rng& r, uint32_t n) {
  std::string s;
  for (uint32_t i = 0; i < n; i++) s += FILLER[r.below(6)];
  return s;
}

int main() {
  Rng r{0xA11};
  size_t words = 0, fast = 0, three = 0, tails = 0, lits = 0, u16 = 0, fails = 0, refused = 0, nine = 0;
  std::vector<u64> rn(CO_NREC), rr(CO_NREC);
  for (int t = 0; t < 500; t++) {
    std::vector<KeyDef> ks;
    const uint32_t n1 = 3 + r.below(8), first = r.below(14 - n1 + 1);
    for (uint32_t i = 0; i < n1; i++) ks.push_back({std::string(1, SINGLE[first + i]), {}});
    const uint32_t nm = 1 + r.below(4), m0 = r.below(6);
    for (uint32_t i = 0; i < nm; i++) ks.push_back({MULTI[(m0 + i) % 6], {}});
    for (size_t i = 0; i < ks.size(); i++) {
      const uint32_t nv = i ? 1 + r.below(7) : 7;
      for (uint32_t v = 0; v < nv; v++) ks[i].vs.push_back(digits(r, r.below(8)));
    }
    ks[0].vs = {"1"};        // R = 2: three of them fill a group
    ks[1].vs = {"2222222"};  // a 7-byte value
    ks[2].vs = {""};         // an empty value
    // every eighth table: a key of R = 9 or with an 8-byte value, which the 8-entry group refuses
    const bool refusing = t % 8 == 7;
    if (refusing) {
      if (t % 16 == 7) ks.back().vs = {"1", "2", "3", "4", "5", "6", "7", "8"};
      else ks.back().vs = {"12345678"};
    }
    size_t tb = 0;
    const std::unique_ptr<uint8_t[]> blob = compile(ks, &tb);
    const Tab T = tab_view(blob.get());
    const std::string r2 = ks[0].k;
    std::vector<std::string> ws = {"", ".", std::string(127, 'x'), r2 + r2 + r2, r2 + r2 + r2 + r2, r2 + r2 + r2 + "......"};
    {
      std::string w;
      for (int i = 0; i < 16; i++) w += r2;
      ws.push_back(w);
    }
    for (uint32_t L : {1u, 6u, 7u, 8u, 9u, 10u, 11u, 12u, 126u, 127u}) {  // filler only, a unit first, a unit last
      ws.push_back(std::string(L, '.'));
      ws.push_back((ks[3 % ks.size()].k + std::string(127, '.')).substr(0, L));
      ws.push_back(std::string(L - 1, '.') + r2);
    }
    for (int i = 0; i < 2200; i++) {
      std::string w;
      const uint32_t style = r.below(100);
      if (style < 45) {
        for (uint32_t u = r.below(9); u; u--) w += fill(r, r.chance(70) ? 0 : 1 + r.below(3)) + ks[r.below((uint32_t)ks.size())].k;
      } else if (style < 75) {
        static const uint32_t gaps[] = {0, 0, 1, 2, 5, 6, 7, 8, 9, 13, 14, 15, 22};
        for (uint32_t u = r.below(9); u; u--) w += fill(r, gaps[r.below(13)]) + ks[r.below((uint32_t)ks.size())].k;
      } else {
        const uint32_t u = 9 + r.below(8), at = r.below(u);
        static const uint32_t gaps[] = {0, 1, 4, 9};
        for (uint32_t i2 = 0; i2 < u; i2++) w += fill(r, i2 == at ? gaps[r.below(4)] : 0) + r2;
      }
      static const uint32_t tl[] = {0, 0, 1, 2, 3, 5, 6, 7, 8, 20};
      w += fill(r, r.chance(90) ? tl[r.below(10)] : 127);
      if (w.size() > 127) w.resize(127);
      ws.push_back(w);
    }
    for (const std::string& w : ws) {
      std::unique_ptr<uint8_t[]> wb(new uint8_t[w.size() ? w.size() : 1]);
      memcpy(wb.get(), w.data(), w.size());
      uint32_t out[CO_NOUT];
      cut_once_compare(wb.get(), (uint32_t)w.size(), T, out, rn.data(), rr.data());
      words++;
      bool ok = out[0] == PB_EQUAL && rn == rr;
      if (out[0] == PB_NOTFAST && out[28] > 8) { ok = true; nine++; }  // (never built: more than 8 groups)
      if (refusing && out[0] == PB_NA && out[18] == out[27] && out[18] > 0) { ok = true; refused++; }
      if (!ok) {
        fails++;
        fprintf(stderr, "table %d word '%s': code %u (units %u np %u ng %u ne %u)\n", t, w.c_str(), out[0], out[1], out[2], out[3], out[4]);
      }
      fast += out[8];
      three += out[5] == 3;
      tails += out[6];
      lits += out[7] >= 2;
      u16 += out[1] == 16;
    }
  }
  printf("%zu words, %zu FAST, %zu with a three-unit group, %zu tails in groups, %zu with >= 2 literal pieces, %zu of 16 units, "
         "%zu refused, %zu of more than 8 groups: %zu failures\n",
         words, fast, three, tails, lits, u16, refused, nine, fails);
  const bool covered = words >= 1000000 && fast > words / 3 && three > 100 && tails > 100 && lits > 100 && u16 > 10 && refused > 100;
  if (!covered) fprintf(stderr, "coverage too thin\n");
  return fails || !covered ? 1 : 0;
}
