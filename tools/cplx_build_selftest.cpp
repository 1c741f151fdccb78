// cplx_build_selftest.cpp -- stand-alone host check of k_keyspace_cplx's lean path
// (csrc/a5x_plan.h cplx_word_lean: CplxDetect, CountPlanner, CplxBuilder) against the generic
// unit walk (classify_word + plan_word_cached / plan_word, the steps of ks_word_once), for
// sanitizer builds:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I hashcat_a5_table_generator_amd/csrc tools/cplx_build_selftest.cpp \
//       -o cplx_build_selftest && ./cplx_build_selftest
//
// Tables of overlapping keys over a small alphabet (1-4 bytes, now and then 5; 1-3 values of
// 0-7 bytes, now and then 8 bytes, 15 or 16 values), compiled here into the device-table layout
// of a5x_format.h in an exact-size heap block; about 200k seeded random words per table, each
// in an exact-size heap block (the planners read a word through GWord::at / ld only, which
// never pass its end).  Every word must agree between the two paths (cplx_build_compare) in
// the four substitution windows of the tests; the counters say how many took which path.
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

// the device table; the keys of a bucket (one first byte) in the order given
static std::unique_ptr<uint8_t[]> compile(std::vector<KeyDef> ks, size_t* bytes) {
  std::stable_sort(ks.begin(), ks.end(), [](const KeyDef& a, const KeyDef& b) { return (uint8_t)a.k[0] < (uint8_t)b.k[0]; });
  std::vector<uint16_t> bucket(257, 0);
  for (auto& k : ks) bucket[(uint8_t)k.k[0] + 1]++;
  uint32_t maxb = 0;
  for (int b = 0; b < 256; b++) {
    maxb = std::max<uint32_t>(maxb, bucket[b + 1]);
    bucket[b + 1] += bucket[b];
  }
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
  h.max_bucket = maxb;
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

static const char* ALPHA = "sta";  // (u: a key of its own in every table, R = 2, in no other key)
static const char* FILLER = ".,_-";

static std::string digits(Rng& r, uint32_t n) {
  std::string s;
  for (uint32_t i = 0; i < n; i++) s += (char)('0' + r.below(10));
  return s;
}

int main(int argc, char** argv) {
  const uint32_t per_table = argc > 1 ? (uint32_t)atoi(argv[1]) : 200000u;
  Rng r{0xC1A5};
  size_t words = 0, lean = 0, built = 0, fails = 0, two = 0, four = 0, why[7] = {0, 0, 0, 0, 0, 0, 0};
  static const int WIN[4][2] = {{0, 15}, {1, 15}, {0, 1}, {2, 2}};
  for (int t = 0; t < 6; t++) {
    // s and ss always (the czech + german overlap), then random keys over the alphabet
    std::vector<KeyDef> ks = {{"s", {}}, {"ss", {}}, {"u", {}}};
    // (table 2: t / ta alone, clusters of three choices, two of which share a group)
    if (t == 2) { ks.push_back({"t", {}}); ks.push_back({"ta", {}}); }
    const uint32_t nk = t == 2 ? 0 : 2 + r.below(5);
    for (uint32_t i = 0; i < nk; i++) {
      std::string k;
      const uint32_t kl = t == 5 && i == 0 ? 5 : 1 + r.below(r.chance(25) ? 4 : 2);
      for (uint32_t j = 0; j < kl; j++) k += ALPHA[r.below(3)];
      bool dup = false;
      for (auto& d : ks) dup = dup || d.k == k;
      if (!dup) ks.push_back({k, {}});
    }
    for (size_t i = 0; i < ks.size(); i++) {
      uint32_t nv = 1 + r.below(3);
      if (t >= 3 && i == 3) nv = t == 3 ? 15 : 16;  // R = 16, and 17
      for (uint32_t v = 0; v < nv; v++) ks[i].vs.push_back(digits(r, r.chance(4) ? 8 : (r.chance(10) ? 7 : r.below(4))));
    }
    ks[2].vs = {"1"};  // four of them fill a group of 16
    if (t == 2) { ks[3].vs = {"3"}; ks[4].vs = {"4"}; }
    if (t == 1) ks[0].vs = {""};  // an empty value: the span shrinks
    size_t tb = 0;
    const std::unique_ptr<uint8_t[]> blob = compile(ks, &tb);
    const Tab T = tab_view(blob.get());
    for (uint32_t i = 0; i < per_table; i++) {
      std::string w;
      const uint32_t target = r.chance(3) ? r.below(128) : r.below(37);
      while (w.size() < target) {
        const uint32_t st = r.below(100), dense = i % 3 == 0;  // a third of the words are dense in keys
        if (st < (dense ? 45u : 15u)) w += ks[r.below((uint32_t)ks.size())].k;
        else if (st < (dense ? 60u : 20u)) w += ALPHA[r.below(3)];
        else if (st < (dense ? 70u : 40u)) w += 'u';
        else for (uint32_t g = 1 + r.below(r.chance(20) ? 9 : 3); g; g--) w += FILLER[r.below(4)];
      }
      if (w.size() > 127) w.resize(127);
      std::unique_ptr<uint8_t[]> wb(new uint8_t[w.size() ? w.size() : 1]);
      memcpy(wb.get(), w.data(), w.size());
      const int* win = WIN[i & 3];
      uint32_t out[12];
      cplx_build_compare(wb.get(), (uint32_t)w.size(), T, win[0], win[1], out);
      words++;
      if (out[0] != 1) {
        if (++fails <= 20)
          fprintf(stderr, "table %d word '%s' window %d %d: differs (why %u flags %x built %u groups %u)\n", t, w.c_str(), win[0],
                  win[1], out[1], out[2], out[3], out[10]);
      }
      if (out[1] == 0) {
        lean++;
        built += out[3];
        four += out[11] == 4;
        two += (out[9] >> 8) & 1u;
      }
      for (int b = 0; b < 7; b++) why[b] += (out[1] >> b) & 1u;
    }
  }
  printf("%zu words, %zu lean (%zu records built, %zu with a four-unit group, %zu with two clusters in a group); generic: long key %zu, units %zu, position %zu, "
         "key index %zu, cluster %zu, clusters %zu, slot %zu: %zu failures\n",
         words, lean, built, four, two, why[0], why[1], why[2], why[3], why[4], why[5], why[6], fails);
  const bool covered = lean > words / 10 && built > words / 20 && why[0] > 50 && why[1] > 50 && why[4] > 50 && why[5] > 50 &&
                       why[6] > 50 && four > 50 && two > 50;
  if (!covered) fprintf(stderr, "coverage too thin\n");
  return fails || !covered ? 1 : 0;
}
