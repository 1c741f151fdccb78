// a5x_rules.h -- hashcat rule-file subset: the line parser and the per-word interpreter,
// host and device (shared by the rules stream kernel, a5x_rules.hip, and the host calls
// a5x_set_rules / a5x_debug_apply_rule / a5x_format_hits_rules, a5x_host.cpp: the CPU
// suite runs the code the kernel runs).
//
// A word lives in a buffer of A5X_RULE_NDW dwords reached only through B::rd(k) / B::wr(k, v)
// (dword k), so the same code runs on a flat host array and on the kernel's dword-
// interleaved LDS lane buffers.  Invariant kept by every function: all buffer bytes at or
// past the current length are zero (the hash sources read up to 8 bytes past the message).
// Shifting functions move whole dwords (v_alignbyte_b32 / v_perm_b32 on the device); single
// byte functions are a read-modify-write of one dword.
//
// An encoded function is one u32: the function character | p0 << 8 | p1 << 16 (positions
// decoded to 0..35, characters literal).  A rule is at most A5X_RULE_OPS_MAX of them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define A5X_RULE_OPS_MAX 31u
#define A5X_RULE_LMAX 128u
#define A5X_RULE_NDW (A5X_RULE_LMAX / 4u + 2u)  // the word + 8 zero bytes for the hash over-read
#define A5X_RULE_STRIDE 32u                     // u32 per rule in a rule table: count, then the functions

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RULE_HD __host__ __device__ __forceinline__
#else
#define RULE_HD inline
#endif

// ({hi, lo} >> 8 * sh) & 0xffffffff, sh in 0..3
RULE_HD uint32_t rule_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
  return sh ? (lo >> (8u * sh)) | (hi << (32u - 8u * sh)) : lo;
#endif
}
RULE_HD uint32_t rule_bswap(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(0u, x, 0x00010203u);
#else
  return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
#endif
}
// bytes (0, 0, 1, 1) / (2, 2, 3, 3) of x
RULE_HD uint32_t rule_dup_lo(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(0u, x, 0x01010000u);
#else
  return (x & 0xffu) * 0x0101u | ((x >> 8) & 0xffu) * 0x01010000u;
#endif
}
RULE_HD uint32_t rule_dup_hi(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(0u, x, 0x03030202u);
#else
  return ((x >> 16) & 0xffu) * 0x0101u | (x >> 24) * 0x01010000u;
#endif
}
// mask of the low n bytes of a dword (n <= 0: none, n >= 4: all)
RULE_HD uint32_t rule_keep(int n) { return n >= 4 ? 0xffffffffu : (n <= 0 ? 0u : ((1u << (8 * n)) - 1u)); }
// 0x80 in every byte of x that is an ASCII letter of the case whose 'A' / 'a' is lo
RULE_HD uint32_t rule_alpha(uint32_t x, uint32_t lo) {
  const uint32_t h = x & 0x7f7f7f7fu;
  const uint32_t ge = h + (0x80u - lo) * 0x01010101u;         // heptet >= lo
  const uint32_t gt = h + (0x7fu - (lo + 25u)) * 0x01010101u;  // heptet > lo + 25
  return ge & ~gt & ~x & 0x80808080u;
}
// 0x80 in every byte of x equal to c
RULE_HD uint32_t rule_eq(uint32_t x, uint32_t c) {
  const uint32_t y = x ^ (c * 0x01010101u);
  return ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);
}

// host buffer
struct RuleFlat {
  uint32_t w[A5X_RULE_NDW];
  RULE_HD uint32_t rd(uint32_t k) const { return w[k]; }
  RULE_HD void wr(uint32_t k, uint32_t v) { w[k] = v; }
};

template <class B> RULE_HD uint32_t rule_get(const B& b, uint32_t i) { return (b.rd(i >> 2) >> (8u * (i & 3u))) & 255u; }
template <class B> RULE_HD void rule_set(B& b, uint32_t i, uint32_t v) {
  const uint32_t k = i >> 2, sh = 8u * (i & 3u);
  b.wr(k, (b.rd(k) & ~(255u << sh)) | (v << sh));
}
// dword k, zero outside the buffer
template <class B> RULE_HD uint32_t rule_dw(const B& b, int k) { return (k >= 0 && k < (int)A5X_RULE_NDW) ? b.rd((uint32_t)k) : 0u; }
// the 4 bytes at byte offset p (any int; bytes outside the buffer read as zero)
template <class B> RULE_HD uint32_t rule_at4(const B& b, int p) {
  const int k = p >> 2;
  const uint32_t r = (uint32_t)p & 3u;
  const uint32_t lo = rule_dw(b, k);
  if (!r) return lo;
  return rule_alignbyte(rule_dw(b, k + 1), lo, r);
}
RULE_HD uint32_t rule_ndw(uint32_t len) { return (len + 3u) >> 2; }

// delete bytes [n, n + m) of a word of len bytes (n + m <= len)
template <class B> RULE_HD void rule_del(B& b, uint32_t len, uint32_t n, uint32_t m) {
  const uint32_t nd = rule_ndw(len);
  for (uint32_t k = n >> 2; k < nd; k++) {
    const uint32_t lo = rule_keep((int)n - (int)(4u * k));
    const uint32_t v = rule_at4(b, (int)(4u * k + m));
    b.wr(k, (b.rd(k) & lo) | (v & ~lo));
  }
}
// open a zero gap of s bytes at n: bytes [n, len) move to [n + s, len + s) (len + s <= LMAX)
template <class B> RULE_HD void rule_gap(B& b, uint32_t len, uint32_t n, uint32_t s) {
  if (!s) return;
  for (int k = (int)((len + s - 1u) >> 2); k >= (int)(n >> 2); k--) {
    const uint32_t lo = rule_keep((int)n - 4 * k), gp = rule_keep((int)(n + s) - 4 * k);
    const uint32_t v = rule_at4(b, 4 * k - (int)s);
    b.wr((uint32_t)k, (b.rd((uint32_t)k) & lo) | (v & ~gp));
  }
}
// cut the word to its first n bytes (n <= len)
template <class B> RULE_HD void rule_trunc(B& b, uint32_t len, uint32_t n) {
  const uint32_t nd = rule_ndw(len);
  uint32_t k = n >> 2;
  if (k < nd) b.wr(k, b.rd(k) & rule_keep((int)(n & 3u)));
  for (k++; k < nd; k++) b.wr(k, 0u);
}
// append slen bytes whose dword j is src(j) (zero past slen) at byte len (len + slen <= LMAX);
// src may read the word's bytes below len: the dwords are written from the top down
template <class B, class F> RULE_HD void rule_append(B& b, uint32_t len, uint32_t slen, const F& src) {
  const uint32_t q = len >> 2, r = len & 3u, ns = rule_ndw(slen);
  if (!ns) return;
  if (!r) {
    for (int j = (int)ns - 1; j >= 0; j--) b.wr(q + (uint32_t)j, src((uint32_t)j));
    return;
  }
  uint32_t hi = 0u;  // src(j)
  for (int j = (int)ns; j >= 1; j--) {
    const uint32_t lo = src((uint32_t)j - 1u);
    b.wr(q + (uint32_t)j, rule_alignbyte(hi, lo, 4u - r));
    hi = lo;
  }
  b.wr(q, (b.rd(q) & rule_keep((int)r)) | (hi << (8u * r)));
}

// source dwords of rule_append
template <class B> struct RuleSrcBytes {  // the word's bytes [off, off + n)
  const B* b;
  uint32_t off, n;
  RULE_HD uint32_t operator()(uint32_t j) const { return rule_at4(*b, (int)(off + 4u * j)) & rule_keep((int)n - (int)(4u * j)); }
};
template <class B> struct RuleSrcRev {  // the word's bytes [0, n) reversed
  const B* b;
  uint32_t n;
  RULE_HD uint32_t operator()(uint32_t j) const { return rule_bswap(rule_at4(*b, (int)n - 4 - (int)(4u * j))); }
};
struct RuleSrcFill {  // n times the byte c
  uint32_t c, n;
  RULE_HD uint32_t operator()(uint32_t j) const { return (c * 0x01010101u) & rule_keep((int)n - (int)(4u * j)); }
};

// lower (up == false) or upper all ASCII letters
template <class B> RULE_HD void rule_case_all(B& b, uint32_t len, bool up) {
  const uint32_t nd = rule_ndw(len);
  for (uint32_t k = 0; k < nd; k++) {
    const uint32_t x = b.rd(k);
    b.wr(k, x ^ (rule_alpha(x, up ? 0x61u : 0x41u) >> 2));
  }
}
// flip the case of byte i when it is a letter of the given case ('A' / 'a'), or of either (lo == 0)
template <class B> RULE_HD void rule_case_at(B& b, uint32_t i, uint32_t lo) {
  const uint32_t k = i >> 2, x = b.rd(k);
  const uint32_t m = lo ? rule_alpha(x, lo) : (rule_alpha(x, 0x41u) | rule_alpha(x, 0x61u));
  b.wr(k, x ^ ((m >> 2) & (0xffu << (8u * (i & 3u)))));
}

// One function on the word in b; returns the new length.  op is wave-uniform in the kernel:
// the switch is a scalar branch there.
template <class B> RULE_HD uint32_t rule_apply_op(B& b, uint32_t len, uint32_t op) {
  const uint32_t fn = op & 255u, p0 = (op >> 8) & 255u, p1 = (op >> 16) & 255u;
  const uint32_t LM = A5X_RULE_LMAX;
  switch (fn) {
    case ':': break;
    case 'l': rule_case_all(b, len, false); break;
    case 'u': rule_case_all(b, len, true); break;
    case 'c': rule_case_all(b, len, false); if (len) rule_case_at(b, 0, 0x61u); break;
    case 'C': rule_case_all(b, len, true); if (len) rule_case_at(b, 0, 0x41u); break;
    case 't': {
      const uint32_t nd = rule_ndw(len);
      for (uint32_t k = 0; k < nd; k++) {
        const uint32_t x = b.rd(k);
        b.wr(k, x ^ ((rule_alpha(x, 0x41u) | rule_alpha(x, 0x61u)) >> 2));
      }
      break;
    }
    case 'T': if (p0 < len) rule_case_at(b, p0, 0u); break;
    case 'E':
    case 'e': {  // lower all, then upper the first byte and every byte after a separator
      const uint32_t sep = fn == 'E' ? 0x20u : p0, nd = rule_ndw(len);
      uint32_t carry = 0x80u;
      for (uint32_t k = 0; k < nd; k++) {
        uint32_t x = b.rd(k);
        x ^= rule_alpha(x, 0x41u) >> 2;
        const uint32_t s = rule_eq(x, sep);
        x ^= (rule_alpha(x, 0x61u) & ((s << 8) | carry)) >> 2;
        carry = s >> 24;
        b.wr(k, x);
      }
      break;
    }
    case 'r': {  // dwords reversed and byte-swapped, then the 0..3 leading pad bytes shifted out
      const uint32_t nd = rule_ndw(len);
      for (uint32_t i = 0; i < nd / 2u; i++) {
        const uint32_t x = b.rd(i), y = b.rd(nd - 1u - i);
        b.wr(i, rule_bswap(y));
        b.wr(nd - 1u - i, rule_bswap(x));
      }
      if (nd & 1u) b.wr(nd / 2u, rule_bswap(b.rd(nd / 2u)));
      if (4u * nd != len) rule_del(b, 4u * nd, 0u, 4u * nd - len);
      break;
    }
    case 'd':
    case 'p': {
      const uint32_t times = fn == 'd' ? 1u : p0;
      if (len * (times + 1u) > LM) break;
      const uint32_t l0 = len;
      RuleSrcBytes<B> s;
      s.b = &b; s.off = 0u; s.n = l0;
      for (uint32_t t = 0; t < times; t++) {
        rule_append(b, len, l0, s);
        len += l0;
      }
      break;
    }
    case 'f': {
      if (2u * len > LM) break;
      RuleSrcRev<B> s;
      s.b = &b; s.n = len;
      rule_append(b, len, len, s);
      len *= 2u;
      break;
    }
    case '{':
      if (len > 1u) {
        const uint32_t c = rule_get(b, 0u);
        rule_del(b, len, 0u, 1u);
        rule_set(b, len - 1u, c);
      }
      break;
    case '}':
      if (len > 1u) {
        const uint32_t c = rule_get(b, len - 1u);
        rule_set(b, len - 1u, 0u);
        rule_gap(b, len - 1u, 0u, 1u);
        rule_set(b, 0u, c);
      }
      break;
    case '$': if (len < LM) { rule_set(b, len, p0); len++; } break;
    case '^': if (len < LM) { rule_gap(b, len, 0u, 1u); rule_set(b, 0u, p0); len++; } break;
    case '[': if (len) { rule_del(b, len, 0u, 1u); len--; } break;
    case ']': if (len) { rule_set(b, len - 1u, 0u); len--; } break;
    case 'D': if (p0 < len) { rule_del(b, len, p0, 1u); len--; } break;
    case 'x':
      if (p0 < len && p0 + p1 <= len) {
        rule_trunc(b, len, p0 + p1);
        rule_del(b, p0 + p1, 0u, p0);
        len = p1;
      }
      break;
    case 'O': if (p0 < len && p0 + p1 <= len) { rule_del(b, len, p0, p1); len -= p1; } break;
    case 'i': if (p0 <= len && len < LM) { rule_gap(b, len, p0, 1u); rule_set(b, p0, p1); len++; } break;
    case 'o': if (p0 < len) rule_set(b, p0, p1); break;
    case '\'': if (p0 < len) { rule_trunc(b, len, p0); len = p0; } break;
    case 's': {
      const uint32_t nd = rule_ndw(len);
      for (uint32_t k = 0; k < nd; k++) {
        const uint32_t x = b.rd(k);
        const uint32_t m = ((rule_eq(x, p0) >> 7) * 0xffu) & rule_keep((int)len - (int)(4u * k));
        b.wr(k, (x & ~m) | ((p1 * 0x01010101u) & m));
      }
      break;
    }
    case '@': {  // compaction: kept bytes gathered into dwords, written behind the read position
      const uint32_t nd = rule_ndw(len);
      uint32_t acc = 0u, na = 0u, ok = 0u, nl = 0u;
      for (uint32_t k = 0; k < nd; k++) {
        const uint32_t x = b.rd(k);
        for (uint32_t t = 0; t < 4u; t++) {
          const uint32_t c = (x >> (8u * t)) & 255u;
          if (4u * k + t < len && c != p0) {
            acc |= c << (8u * na);
            nl++;
            if (++na == 4u) { b.wr(ok++, acc); acc = 0u; na = 0u; }
          }
        }
      }
      if (ok < nd) b.wr(ok++, acc);
      for (; ok < nd; ok++) b.wr(ok, 0u);
      len = nl;
      break;
    }
    case 'z':
      if (len && len + p0 <= LM && p0) {
        RuleSrcFill s;
        s.c = rule_get(b, 0u); s.n = p0;
        rule_gap(b, len, 0u, p0);
        for (uint32_t k = 0; k < rule_ndw(p0); k++) b.wr(k, b.rd(k) | s(k));
        len += p0;
      }
      break;
    case 'Z':
      if (len && len + p0 <= LM) {
        RuleSrcFill s;
        s.c = rule_get(b, len - 1u); s.n = p0;
        rule_append(b, len, p0, s);
        len += p0;
      }
      break;
    case 'q':
      if (2u * len <= LM) {
        for (int k = (int)rule_ndw(len) - 1; k >= 0; k--) {
          const uint32_t x = b.rd((uint32_t)k);
          b.wr(2u * (uint32_t)k + 1u, rule_dup_hi(x));
          b.wr(2u * (uint32_t)k, rule_dup_lo(x));
        }
        len *= 2u;
      }
      break;
    case 'k':
    case 'K':
    case '*': {
      uint32_t i = p0, j = p1;
      if (fn == 'k') { i = 0u; j = 1u; }
      if (fn == 'K') { i = len - 2u; j = len - 1u; }
      if (fn != '*' && len < 2u) break;
      if (i >= len || j >= len) break;
      const uint32_t x = rule_get(b, i), y = rule_get(b, j);
      rule_set(b, i, y);
      rule_set(b, j, x);
      break;
    }
    case 'L': if (p0 < len) rule_set(b, p0, (rule_get(b, p0) << 1) & 255u); break;
    case 'R': if (p0 < len) rule_set(b, p0, rule_get(b, p0) >> 1); break;
    case '+': if (p0 < len) rule_set(b, p0, (rule_get(b, p0) + 1u) & 255u); break;
    case '-': if (p0 < len) rule_set(b, p0, (rule_get(b, p0) + 255u) & 255u); break;
    case '.': if (p0 + 1u < len) rule_set(b, p0, rule_get(b, p0 + 1u)); break;
    case ',': if (p0 && p0 < len) rule_set(b, p0, rule_get(b, p0 - 1u)); break;
    case 'y':
      if (p0 <= len && len + p0 <= LM && p0) {
        rule_gap(b, len, 0u, p0);
        for (uint32_t k = 0; k < rule_ndw(p0); k++)
          b.wr(k, b.rd(k) | (rule_at4(b, (int)(p0 + 4u * k)) & rule_keep((int)p0 - (int)(4u * k))));
        len += p0;
      }
      break;
    case 'Y':
      if (p0 <= len && len + p0 <= LM) {
        RuleSrcBytes<B> s;
        s.b = &b; s.off = len - p0; s.n = p0;
        rule_append(b, len, p0, s);
        len += p0;
      }
      break;
    default: break;
  }
  return len;
}

// ---- rule lines ---------------------------------------------------------------
// parameter kinds of a function: 0 none, 1 N, 2 X, 3 N M, 4 N X, 5 X Y; -1: not supported
RULE_HD int rule_fn_kind(uint8_t f) {
  switch (f) {
    case ':': case 'l': case 'u': case 'c': case 'C': case 't': case 'r': case 'd': case 'f': case '{': case '}':
    case '[': case ']': case 'q': case 'k': case 'K': case 'E':
      return 0;
    case 'T': case 'p': case 'D': case '\'': case 'z': case 'Z': case 'L': case 'R': case '+': case '-': case '.':
    case ',': case 'y': case 'Y':
      return 1;
    case '$': case '^': case '@': case 'e':
      return 2;
    case 'x': case 'O': case '*':
      return 3;
    case 'i': case 'o':
      return 4;
    case 's':
      return 5;
    default:
      return -1;
  }
}
RULE_HD int rule_pos(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'A' && c <= 'Z' ? c - 'A' + 10 : -1); }

enum { RULE_LINE_OK = 0, RULE_LINE_IGNORED = 1, RULE_LINE_SKIPPED = 2 };
// One line of a rule file (without its '\n') into ops[A5X_RULE_OPS_MAX]: OK (*nops
// functions), IGNORED (empty or comment) or SKIPPED (unsupported or malformed).
RULE_HD int rule_parse_line(const uint8_t* s, size_t n, uint32_t* ops, uint32_t* nops) {
  *nops = 0;
  if (n && s[n - 1] == '\r') n--;
  size_t i = 0;
  while (i < n && (s[i] == ' ' || s[i] == '\t')) i++;
  if (i == n || s[i] == '#') return RULE_LINE_IGNORED;
  uint32_t k = 0;
  while (i < n) {
    if (s[i] == ' ') { i++; continue; }
    const uint8_t f = s[i++];
    const int kind = rule_fn_kind(f);
    if (kind < 0 || k == A5X_RULE_OPS_MAX) return RULE_LINE_SKIPPED;
    const size_t need = kind == 0 ? 0u : (kind <= 2 ? 1u : 2u);
    if (n - i < need) return RULE_LINE_SKIPPED;
    uint32_t p0 = 0, p1 = 0;
    if (kind == 1 || kind == 3 || kind == 4) {
      const int v = rule_pos(s[i]);
      if (v < 0) return RULE_LINE_SKIPPED;
      p0 = (uint32_t)v;
    } else if (kind == 2 || kind == 5) {
      p0 = s[i];
    }
    if (kind == 3) {
      const int v = rule_pos(s[i + 1]);
      if (v < 0) return RULE_LINE_SKIPPED;
      p1 = (uint32_t)v;
    } else if (kind == 4 || kind == 5) {
      p1 = s[i + 1];
    }
    i += need;
    ops[k++] = (uint32_t)f | (p0 << 8) | (p1 << 16);
  }
  *nops = k;
  return RULE_LINE_OK;
}

// the whole rule on a word of len bytes in b (len <= A5X_RULE_LMAX); returns the new length
template <class B> RULE_HD uint32_t rule_apply(B& b, uint32_t len, const uint32_t* ops, uint32_t nops) {
  for (uint32_t j = 0; j < nops; j++) len = rule_apply_op(b, len, ops[j]);
  return len;
}
