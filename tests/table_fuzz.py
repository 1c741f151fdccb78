"""Synthetic tables and word lists at the planner's limits (helper module, no tests here).

The shipped .table files have 1-2 code point keys with 1-3 short values and one overlap
family (czech+german s/ss), so they never straddle the constants that decide which kernel
takes a word (csrc/a5x_plan.h FW_* / FB_* / UC_*, k_keyspace_vsub VS_*, the mode engines'
A5X_M_*).  This module builds named *corpora*: a synthetic table (written to a temporary
.table file, so the C oracle, the Python oracle and Context.load_tables parse the same
bytes), a word list assembled from the table's own keys plus filler bytes that occur in no
key, and the (mode, min, max) windows to run.  Everything is deterministic (seeded).

A word's size is bounded by construction: tokens are appended while the product of
(nvals + 1) over its matches stays below BUDGET; nothing is rejected afterwards.  The few
directed words sized on purpose (five R = 9 pieces, 17 distinct patterns)
go up to 2^17 candidates.

census() is the evidence that a corpus reaches both sides of each limit: it is built from
the flags a5x_debug_plan_word returns, the plan sizes of a5x_debug_plan_sizes and facts
computed here from table and word.  tests/test_table_fuzz.py asserts it; the GPU file uses
it to pick words.
"""
from __future__ import annotations

import ctypes
import functools
import os
import random
import tempfile
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

BUDGET = 20_000
WINDOWS = [(0, 15), (1, 15), (0, 3), (2, 5)]
REVERSE_EXTRA = (-1, 8)   # added for the -r modes (1, 3)
NARROW = [(0, 3)]         # words with ~64 patterns / positions: C(64, <= 3) candidates
R_POSITIONS = 16

FAST = 1 << 5
DEFER = 1 << 4
RADIX = 1 << 0
E_BOUNDS = -6
E_UNSUPPORTED = -9

FILL = b".,_-+~"  # in no key of any corpus


def _plain(b: bytes) -> bool:
    return len(b) > 0 and all(0x30 <= c <= 0x39 or 0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A for c in b)


def _field(b: bytes) -> bytes:
    # $HEX[] needs >= 7 bytes to be decoded (main.go:147-162): the empty string stays plain
    return b if (_plain(b) or not b) else b"$HEX[" + b.hex().encode() + b"]"


class Corpus:
    def __init__(self, name: str, table: Dict[bytes, List[bytes]], words: Sequence[bytes], modes=(0, 1, 2, 3),
                 narrow: Sequence[bytes] = ()):
        self.name = name
        self.table = table
        self.modes = tuple(modes)
        seen, self.words = set(), []
        for w in words:  # (duplicates of directed words, not a size filter)
            if w not in seen:
                seen.add(w)
                self.words.append(w)
        self.narrow = [w for w in narrow]
        # -r walks every combination of match positions, overlapping ones included
        # (main.go:263-281): the reference's cost is 2^positions whatever it emits, so words
        # with more than R_POSITIONS matches run -r in the narrow window only
        self.rheavy = [w for w in self.words if len(matches(table, w)) > R_POSITIONS]
        self._dir = None

    def table_text(self) -> bytes:
        return b"".join(_field(k) + b"=" + _field(v) + b"\n" for k, vs in self.table.items() for v in vs)

    @property
    def path(self) -> str:
        if self._dir is None:
            self._dir = tempfile.TemporaryDirectory(prefix="a5x_fuzz_")
            with open(os.path.join(self._dir.name, self.name + ".table"), "wb") as f:
                f.write(self.table_text())
        return os.path.join(self._dir.name, self.name + ".table")

    def runs(self) -> List[Tuple[int, int, int, str]]:
        """(mode, min, max, which) for every window of the corpus; which = 'words' or 'narrow'."""
        out = []
        for mode in self.modes:
            for mn, mx in WINDOWS + ([REVERSE_EXTRA] if mode in (1, 3) else []):
                out.append((mode, mn, mx, "words"))
            if self.word_list("narrow", mode):
                for mn, mx in NARROW:
                    out.append((mode, mn, mx, "narrow"))
        return out

    def word_list(self, which: str, mode: int = 0) -> List[bytes]:
        if mode != 1:
            return self.words if which == "words" else self.narrow
        heavy = set(self.rheavy)
        return [w for w in self.words if w not in heavy] if which == "words" else self.narrow + self.rheavy


def assemble(rng: random.Random, table, keys: Sequence[bytes], n: int, maxlen: int = 40, fill: bytes = FILL,
             budget: int = BUDGET) -> List[bytes]:
    """n words of keys and filler runs; a token is appended only while the product of
    (nvals + 1) over the word's matches stays below budget."""
    out = []
    for _ in range(n):
        w, target = b"", rng.randint(1, maxlen)
        while len(w) < target:
            if rng.random() < 0.55:
                tok = rng.choice(keys)
            else:
                tok = bytes(rng.choice(fill) for _ in range(rng.choice((1, 1, 2, 3, 7, 8))))
            if match_product(table, w + tok) >= budget:
                break
            w += tok
        out.append(w)
    return out


# ---------------------------------------------------------------------------
# facts computed from table and word (default mode)
# ---------------------------------------------------------------------------
def matches(table, word: bytes) -> List[Tuple[int, bytes]]:
    lens = sorted({len(k) for k in table if k})
    out = []
    for p in range(len(word)):
        for kl in lens:
            if p + kl <= len(word) and word[p:p + kl] in table:
                out.append((p, word[p:p + kl]))
    return out


def match_product(table, word: bytes) -> int:
    r = 1
    for _, k in matches(table, word):
        r *= len(table[k]) + 1
    return r


def units(table, word: bytes) -> List[dict]:
    """The substitution units of a5x_plan.h next_unit: a lone match or a cluster of
    overlapping matches (the span grows over every match that starts inside it)."""
    ms = matches(table, word)
    by_pos: Dict[int, List[bytes]] = {}
    for p, k in ms:
        by_pos.setdefault(p, []).append(k)
    out, p = [], 0
    while p < len(word):
        if p not in by_pos:
            p += 1
            continue
        e, q, um = p, p, []
        while q < e or q == p:
            for k in by_pos.get(q, ()):
                um.append((q, k))
                e = max(e, q + len(k))
            q += 1
        # choices: non-overlapping subsets of the matches times their values (+ the empty one)
        ways = {e: 1}
        for s in range(e - 1, p - 1, -1):
            ways[s] = ways[s + 1] + sum(len(table[k]) * ways[q2 + len(k)] for q2, k in um if q2 == s)
        out.append({"s": p, "e": e, "nm": len(um), "R": ways[p], "cluster": len(um) > 1,
                    "maxv": max(max(len(v) for v in table[k]) for _, k in um),
                    "minv": min(min(len(v) for v in table[k]) for _, k in um)})
        p = e
    return out


def facts(table, word: bytes) -> dict:
    us = units(table, word)
    cl = [u for u in us if u["cluster"]]
    return {
        "L": len(word), "units": len(us), "clusters": len(cl), "nmatch": sum(u["nm"] for u in us),
        "maxR": max((u["R"] for u in us), default=1), "maxR_lone": max((u["R"] for u in us if not u["cluster"]), default=1),
        "maxR_cluster": max((u["R"] for u in cl), default=0), "max_cluster_matches": max((u["nm"] for u in cl), default=0),
        "maxv": max((u["maxv"] for u in us), default=0), "minv": min((u["minv"] for u in us), default=0),
        "cluster_starts": [u["s"] for u in cl], "P": int(np.prod([u["R"] for u in us], dtype=object)) if us else 1,
    }


# ---------------------------------------------------------------------------
# host replay (a5x_debug_plan_word / a5x_debug_plan_sizes) and the oracles
# ---------------------------------------------------------------------------
class HostPlan:
    """A host-only context (device -1) with the corpus table loaded from its file."""

    def __init__(self, corpus: Corpus):
        from hashcat_a5_table_generator_amd import _lib
        self.L = _lib.load()
        self.h = ctypes.c_void_p()
        assert self.L.a5x_create(-1, ctypes.byref(self.h)) == 0
        assert self.L.a5x_load_table_file(self.h, corpus.path.encode()) == 0, self.L.a5x_last_error(self.h)

    def plan(self, word: bytes, mn=0, mx=15, cap=1 << 22):
        """(rc, count, bytes, flags, nbig, bent, candidates or None)"""
        info = np.zeros(4, dtype=np.uint64)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        wb = np.frombuffer(word + b"\0", dtype=np.uint8)
        rc = self.L.a5x_debug_plan_word(self.h, wb.ctypes.data, len(word), mn, mx, out.ctypes.data, cap,
                                        info.ctypes.data)
        fl = int(info[2])
        if rc == -8 and int(info[1]) > cap:  # too many candidates to replay here
            return 0, int(info[0]), int(info[1]), fl & 0xFFFFFFFF, (fl >> 32) & 255, fl >> 40, None
        if rc:
            return rc, 0, 0, 0, 0, 0, None
        n = int(info[3])
        cands = out[:n].tobytes().split(b"\n")[:-1] if n else []
        return 0, int(info[0]), int(info[1]), fl & 0xFFFFFFFF, (fl >> 32) & 255, fl >> 40, cands

    def classify(self, word: bytes, mn=0, mx=15):
        """(rc, count, bytes, flags, nbig, bent): no replay"""
        info = np.zeros(4, dtype=np.uint64)
        wb = np.frombuffer(word + b"\0", dtype=np.uint8)
        rc = self.L.a5x_debug_plan_word(self.h, wb.ctypes.data, len(word), mn, mx, None, 0, info.ctypes.data)
        fl = int(info[2])
        return rc, int(info[0]), int(info[1]), fl & 0xFFFFFFFF, (fl >> 32) & 255, fl >> 40

    def sizes(self, word: bytes) -> Optional[dict]:
        """The piece plan of any word of <= 64 bytes, FAST or not (build-mode planner), and the
        route of k_keyspace_cplx: 1 one walk (cached units), 2 two walks (UnitCache full), 3 not FAST."""
        if len(word) > 64:
            return None
        o = np.zeros(40, dtype=np.uint32)
        wb = np.frombuffer(word + b"\0", dtype=np.uint8)
        if self.L.a5x_debug_plan_sizes(self.h, wb.ctypes.data, len(word), o.ctypes.data):
            return None
        names = ("ok", "np", "ng", "ne", "maxl", "minl", "nbig", "bent")
        d = {k: int(v) for k, v in zip(names, o[8:16])}
        d["count_mode"] = {k: int(v) for k, v in zip(names, o[0:8])}
        d["route"] = int(o[32])
        return d

    def close(self):
        self.L.a5x_destroy(self.h)


def c_table(corpus: Corpus):
    from oracle import c_oracle as co
    return co.CTable([corpus.path])


def c_count(ct, word: bytes, mode: int, mn: int, mx: int) -> int:
    """Output bytes of one word (size-only call), or a negative code where the reference panics."""
    from oracle import c_oracle as co
    data, offs = co.pack_words([word])
    wb = np.zeros(1, dtype=np.uint64)
    return int(co.lib().a5o_expand_batch(ct.h, data.ctypes.data, offs.ctypes.data, 1, mode, mn, mx, None, 0,
                                         wb.ctypes.data))


@functools.lru_cache(maxsize=None)
def split_panics(name: str, which: str, mode: int, mn: int, mx: int) -> Tuple[Tuple[bytes, ...], Tuple[bytes, ...]]:
    """(words the reference expands, words on which it panics or overflows its stack) of a run.
    Only -r runs can panic (main.go:255, 263-281)."""
    c = corpus(name)
    words = c.word_list(which, mode)
    if mode != 1 and not (mode == 3 and mn < 0):
        return tuple(words), ()
    ct = c_table(c)
    good, bad = [], []
    for w in words:
        (bad if c_count(ct, w, mode, mn, mx) < 0 else good).append(w)
    return tuple(good), tuple(bad)


def suball_pruned(word: bytes, sub, mn: int, mx: int, reverse: bool) -> List[bytes]:
    """-s / -s -r for words with ~64 patterns, where the reference's recursion (and both
    oracles, which restate it) visits all 2^patterns leaves before the window filters them
    (main.go:329-365, 392-440).  The same leaves enumerated by size: every subset of the
    sorted patterns with min <= size <= max, every value (-s) or subs[0] (-s -r) per chosen
    pattern, applied in sorted pattern order.  test_table_fuzz checks it against the Python
    oracle on every small word before the GPU tests rely on it."""
    import itertools
    from oracle import a5_oracle as o
    pats = o.unique_patterns(word, sub)
    if reverse and len(pats) < mn:
        return []
    out = []
    for k in range(max(mn, 0), min(mx, len(pats)) + 1):
        for comb in itertools.combinations(pats, k):
            for vals in itertools.product(*[(sub[p][:1] if reverse else sub[p]) for p in comb]):
                r = word
                for p, v in zip(comb, vals):
                    r = o.replace_all(r, p, v)
                out.append(r)
    return out


def reference_lists(c: Corpus, words: Sequence[bytes], mode: int, mn: int, mx: int, which: str) -> List[List[bytes]]:
    """Per-word sorted candidate lists: the C oracle, or suball_pruned for the narrow -s runs."""
    if which == "narrow" and mode in (2, 3):
        return [sorted(suball_pruned(w, c.table, mn, mx, mode == 3)) for w in words]
    return c_oracle_lists(c, words, mode, mn, mx)


def c_oracle_lists(c: Corpus, words: Sequence[bytes], mode: int, mn: int, mx: int) -> List[List[bytes]]:
    """Per-word sorted candidate lists of the C oracle."""
    from oracle import c_oracle as co
    if not words:
        return []
    data, offs = co.pack_words(list(words))
    out, wb = c_table(c).expand_batch(data, offs, mode, mn, mx)
    res, pos = [], 0
    for b in wb:
        seg = out[pos:pos + int(b)]
        pos += int(b)
        res.append(sorted(seg.split(b"\n")[:-1]) if seg else [])
    return res


# ---------------------------------------------------------------------------
# the corpora
# ---------------------------------------------------------------------------
def _vals(n: int, alphabet: bytes = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ") -> List[bytes]:
    return [alphabet[i:i + 1] for i in range(n)]


def _choices() -> Corpus:
    # one-byte keys with 1, 2, 3, 7, 14, 15, 16, 17 one-byte values: R = nvals + 1 of 15, 16,
    # 17, 18 on both sides of FW_UMAXR (16) and of the positional path's 14 values (i, j: R = 7, 9 for
    # the 63-entry big pieces of the pinned huge words)
    nv = {b"a": 1, b"b": 2, b"c": 3, b"d": 7, b"e": 14, b"f": 15, b"g": 16, b"h": 17, b"i": 6, b"j": 8}
    table = {k: _vals(n) for k, n in nv.items()}
    rng = random.Random(0xC401)
    words = []
    # "only oddity" templates: the same word with the 14-, 15-, 16- and 17-value key
    for t in (b"ab.%s.c", b"%s..a", b".%s", b"c%sb", b"%s_", b"12%s34", b"a%sa", b"b-%s-", b"%s+b", b"..%s.."):
        words += [t % k for k in (b"e", b"f", b"g", b"h")]
    words += [k * 2 for k in nv] + [b"d" + k + b"d" for k in (b"e", b"f", b"g", b"h")]
    words += assemble(rng, table, list(nv), 170, 24)
    return Corpus("choices", table, words)


def _lengths() -> Corpus:
    # values of 0, 1, 6, 7, 8, 9 and 40 bytes: empty values give candidates down to 0 bytes
    # (minl >= 3 flips), 8+ byte values are past FW_PLEN
    table = {b"a": [b"", b"X"], b"b": [b"Y" * 6], b"c": [b"Z" * 7], b"d": [b"W" * 8], b"e": [b"V" * 9],
             b"f": [b"U" * 40], b"g": [b"Q", b""], b"h": [b"H"]}
    rng = random.Random(0x1E46)
    words = [b"a", b"aa", b"aaa", b"aaaa", b"g", b"ga", b"ag", b"a.", b".a", b"a..", b".a.", b"a...", b"g.", b"g..",
             b"ah", b"ha", b"h", b"h.", b"hh", b"hah", b"gh.", b".g", b"ab", b"ba", b"b", b"c", b"d", b"e", b"f"]
    for k in (b"b", b"c", b"d", b"e", b"f"):
        words += [b".." + k + b"..", k + b"h", b"h." + k, k + b"." + k, b"a" + k + b"a", b"1234567" + k, k + b"+-"]
    words += assemble(rng, table, list(table), 170, 20)
    return Corpus("lengths", table, words)


def _longkeys() -> Corpus:
    # keys of 1 to 6 bytes: prefixes of one another, a match inside another key's span, two
    # keys at one position (ab, abc, bc, c); a 5-byte key with no shorter sibling (pqrst) and
    # words that differ from it in the 5th byte only (k_keyspace_vsub compares 4 bytes)
    table = {b"ab": [b"1"], b"abc": [b"2", b"22"], b"bc": [b"3"], b"c": [b"4"], b"abcdef": [b"6"], b"cdefg": [b"5"],
             b"defg": [b"7", b"77"], b"x": [b"8"], b"xy": [b"9"], b"xyzw": [b"0"], b"pqrst": [b"55555"],
             b"k": [b"K"], b"m": [b"M", b"N"], b"uvwx": [b"4444"], b"uvwxyz": [b"666666", b"6"]}
    rng = random.Random(0x10E6)
    words = [b"ab", b"abc", b"bc", b"c", b"abcd", b"abcdef", b"abcdefg", b"..abc..", b"xabc", b"cdefg", b"defg",
             b"xyzw", b"xyz", b"xy", b"xyzwxyzw", b"k.xyzw.k", b"pqrst", b"pqrs", b"pqrsT", b"k.pqrst.k",
             b"k.pqrsX.k", b"kpqrsXk", b"kpqrstk", b"pqrsX", b"mkpqrsXkm", b"m.pqrsY.m", b"mpqrs9m", b"kkpqrs.",
             b"pqrst.pqrst", b"pqrsX.pqrsX", b"k.k", b"m.m.k.k", b"uvwx", b"uvwxyz", b"uvwxy", b"k.uvwx.k",
             b"k.uvwxyz.k", b"k.uvwxy_.k", b"uvwxuvwx", b"m.uvwxyz.uvwx.m", b"abcabc", b"ababab", b"cabcab"]
    words += assemble(rng, table, list(table) + [b"pqrs", b"uvwxy", b"abcde"], 160, 24)
    return Corpus("longkeys", table, words)


def _clusters() -> Corpus:
    # chains a/aa/aaa, b/bb/bbbb over runs (cluster matches 7, 8, 9 around FW_UMAXM), cluster
    # choices 15 / 16 / 17 around FW_UMAXR (c/cc, d/dd, e/ee over a pair: (1 + 2)^2 + 6 / 7 / 8),
    # >= 3 clusters (UC_CLUSTERS), >= 9 units (UC_UNITS), a cluster at byte 62, 63, 64
    table = {b"a": [b"1"], b"aa": [b"2"], b"aaa": [b"3"], b"b": [b"4"], b"bb": [b"5"], b"bbbb": [b"6"],
             b"c": [b"7", b"8"], b"cc": _vals(6), b"d": [b"7", b"8"], b"dd": _vals(7), b"e": [b"7", b"8"],
             b"ee": _vals(8), b"k": [b"K"], b"s": [b"S"], b"ss": [b"Z"]}
    rng = random.Random(0xC1A5)
    words = [b"a" * k for k in range(2, 11)] + [b"b" * k for k in range(2, 9)]
    words += [b"." + b"a" * k + b"." for k in range(2, 7)] + [b"x" + b"b" * k for k in range(2, 7)]
    for pair in (b"cc", b"dd", b"ee"):
        words += [pair, b"." + pair, pair + b".", b"k" + pair, pair + b"k", b"12" + pair + b"3", b"k." + pair + b".k"]
    words += [b"ss.ss.ss", b"ss.ss", b"ss.ss.ss.ss", b"aa.ss.bb", b"aa.aa.aa", b"ss.aa.ss.k", b"ss_ss_ss_k_k",
              b"aa.bb.ss.k", b"ss.ss.k.ss"]
    words += [b".".join([b"k"] * n) for n in range(6, 12)] + [b"k" * n for n in range(7, 12)]
    words += [b"ss." + b".".join([b"k"] * n) for n in range(6, 10)] + [b".".join([b"k"] * n) + b".ss" for n in range(6, 10)]
    for n in (60, 61, 62, 63, 64, 65):
        words += [b"." * n + b"ss", b"." * n + b"aa", b"k" + b"_" * (n - 1) + b"ss"]
    words += assemble(rng, table, [b"a", b"b", b"c", b"d", b"e", b"k", b"s", b"ss", b"aa"], 120, 14)
    return Corpus("clusters", table, words)


def _pieces() -> Corpus:
    # units spaced by filler so that the plan has 7, 8, 9 small pieces; piece products around
    # FB_RMAX (five R = 8 pieces join into 3 big pieces, five R = 9 pieces stay 5, past
    # FB_NMAX); words of 60-64 bytes; candidates of 990-1010 bytes (a 157-byte value)
    table = {b"p": _vals(7), b"q": _vals(8), b"r": [b"R"], b"s": _vals(3), b"t": _vals(2), b"u": _vals(5),
             b"v": [b"V" * 157], b"w": [b"55555"]}
    rng = random.Random(0x91EC)
    words = []
    for key in (b"r", b"t", b"s"):
        for gap in (5, 6, 7, 8):
            for n in range(4, 10):
                w = (key + b"." * gap) * n
                if len(w) <= 64 and match_product(table, w) < BUDGET:
                    words += [w, w[:-1]]
    for key in (b"p", b"q"):
        for n in (3, 4, 5):
            words += [(key + b"." * 6) * n, (b"." * 6 + key) * n, (key + b"_" * 7) * n]
    words += [(b"q" + b"." * g) * 5 for g in (2, 3, 4, 5)] + [b"q..p..q..p..q", b"p.q.p.q.q", b"q-p-q-p-q-"]
    words += [b"r.." * 12, b"r.." * 13, b"r" + b"." * 59, b"r" + b"." * 62 + b"r", b"." * 63 + b"r", b"." * 64,
              b"t" + b"." * 60 + b"t", b"r...w.w", b"t...w.w.t", b"r...w", b"prprpr", b"pp.pp", b"qq", b"ppp", b"ut.ut"]
    for n in range(46, 70, 2):
        words.append(b"v" * 6 + b"." * n)  # longest candidate n + 6 * 157
    words += [b"v.." * 6 + b"." * 40, b"." * 30 + b"v" * 6 + b"." * 26]
    words += assemble(rng, table, [b"p", b"q", b"r", b"s", b"t", b"u", b"w"], 110, 64, budget=4000)
    return Corpus("pieces", table, words)


def _utf8(name: str, cont_key: bool, empty_key: bool = False) -> Corpus:
    # a key that starts on a UTF-8 continuation byte clears lead_only (the keyspace walk then
    # visits every byte); the same table without it keeps the walk that steps over them
    e, a, ss = "é".encode(), "á".encode(), "ß".encode()
    table = {e: [b"e", b"E"], b"a": [a], ss: [b"ss"], b"o": ["ö".encode(), b"0"], "€".encode(): [b"EUR"], b"z": [b"Z"]}
    if cont_key:
        table[b"\xa9"] = [b"C"]
        table[b"\x82\xac"] = [b"c"]
    if empty_key:
        table[b""] = [b"x"]
    rng = random.Random(0x07F8 + cont_key + 2 * empty_key)
    words = [e, e + e, b"caf" + e, a, b"a" + e + b"o", ss, b"stra" + ss + b"e", "€".encode(), b"1" + "€".encode() + b"o",
             b"\xa9", b"a\xa9", b"\xa9a", b"\xc3", b"\xc3\xa9\xa9", b"\xe2\x82", b"\xe2\x82\xac\xac", b"o\x82\xaco",
             b"\xa9\xa9\xa9", b"z\xa9z", b"\xff\xa9", "日本".encode() + e, b"az", b"zoo", b"", b"z", b"oz" + e + ss]
    toks = [e, b"a", ss, b"o", "€".encode(), b"z", b"\xa9", b"\x82\xac", b"\xc3", "ü".encode(), "日".encode(), b"\xbf"]
    words += assemble(rng, table, toks, 120 if not empty_key else 60, 16 if not empty_key else 8)
    return Corpus(name, table, words, modes=(2, 3) if empty_key else (0, 1, 2, 3))


def _manykeys() -> Corpus:
    # more than 1024 two-byte keys with one value each.  The mode table (16 B per key + 8 B per
    # value + blob) fits A5X_MTAB_LDS_MAX; the default engine's table (>= 73 B per key) does
    # not fit A5X_TABLE_LDS_MAX beyond ~420 keys, so a key index >= 1024 never reaches
    # next_unit, UnitCache or k_keyspace_vsub (test_table_fuzz asserts the refusal) and this
    # corpus runs the -r / -s / -s -r mode engines only.
    firsts = bytes(range(0x61, 0x7B)) + bytes(range(0x41, 0x5B))  # 52
    seconds = bytes(range(0x61, 0x77))                             # 22 -> 1144 keys
    table = {bytes((f, s)): [bytes((0x30 + (f + s) % 10,))] for f in firsts for s in seconds}
    keys = sorted(table)  # compiled order of both tables (first byte, then equal lengths in file order)
    rng = random.Random(0x3A17)
    words = []
    for i in (0, 1, 500, 1022, 1023, 1024, 1025, 1100, len(keys) - 1):
        k = keys[i]
        words += [k, b"." + k, k + b"..", k + k, k + b"." + keys[(i * 7 + 3) % len(keys)], k + b"-" + k + b"-" + keys[1023]]
    words += assemble(rng, table, keys[1000:1050] + keys[:20] + keys[-20:], 80, 16)
    return Corpus("manykeys", table, words, modes=(1, 2, 3))


TIED_KEYS = (b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ" + b"!@#$%^&*()[]{}")  # 66 one-byte keys


def _tied() -> Corpus:
    # -s / -s -r around VS_OCC (16), VS_TMAX (4), VS_SMAX (16) and A5X_M_NMAX (63): repeated
    # patterns, tied patterns, sub-word products, distinct patterns, values that contain a
    # key, fixed-width and other values, 127-129 byte words and 126-128 byte candidates
    table = {b"a": [b"4"], b"b": [b"8", b"6"], b"c": [b"<<"], b"d": [b""], b"e": [b"3", b"33"], b"f": [b"a"],
             b"g": [b"9", b"6", b"0"], b"h": [b"1", b"2", b"5"], b"i": [b"7", b"0"]}
    for j, k in enumerate(TIED_KEYS[9:20]):
        table[bytes((k,))] = [bytes((0x30 + j % 10,))]
    for j, k in enumerate(TIED_KEYS[20:]):
        table[bytes((k,))] = [bytes((0xC3, 0x80 + j))]
    K = [bytes((k,)) for k in TIED_KEYS]
    rng = random.Random(0x71ED)
    words = []
    for n in (2, 3, 14, 15, 16, 17):
        words += [b"a" * n, b"a." * n, b"aj" * (n // 2) + b"a" * (n % 2), b"j" * n + b"k", b"." + b"j_" * n]
    words += [b"ajklajkl", b"ajkajk", b"ajklmajklm", b"a.j.k.l.a.j.k.l", b"ajkl.m.ajkl.m", b"jklmnjklmn", b"jklmnojklmno", b"a.j.k.l.m.a.j.k.l.m", b"jkjklmlmnn",
              b"nopqrnopqr", b"ajklm-mlkja", b"abab",
              b"ghgh", b"bgbg", b"biabia", b"gbagba", b"ghagha", b"g.h.g.h", b"bibi", b"gg", b"hh.gg", b"bb.ii.aa",
              b"fa", b"faf", b"ff", b"f.f", b"afa", b"cc", b"c.c", b"dd", b"d.d", b"ee", b"e.e.e", b"cdcd", b"acac",
              b"u.u", b"uvuv", b"aua", b"juj.u"]
    for n in (15, 16, 17):
        words += [b"".join(K[9:9 + n]), b".".join(K[9:9 + n]), b"".join(K[9:9 + n]) + b"j"]
    for n in (124, 125, 126, 127, 128, 129):
        for k in (b"a", b"c", b"d", b"u"):
            words += [b"." * (n - 1) + k, k + b"_" * (n - 1), b"." * (n - 2) + k + k]
    words += assemble(rng, table, K[:24], 100, 20, budget=4000)
    narrow = []
    for n in (62, 63, 64, 65):
        narrow += [b"".join(K[:n]), b".".join(K[1:n + 1])[:128], b"".join(K[:n]) + b"e"]
    return Corpus("tied", table, words, narrow=narrow)


_BUILDERS = {
    "choices": _choices, "lengths": _lengths, "longkeys": _longkeys, "clusters": _clusters, "pieces": _pieces,
    "utf8_cont": lambda: _utf8("utf8_cont", True), "utf8_lead": lambda: _utf8("utf8_lead", False),
    "utf8_empty": lambda: _utf8("utf8_empty", True, True), "manykeys": _manykeys, "tied": _tied,
}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def corpus(name: str) -> Corpus:
    return _BUILDERS[name]()


# ---------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def census(name: str) -> Tuple[dict, ...]:
    """One row per word of the corpus (words + narrow), default-mode window (0, 15): the facts
    of facts(), the class flags and FAST fields of a5x_debug_plan_word, the plan sizes of
    a5x_debug_plan_sizes (words of <= 64 bytes), and the oracle's candidate lengths."""
    c = corpus(name)
    if 0 not in c.modes and name == "manykeys":
        return ()
    hp = HostPlan(c)
    ct = c_table(c)
    rows = []
    for w in c.words + c.narrow:
        f = facts(c.table, w)
        rc, cnt, byt, fl, nbig, bent = hp.classify(w)
        assert rc == 0, (name, w, rc)
        f.update(word=w, count=cnt, bytes=byt, flags=fl, fast=bool(fl & FAST), defer=bool(fl & DEFER),
                 radix=bool(fl & RADIX), np=(fl >> 24) & 31 if fl & FAST else None,
                 ne=(fl >> 16) & 255 if fl & FAST else None, ng=(fl >> 10) & 31 if fl & FAST else None,
                 nbig=nbig, bent=bent, sizes=hp.sizes(w))
        rows.append(f)
    hp.close()
    del ct
    return tuple(rows)


def candidate_lengths(name: str, mode: int = 0, mn: int = 0, mx: int = 15) -> List[Tuple[bytes, int, int]]:
    """(word, shortest, longest candidate) from the C oracle, for the words with candidates."""
    c = corpus(name)
    good, _ = split_panics(name, "words", mode, mn, mx)
    out = []
    for w, cands in zip(good, c_oracle_lists(c, good, mode, mn, mx)):
        if cands:
            ls = [len(x) for x in cands]
            out.append((w, min(ls), max(ls)))
    return out


def side_counts(rows, key, limit) -> Tuple[int, int]:
    """words with key(row) <= limit / > limit (rows where key gives None are left out)"""
    vals = [key(r) for r in rows]
    vals = [v for v in vals if v is not None]
    return sum(v <= limit for v in vals), sum(v > limit for v in vals)


def tied_facts(table, word: bytes) -> dict:
    """-s / -s -r facts of a word (k_keyspace_vsub's limits): occurrences of all patterns,
    distinct patterns, tied patterns (>= 2 occurrences) and the product of their choices."""
    ms = matches(table, word)
    occ: Dict[bytes, int] = {}
    for _, k in ms:
        occ[k] = occ.get(k, 0) + 1
    tied = [k for k, n in occ.items() if n >= 2]
    prod = 1
    for k in tied:
        prod *= len(table[k]) + 1
    keys = set(table)
    return {"occ": len(ms), "patterns": len(occ), "tied": len(tied), "subwords": prod, "subwords_r": 2 ** len(tied),
            "maxklen": max((len(k) for k in occ), default=0), "maxpos": max((p for p, _ in ms), default=-1),
            "fixed": all(len(v) == len(k) for k in occ for v in table[k]),
            "value_has_key": any(any(kk in v for kk in keys if kk) for k in occ for v in table[k])}


# ---------------------------------------------------------------------------
# huge lone-match words over the choices table, pinned (found with a5x_debug_plan_word):
# (word, P = product of R, FAST, DEFER, big pieces, big entries) in the window (0, HUGE_MAX)
# ---------------------------------------------------------------------------
HUGE_MAX = 32
HUGE = [
    (b"fcfcjiji", 64 * 64 * 63 * 63, True, False, 4, 254),   # big pieces 64 + 64 + 63 + 63: the largest FAST word
    (b"fcfcfcji", 64 * 64 * 64 * 63, False, False, 4, 255),  # 64 + 64 + 64 + 63: one entry past FB_EMAX
    (b"fcfcfcfc", 1 << 24, False, False, 4, 256),            # P = 2^24 needs 256 big entries
    (b"ffffff", 1 << 24, False, False, 6, 96),               # P = 2^24 as six 16-choice keys: 6 big pieces
    (b"aaaaaaaaabbbbbbbe", 16796160, False, False, 6, 119),  # the smallest P > 2^24 of this table's radices
    (b"fffffffe", 15 * 16 ** 7, False, False, 8, 127),       # P just below 2^32
    (b"ffffffff", 1 << 32, False, False, 8, 128),            # P = 2^32: the last word counted in closed form
    (b"aaaaaaaaaaaaaabdejjj", 4299816960, False, True, 9, 110),  # the smallest P > 2^32: deferred to the DP
]
HUGE_OVERFLOW = b"h" * 16  # 18^16 > 2^64


def huge_closed_form(table, word: bytes) -> Tuple[int, int]:
    """count = prod R - 1 and bytes = sum over candidates of (len + 1) of a lone-match word,
    in Python integers: sum over units of (sum of its choices' lengths) * (P / R), minus the
    unchanged word, plus the literal bytes and newline of every candidate."""
    us = [(bytes((b,)), [bytes((b,))] + table[bytes((b,))]) if bytes((b,)) in table else None for b in word]
    P = 1
    for u in us:
        if u:
            P *= len(u[1])
    lit = sum(1 for u in us if u is None) + 1
    total = P * lit + sum(sum(len(x) for x in u[1]) * (P // len(u[1])) for u in us if u)
    return P - 1, total - (len(word) + 1)


def decode_rank(table, word: bytes, rank: int) -> bytes:
    """The documented numbering (csrc/a5x_plan.h record comment, INTEGRATION.md "Candidate
    order"): n = rank + 1 in mixed radix over the word's units, left unit least significant;
    digit 0 keeps the key, digit 1 + v is value v in file order.  Lone one-byte keys only.
    The one place to update if the numbering is ever changed on purpose."""
    n, out = rank + 1, bytearray()
    for b in word:
        k = bytes((b,))
        if k not in table:
            out += k
            continue
        R = len(table[k]) + 1
        n, d = divmod(n, R)
        out += k if d == 0 else table[k][d - 1]
    assert n == 0, "rank beyond the word's keyspace"
    return bytes(out)
