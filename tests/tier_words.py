"""Words at the limits that route a non-FAST word to pass A, B or G (helper module, no tests here).

A word that k_expand_fast does not take is sized by wave_setup (csrc/a5x_kernels.hip) against
one of three budgets: pass A (LDS, several waves per workgroup), pass B (one wave, large LDS),
pass G (HBM scratch slots); past pass G it is refused with A5X_E_UNSUPPORTED.  The budgets are
the constants of csrc/a5x_format.h restated in LIMITS below.  This module holds one small
synthetic table and, for every limit, a pair of words: one with the deciding fact exactly at
the limit and one at the next reachable value, every other fact of both inside the smaller
pass's budget (census() is the evidence; tests/test_tier_words.py asserts it).

facts() restates in Python what wave_setup, k_keyspace_wave and k_keyspace_g compute from a
word and the table, and the tier that follows.  reference() enumerates the candidates of a
word whose matches are disjoint and single-key by subset size, because neither oracle can
walk an (n, n) window: their recursion visits every smaller subset first.
"""
from __future__ import annotations

import atexit
import functools
import itertools
import math
import os
import shutil
import tempfile
from typing import Dict, List, Optional, Tuple

# csrc/a5x_format.h (a test of the constants, not a copy to keep in step silently:
# test_tier_words.py reads the header and compares)
LIMITS = {
    "A": {"L": 64, "nmatch": 128, "dp": 256, "maxlen": 4096 - 16},
    "B": {"L": 2048, "nmatch": 4096, "dp": 4096, "maxlen": 16384 - 16},
    "G": {"L": 65535, "nmatch": 65536, "dp": 1 << 20, "maxlen": (1 << 20) - 16},
}
WMAX = 64
HEADER_NAMES = {"A": ("A5X_LMAX_A", "A5X_MLMAX_A", "A5X_DPENT_A", "A5X_RING_A"),
                "B": ("A5X_LMAX_B", "A5X_MLMAX_B", "A5X_DPENT_B", "A5X_RING_B"),
                "G": ("A5X_LMAX_G", "A5X_MLMAX_G", "A5X_DPENT_G", "A5X_RING_G")}
TABLE_LDS_MAX = 32768

# per-word flags (csrc/a5x_format.h)
RADIX, BIN, GENERAL, BIG, DEFER, FAST, GLOB, VIRT, ERR_OVF, ERR_BIG = (1 << i for i in range(10))
E_OVERFLOW, E_UNSUPPORTED = -7, -9
WHY = {"L": 1, "nmatch": 2, "W": 3, "dp": 4, "maxlen": 5}  # bits 16..23 of a refused word's flags

FILL = b"."
# one-byte keys with one long value: (value length) chosen so that sums of them, plus filler
# bytes, hit 4080 / 16368 / 1048560 with at most 63 matches
LONG = {b"v": 24000, b"u": 4070, b"w": 1000, b"x": 100, b"y": 10}
TABLE: Dict[bytes, List[bytes]] = {
    b"a": [b"1"], b"aa": [b"22"], b"aaa": [b"333"], b"c": [b"C"],
    b"g": [bytes((0x41 + i,)) for i in range(17)],   # R = 18 > FW_UMAXR: radix, never FAST
}
for _k, _n in LONG.items():
    TABLE[_k] = [_k.upper() * _n]


def table_text() -> bytes:
    return b"".join(k + b"=" + v + b"\n" for k, vs in TABLE.items() for v in vs)


@functools.lru_cache(maxsize=None)
def table_file() -> str:
    d = tempfile.mkdtemp(prefix="a5x_tier_")
    atexit.register(shutil.rmtree, d, True)
    p = os.path.join(d, "tier.table")
    with open(p, "wb") as f:
        f.write(table_text())
    return p


# ---------------------------------------------------------------------------
# facts: wave_setup / k_keyspace_wave / k_keyspace_g in Python
# ---------------------------------------------------------------------------
_KLENS = sorted({len(k) for k in TABLE})


def _positions(word: bytes) -> List[Tuple[int, List[bytes]]]:
    """(position, keys matching there) for every position with a match (an event).  Linear in
    L: a position is looked at only where its byte starts a key."""
    firsts = {k[0] for k in TABLE}
    out = []
    for p, b in enumerate(word):
        if b not in firsts:
            continue
        ks = [word[p:p + kl] for kl in _KLENS if p + kl <= len(word) and word[p:p + kl] in TABLE]
        if ks:
            out.append((p, ks))
    return out


def _fits(f: dict, lim: dict) -> Optional[str]:
    """The first fact that does not fit a pass's WaveLds, in wave_setup's order, or None."""
    if f["L"] > lim["L"]:
        return "L"
    if f["nmatch"] > lim["nmatch"]:
        return "nmatch"
    if f["general"]:
        if f["W"] > WMAX:
            return "W"
        if f["dp"] > lim["dp"]:
            return "dp"
    return None


def facts(word: bytes, mn: int, mx: int) -> dict:
    ev = _positions(word)
    L = len(word)
    nmatch = sum(len(ks) for _, ks in ev)
    multi = any(len(ks) > 1 for _, ks in ev)
    conflict, end = False, 0
    for p, ks in ev:
        if end > p:
            conflict = True
        end = max(end, p + max(len(k) for k in ks))
    maxlen = L + 1 + sum(max(0, max(max(len(v) for v in TABLE[k]) - len(k) for k in ks)) for p, ks in ev)
    f = {"L": L, "nmatch": nmatch, "nev": len(ev), "conflict": conflict, "multi": multi, "maxlen": maxlen}
    if mx < 1 or L == 0 or nmatch == 0:
        f.update(freew=True, W=2, dp=0, general=False, radix=False, tier="none", why=None)
        return f
    freew = mn <= 1 and nmatch <= mx
    P = 1
    for _, ks in ev:
        P *= len(TABLE[ks[0]]) + 1
    radix = (not conflict) and (not multi) and freew and P < (1 << 64)
    W = 2 if freew else min(mx, nmatch) + 1
    f.update(freew=freew, W=W, general=not radix, radix=radix, dp=0 if radix else (len(ev) + 1) * W)
    cnt, byt, ovf = event_dp(word, ev, mn, mx, freew, nmatch)
    f.update(count=cnt, bytes=byt, ovf=ovf)
    why = None
    if _fits(f, LIMITS["A"]) is None and maxlen <= LIMITS["A"]["maxlen"]:
        tier = "A"
    elif _fits(f, LIMITS["B"]) is None and maxlen <= LIMITS["B"]["maxlen"]:
        tier = "B"
    elif _fits(f, LIMITS["B"]) == "W":      # k_keyspace_wave refuses it: pass G has no more columns
        tier, why = "refused", "W"
    else:
        why = _fits(f, LIMITS["G"]) or ("maxlen" if maxlen > LIMITS["G"]["maxlen"] else None)
        tier = "G" if why is None else "refused"
    if ovf and tier != "refused":           # (a refused word's DP is never run)
        tier = "overflow"
    f.update(tier=tier, why=why)
    return f


def event_dp(word: bytes, ev, mn: int, mx: int, freew: bool, nmatch: int) -> Tuple[int, int, bool]:
    """(count, bytes, overflow) by wave_setup's DP over events: G[e][c] completions from event e
    having made c substitutions (c clamped to 1 in the free window), H[e][c] their bytes from
    the event's position on, newline included.  Overflow is that of the word's own count or
    bytes: the table also holds states no candidate reaches (c substitutions made before
    event e < c), whose entries pass 64 bits long before the keyspace does -- C(63, 31) ways
    of 64 bytes for the one candidate of 'c' * 63 in the window (63, 63)."""
    import bisect
    m, L = len(ev), len(word)
    pos = [p for p, _ in ev] + [L]
    C = 1 if freew else min(mx, nmatch)
    W, lo = C + 1, (1 if mn <= 1 else mn)
    G = [[0] * W for _ in range(m + 1)]
    H = [[0] * W for _ in range(m + 1)]
    for c in range(W):
        G[m][c] = H[m][c] = int(c == 1 if freew else c >= lo)
    for e in range(m - 1, -1, -1):
        q, ks = ev[e]
        for c in range(W):
            g = G[e + 1][c]
            h = H[e + 1][c] + g * (pos[e + 1] - q)
            nc = 1 if freew else c + 1
            if nc <= C:
                for k in ks:
                    p2 = q + len(k)
                    e2 = bisect.bisect_left(pos, p2)
                    lit, nv = pos[e2] - p2, len(TABLE[k])
                    gs, hs = G[e2][nc], H[e2][nc]
                    g += gs * nv
                    h += hs * nv + gs * (sum(len(v) for v in TABLE[k]) + nv * lit)
            G[e][c], H[e][c] = g, h
    cnt, byt = G[0][0], H[0][0] + G[0][0] * pos[0]
    return cnt, byt, cnt >= (1 << 64) - 1 or byt >= (1 << 64) - 1


def tier_flags(f: dict) -> Tuple[int, int]:
    """(mask, value) of the flag bits a word of these facts must carry after the keyspace."""
    mask = BIG | GLOB | ERR_BIG | ERR_OVF | DEFER | FAST
    if f["tier"] == "overflow":
        return ERR_BIG | ERR_OVF | FAST, ERR_OVF
    if f["tier"] == "refused":
        # (a word refused for its columns by pass B is not BIG; pass G's refusals are BIG | GLOB)
        return ERR_BIG | ERR_OVF | FAST | (0xFF << 16), ERR_BIG | (WHY[f["why"]] << 16)
    v = {"A": 0, "B": BIG, "G": BIG | GLOB}[f["tier"]]
    return mask | RADIX | GENERAL, v | (RADIX if f["radix"] else GENERAL)


# ---------------------------------------------------------------------------
# reference: disjoint single-key matches, enumerated by subset size
# ---------------------------------------------------------------------------
def reference(word: bytes, mn: int, mx: int) -> List[bytes]:
    ev = _positions(word)
    f = facts(word, mn, mx)
    assert not f["conflict"] and not f["multi"], "reference() takes disjoint single-key matches only"
    out = []
    for k in range(max(mn, 1), min(mx, len(ev)) + 1):
        for comb in itertools.combinations(range(len(ev)), k):
            vals = [TABLE[ev[i][1][0]] for i in comb]
            for pick in itertools.product(*vals):
                parts, pos = [], 0
                for i, v in zip(comb, pick):
                    p, ks = ev[i]
                    parts.append(word[pos:p])
                    parts.append(v)
                    pos = p + len(ks[0])
                parts.append(word[pos:])
                out.append(b"".join(parts))
    return out


def reference_count(word: bytes, mn: int, mx: int) -> int:
    """len(reference()) for words of one-valued keys, without enumerating."""
    ev = _positions(word)
    assert all(len(TABLE[ks[0]]) == 1 and len(ks) == 1 for _, ks in ev)
    return sum(math.comb(len(ev), k) for k in range(max(mn, 1), min(mx, len(ev)) + 1))


def reverse_pruned(word: bytes, table: Dict[bytes, List[bytes]], mn: int, mx: int) -> List[bytes]:
    """-r (processWordReverse, main.go:208-261) for words of many overlapping positions, where the
    reference and both oracles walk every C(positions, k) combination before they drop the
    overlapping ones.  The same candidates from the non-overlapping subsets alone, sizes max
    down to min, each applied in descending position index with the running offset.
    test_tier_words checks it against the C oracle on small instances."""
    pos = [(i, kl, table[word[i:i + kl]][0]) for i in range(len(word)) for kl in range(1, len(word) - i + 1)
           if word[i:i + kl] in table]
    if len(pos) < mn:
        return []
    out: List[bytes] = []
    minkl = min(kl for _, kl, _ in pos) if pos else 1

    def subsets(j, k, end, acc):  # indices ascending, intervals disjoint
        if k == 0:
            yield list(acc)
            return
        for t in range(j, len(pos) - k + 1):
            if pos[t][0] + k * minkl > len(word):  # (k more disjoint keys do not fit behind here)
                break
            if pos[t][0] >= end:
                acc.append(t)
                yield from subsets(t + 1, k - 1, pos[t][0] + pos[t][1], acc)
                acc.pop()

    for k in range(min(mx, len(pos)), mn - 1, -1):
        for comb in subsets(0, k, 0, []):
            res, off = word, 0
            for t in reversed(comb):
                st, kl, s0 = pos[t]
                a = st + off
                assert 0 <= a and a + kl <= len(res)
                res = res[:a] + s0 + res[a + kl:]
                off += len(s0) - kl
            out.append(res)
    return out


# A5X_M_DPMAX with 63 positions: one 4-byte key over a run of 66 bytes.  15 disjoint
# occurrences fit 66 bytes in C(21, 15) = 54264 ways, 16 in C(18, 16) = 153
DP63_TABLE = {b"aaaa": [b"1234"]}
DP63_WORD = b"a" * 66


# ---------------------------------------------------------------------------
# the pairs
# ---------------------------------------------------------------------------
def maxlen_word(target: int, keys: Tuple[bytes, ...]) -> bytes:
    """A word of one-valued long keys and filler with maxlen == target: every key occurrence
    adds its value's length (its byte of L plus its delta), every filler byte 1, plus the 1."""
    rest, w = target - 1, b""
    for k in keys:
        n, rest = divmod(rest, LONG[k])
        w += k * n
    return w + FILL * rest


def _run(nmatch: int) -> bytes:
    """A run of a (3k - 3 matches under a / aa / aaa) plus c bytes: exactly nmatch matches."""
    k = (nmatch + 3) // 3
    return b"a" * k + b"c" * (nmatch - (3 * k - 3))


def _n(w: bytes) -> int:
    return sum(w.count(k) for k in LONG) + w.count(b"c")


class Pair:
    """limit: (pass, fact); at / over: (word, mn, mx); expect_*: tier, or an error code.
    expand: the GPU tests expand the word whole (its output is a few MiB at the most)."""

    def __init__(self, name, limit, at, over, t_at, t_over, expand=(True, True), err=(None, None)):
        self.name, self.limit, self.expand, self.err = name, limit, expand, err
        self.sides = {"at": at, "over": over}
        self.tier = {"at": t_at, "over": t_over}


@functools.lru_cache(maxsize=None)
def pairs() -> Tuple[Pair, ...]:
    out = []

    def nn(w):
        return (w, _n(w), _n(w))

    # ---- pass A | B
    out.append(Pair("A.L", ("A", "L"), (b"gc" + FILL * 62, 0, 15), (b"gc" + FILL * 63, 0, 15), "A", "B"))
    out.append(Pair("A.nmatch", ("A", "nmatch"), (_run(128), 0, 1), (_run(129), 0, 1), "A", "B"))
    out.append(Pair("A.dp", ("A", "dp"), (b"c" * 15, 15, 15), (b"c" * 16, 16, 16), "A", "B"))
    out.append(Pair("A.maxlen", ("A", "maxlen"), nn(maxlen_word(4080, (b"w", b"x", b"y"))),
                    nn(maxlen_word(4081, (b"w", b"x", b"y"))), "A", "B"))
    # k_keyspace_thread's own decision (classify_finish): slow list against deferral
    out.append(Pair("A.thread_maxl", ("A", "maxlen"), (b"gu" + FILL * 8, 0, 15), (b"gu" + FILL * 9, 0, 15), "A", "B"))
    # ---- pass B | G
    out.append(Pair("B.L", ("B", "L"), (b"gc" + FILL * 2046, 0, 15), (b"gc" + FILL * 2047, 0, 15), "B", "G"))
    out.append(Pair("B.nmatch", ("B", "nmatch"), (_run(4096), 0, 1), (_run(4097), 0, 1), "B", "G"))
    out.append(Pair("B.dp_square", ("B", "dp"), (b"c" * 63, 63, 63), (b"c" * 64, 63, 63), "B", "G"))
    out.append(Pair("B.dp_events", ("B", "dp"), (b"c" * 2047, 0, 1), (b"c" * 2048, 0, 1), "B", "G"))
    out.append(Pair("B.maxlen", ("B", "maxlen"), nn(maxlen_word(16368, (b"u", b"w", b"x", b"y"))),
                    nn(maxlen_word(16369, (b"u", b"w", b"x", b"y"))), "B", "G"))
    # ---- the count columns: 64 in any pass
    out.append(Pair("W", ("G", "W"), (b"c" * 64, 63, 63), (b"c" * 64, 64, 64), "G", "refused",
                    err=(None, E_UNSUPPORTED)))
    # ---- pass G | refused
    out.append(Pair("G.L", ("G", "L"), (b"gc" + FILL * 65533, 0, 15), (b"gc" + FILL * 65534, 0, 15), "G", "refused",
                    err=(None, E_UNSUPPORTED)))
    # 65536 matches are 65536 candidates of 21.8 KB each in the window (0, 1): never expanded whole
    out.append(Pair("G.nmatch", ("G", "nmatch"), (_run(65536), 0, 1), (_run(65537), 0, 1), "G", "refused",
                    expand=(False, False), err=(None, E_UNSUPPORTED)))
    # a DP of 2^20 entries is reachable only beside a count overflow: sum of C(16383, 2..63) > 2^64.
    # The near side runs the full-size DP and reports the overflow, the far side is refused
    out.append(Pair("G.dp", ("G", "dp"), (b"c" * 16383, 2, 63), (b"c" * 16384, 2, 63), "overflow", "refused",
                    expand=(False, False), err=(E_OVERFLOW, E_UNSUPPORTED)))
    out.append(Pair("G.maxlen", ("G", "maxlen"), nn(maxlen_word((1 << 20) - 16, (b"v", b"u", b"w", b"x", b"y"))),
                    nn(maxlen_word((1 << 20) - 15, (b"v", b"u", b"w", b"x", b"y"))), "G", "refused",
                    err=(None, E_UNSUPPORTED)))
    return tuple(out)


def pair(name: str) -> Pair:
    return next(p for p in pairs() if p.name == name)


def near_words(prefix: str = "") -> List[Tuple[str, bytes, int, int]]:
    """(pair name / side, word, mn, mx) of every word the engine must take (no error expected)."""
    out = []
    for p in pairs():
        if not p.name.startswith(prefix):
            continue
        for i, side in enumerate(("at", "over")):
            if p.err[i] is None:
                out.append((p.name + "/" + side,) + p.sides[side])
    return out


def short_fast_words(n: int = 200) -> List[bytes]:
    """Short words of one lone one-valued key in filler: FAST in every window that lets one
    substitution through (min <= 1 <= max)."""
    import random
    rng = random.Random(0x7157)
    out = []
    while len(out) < n:
        w = bytearray(rng.choice(b".-_") for _ in range(rng.randint(3, 12)))
        w[rng.randrange(len(w))] = ord("c")
        out.append(bytes(w))
    return out


def census() -> List[dict]:
    """One row per word of every pair: its facts, the deciding fact's value and the limit."""
    rows = []
    for p in pairs():
        for i, side in enumerate(("at", "over")):
            w, mn, mx = p.sides[side]
            f = facts(w, mn, mx)
            f.update(pair=p.name, side=side, word=w, mn=mn, mx=mx, limit=p.limit, expect=p.tier[side], err=p.err[i])
            rows.append(f)
    return rows
