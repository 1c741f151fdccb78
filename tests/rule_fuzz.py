"""The rule corpus of the digest + lookup stage (helper module, no tests here).

The host half of the rule interpreter (csrc/a5x_rules.h) is fuzzed against rule_oracle.py by
test_rules.py; the device half -- the v_perm / v_alignbyte branches, the dword-interleaved lane
buffer of a5x_stream.h, the candidate load at every (start & 3, length & 3) and the per-lane
`dirty` zeroing of k_rules_stream -- only runs on a GPU.  This module builds what both sides
run, deterministically and without any GPU code:

  grid_rules    every function alone: the N functions at every position 0..Z, the N M
                functions at all 36 x 36 pairs, i / o at every position, the parameterless
                ones, and the character functions with the characters of CHARS;
  chain_rules   random chains of 1..31 functions in test_rules' grammar, at least 50 of them
                31 long and 100 of 16 or more, each chain of 8 or more with a growing and a
                shrinking function;
  ordered       a fixed shuffle in which every rule that can grow a word is directly followed
                by one that cannot, so the next rule on the lane meets the longest leftovers;
  lines         the stream's lines: every length 0..128 twice (letters and boundary bytes;
                arbitrary bytes), a run of 220 lines of 0..8 bytes that starts on a block edge,
                lines over the 128-byte cap in the middle, pads that put one line's end exactly
                on a block edge and other lines across one, a last line without newline;
  census        what the oracle says the corpus reaches, per function.

corpus(kind) caches rules, lines, the oracle's ruled words and the census for one session.
Truth is rule_oracle.apply_op alone; the cap predicates of census() restate the specification
table (DESIGN.md "Rules"), not the interpreter.
"""
from __future__ import annotations

import functools
from collections import Counter
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import rule_oracle as ro

BLOCK = 4096   # STREAM_BLK of a5x_stream.h
MARGIN = 256   # STREAM_MARGIN of a5x_stream.h
LMAX = ro.LMAX
OPS_MAX = ro.OPS_MAX
POSITIONS = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
# NUL, 0xff, a space, a letter, and two bytes that are letters but for their high bit
CHARS = (0x00, 0xff, 0x20, 0x61, 0xc1, 0xe1)
GROW = "dpfqzZyY$^i"
SHRINK = "[]DxO'@"
AMOUNT_P1 = "xO"       # functions whose second parameter is a byte count
AMOUNT_P0 = "zZyYp"    # functions whose first parameter is a byte or copy count
OVER = (129, 256, 257, 400)  # rejected lines; 257 and 400 do not fit the staged margin
SHORT_RUN = 220
SEED = 20240


# ---- the grammar of test_rules' fuzz (moved here; test_rules imports it) ------------------
def random_rule(rng, fns):
    """A grammar-generated rule line of the given functions, with random spacing."""
    out = b""
    for f in fns:
        ps = b""
        for k in ro.KINDS[f]:
            if k in "NM":
                # mostly small positions, some up to 'Z' (35)
                v = int(rng.integers(0, 12)) if rng.random() < 0.8 else int(rng.integers(0, 36))
                ps += bytes([0x30 + v if v < 10 else 0x41 + v - 10])
            else:
                ps += bytes([int(rng.choice(list(b"aeiostAEZ 0159!-@\x00\xff\xe9")))])
        out += f.encode() + ps + (b" " if rng.random() < 0.3 else b"")
    return out


WORD_ALPHA = list(b"abcxyzABCXYZ019 -@!") + [0, 0x7f, 0x80, 0xe9, 0xff, 0x5b, 0x60, 0x7b, 0x40]


def random_word(rng, n, alpha=WORD_ALPHA):
    # letters of both cases, digits, separators, high and zero bytes
    return bytes(rng.choice(alpha, size=n).astype(np.uint8)) if n else b""


# ---- rules ----------------------------------------------------------------------------------
def grid_rules() -> List[bytes]:
    out = []
    for f, kind in sorted(ro.KINDS.items()):
        fb = f.encode()
        if kind == "":
            out.append(fb)
        elif kind == "N":
            out += [fb + bytes([p]) for p in POSITIONS]
        elif kind == "NM":
            out += [fb + bytes([p, q]) for p in POSITIONS for q in POSITIONS]
        elif kind == "NX":
            out += [fb + bytes([p, CHARS[i % len(CHARS)]]) for i, p in enumerate(POSITIONS)]
        elif kind == "X":
            out += [fb + bytes([c]) for c in CHARS]
        else:  # s X Y: each character once as X and once as Y
            out += [fb + bytes([c, CHARS[(i + 1) % len(CHARS)]]) for i, c in enumerate(CHARS)]
    assert all(b"\n" not in r and not r.endswith(b"\r") for r in out)
    return out


def chain_lengths(n: int) -> List[int]:
    """n chain lengths: a seventh each of 31 and of 16..30, a tenth of 8..15, the rest 1..7"""
    long_, mid, low = max(56, n // 7), max(56, n // 7), n // 10
    out = [OPS_MAX] * long_ + [16 + i % 15 for i in range(mid)] + [8 + i % 8 for i in range(low)]
    return out + [1 + i % 7 for i in range(n - len(out))]


def chain_rules(seed: int = SEED, n: int = 300) -> List[bytes]:
    rng = np.random.default_rng(seed)
    fns_all = sorted(ro.KINDS)
    lens = chain_lengths(n)
    rng.shuffle(lens)
    out = []
    for k in lens:
        fns = [str(rng.choice(fns_all)) for _ in range(k)]
        if k >= 8:  # a growing and a shrinking function in every longer chain
            a, b = (int(x) for x in rng.choice(k, size=2, replace=False))
            if not any(f in GROW for f in fns):
                fns[a] = str(rng.choice(list(GROW)))
            if not any(f in SHRINK for f in fns):
                if fns[b] in GROW and sum(f in GROW for f in fns) == 1:  # not in the only grower's place
                    b = (b + 1) % k
                fns[b] = str(rng.choice(list(SHRINK)))
        out.append(random_rule(rng, fns))
    assert all(b"\n" not in r and not r.endswith(b"\r") for r in out)
    return out


def functions(rule: bytes) -> List[str]:
    ops = ro.parse_line(rule)
    assert isinstance(ops, list), rule
    return [f for f, _, _ in ops]


def can_grow(rule: bytes) -> bool:
    return any(f in GROW for f in functions(rule))


def ordered(rules: Sequence[bytes], seed: int = SEED) -> List[bytes]:
    """The rules in a fixed shuffle; every rule that can grow is directly followed by one that cannot."""
    rng = np.random.default_rng(seed)
    grow = [r for r in rules if can_grow(r)]
    rest = [r for r in rules if not can_grow(r)]
    if len(rest) < len(grow):
        raise ValueError("more growing rules than others")
    rng.shuffle(grow)
    rng.shuffle(rest)
    units = [[g, s] for g, s in zip(grow, rest)] + [[s] for s in rest[len(grow):]]
    rng.shuffle(units)
    return [r for u in units for r in u]


# ---- lines ----------------------------------------------------------------------------------
def _pads(rng, gap: int) -> List[bytes]:
    """Lines of arbitrary bytes that take exactly gap stream bytes, newlines included."""
    out = []
    while gap > 0:
        n = min(gap, 100)
        out.append(_bytes(rng, n - 1))
        gap -= n
    return out


def _bytes(rng, n: int) -> bytes:
    return bytes(rng.integers(0, 256, size=n, dtype=np.uint8)).replace(b"\n", b"\x0b") if n else b""


def lines(seed: int = SEED) -> List[bytes]:
    """The stream's lines in stream order; stream() joins them (the last without a newline)."""
    rng = np.random.default_rng(seed)
    alpha = WORD_ALPHA + [0xc1, 0xe1]
    body = [random_word(rng, n, alpha) for n in range(LMAX + 1)] + [_bytes(rng, n) for n in range(LMAX + 1)]
    order = rng.permutation(len(body))
    body = [body[i] for i in order]
    if not body[-1]:  # (an empty last line without newline is no line)
        body[-1], body[-2] = body[-2], body[-1]
    out: List[bytes] = []
    pos = 0

    def put(xs):
        nonlocal pos
        for x in xs:
            out.append(x)
            pos += len(x) + 1

    def edge(back=0):  # pads up to `back` bytes before the next block edge
        put(_pads(rng, (-pos - back) % BLOCK))

    put(body[:90])
    put([_bytes(rng, OVER[0])])
    put(body[90:130])
    put([_bytes(rng, OVER[2])])           # 257 bytes, inside a block
    edge()                                # the pad before ends exactly on a block edge
    put([_bytes(rng, int(n)) for n in rng.integers(0, 9, size=SHORT_RUN)])
    put(body[130:170])
    edge(20)
    put([_bytes(rng, 100)])               # starts 20 bytes before an edge, ends behind it
    put(body[170:215])
    edge(20)
    put([_bytes(rng, OVER[3])])           # 400 bytes from 20 before an edge: ends past the staged margin
    put([_bytes(rng, OVER[1])])
    put(body[215:])
    return out


def starts(ls: Sequence[bytes]) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([len(x) + 1 for x in ls])])[:-1].astype(np.int64)


def stream(ls: Sequence[bytes]) -> bytes:
    return b"\n".join(ls)


# ---- the oracle's walk ----------------------------------------------------------------------
def _refused(f: str, a: int, n: int) -> bool:
    """The specification's cap conditions: the function would grow a word of n bytes past LMAX."""
    if f in "dfq":
        return 2 * n > LMAX
    if f == "p":
        return n * (a + 1) > LMAX
    if f in "$^":
        return n == LMAX
    if f == "i":
        return a <= n and n == LMAX
    if f in "zZ":
        return n > 0 and n + a > LMAX
    if f in "yY":
        return a <= n and n + a > LMAX
    return False


def walk(rules: Sequence[bytes], ls: Sequence[bytes]) -> Tuple[List[Optional[List[bytes]]], Dict]:
    """(ruled words [line][rule], None for a line over the cap; census) by rule_oracle.apply_op.

    Census, per function f: changed[f] counts (p0 & 3, length & 3) of the applications that
    changed the word (length before the function); amount[f] the byte count & 3 of those, for
    the functions that have one; full[f] the applications of a growing function whose result
    has exactly LMAX bytes; refused[f] those it declined at the cap; chains_31 the rules of
    OPS_MAX functions; full_words the (line, rule) pairs whose ruled word has LMAX bytes."""
    parsed = [ro.parse_line(r) for r in rules]
    assert all(isinstance(o, list) for o in parsed)
    changed: Dict[str, Counter] = {f: Counter() for f in ro.KINDS}
    amount: Dict[str, Counter] = {f: Counter() for f in AMOUNT_P0 + AMOUNT_P1}
    full, refused = Counter(), Counter()
    full_words = 0
    apply_op = ro.apply_op
    ruled: List[Optional[List[bytes]]] = []
    for ln in ls:
        if len(ln) > LMAX:
            ruled.append(None)
            continue
        row = []
        for ops in parsed:
            w = ln
            for op in ops:
                v = apply_op(w, op)
                f, a, b = op
                if v != w:
                    changed[f][(a & 3, len(w) & 3)] += 1
                    if f in AMOUNT_P0:
                        amount[f][a & 3] += 1
                    elif f in AMOUNT_P1:
                        amount[f][b & 3] += 1
                    if len(v) == LMAX and f in GROW:
                        full[f] += 1
                elif f in GROW and _refused(f, a, len(w)):
                    refused[f] += 1
                w = v
            full_words += len(w) == LMAX
            row.append(w)
        ruled.append(row)
    cen = {"changed": changed, "amount": amount, "full": full, "refused": refused, "full_words": full_words,
           "chains_31": sum(1 for o in parsed if len(o) == OPS_MAX),
           "chains_16": sum(1 for o in parsed if len(o) >= 16),
           "pairs": sum(1 for r in ruled if r is not None) * len(rules)}
    return ruled, cen


def census(rules: Sequence[bytes], ls: Sequence[bytes]) -> Dict:
    return walk(rules, ls)[1]


@functools.lru_cache(maxsize=None)
def corpus(kind: str):
    """kind "grid": ordered(grid_rules()); "chains": chain_rules().  -> (rules, lines, ruled, census)"""
    rules = ordered(grid_rules()) if kind == "grid" else chain_rules()
    ls = lines()
    ruled, cen = walk(rules, ls)
    return rules, ls, ruled, cen
