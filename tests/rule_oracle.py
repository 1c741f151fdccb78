"""Plain-Python statement of the rule language of the digest + lookup stage (DESIGN.md "Rules"):
the rule-file parser and the interpreter, written from the specification table, not from
csrc/a5x_rules.h.  Words are bytes; case functions touch ASCII letters only."""
from __future__ import annotations

from typing import List, Optional, Tuple

OPS_MAX = 31
LMAX = 128

# parameter kinds: '' none, 'N' position, 'X' character, 'NM', 'NX', 'XY'
KINDS = {}
for _f in ":lucCtrdf{}[]qkKE":
    KINDS[_f] = ""
for _f in "TpD'zZLR+-.,yY":
    KINDS[_f] = "N"
for _f in "$^@e":
    KINDS[_f] = "X"
for _f in "xO*":
    KINDS[_f] = "NM"
for _f in "io":
    KINDS[_f] = "NX"
KINDS["s"] = "XY"


def pos(c: int) -> Optional[int]:
    if 0x30 <= c <= 0x39:
        return c - 0x30
    if 0x41 <= c <= 0x5A:
        return c - 0x41 + 10
    return None


def parse_line(line: bytes):
    """'ignored' (empty / comment), 'skipped' (unsupported or malformed), or the list of
    (function, p0, p1) of one rule line (without its newline)."""
    if line.endswith(b"\r"):
        line = line[:-1]
    i = 0
    while i < len(line) and line[i] in b" \t":
        i += 1
    if i == len(line) or line[i] == 0x23:
        return "ignored"
    ops = []
    while i < len(line):
        if line[i] == 0x20:
            i += 1
            continue
        f = chr(line[i])
        i += 1
        if f not in KINDS or len(ops) == OPS_MAX:
            return "skipped"
        kind = KINDS[f]
        if len(line) - i < len(kind):
            return "skipped"
        ps = []
        for k in kind:
            c = line[i]
            i += 1
            if k in "NM":
                c = pos(c)
                if c is None:
                    return "skipped"
            ps.append(c)
        ps += [0] * (2 - len(ps))
        ops.append((f, ps[0], ps[1]))
    return ops


def parse_rules(text: bytes) -> Tuple[List[list], int]:
    """(accepted rules in file order, skipped line count) of rule-file text."""
    rules, skipped = [], 0
    for line in text.split(b"\n"):
        r = parse_line(line)
        if r == "skipped":
            skipped += 1
        elif r != "ignored":
            rules.append(r)
    return rules, skipped


def _lower(c):
    return c + 32 if 0x41 <= c <= 0x5A else c


def _upper(c):
    return c - 32 if 0x61 <= c <= 0x7A else c


def _toggle(c):
    return _lower(c) if 0x41 <= c <= 0x5A else _upper(c)


def apply_op(w: bytes, op) -> bytes:
    f, a, b = op
    n = len(w)
    if f == ":":
        return w
    if f == "l":
        return bytes(map(_lower, w))
    if f == "u":
        return bytes(map(_upper, w))
    if f == "c":
        return bytes([_upper(_lower(w[0]))]) + bytes(map(_lower, w[1:])) if n else w
    if f == "C":
        return bytes([_lower(_upper(w[0]))]) + bytes(map(_upper, w[1:])) if n else w
    if f == "t":
        return bytes(map(_toggle, w))
    if f == "T":
        return w if a >= n else w[:a] + bytes([_toggle(w[a])]) + w[a + 1:]
    if f == "r":
        return w[::-1]
    if f == "d":
        return w + w if 2 * n <= LMAX else w
    if f == "p":
        return w * (a + 1) if n * (a + 1) <= LMAX else w
    if f == "f":
        return w + w[::-1] if 2 * n <= LMAX else w
    if f == "{":
        return w[1:] + w[:1]
    if f == "}":
        return w[-1:] + w[:-1]
    if f == "$":
        return w + bytes([a]) if n < LMAX else w
    if f == "^":
        return bytes([a]) + w if n < LMAX else w
    if f == "[":
        return w[1:]
    if f == "]":
        return w[:-1]
    if f == "D":
        return w if a >= n else w[:a] + w[a + 1:]
    if f == "x":
        return w if a >= n or a + b > n else w[a:a + b]
    if f == "O":
        return w if a >= n or a + b > n else w[:a] + w[a + b:]
    if f == "i":
        return w if a > n or n == LMAX else w[:a] + bytes([b]) + w[a:]
    if f == "o":
        return w if a >= n else w[:a] + bytes([b]) + w[a + 1:]
    if f == "'":
        return w if a >= n else w[:a]
    if f == "s":
        return w.replace(bytes([a]), bytes([b]))
    if f == "@":
        return w.replace(bytes([a]), b"")
    if f == "z":
        return w if n == 0 or n + a > LMAX else w[:1] * a + w
    if f == "Z":
        return w if n == 0 or n + a > LMAX else w + w[-1:] * a
    if f == "q":
        return bytes(c for c in w for _ in (0, 1)) if 2 * n <= LMAX else w
    if f == "k":
        return w if n < 2 else w[1:2] + w[0:1] + w[2:]
    if f == "K":
        return w if n < 2 else w[:-2] + w[-1:] + w[-2:-1]
    if f == "*":
        if a >= n or b >= n:
            return w
        l = list(w)
        l[a], l[b] = l[b], l[a]
        return bytes(l)
    if f in "LR+-":
        if a >= n:
            return w
        c = w[a]
        c = {"L": (c << 1) & 255, "R": c >> 1, "+": (c + 1) & 255, "-": (c - 1) & 255}[f]
        return w[:a] + bytes([c]) + w[a + 1:]
    if f == ".":
        return w if a + 1 >= n else w[:a] + w[a + 1:a + 2] + w[a + 1:]
    if f == ",":
        return w if a == 0 or a >= n else w[:a] + w[a - 1:a] + w[a + 1:]
    if f == "y":
        return w if a > n or n + a > LMAX else w[:a] + w
    if f == "Y":
        return w if a > n or n + a > LMAX else w + w[n - a:]
    if f in "Ee":
        # lower all; then the first byte and every byte that follows a separator of the
        # lowered word goes upper
        sep = 0x20 if f == "E" else a
        low = bytes(map(_lower, w))
        return bytes(_upper(c) if i == 0 or low[i - 1] == sep else c for i, c in enumerate(low))
    raise ValueError(f)


def apply_ops(w: bytes, ops) -> bytes:
    for op in ops:
        w = apply_op(w, op)
        assert len(w) <= LMAX
    return w


def apply_rule(rule: bytes, word: bytes) -> bytes:
    ops = parse_line(rule)
    if isinstance(ops, str):
        raise ValueError(f"{ops} rule line {rule!r}")
    return apply_ops(word, ops)
