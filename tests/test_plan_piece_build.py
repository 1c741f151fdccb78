"""The build pass of k_keyspace_thread for replayed words (csrc/a5x_plan.h PieceBuilder) against
the build-mode planner, on the CPU.

Planner<true> rewrites every entry of the open group at every merge; PieceBuilder decides
the same cuts per unit and writes a group's entries once per piece.  a5x_debug_piece_build
plans one word with both and compares the records (header, piece descriptors, entries):
0 equal, 1 different, 2 not applicable (overlapping matches or a unit that an 8-entry group
refuses), 3 not FAST and not comparable (more than 8 group pieces).  Words that are not FAST
but fit the builder's group list are compared as well.
"""
import ctypes
import random

import numpy as np
import pytest

import table_fuzz as tf
from conftest import table_path

EQUAL, DIFFERENT, NA, NOTFAST = 0, 1, 2, 3
FIELDS = ("code", "units", "np", "ng", "ne", "members", "tails", "literals", "fast")


class Hook:
    def __init__(self, tables=None, table_map=None, path=None):
        from hashcat_a5_table_generator_amd import _lib
        self.L = _lib.load()
        self.h = ctypes.c_void_p()
        assert self.L.a5x_create(-1, ctypes.byref(self.h)) == 0
        if path:
            assert self.L.a5x_load_table_file(self.h, path.encode()) == 0, self.L.a5x_last_error(self.h)
        elif tables:
            for t in tables:
                assert self.L.a5x_load_table_file(self.h, table_path(t).encode()) == 0
        else:
            txt = b"".join(k + b"=" + v + b"\n" for k, vs in table_map.items() for v in vs)
            assert self.L.a5x_parse_table(self.h, txt, len(txt)) == 0, self.L.a5x_last_error(self.h)
        self.out = np.zeros(9, dtype=np.uint32)

    def check(self, word: bytes) -> dict:
        wb = np.frombuffer(word + b"\0", dtype=np.uint8)
        rc = self.L.a5x_debug_piece_build(self.h, wb.ctypes.data, len(word), self.out.ctypes.data)
        assert rc == 0, self.L.a5x_last_error(self.h)
        return dict(zip(FIELDS, (int(x) for x in self.out)))

    def close(self):
        self.L.a5x_destroy(self.h)


# ---------------------------------------------------------------------------
# family A: keys that cannot overlap
# ---------------------------------------------------------------------------
SINGLE = b"abcdefghijklmn"
MULTI = [b"PQ", b"RS", b"TUV", b"WXYZ", b"ABC", b"DE"]  # no letter twice: no two matches overlap
FILLER = b".,_-+~"


def family_a_table(rng: random.Random) -> dict:
    """Distinct one-byte keys and some 2-4 byte keys over their own letters; R = 2..8, values
    of 0..7 bytes (digits: in no key)."""
    t = {}
    keys = [bytes((c,)) for c in rng.sample(SINGLE, rng.randint(3, 10))] + rng.sample(MULTI, rng.randint(1, 4))
    for i, k in enumerate(keys):
        nv = rng.randint(1, 7) if i else 7
        t[k] = [bytes(rng.choice(b"0123456789") for _ in range(rng.choice((0, 1, 1, 1, 2, 3, 4, 5, 6, 7)))) for _ in range(nv)]
    one = [k for k in t if len(k) == 1]
    t[one[0]] = [b"1"]            # an R = 2 key (three of them make a full group)
    t[one[1]] = [b"2222222"]      # a 7-byte value: a group of its own
    t[one[2]] = [b""]             # an empty value
    return t


def family_a_words(rng: random.Random, table: dict, n: int):
    """Directed and random words of 0..127 bytes with 0..16 units and at most 8 group pieces (the
    builder's group list, as for any FAST word): more than 8 units only as neighbouring R = 2
    keys, which share groups of three."""
    keys = list(table)
    r2 = [k for k in keys if len(k) == 1 and len(table[k]) == 1 and len(table[k][0]) <= 1]  # three fit a piece
    out = [b"", b".", b"x" * 127, b"." * 8, b"." * 14, b"." * 15]
    out += [keys[0], keys[1], r2[0] * 3, r2[0] * 4, r2[0] * 16, (r2[0] + b"...") * 3, r2[0] * 3 + b"..", r2[0] * 3 + b"......"]

    def fill(g):
        return bytes(rng.choice(FILLER) for _ in range(g))

    for _ in range(n):
        style = rng.random()
        if style < 0.45:    # dense: units merge into groups
            w = b"".join(fill(0 if rng.random() < 0.7 else rng.randint(1, 3)) + rng.choice(keys)
                         for _ in range(rng.randint(0, 8)))
        elif style < 0.75:  # runs of every length, up to several literal pieces
            w = b"".join(fill(rng.choice((0, 0, 1, 2, 5, 6, 7, 8, 9, 13, 14, 15, 22))) + rng.choice(keys)
                         for _ in range(rng.randint(0, 8)))
        else:               # 9..16 units: R = 2 keys side by side, one run somewhere
            u = rng.randint(9, 16)
            at = rng.randrange(u)
            w = b"".join(fill(rng.choice((0, 1, 4, 9)) if i == at else 0) + rng.choice(r2) for i in range(u))
        tail = rng.choice((0, 0, 1, 2, 3, 5, 6, 7, 8, 20)) if rng.random() < 0.9 else 127
        out.append((w + fill(tail))[:127])
    for L in (1, 6, 7, 8, 9, 10, 11, 12, 126, 127):
        out += [b"." * L, (keys[0] + b"." * 127)[:L], b"." * (L - 1) + r2[0]]
    return out


def test_family_a_every_word_equal():
    rng = random.Random(0xA11)
    seen = {"members3": 0, "tail_in": 0, "tail_out": 0, "literals2": 0, "fast": 0, "units16": 0, "units0": 0,
            "len127": 0, "R": set(), "vlen": set(), "notfast_compared": 0}
    n = 0
    for _ in range(40):
        t = family_a_table(rng)
        for vs in t.values():
            seen["R"].add(len(vs) + 1)
            seen["vlen"].update(len(v) for v in vs)
        h = Hook(table_map=t)
        for w in family_a_words(rng, t, 150):
            r = h.check(w)
            n += 1
            assert r["code"] == EQUAL, (w, r, t)
            f = r["fast"]
            seen["fast"] += f
            seen["notfast_compared"] += not f
            seen["members3"] += f and r["members"] == 3
            seen["tail_in"] += f and r["tails"] == 1
            seen["tail_out"] += f and r["ng"] >= 1 and r["tails"] == 0
            seen["literals2"] += f and r["units"] >= 1 and r["literals"] >= 2
            seen["units16"] += r["units"] == 16
            seen["units0"] += r["units"] == 0
            seen["len127"] += len(w) == 127
        h.close()
    assert seen["R"] == set(range(2, 9)) and seen["vlen"] == set(range(0, 8)), seen
    for k in ("members3", "tail_in", "tail_out", "literals2", "units16", "units0", "len127", "notfast_compared"):
        assert seen[k] >= 20, (k, seen)
    assert seen["fast"] > n // 3, (seen, n)


def test_family_a_directed_cuts():
    """Where a group closes: on cR * Ru > 8, on the 7-byte limit, with and without the tail."""
    h = Hook(table_map={b"a": [b"1"], b"b": [b"B", b"C", b"D"], b"c": [b"2222222"], b"d": [b""], b"PQ": [b"x", b"yz"]})
    want = {
        b"aaa": dict(np=1, ng=1, ne=8, members=3, tails=1),               # three R = 2 members + '\n': 4 bytes
        b"aaaa": dict(np=2, ng=2, ne=10, members=3, tails=1),             # closes on 2 * 2 * 2 * 2 > 8
        b"ab": dict(np=1, ng=1, ne=8, members=2, tails=1),                # 2 * 4 = 8 fits
        b"aba": dict(np=2, ng=2, ne=10, members=2, tails=1),              # 8 * 2 > 8
        b"a..a..a": dict(np=2, ng=1, ne=9, members=3, tails=0),           # 1 + 2 + 1 + 2 + 1 = 7 fits; '\n' would be the 8th byte
        b"a...a...a": dict(np=2, ng=2, ne=6, members=2, tails=1),         # a...a = 5, + ...a = 9 > 7
        b"aaa....": dict(np=2, ng=1, ne=9, members=3, tails=0),           # tail of 5 does not join 3
        b"aaa...": dict(np=1, ng=1, ne=8, members=3, tails=1),            # 3 + 3 + 1 = 7 joins
        b"c": dict(np=2, ng=1, ne=3, members=1, tails=0),                 # 7-byte value: '\n' is a literal piece
        b"ac": dict(np=3, ng=2, ne=5, members=1, tails=0),
        b"dPQd": None,
        b"." * 19 + b"a": dict(np=3, ng=1, ne=4, members=1, tails=1, literals=2),  # 7 + 7, then 5 + a + '\n'
        b"." * 20 + b"a": dict(np=4, ng=1, ne=5, members=1, tails=0, literals=3),  # 7 + 7, 6 + a, '\n' alone
        b"a" + b"." * 20: dict(np=4, ng=1, ne=5, members=1, tails=0, literals=3),
    }
    for w, exp in want.items():
        r = h.check(w)
        assert r["code"] == EQUAL, (w, r)
        if exp:
            got = {k: r[k] for k in exp}
            assert got == exp, (w, got, exp)
    h.close()


# ---------------------------------------------------------------------------
# family B: the planner-limit corpora (values > 7 bytes, R > 8, overlapping keys)
# ---------------------------------------------------------------------------
ROW = ("ok", "np", "ng", "ne", "maxl", "minl", "nbig", "bent")


def _count_rows(hp, w: bytes):
    """a5x_debug_plan_sizes: the count-mode plan with groups of <= 16 entries (what
    a5x_debug_plan_word classifies with) and of <= 8 (k_keyspace_thread, the hook); <= 64 bytes."""
    o = np.zeros(40, dtype=np.uint32)
    wb = np.frombuffer(w + b"\0", dtype=np.uint8)
    assert hp.L.a5x_debug_plan_sizes(hp.h, wb.ctypes.data, len(w), o.ctypes.data) == 0
    return ({k: int(v) for k, v in zip(ROW, o[0:8])}, {k: int(v) for k, v in zip(ROW, o[16:24])})


def _fast_by_sizes(row: dict, units: int, P: int) -> bool:
    """classify_finish's FAST conditions (csrc/a5x_plan.h) on a plan's sizes, free window"""
    if units == 0:
        return True
    return bool(row["ok"]) and row["np"] <= 8 and row["ne"] <= 255 and 1 + row["np"] + row["ne"] <= 250 and \
        row["maxl"] <= 1000 and row["minl"] >= 3 and P <= 1 << 24 and row["nbig"] <= 4 and row["bent"] <= 254


# manykeys is left out: its default table is refused (1024 keys or more do not fit the LDS table,
# tests/test_table_fuzz.py), so no word can be planned and the hook's "key index >= 1024" answer
# (not applicable) is reachable from no table that loads.
@pytest.mark.parametrize("name", [n for n in tf.NAMES if n != "manykeys"])
def test_family_b_corpora(name):
    """Never "different"; "not applicable" and "not FAST" agree with a5x_debug_plan_word.  That
    hook classifies with groups of <= 16 entries, this one with the kernel's 8: each FAST
    decision is checked against classify_finish's conditions on its own group size's plan
    (a5x_debug_plan_sizes), so where the two sizes cut a word alike the two hooks agree."""
    c = tf.corpus(name)
    h = Hook(path=c.path)
    hp = tf.HostPlan(c)
    codes = [0, 0, 0, 0]
    agree = 0
    for w in c.words + c.narrow:
        if len(w) > 127:
            continue
        r = h.check(w)
        codes[r["code"]] += 1
        assert r["code"] != DIFFERENT, (name, w, r)
        f = tf.facts(c.table, w)
        rc, cnt, byt, fl, nbig, bent = hp.classify(w, 0, 1 << 20)
        assert rc == 0, (name, w)
        fast16 = bool(fl & tf.FAST) and not fl & tf.DEFER
        if len(w) > 64:  # a5x_debug_plan_word leaves such a word to the wave kernel whatever it holds
            assert fl == tf.DEFER, (name, w, hex(fl))
            continue
        row16, row8 = _count_rows(hp, w)
        if r["code"] == NA:
            # a cluster, a lone unit of more than 8 choices, or a choice of more than 7 bytes
            assert f["clusters"] or f["maxR_lone"] > 8 or f["maxv"] > 7, (name, w, r, f)
            if f["clusters"]:
                assert fl & tf.DEFER or not fl & tf.RADIX, (name, w, hex(fl))
            else:  # the count pass's planner refuses the unit as well
                assert not row8["ok"], (name, w, row8)
                if f["maxv"] > 7 or f["maxR_lone"] > 16:
                    assert not fast16, (name, w, hex(fl))
            continue
        assert not f["clusters"] and f["maxR_lone"] <= 8 and f["maxv"] <= 7, (name, w, r, f)
        fast8 = _fast_by_sizes(row8, f["units"], f["P"])
        assert fast16 == _fast_by_sizes(row16, f["units"], f["P"]), (name, w, hex(fl), row16)
        if r["code"] == NOTFAST:
            assert row8["ok"] and row8["ng"] == r["ng"] > 8 and row8["np"] > 8 and not fast8 and not r["fast"], (name, w, r, row8)
        else:
            assert (r["np"], r["ng"], r["ne"]) == (row8["np"], row8["ng"], row8["ne"]), (name, w, r, row8)
            assert bool(r["fast"]) == fast8, (name, w, r, row8)
            if r["fast"] and cnt:
                assert cnt == f["P"] - 1, (name, w, cnt, f["P"])
        if row16 == row8:
            assert fast16 == bool(r["fast"]), (name, w, r, hex(fl))
            agree += 1
    h.close()
    hp.close()
    assert codes[EQUAL] >= 20 and agree >= 20, (name, codes, agree)


# ---------------------------------------------------------------------------
# the benchmark's words
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("wl,n", [("c3", 20000), ("c5", 20000)])
def test_benchmark_words_equal(wl, n):
    from hashcat_a5_table_generator_amd import synth
    tables, (data, offs) = synth.config_words(wl, n)
    h = Hook(tables=tables)
    raw = data.tobytes()
    codes = [0, 0, 0, 0]
    fast = 0
    for i in range(n):
        w = raw[int(offs[i]):int(offs[i + 1])]
        r = h.check(w)
        codes[r["code"]] += 1
        fast += r["fast"]
        assert r["code"] in (EQUAL, NA), (w, r)  # NA: czech+german's s / ss clusters
    h.close()
    assert codes[EQUAL] > n // 2 and fast > n // 2, (codes, fast)
    if wl == "c5":
        assert codes[NA] == 0, codes  # greek-hebrew has no overlapping keys
