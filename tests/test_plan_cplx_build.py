"""The lean path of k_keyspace_cplx (csrc/a5x_plan.h cplx_word_lean) against the generic unit
walk, on the CPU.

a5x_debug_cplx_build runs one word through both on the host, over the code the kernel runs:
the lean path finds the matches with the compact key records, groups them into units as
next_unit does, counts by unit index (CountPlanner, every cluster enumerated once) and builds
the record per piece (CplxBuilder); the generic path is classify_word + plan_word_cached.  The
two must agree in flags, count, bytes and every u64 of the record, and the hook says which
words the lean path takes (why = 0) and why it leaves the others (a sum of WHY_*).  Every
test predicts why from the table and the word alone (predict_why, over tests/table_fuzz.py's
units), so a lean path that silently took nothing, or everything, fails.

Two reasons cannot be told apart from the word slot's on the device: a unit at byte >= 64 sits
in a word longer than the 36-byte slot.  The host hook reports every reason of such a word, so
the cluster at byte 63 is slot only and the one at byte 64 slot + position.  A key index >= 1024
is reachable from no table that loads (tests/test_table_fuzz.py).
"""
import ctypes
import random

import numpy as np
import pytest

import table_fuzz as tf
from conftest import table_path

WHY_LONGKEY, WHY_UNITS, WHY_POS, WHY_KEY, WHY_CLUSTER, WHY_NCL, WHY_SLOT = 1, 2, 4, 8, 16, 32, 64
WINDOWS = [(0, 15), (1, 15), (0, 1), (2, 2)]
GOLDEN = ["czech", "german", "qwerty-azerty", "qwerty-greek", "qwerty-cyrillic", "greek-hebrew"]
FIELDS = ("agree", "why", "flags", "built", "count_lo", "count_hi", "bytes_lo", "bytes_hi", "units", "clusters",
          "groups", "members")


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
        self.out = np.zeros(12, dtype=np.uint32)

    def check(self, word: bytes, mn=0, mx=15) -> dict:
        wb = np.frombuffer(word + b"\0", dtype=np.uint8)
        rc = self.L.a5x_debug_cplx_build(self.h, wb.ctypes.data, len(word), mn, mx, self.out.ctypes.data)
        assert rc == 0, self.L.a5x_last_error(self.h)
        d = dict(zip(FIELDS, (int(x) for x in self.out)))
        d["count"] = d["count_lo"] | d["count_hi"] << 32
        return d

    def close(self):
        self.L.a5x_destroy(self.h)


def _cluster_facts(table, word, u):
    """(matches, choices, longest choice) of the cluster u of tf.units: its choices are the sets of
    pairwise disjoint matches times their values."""
    ms = [(p, k) for p, k in tf.matches(table, word) if u["s"] <= p < u["e"]]

    def go(i, end):  # (choices, longest) over the matches from i on that start at or after end, as a delta to the span
        if i == len(ms):
            return 1, 0
        n, best = go(i + 1, end)
        p, k = ms[i]
        if p >= end:
            n2, b2 = go(i + 1, p + len(k))
            n += len(table[k]) * n2
            best = max(best, max(len(v) for v in table[k]) - len(k) + b2)
        return n, best
    n, best = go(0, u["s"])
    return len(ms), n, u["e"] - u["s"] + best


def predict_why(table, word: bytes, mx=15) -> int:
    if mx < 1 or not word:
        return WHY_SLOT if len(word) > 36 else 0
    why = WHY_SLOT if len(word) > 36 else 0
    for q in range(len(word)):
        if any(len(k) > 4 and k[0] == word[q] and q + len(k) <= len(word) for k in table):
            why |= WHY_LONGKEY
    # (a key longer than 4 bytes is no match to the lean path: the other reasons are those of the rest)
    table = {k: v for k, v in table.items() if len(k) <= 4}
    us = tf.units(table, word)
    if len(us) > 16:
        why |= WHY_UNITS
    if any(u["s"] >= 64 for u in us):
        why |= WHY_POS
    cl = [u for u in us if u["cluster"]]
    if len(cl) > 2:
        why |= WHY_NCL
    if any(u["nm"] > 8 for u in cl):
        why |= WHY_CLUSTER
    if why == 0:  # the count pass enumerates the clusters only of a word that got this far
        for u in cl:
            nm, R, ml = _cluster_facts(table, word, u)
            if R > 16 or ml > 7:
                why |= WHY_CLUSTER
    return why


def _run(h, table, words, windows=WINDOWS):
    """Every word agrees in every window and takes the path predicted; returns (lean, generic, built)."""
    lean = gen = built = 0
    for w in words:
        for mn, mx in windows:
            r = h.check(w, mn, mx)
            want = predict_why(table, w, mx)
            assert r["agree"] == 1, (w, mn, mx, r)
            assert r["why"] == want, (w, mn, mx, r, want)
            lean += r["why"] == 0
            gen += r["why"] != 0
            built += r["why"] == 0 and r["built"]
    return lean, gen, built


# ---------------------------------------------------------------------------
# czech + german: s / ss
# ---------------------------------------------------------------------------
def test_czech_german_ss_words():
    from oracle import a5_oracle as o
    table = o.load_tables([table_path(t) for t in ("czech", "german")])
    h = Hook(tables=["czech", "german"])
    words = []
    for run in (b"ss", b"sss", b"ssss", b"sssss"):
        words += [run, run + b"xyz", b"xyz" + run, b"xy" + run + b"zw", b"q" + run, run + b"q"]
    words += [b"ssxss", b"ssxxxxxxxxss", b"ssxssxss", b"sst", b"tss", b"ess", b"sse", b"tsst", b"usssu", b"strasse",
              b"wasserschloss", b"x" * 34 + b"ss", b"x" * 35 + b"ss", b"ss" + b"x" * 35]
    lean, gen, built = _run(h, table, words)
    for w, why in ((b"ss", 0), (b"ssxss", 0), (b"ssxssxss", WHY_NCL), (b"x" * 34 + b"ss", 0), (b"x" * 35 + b"ss", WHY_SLOT),
                   (b"sss", 0), (b"ssss", WHY_CLUSTER), (b"sssss", WHY_CLUSTER), (b"tsst", 0)):  # 12, 29 choices; 9 matches
        r = h.check(w)
        assert r["why"] == why and r["agree"] == 1, (w, r)
        if why == 0:
            assert r["built"] == 1 and r["clusters"] >= 1, (w, r)
    assert h.check(b"ss")["count"] == 4  # s0, s1, s0 + s1, ss
    h.close()
    assert lean > gen and built >= lean // 4, (lean, gen, built)  # (the capped windows build nothing)


# ---------------------------------------------------------------------------
# a table at the limits
# ---------------------------------------------------------------------------
V = [bytes((c,)) for c in b"0123456789ABCDEFGHIJ"]
LIMITS = {
    # every key holds 'd': in a word they overlap pairwise, so k matches are 1 + k choices ("d" has an empty value)
    b"abcd": [b"1"], b"bcd": [b"2"], b"cd": [b"3"], b"d": [b""], b"de": [b"4"], b"def": [b"5"], b"defg": [b"6"], b"cde": [b"7"],
    b"bcde": [b"8"],
    b"u": [b"1"],                      # R = 2: four fill a group
    b"x": V[:15], b"y": V[:16],        # lone units of 16 and 17 choices
    b"PQ": V[:7], b"Q": V[:8],         # a cluster of 1 + 7 + 8 = 16 choices
    b"RT": V[:8], b"T": V[:8],         # and of 17
    b"v": [b"1234567"], b"w": [b"12345678"],   # values of 7 and 8 bytes
    b"GH": [b"1234567"], b"H": [b"1"],         # a cluster choice of 7 bytes
    b"JK": [b"12345678"], b"K": [b"1"],        # and of 8
    b"lmnop": [b"1"],                  # a 5-byte key
    b"m": [b"1"],
}


def test_limits_directed():
    h = Hook(table_map=LIMITS)
    want = {
        # clusters of 2 to 8 matches, and 9
        b"cd": (0, 2), b"bcd": (0, 3), b"abcd": (0, 4), b"cdef": (0, 5), b"bcde": (0, 6), b"abcde": (0, 7), b"abcdef": (0, 8),
        b"abcdefg": (WHY_CLUSTER, 9),
        # a cluster next to a lone unit, no literal between them
        b"ucd": (0, None), b"cdu": (0, None), b"ucdu": (0, None), b"uuuucd": (0, None),
        # two and three clusters
        b"cd.cd": (0, None), b"cdcd": (0, None), b"cd..de..cd": (WHY_NCL, None), b"cdcdcd": (WHY_NCL, None),
        # R of 16 and 17, lone and in a cluster
        b"x": (0, None), b"y": (0, None), b".PQ.": (0, None), b".RT.": (WHY_CLUSTER, None),
        # choices of 7 and 8 bytes
        b"v": (0, None), b"w": (0, None), b"GH": (0, None), b"JK": (WHY_CLUSTER, None),
        # a 5-byte key where it fits, where it does not, and its first byte alone
        b"lmnop": (WHY_LONGKEY, None), b".lmnop.cd": (WHY_LONGKEY, None), b"cd.lmno": (0, None), b"cdl": (0, None),
        # 16 logged units, and 17
        b"u" * 16: (0, None), b"u" * 17: (WHY_UNITS, None), b"u.u" * 8: (0, None), b"cd" + b"u" * 15: (0, None),
        b"cd" + b"u" * 16: (WHY_UNITS, None),
        # a cluster at byte 63, and at byte 64 (both past the word slot)
        b"." * 63 + b"cd": (WHY_SLOT, None), b"." * 64 + b"cd": (WHY_SLOT | WHY_POS, None),
        b"." * 34 + b"cd": (0, None), b"." * 35 + b"cd": (WHY_SLOT, None),
        b"": (0, None), b".": (0, None), b"." * 36: (0, None),
    }
    nmatch = {w: len(tf.matches(LIMITS, w)) for w in want}
    for w, (why, k) in want.items():
        if k is not None:
            assert nmatch[w] == k, (w, nmatch[w])
        for mn, mx in WINDOWS + [(0, 40)]:
            r = h.check(w, mn, mx)
            assert r["agree"] == 1 and r["why"] == why, (w, mn, mx, r)
            assert r["why"] == predict_why(LIMITS, w, mx), (w, mn, mx, r)
    # what the lean path built
    r = h.check(b"abcdef")
    assert r["built"] and r["count"] == 8 and r["clusters"] == 1 and r["units"] == 1, r
    r = h.check(b"cdcd")  # two clusters of 3 choices in one group (9 entries)
    assert r["built"] and r["count"] == 8 and r["clusters"] == 2 | 256 and r["members"] == 2, r
    r = h.check(b"uuuu")
    assert r["built"] and r["count"] == 15 and r["members"] == 4 and r["groups"] == 1, r
    r = h.check(b".x.")  # (a FAST word's candidates have >= 3 bytes)
    assert r["built"] and r["count"] == 15, r
    for w in (b"y", b"w"):  # the unit does not fit a piece: not FAST on either path, no record
        r = h.check(w)
        assert not r["built"] and not r["flags"] & tf.FAST, (w, r)
    r = h.check(b"d.d")  # empty values: a candidate of 2 bytes, below the 3 a FAST word needs
    assert r["why"] == 0 and not r["built"], r
    r = h.check(b"u" * 16, 0, 40)
    assert r["built"] and r["count"] == 65535 and r["units"] == 16, r
    h.close()


def test_limits_random():
    rng = random.Random(0xC1EA)
    h = Hook(table_map=LIMITS)
    toks = list(LIMITS) + [b"abc", b"ef", b"s", b".", b"..", b"_", b"lmno", b"-------"]
    words = []
    for _ in range(1500):
        w = b""
        for _ in range(rng.randint(1, 7)):
            w += rng.choice(toks)
        words.append(w[:rng.choice((36, 36, 36, 40, 127))])
    lean, gen, built = _run(h, LIMITS, words, [(0, 15), (2, 2)])
    h.close()
    assert lean > 300 and gen > 300 and built > 100, (lean, gen, built)


# ---------------------------------------------------------------------------
# the golden tables, the fuzz corpora, the benchmark's words
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN)
def test_golden_tables(name):
    from oracle import a5_oracle as o
    table = o.load_tables([table_path(name)])
    keys = [k for k in table if k]
    rng = random.Random(len(name))
    words = tf.assemble(rng, table, keys, 150, 40, budget=1 << 20)
    h = Hook(tables=[name])
    lean, gen, built = _run(h, table, words, [(0, 15), (1, 15)])
    h.close()
    assert lean > gen and built > 50, (name, lean, gen, built)


@pytest.mark.parametrize("name", [n for n in tf.NAMES if n != "manykeys"])
def test_fuzz_corpora(name):
    c = tf.corpus(name)
    h = Hook(path=c.path)
    words = [w for w in c.words + c.narrow if len(w) <= 127]
    lean, gen, built = _run(h, c.table, words)
    h.close()
    assert lean >= 40, (name, lean, gen, built)
    if name in ("clusters", "longkeys"):
        assert gen >= 40 and built >= 20, (name, lean, gen, built)


def test_benchmark_words():
    """C3 (czech + german): the words with ss are the complex ones, and the lean path takes them."""
    from hashcat_a5_table_generator_amd import synth
    from oracle import a5_oracle as o
    tables, (data, offs) = synth.config_words("c3", 20000)
    table = o.load_tables([table_path(t) for t in tables])
    h = Hook(tables=tables)
    raw = data.tobytes()
    ss = lean_ss = 0
    for i in range(20000):
        w = raw[int(offs[i]):int(offs[i + 1])]
        r = h.check(w)
        assert r["agree"] == 1, (w, r)
        if b"ss" in w:
            ss += 1
            lean_ss += r["why"] == 0
            assert r["why"] == predict_why(table, w), (w, r)
    h.close()
    assert ss > 100 and lean_ss > 0.9 * ss, (ss, lean_ss)
