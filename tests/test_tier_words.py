"""The tier words of tests/tier_words.py checked on the CPU: the helper's reference against both
oracles, its facts against the closed-form keyspace, the census of the pairs (both sides of
every limit of the per-word path, nothing else past the smaller budget), and the thread-level
classifier's deferral on the host replay.  tests/test_gpu_tier_words.py runs the same words
through the kernels."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import tier_words as tw
from conftest import ROOT


@pytest.fixture(scope="module")
def host():
    from hashcat_a5_table_generator_amd import Context
    c = Context(-1)
    c.load_tables([tw.table_file()])
    yield c
    c.close()


def _plan(c, word, mn, mx):
    info = np.zeros(4, dtype=np.uint64)
    wb = np.frombuffer(word + b"\0", dtype=np.uint8)
    rc = c._L.a5x_debug_plan_word(c.h, wb.ctypes.data, len(word), mn, mx, None, 0, info.ctypes.data)
    assert rc == 0, rc
    return int(info[0]), int(info[1]), int(info[2]) & 0xFFFFFFFF


def test_limits_are_the_headers():
    with open(os.path.join(ROOT, "hashcat_a5_table_generator_amd", "csrc", "a5x_format.h")) as f:
        src = f.read()

    def define(name):
        text = re.search(r"#define\s+" + name + r"\s+([^/\n]+)", src).group(1).strip()
        m = re.fullmatch(r"\(\s*(\d+)u?\s*<<\s*(\d+)\s*\)", text)  # "(1u << 20)", else "65535"
        return int(m.group(1)) << int(m.group(2)) if m else int(text.rstrip("u"), 0)

    for tier, (l, ml, dp, ring) in tw.HEADER_NAMES.items():
        lim = tw.LIMITS[tier]
        assert (lim["L"], lim["nmatch"], lim["dp"], lim["maxlen"]) == (define(l), define(ml), define(dp), define(ring) - 16)
    assert tw.WMAX == define("A5X_CMAX") + 1 and tw.TABLE_LDS_MAX == define("A5X_TABLE_LDS_MAX")


def test_table_is_staged_under_32k(host):
    """The default engine compiles the table (it refuses one beyond A5X_TABLE_LDS_MAX) and the
    library reads it back as written."""
    assert len(tw.table_text()) < tw.TABLE_LDS_MAX
    n = ctypes.c_uint32()
    assert host._L.a5x_debug_keyspace_small_stage(host.h, ctypes.byref(n)) == 0
    assert host.table() == tw.TABLE


def _small_instances():
    """(word, mn, mx): disjoint single-key words of n <= 12 matches in every kind of window the
    pairs use: free (0, 15), one substitution (0, 1), exact (n, n), (n - 1, n - 1), a capped
    window with a floor (2, 63), and windows past the matches."""
    words = [b"c" * n for n in range(1, 13)] + [b"c.g", b"g", b"gy.c", b"x.yy..c", b".c.y.c.x.", b"ycgc", b"w.c",
                                                 b"cccc.cccc.cccc", b"y" * 7 + b"." * 9, b"gg"]
    out = []
    for w in words:
        n = len(tw._positions(w))
        for mn, mx in {(0, 15), (1, 15), (0, 1), (n, n), (max(n - 1, 1), max(n - 1, 1)), (2, 63), (63, 63), (2, 3)}:
            out.append((w, mn, mx))
    return out


def test_reference_equals_both_oracles():
    from oracle import a5_oracle as o
    from oracle import c_oracle as co
    sub = o.load_tables([tw.table_file()])
    ct = co.CTable([tw.table_file()])
    total = 0
    for w, mn, mx in _small_instances():
        ref = sorted(tw.reference(w, mn, mx))
        assert ref == sorted(o.process_word(w, sub, mn, mx)), (w, mn, mx)
        assert ref == sorted(ct.expand_word(w, 0, mn, mx)), (w, mn, mx)
        f = tw.facts(w, mn, mx)
        if f["tier"] != "none":
            assert (f["count"], f["bytes"]) == (len(ref), sum(len(x) + 1 for x in ref)), (w, mn, mx)
        total += len(ref)
    assert total > 10000


def test_reverse_pruned_equals_the_c_oracle(tmp_path):
    """reverse_pruned (the non-overlapping subsets alone) == the C oracle's -r on overlapping
    runs small enough for it, values longer and (where the reference does not panic) shorter than their keys included."""
    import math
    from oracle import c_oracle as co
    table = {b"aaaa": [b"1234"], b"aa": [b"XY"], b"b": [b"YYY", b"unused"], b"ab": [b"Z"]}
    p = tmp_path / "r.table"
    p.write_bytes(b"".join(k + b"=" + v + b"\n" for k, vs in table.items() for v in vs))
    ct = co.CTable([str(p)])
    n = 0
    for w in (b"a" * 9, b"aaaab.aa", b"baab", b"a" * 6 + b"b" + b"a" * 5):
        for mn, mx in ((0, 15), (1, 2), (2, 2), (3, 3), (2, 16)):
            try:
                want = sorted(ct.expand_word(w, 1, mn, mx))
            except RuntimeError:  # the reference's slice-bounds panic (main.go:255)
                with pytest.raises(AssertionError):
                    tw.reverse_pruned(w, table, mn, mx)
                continue
            assert sorted(tw.reverse_pruned(w, table, mn, mx)) == want, (w, mn, mx)
            n += len(want)
    assert n > 300
    # the 63-position word: the counts the GPU test relies on
    assert len(tw.DP63_WORD) - 3 == 63
    assert len(tw.reverse_pruned(tw.DP63_WORD, tw.DP63_TABLE, 15, 15)) == math.comb(21, 15)


def test_facts_equal_the_closed_form():
    """count and bytes of facts() (the kernel's event DP restated) == a5_oracle.keyspace_default
    (a DP over byte positions) for every word of every pair that has a 64-bit keyspace."""
    from oracle import a5_oracle as o
    sub = o.load_tables([tw.table_file()])
    for r in tw.census():
        if r["ovf"]:
            continue
        assert o.keyspace_default(r["word"], sub, r["mn"], r["mx"]) == (r["count"], r["bytes"]), (r["pair"], r["side"])
    # the overflow pair: one-valued keys, so the count is a sum of binomials
    for side in ("at", "over"):
        w, mn, mx = tw.pair("G.dp").sides[side]
        want = sum(math.comb(len(w), k) for k in range(mn, mx + 1))
        assert tw.facts(w, mn, mx)["count"] == want and want >> 64


def test_reference_counts_of_the_pairs():
    """The (n, n) words have exactly one candidate, of maxlen - 1 bytes: the ring is filled to
    the limit, not only bounded by it."""
    for name in ("A.maxlen", "B.maxlen", "G.maxlen"):
        for side in ("at", "over"):
            w, mn, mx = tw.pair(name).sides[side]
            ref = tw.reference(w, mn, mx)
            assert len(ref) == 1 and len(ref[0]) + 1 == tw.facts(w, mn, mx)["maxlen"]
    w, mn, mx = tw.pair("W").sides["at"]
    assert tw.reference_count(w, mn, mx) == 64 == len(tw.reference(w, mn, mx))


def test_census():
    """Both words of every pair exist, the deciding fact has exactly the limit and the next
    reachable value, every other fact of both is inside the smaller pass's budget, the tier
    that facts() derives is the one the pair states, and only far-side words (and the near
    side of the 2^20 DP, which can only overflow) carry an error code."""
    rows = tw.census()
    seen = set()
    print()
    print("%-14s %-5s %6s %6s %6s %3s %8s %8s %-5s %-9s %s" % ("pair", "side", "L", "nmatch", "nev", "W", "dp", "maxlen",
                                                               "class", "tier", "error"))
    for r in rows:
        print("%-14s %-5s %6d %6d %6d %3d %8d %8d %-5s %-9s %s" % (
            r["pair"], r["side"], r["L"], r["nmatch"], r["nev"], r["W"], r["dp"], r["maxlen"],
            "radix" if r["radix"] else "gen", r["tier"] + ("(%s)" % r["why"] if r["why"] else ""), r["err"]))
        tier, fact = r["limit"]
        lim = dict(tw.LIMITS[tier], W=tw.WMAX)
        if r["side"] == "at":
            assert r[fact] == lim[fact], (r["pair"], r[fact])
        else:
            assert lim[fact] < r[fact] <= lim[fact] + 65, (r["pair"], r[fact])
        for other in ("L", "nmatch", "dp", "maxlen", "W"):
            if other != fact:
                assert r[other] <= lim[other], (r["pair"], r["side"], other, r[other])
        assert r["tier"] == r["expect"], (r["pair"], r["side"], r["tier"])
        if r["tier"] == "refused":
            assert r["why"] == fact and r["err"] == tw.E_UNSUPPORTED and r["side"] == "over"
        elif r["tier"] == "overflow":
            assert r["err"] == tw.E_OVERFLOW and (r["pair"], r["side"]) == ("G.dp", "at")
        else:
            assert r["err"] is None
        assert not (r["radix"] and r["general"]) and r["nev"] >= 1
        seen.add((tier, fact, r["side"]))
    # the issue's tables: four facts per pass, and the count columns
    for tier in "ABG":
        for fact in ("L", "nmatch", "dp", "maxlen"):
            assert (tier, fact, "at") in seen and (tier, fact, "over") in seen, (tier, fact)
    assert ("G", "W", "at") in seen and ("G", "W", "over") in seen
    # next reachable: the far side is one past the limit wherever one is reachable (a square DP
    # grows by a row and a column, an event adds a row of W entries)
    step = {(r["pair"]): r[r["limit"][1]] - dict(tw.LIMITS[r["limit"][0]], W=tw.WMAX)[r["limit"][1]]
            for r in rows if r["side"] == "over"}
    assert all(v == 1 for k, v in step.items() if not k.endswith(("dp", "dp_square", "dp_events"))), step
    assert step["A.dp"] == 33 and step["B.dp_square"] == 64 and step["B.dp_events"] == 2 and step["G.dp"] == 64


def test_thread_level_deferral(host):
    """k_keyspace_thread's own classifier (classify_finish through a5x_debug_plan_word): a radix
    word in a free window is kept for the slow list up to 64 bytes and up to a longest candidate
    of A5X_RING_A - 16 bytes with its newline, and deferred to the wave kernel one past either."""
    for name in ("A.L", "A.thread_maxl"):
        p = tw.pair(name)
        w, mn, mx = p.sides["at"]
        f = tw.facts(w, mn, mx)
        cnt, byt, fl = _plan(host, w, mn, mx)
        assert not fl & (tw.DEFER | tw.FAST) and fl & tw.RADIX, (name, hex(fl))
        assert (cnt, byt) == (f["count"], f["bytes"])
        w, mn, mx = p.sides["over"]
        cnt, byt, fl = _plan(host, w, mn, mx)
        assert fl == tw.DEFER and (cnt, byt) == (0, 0), (name, hex(fl))
    # capped windows are never the thread kernel's: every general pair word is deferred
    for r in tw.census():
        if r["general"] and r["L"] <= 64:
            assert _plan(host, r["word"], r["mn"], r["mx"])[2] == tw.DEFER, r["pair"]


def test_short_words_are_fast(host):
    """The 200 words the GPU tests interleave with the tier words take the FAST path."""
    words = tw.short_fast_words()
    assert len(words) == 200
    for w in words:
        cnt, _, fl = _plan(host, w, 0, 15)
        assert fl & tw.FAST and cnt == 2 ** w.count(b"c") - 1, w
