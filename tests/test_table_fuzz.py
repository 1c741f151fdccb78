"""Differential tests on synthetic tables at the planner's limits (CPU).

tests/table_fuzz.py builds the corpora.  Here, for every corpus:
(a) the C oracle equals the Python oracle per word in all four modes (Python on the words
    with at most 2000 candidates, at least half of each corpus), the words on which the
    reference panics under -r (main.go:255, 263-281) raise in both;
(b) the host replay a5x_debug_plan_word (the code the keyspace and k_expand_fast kernels run
    per word) gives the oracle's count and bytes for every non-deferred word and its
    candidate multiset for every FAST word;
(c) a census proves that each limit named in csrc/a5x_plan.h and friends has at least
    MIN_SIDE words on either side, that the side decides the class where the class is
    observable, and that the limits argued unreachable were not reached.  Run with -s to
    print the census table.
"""
import collections
import math

import pytest

import table_fuzz as tf
from oracle import a5_oracle as o

MIN_SIDE = 5
PY_MAX = 2000
DEFAULT_CORPORA = [n for n in tf.NAMES if 0 in tf.corpus(n).modes]

FW_PLEN, FW_UMAXM, FW_UMAXR, FW_PMAX, FW_RMAX, FW_MAXL = 7, 8, 16, 8, 250, 1000
FB_RMAX, FB_NMAX, FB_EMAX = 64, 4, 254
UC_UNITS, UC_CLUSTERS = 8, 2


# ---------------------------------------------------------------------------
# (a) C oracle == Python oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [(n, m) for n in tf.NAMES for m in tf.corpus(n).modes])
def test_c_oracle_equals_python_oracle(name, mode):
    c = tf.corpus(name)
    for m, mn, mx, which in c.runs():
        if m != mode:
            continue
        good, bad = tf.split_panics(name, which, mode, mn, mx)
        for w in bad[:40]:  # the reference panics: both oracles raise
            with pytest.raises(o.GoPanic):
                o.expand(w, c.table, mode, mn, mx)
        if which == "narrow":
            continue  # ~64 patterns / positions: past the Python oracle (see test_pruned_suball_*)
        lists = tf.c_oracle_lists(c, good, mode, mn, mx)
        small = 0
        for w, want in zip(good, lists):
            # (the reference's own cost is 2^positions under -r and 2^patterns under -s / -s -r)
            if len(want) > PY_MAX or (mode and len(tf.matches(c.table, w)) > 10):
                continue
            small += 1
            assert sorted(o.expand(w, c.table, mode, mn, mx)) == want, (name, mode, mn, mx, w)
        assert 2 * small >= len(good), (name, mode, mn, mx, small, len(good))


@pytest.mark.parametrize("name", ["tied", "choices", "utf8_empty"])
def test_pruned_suball_equals_python_oracle(name):
    """suball_pruned (the reference of the narrow -s / -s -r runs) on every small word."""
    c = tf.corpus(name)
    n = 0
    for w in c.words:
        if len(o.unique_patterns(w, c.table)) > 10:
            continue
        for mode in (2, 3):
            for mn, mx in tf.WINDOWS + [tf.REVERSE_EXTRA]:
                assert sorted(tf.suball_pruned(w, c.table, mn, mx, mode == 3)) == sorted(o.expand(w, c.table, mode, mn, mx)), \
                    (name, w, mode, mn, mx)
                n += 1
    assert n > 500


# ---------------------------------------------------------------------------
# (b) host replay
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEFAULT_CORPORA)
def test_host_replay_matches_oracle(name):
    c = tf.corpus(name)
    hp = tf.HostPlan(c)
    kinds = collections.Counter()
    for mn, mx in tf.WINDOWS:
        for which in ("words", "narrow"):
            words = c.word_list(which)
            if which == "narrow" and (mn, mx) not in tf.NARROW:
                continue
            for w, want in zip(words, tf.c_oracle_lists(c, words, 0, mn, mx)):
                rc, cnt, byt, fl, _, _, cands = hp.plan(w, mn, mx)
                assert rc == 0, (name, w, rc)
                if fl & tf.DEFER:
                    kinds["defer"] += 1
                    continue
                assert (cnt, byt) == (len(want), sum(len(x) + 1 for x in want)), (name, w, mn, mx, fl)
                if fl & tf.FAST and cands is not None:
                    assert sorted(cands) == want, (name, w, mn, mx)
                    kinds["fast"] += 1
                else:
                    kinds["slow"] += 1
    hp.close()
    assert kinds["fast"] > 50 and kinds["slow"] > 0, kinds


@pytest.mark.parametrize("name", DEFAULT_CORPORA)
def test_count_planner_equals_build_planner(name):
    """CountPlanner (the count pass of k_keyspace_thread) cuts every word as Planner does, and
    k_keyspace_cplx's record from cached units equals plan_word's (a5x_debug_plan_sizes)."""
    for r in tf.census(name):
        s = r["sizes"]
        if s is None or not s["ok"]:
            continue
        cm = s["count_mode"]
        assert {k: cm[k] for k in ("ok", "np", "ng", "ne", "maxl", "minl", "nbig", "bent")} == \
               {k: s[k] for k in ("ok", "np", "ng", "ne", "maxl", "minl", "nbig", "bent")}, (name, r["word"])
        assert s["route"] in (1, 2, 3), (name, r["word"], "cached-unit record differs from plan_word's")
        if r["fast"] and r["count"]:
            assert s["route"] != 3, (name, r["word"])


# ---------------------------------------------------------------------------
# (c) census
# ---------------------------------------------------------------------------
_TABLE = []


def _sides(label, rows, key, limit, corpus):
    lo, hi = tf.side_counts(rows, key, limit)
    _TABLE.append((label, corpus, limit, lo, hi))
    assert lo >= MIN_SIDE and hi >= MIN_SIDE, (label, corpus, limit, lo, hi)


def _plan(r):  # the plan of a word whose every unit fits a piece (ok), else None
    return r["sizes"] if r["sizes"] and r["sizes"]["ok"] else None


def _plain(r):
    """a word the other FAST conditions accept: what is left decides the class"""
    p = _plan(r)
    return (p and p["np"] <= FW_PMAX and p["nbig"] <= FB_NMAX and p["bent"] <= FB_EMAX and p["minl"] >= 3 and
            r["P"] <= 1 << 24 and r["nmatch"] <= 15 and not r["defer"])


def test_census_choices():
    rows = tf.census("choices")
    _sides("FW_UMAXR: choices of a lone key", rows, lambda r: r["maxR_lone"], FW_UMAXR, "choices")
    # the positional path's 14 values (-s / -s -r): words with the 14- and the 15-value key
    has = lambda k: sum(1 for r in rows if k in r["word"])
    _TABLE.append(("positional path: 14 / 15 values", "choices", 14, has(b"e"), has(b"f")))
    assert has(b"e") >= MIN_SIDE and has(b"f") >= MIN_SIDE
    # the side decides the class: the same word with the 16-choice key is FAST, with the 17-choice key not
    by = {r["word"]: r for r in rows}
    pairs = 0
    for t in (b"ab.%s.c", b"%s..a", b".%s", b"c%sb", b"%s_", b"12%s34", b"a%sa", b"b-%s-", b"%s+b", b"..%s.."):
        assert by[t % b"e"]["fast"] and by[t % b"f"]["fast"], t
        assert not by[t % b"g"]["fast"] and not by[t % b"h"]["fast"], t
        assert by[t % b"g"]["radix"], t  # (a radix word of the per-word path, counted in closed form)
        pairs += 1
    assert pairs >= MIN_SIDE
    for r in rows:
        if r["maxR_lone"] > FW_UMAXR:
            assert not r["fast"], r["word"]


def test_census_lengths():
    rows = tf.census("lengths")
    _sides("FW_PLEN: longest value", rows, lambda r: r["maxv"] if r["units"] else None, FW_PLEN, "lengths")
    by = {r["word"]: r for r in rows}
    assert by[b"..c.."]["fast"] and not by[b"..d.."]["fast"] and not by[b"..e.."]["fast"] and not by[b"..f.."]["fast"]
    for r in rows:
        if r["maxv"] > FW_PLEN:
            assert not r["fast"], r["word"]
        elif _plain(r):
            assert r["fast"], r["word"]
    # minl >= 3 (shortest candidate + newline): plans on both sides, and the side decides
    _sides("minl >= 3: shortest candidate + newline", rows, lambda r: _plan(r)["minl"] if _plan(r) and r["units"] else None,
           2, "lengths")
    for r in rows:
        p = _plan(r)
        if p and r["units"] and p["minl"] < 3:
            assert not r["fast"], r["word"]
    assert by[b"a.."]["fast"] and not by[b"a."]["fast"] and not by[b"a"]["fast"]
    # ... and the oracle's candidates really are that short: 0, 1 and 2 bytes
    short = collections.Counter(mn for _, mn, _ in tf.candidate_lengths("lengths"))
    _TABLE.append(("shortest candidate 0 / 1 / 2 bytes (oracle)", "lengths", "-", short[0], short[1] + short[2]))
    assert short[0] >= MIN_SIDE and short[1] >= MIN_SIDE and short[2] >= MIN_SIDE


def test_census_clusters():
    rows = tf.census("clusters") + tf.census("longkeys")
    cl = [r for r in rows if r["clusters"]]
    _sides("FW_UMAXM: matches of a cluster", cl, lambda r: r["max_cluster_matches"], FW_UMAXM, "clusters+longkeys")
    for m in (7, 8, 9):
        assert any(r["max_cluster_matches"] == m for r in cl), m
    _sides("FW_UMAXR: choices of a cluster", cl, lambda r: r["maxR_cluster"], FW_UMAXR, "clusters+longkeys")
    for R in (15, 16, 17):
        assert sum(r["maxR_cluster"] == R for r in cl) >= MIN_SIDE, R
    for r in cl:
        if r["max_cluster_matches"] > FW_UMAXM or r["maxR_cluster"] > FW_UMAXR:
            assert not r["fast"], r["word"]
        elif _plain(r):
            assert r["fast"], r["word"]
    by = {r["word"]: r for r in rows}
    assert by[b"k.cc.k"]["fast"] and by[b"k.dd.k"]["fast"] and not by[b"k.ee.k"]["fast"]
    # UnitCache: the one-walk and the two-walk route of k_keyspace_cplx (route 1 / 2)
    fast = [r for r in tf.census("clusters") if r["fast"] and r["count"] and r["sizes"]]
    _sides("UC_UNITS: units of a FAST word", fast, lambda r: r["units"], UC_UNITS, "clusters")
    _sides("UC_CLUSTERS: clusters of a FAST word", fast, lambda r: r["clusters"], UC_CLUSTERS, "clusters")
    for r in fast:
        if r["units"] > UC_UNITS or r["clusters"] > UC_CLUSTERS:
            assert r["sizes"]["route"] == 2, r["word"]
        elif max(r["cluster_starts"], default=0) < 64:
            assert r["sizes"]["route"] == 1, r["word"]
    # a cluster that starts at byte 62 / 63 / 64 (words past 64 bytes leave pass A)
    st = collections.Counter(s for r in tf.census("clusters") for s in r["cluster_starts"] if s >= 60)
    _TABLE.append(("cluster start <= 62 / >= 63", "clusters", 62, st[60] + st[61] + st[62], st[63] + st[64] + st[65]))
    assert st[62] >= 2 and st[63] >= 2 and st[64] >= 2 and st[63] + st[64] + st[65] >= MIN_SIDE
    # keys longer than 4 bytes (psk_walk, k_keyspace_vsub compare 4 bytes)
    lk = tf.census("longkeys")
    c = tf.corpus("longkeys")
    _sides("key length 4 / 5+ in a word", lk, lambda r: tf.tied_facts(c.table, r["word"])["maxklen"] or None, 4, "longkeys")


def test_census_pieces():
    rows = tf.census("pieces")
    ok = [r for r in rows if _plan(r) and r["units"]]
    _sides("FW_PMAX: small pieces", ok, lambda r: r["sizes"]["np"], FW_PMAX, "pieces")
    for n in (7, 8, 9):
        assert sum(r["sizes"]["np"] == n for r in ok) >= MIN_SIDE, n
    np8 = [r for r in ok if r["sizes"]["np"] <= FW_PMAX]
    _sides("FB_NMAX: big pieces (np <= 8)", np8, lambda r: r["sizes"]["nbig"], FB_NMAX, "pieces")
    for r in ok:
        s = r["sizes"]
        if s["np"] > FW_PMAX or s["nbig"] > FB_NMAX:
            assert not r["fast"], r["word"]
        elif _plain(r) and r["maxv"] <= FW_PLEN:
            assert r["fast"], r["word"]
    # FB_RMAX: five R = 8 pieces join into 3 big pieces (8 * 8 = 64), five R = 9 pieces stay 5
    by = {r["word"]: r for r in rows}
    p8, p9 = by[(b"p" + b"." * 6) * 5], by[(b"q" + b"." * 6) * 5]
    assert p8["fast"] and p8["sizes"]["nbig"] == 3 and p8["P"] == 8 ** 5
    assert not p9["fast"] and p9["sizes"]["nbig"] == 5 and p9["P"] == 9 ** 5
    _sides("word bytes <= 59 / 60-64+", rows, lambda r: r["L"], 59, "pieces")
    # candidates of 990-1010 bytes around FW_MAXL: they exist, and none is FAST (see below)
    longest = {w: mx for w, _, mx in tf.candidate_lengths("pieces", 0, 0, 15)}
    near = [(w, m) for w, m in longest.items() if 985 <= m + 1 <= 1015]
    lo, hi = sum(m + 1 <= FW_MAXL for _, m in near), sum(m + 1 > FW_MAXL for _, m in near)
    _TABLE.append(("FW_MAXL: longest candidate + newline (985-1015)", "pieces", FW_MAXL, lo, hi))
    assert lo >= MIN_SIDE and hi >= MIN_SIDE
    for w, _ in near:
        assert not by[w]["fast"], w


def test_census_tied_and_utf8():
    c = tf.corpus("tied")
    tf_rows = [(w, tf.tied_facts(c.table, w)) for w in c.words + c.narrow]
    rep = [(w, f) for w, f in tf_rows if f["tied"]]
    _sides("VS_OCC: occurrences in a word with a repeated pattern", [f for _, f in rep], lambda f: f["occ"], 16, "tied")
    for n in (15, 16, 17):
        assert sum(f["occ"] == n for _, f in rep) >= 3, n
    _sides("VS_TMAX: tied patterns", [f for _, f in rep], lambda f: f["tied"], 4, "tied")
    _sides("VS_SMAX: sub-words (-s)", [f for _, f in rep], lambda f: f["subwords"], 16, "tied")
    assert any(f["subwords"] == 16 for _, f in rep) and any(f["subwords"] in (17, 18) for _, f in rep)
    _sides("VS_SMAX: sub-words (-s -r)", [f for _, f in rep], lambda f: f["subwords_r"], 16, "tied")
    allf = [f for _, f in tf_rows]
    _sides("positional path: distinct patterns", allf, lambda f: f["patterns"], 16, "tied")
    assert any(f["patterns"] == 16 for f in allf) and any(f["patterns"] == 17 for f in allf)
    _sides("A5X_M_NMAX: patterns / positions", allf, lambda f: f["occ"], 63, "tied")
    assert any(f["patterns"] == 63 for f in allf) and any(f["patterns"] == 64 for f in allf)
    _sides("A5X_M_LMAX: word bytes", [w for w, _ in tf_rows], len, 128, "tied")
    for n in (127, 128, 129):
        assert sum(len(w) == n for w, _ in tf_rows) >= MIN_SIDE, n
    longest = [mx for _, _, mx in tf.candidate_lengths("tied", 2, 0, 3)]
    _TABLE.append(("A5X_M_CBUF: longest -s candidate", "tied", 127, sum(126 <= m <= 127 for m in longest),
                   sum(128 <= m <= 130 for m in longest)))
    assert sum(m == 126 for m in longest) >= 2 and sum(m == 127 for m in longest) >= MIN_SIDE
    assert sum(m == 128 for m in longest) >= MIN_SIDE
    fixed = collections.Counter(f["fixed"] for _, f in rep)
    vhk = collections.Counter(f["value_has_key"] for _, f in tf_rows if f["patterns"])
    _TABLE.append(("fixed-width tied words yes / no", "tied", "-", fixed[True], fixed[False]))
    _TABLE.append(("value contains a key yes / no", "tied", "-", vhk[True], vhk[False]))
    assert min(fixed[True], fixed[False], vhk[True], vhk[False]) >= MIN_SIDE
    # lead_only: words in which a key that starts on a continuation byte matches, and the
    # same words under the table without such keys
    cc = tf.corpus("utf8_cont")
    hit = sum(1 for w in cc.words if any(0x80 <= k[0] <= 0xBF for _, k in tf.matches(cc.table, w)))
    _TABLE.append(("lead_only: words matching a continuation-byte key / not", "utf8_cont", "-", hit, len(cc.words) - hit))
    assert hit >= MIN_SIDE and len(cc.words) - hit >= MIN_SIDE
    assert not any(0x80 <= k[0] <= 0xBF for k in tf.corpus("utf8_lead").table if k)
    assert b"" in tf.corpus("utf8_empty").table


def test_census_unreachable_limits():
    """Limits no word can reach; each with the argument and the largest value seen.

    * ne <= 255 and 1 + np + ne <= FW_RMAX (250): a FAST word has np <= 8 pieces of R <= 16
      entries, so ne <= 128 and the record is <= 137 u64.
    * FW_MAXL (1000): np <= 8 pieces of <= FW_PLEN (7) bytes: a FAST word's longest candidate
      with its newline is <= 56 bytes.  (Candidates around 1000 bytes exist -- pieces corpus --
      but only on the per-word path; there A.maxl against the ring decides.)
    * A.P <= FW_PMAX_CNT (2^24): a FAST word has <= 4 big pieces of R <= 64 with at most
      FB_EMAX = 254 entries in all.  P >= 2^24 needs four pieces whose product is >= 64^4,
      i.e. (AM-GM) whose sum is >= 256 > 254.  The largest FAST P is 64 * 64 * 63 * 63.
    * key index >= 1024 (next_unit, UnitCache, k_keyspace_vsub) and UC_CL: the default
      engine's table takes >= 73 bytes per key (32 key + 8 kmatch + 2 x (8 choice + 8 cval) +
      >= 1 blob) of A5X_TABLE_LDS_MAX = 32768, so it holds < 450 keys; a larger table is
      refused (A5X_E_UNSUPPORTED) and -r / -s / -s -r then run without the FAST probe.
    """
    max_ne = max_rec = max_maxl = max_P = 0
    for name in DEFAULT_CORPORA:
        for r in tf.census(name):
            if r["fast"] and r["count"]:
                max_ne = max(max_ne, r["ne"])
                max_rec = max(max_rec, 1 + r["np"] + r["ne"])
                max_maxl = max(max_maxl, r["sizes"]["maxl"])
                max_P = max(max_P, r["P"])
    hp = tf.HostPlan(tf.corpus("choices"))
    top = hp.classify(b"fcfcjiji", 0, 15)
    assert top[3] & tf.FAST and top[1] + 1 == 64 * 64 * 63 * 63
    max_P = max(max_P, top[1] + 1)
    max_ne = max(max_ne, (top[3] >> 16) & 255)
    max_rec = max(max_rec, 1 + ((top[3] >> 24) & 31) + ((top[3] >> 16) & 255))
    hp.close()
    _TABLE.append(("unreachable: ne <= 255 (bound 128), max seen", "all", 255, max_ne, 0))
    _TABLE.append(("unreachable: record u64 <= FW_RMAX (bound 137), max seen", "all", FW_RMAX, max_rec, 0))
    _TABLE.append(("unreachable: FAST maxl <= FW_MAXL (bound 56), max seen", "all", FW_MAXL, max_maxl, 0))
    _TABLE.append(("unreachable: FAST P = 2^24 (bound 64*64*63*63), max seen", "all", 1 << 24, max_P, 0))
    assert max_ne <= FW_PMAX * FW_UMAXR and max_rec <= 1 + FW_PMAX + FW_PMAX * FW_UMAXR < FW_RMAX
    assert max_maxl <= FW_PMAX * FW_PLEN < FW_MAXL
    assert max_P == 64 * 64 * 63 * 63 < 1 << 24
    # four integers <= 64 with sum <= 254 never reach a product of 2^24
    assert max(a * b * c * d for a in range(60, 65) for b in range(60, 65) for c in range(60, 65)
               for d in range(60, 65) if a + b + c + d <= FB_EMAX) == max_P
    # key index >= 1024: the default engine refuses the 1144-key table
    mk = tf.corpus("manykeys")
    assert len(mk.table) > 1024
    from hashcat_a5_table_generator_amd import _lib
    import ctypes
    import numpy as np
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.a5x_create(-1, ctypes.byref(h)) == 0
    assert L.a5x_load_table_file(h, mk.path.encode()) == 0
    info = np.zeros(4, dtype=np.uint64)
    assert L.a5x_debug_plan_word(h, b"aa", 2, 0, 15, None, 0, info.ctypes.data) == tf.E_UNSUPPORTED
    L.a5x_destroy(h)
    _TABLE.append(("unreachable: key index >= 1024 (default table refused)", "manykeys", 1024, len(mk.table), 0))


# ---------------------------------------------------------------------------
# the pinned huge words (classes on the host; windows on the GPU, test_gpu_table_fuzz.py)
# ---------------------------------------------------------------------------
def test_huge_words_classes():
    c = tf.corpus("choices")
    hp = tf.HostPlan(c)
    for w, P, fast, defer, nbig, bent in tf.HUGE:
        R = [len(c.table[bytes((b,))]) + 1 for b in w]
        assert math.prod(R) == P, w
        rc, cnt, byt, fl, nb, be = hp.classify(w, 0, tf.HUGE_MAX)
        assert rc == 0 and bool(fl & tf.DEFER) == defer and bool(fl & tf.FAST) == fast, (w, fl)
        if not defer:
            assert (cnt, byt) == tf.huge_closed_form(c.table, w), w
        if fast:
            assert (nb, be) == (nbig, bent), w
        else:
            s = hp.sizes(w)
            assert (s["nbig"], s["bent"]) == (nbig, bent), (w, s)
    hp.close()


def test_zz_print_census(capsys):
    """The census table of this run (pytest -s); after the census tests by name order."""
    with capsys.disabled():
        print("\nlimit | corpus | limit value | words at or below | words above")
        for row in _TABLE:
            print(" | ".join(str(x) for x in row))
