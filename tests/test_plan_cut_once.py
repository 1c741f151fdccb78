"""The cut-once path of k_keyspace_thread (csrc/a5x_plan.h: CutPlanner in the count pass, the
record from its group descriptors by PieceBuilder::place_cuts / build_group / place_tail)
against the planners it replaces, on the CPU.

a5x_debug_cut_once plans one word of lone matches three ways: CountPlanner<8> (the count pass
so far), Planner<true, ., ., 8> (the reference record) and the new path, which cuts the word
once, in the count pass, and builds the record without looking at a unit again.  Every
count-pass field (ok, np, ng, ne, maxl, minl, nbig, big entries, refused units) must be the
same number, and the two records the same u64 by u64.  Codes as a5x_debug_piece_build: 0
equal, 1 different, 2 not applicable (overlapping matches, or a unit that an 8-entry group
refuses), 3 not FAST with more than 8 group pieces (never built; the count-pass fields are
compared all the same).
"""
import numpy as np
import pytest

from conftest import table_path

EQUAL, DIFFERENT, NA, NOTFAST = 0, 1, 2, 3
COUNT = ("ok", "np", "ng", "ne", "maxl", "minl", "nbig", "bent", "refused")
RUNS = (0, 6, 7, 8, 13, 14, 15)  # FW_PLEN = 7: two full literal pieces fill a big piece

CG = ["czech", "german"]   # R = 2: c d n r t z i y, R = 3: a e o, R = 4: u; every value 2 bytes; s / ss overlap
GH = ["greek-hebrew"]      # 2-byte letters, R = 2, 2-byte values
PLAIN = b"bfghjklmpqvwx"   # no key of czech + german starts with these
GREEK = "ερτυθιοπαδφγηξκλζχψωβνμ"


def _ctx(tables=None, text=None):
    from hashcat_a5_table_generator_amd import Context
    c = Context(-1)
    if tables:
        c.load_tables([table_path(t) for t in tables])
    else:
        c.parse_table(text)
    return c


def _check(c, w: bytes) -> dict:
    """One word through the hook: never "different", the count-pass fields of the new planner
    equal to CountPlanner's, the records equal u64 by u64."""
    out, rn, rr = c.cut_once(w)
    r = dict(code=int(out[0]), units=int(out[1]), np=int(out[2]), ng=int(out[3]), ne=int(out[4]), members=int(out[5]),
             tails=int(out[6]), literals=int(out[7]), fast=int(out[8]), rec=int(out[9]), ref_ng=int(out[28]))
    new, old = dict(zip(COUNT, map(int, out[10:19]))), dict(zip(COUNT, map(int, out[19:28])))
    r["count"] = old
    assert r["code"] != DIFFERENT, (w, r, new, old)
    if r["code"] == NA and r["units"] and not (new["ok"] or old["ok"] or new["refused"]):
        return r  # overlapping matches: no planner ran
    assert new["ok"] == old["ok"] and new["refused"] == old["refused"], (w, new, old)
    if old["ok"]:
        assert new == old, (w, new, old)
    if r["code"] == EQUAL:
        n = r["rec"]
        assert n == 1 + old["np"] + old["ne"] and (r["np"], r["ng"], r["ne"]) == (old["np"], old["ng"], old["ne"]), (w, r)
        bad = np.nonzero(rn != rr)[0]
        assert len(bad) == 0, (w, int(bad[0]), hex(int(rn[bad[0]])), hex(int(rr[bad[0]])))
        assert rn[0] != 0 and not rn[n:].any(), (w, n)
    return r


@pytest.fixture(scope="module")
def cg():
    c = _ctx(CG)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gh():
    c = _ctx(GH)
    yield c
    c.close()


def _fill(rng, n, plain=PLAIN):
    return bytes(rng.choice(np.frombuffer(plain, dtype=np.uint8), size=n)) if n else b""


def _random_words(rng, n, letters, plain):
    """0..64 bytes: most of them short enough for the 8 pieces of a FAST word, 1..6 key letters
    (some none), the rest filler"""
    ws = []
    for _ in range(n):
        L = int(rng.integers(0, 65)) if rng.random() < 0.25 else int(rng.integers(0, 26))
        k = int(rng.integers(1, 7)) if rng.random() < 0.95 else 0
        parts = [letters[int(rng.integers(0, len(letters)))] for _ in range(k)]
        room = L - sum(len(p) for p in parts)
        while room < 0 and parts:
            room += len(parts.pop())
        cuts = sorted(int(x) for x in rng.integers(0, room + 1, size=len(parts))) if room >= 0 else []
        w, at = b"", 0
        for p, cpos in zip(parts, cuts):
            w += _fill(rng, cpos - at, plain) + p
            at = cpos
        ws.append(w + _fill(rng, max(room, 0) - at, plain))
        assert len(ws[-1]) <= 64
    return ws


@pytest.mark.parametrize("which", ["czech-german", "greek-hebrew"])
def test_random_words(which, cg, gh):
    rng = np.random.default_rng(0xC07 if which == "czech-german" else 0xC08)
    if which == "czech-german":
        c, letters, plain = cg, [bytes((b,)) for b in b"cdnrtziyaeouCDNAEU"], PLAIN
    else:
        c, letters, plain = gh, [ch.encode() for ch in GREEK] + [b"'", b",", b"."], b"xq7-"
    words = _random_words(rng, 4000, letters, plain)
    grouped = lens = slow = 0
    codes = [0, 0, 0, 0]
    for w in words:
        r = _check(c, w)
        codes[r["code"]] += 1
        grouped += bool(r["fast"] and r["ref_ng"] >= 1 and r["code"] == EQUAL)  # FAST by the reference planners alone
        slow += bool(not r["fast"] and r["code"] == EQUAL)                      # not FAST, compared all the same
        lens += len(w) > 40
    assert grouped * 2 >= len(words), (grouped, codes)
    assert codes[EQUAL] == len(words) and slow > 100 and lens > 200, (codes, slow, lens)


def test_literal_runs_everywhere(cg, gh):
    """Runs of 0, 6, 7, 8, 13, 14, 15 bytes before the first unit, between two units and in the
    tail, every combination; the tail joins the last group or not."""
    rng = np.random.default_rng(0x11E)
    for c, k1, k2, plain in ((cg, b"c", b"u", PLAIN), (gh, "α".encode(), "β".encode(), b"xq7-")):
        joined = apart = three = 0
        for a in RUNS:
            for b in RUNS:
                for t in RUNS:
                    w = _fill(rng, a, plain) + k1 + _fill(rng, b, plain) + k2 + _fill(rng, t, plain)
                    r = _check(c, w)
                    assert r["code"] == EQUAL and r["units"] == 2, (w, r)
                    # the pieces, by hand: full literal pieces of the lead, then a group that takes
                    # up to 7 - 2 bytes before a 2-byte choice; b = 0: one group of two units
                    assert r["ng"] == (1 if b <= 3 else 2), (w, r)
                    # (c d / alpha beta: 2-byte choices) the last group is 2..5 bytes, so only an empty tail's '\n' joins it
                    assert r["tails"] == (1 if t == 0 else 0), (w, r)
                    joined += r["tails"]
                    apart += r["tails"] == 0
                    three += r["literals"] >= 3
        assert joined >= 7 and apart >= 100 and three >= 100, (joined, apart, three)
    # a single unit, and one literal run only
    for c, k1, plain in ((cg, b"a", PLAIN), (gh, "ω".encode(), b"xq7-")):
        for a in RUNS:
            for t in RUNS:
                r = _check(c, _fill(rng, a, plain) + k1 + _fill(rng, t, plain))
                assert r["code"] == EQUAL and r["ng"] == 1, r
                lead = a % 7 if a % 7 + 2 <= 7 else 0
                assert r["tails"] == (1 if lead + 2 + t + 1 <= 7 else 0), (a, t, r)


def test_groups_closing_on_entries_and_on_bytes(cg):
    """czech + german: c d n R = 2, a e o R = 3, u R = 4, every longest choice 2 bytes."""
    want = {
        b"cdn": dict(ng=1, members=3, ne=8, tails=1, np=1),            # 2 * 2 * 2 = 8, 6 bytes + '\n'
        b"cdnr": dict(ng=2, members=3, ne=10, tails=1, np=2),          # a fourth R = 2 unit: 16 > 8 closes three members
        b"ucd": dict(ng=2, members=2, ne=10, tails=1, np=2),           # 4 * 2 = 8 closes two members
        b"uua": dict(ng=3, members=1, ne=11, tails=1, np=3),           # 4 * 4 = 16, 4 * 3 = 12: groups of one member
        b"uac": dict(ng=2, members=2, ne=10, tails=1, np=2),           # u | a c
        b"cxxdxxn": dict(ng=2, members=2, ne=6, tails=1, np=2),        # 2 + 2 + 2 = 6, + 2 + 2 > 7: closes on bytes
        b"cxxxxxd": dict(ng=2, members=1, ne=5, tails=0, np=3),        # 2 + 5 + 2 > 7; xxxxxd is 7 bytes: '\n' a piece
        b"cxxxd": dict(ng=1, members=2, ne=5, tails=0, np=2),          # 2 + 3 + 2 = 7: '\n' is a literal piece
        b"cxxd": dict(ng=1, members=2, ne=4, tails=1, np=1),           # 6 bytes + '\n'
        b"cdnxxxxxxx": dict(ng=1, members=3, ne=10, tails=0, np=3),    # tail of 7 + '\n': two literal pieces
    }
    for w, exp in want.items():
        r = _check(cg, w)
        assert r["code"] == EQUAL and r["fast"], (w, r)
        assert {k: r[k] for k in exp} == exp, (w, r, exp)


def test_eight_groups_and_nine(cg):
    g = b"xxxxxc"  # a group of 5 + 2 = 7 bytes: nothing joins it
    r = _check(cg, g * 7 + b"xxxxc")
    assert r["code"] == EQUAL and r["fast"] and (r["ng"], r["np"], r["count"]["nbig"]) == (8, 8, 4), r
    r = _check(cg, g * 8 + b"xxxxc")
    assert r["code"] == NOTFAST and not r["fast"] and (r["count"]["ng"], r["count"]["nbig"]) == (9, 5), r
    r = _check(cg, b"uuuuuuuu")  # 8 groups of one R = 4 member
    assert r["code"] == EQUAL and r["fast"] and (r["ng"], r["ne"], r["members"]) == (8, 32, 1), r
    r = _check(cg, b"uuuuuuuuu")
    assert r["code"] == NOTFAST and r["count"]["ng"] == 9, r


def test_four_big_pieces_and_a_fifth(cg):
    """A big piece takes two 7-byte pieces (15 bytes) or 64 combinations; a FAST word has four."""
    g = b"xxxxxc"
    r = _check(cg, g * 7 + b"xxxxc")
    assert r["fast"] and r["count"]["nbig"] == 4 and r["count"]["bent"] == 16, r
    r = _check(cg, b"cdn" * 7 + b"cd")  # groups of 8 entries: two fill a big piece of 64
    assert r["code"] == EQUAL and r["fast"] and r["count"]["nbig"] == 4 and r["count"]["bent"] == 3 * 64 + 32, r
    r = _check(cg, b"cdn" * 8)          # 4 * 64 big entries are more than a window holds
    assert r["code"] == EQUAL and not r["fast"] and r["count"]["nbig"] == 4 and r["count"]["bent"] == 256, r
    # 8 groups behind one full literal piece: 9 pieces, a fifth big piece -- not FAST, compared all the same
    r = _check(cg, b"x" * 7 + g * 7 + b"xxxxc")
    assert r["code"] == EQUAL and not r["fast"] and (r["ng"], r["np"], r["count"]["nbig"]) == (8, 9, 5), r
    r = _check(cg, b"x" * 21 + g * 6 + b"xxxxc")  # lit_full: three full literal pieces open two big pieces
    assert r["code"] == EQUAL and not r["fast"] and (r["np"], r["count"]["nbig"]) == (10, 5), r
    r = _check(cg, b"x" * 14 + b"cdn" * 4 + b"x" * 15)  # literal big pieces around group ones
    assert r["code"] == EQUAL and r["count"]["nbig"] == 5 and not r["fast"], r
    r = _check(cg, b"x" * 14 + b"cdn" * 4 + b"x" * 6)
    assert r["code"] == EQUAL and r["count"]["nbig"] == 4 and r["fast"], r


def test_refused_units():
    """No unit of czech + german or greek-hebrew is refused (R <= 4, 2-byte values): a table of
    its own with R = 8, R = 9, a 7-byte and an 8-byte value."""
    text = (b"".join(b"a=%d\n" % i for i in range(7)) + b"".join(b"b=%d\n" % i for i in range(8)) +
            b"c=1234567\nd=12345678\ne=E\n")
    c = _ctx(text=text)
    r = _check(c, b"a")
    assert r["code"] == EQUAL and (r["ng"], r["ne"], r["members"]) == (1, 8, 1), r   # one member closes on 8 entries
    r = _check(c, b"ae")
    assert r["code"] == EQUAL and (r["ng"], r["ne"]) == (2, 10), r
    r = _check(c, b"xcx")
    assert r["code"] == EQUAL and r["ng"] == 1 and r["count"]["refused"] == 0, r      # 7 bytes: a group of its own
    for w, n in ((b"b", 1), (b"xbx", 1), (b"ebe", 1), (b"bb", 2), (b"d", 1), (b"eexdx", 1), (b"dxb", 2), (b"a" * 3 + b"d", 1)):
        r = _check(c, w)
        assert r["code"] == NA and r["count"]["ok"] == 0 and r["count"]["refused"] == n, (w, r)
    c.close()


def test_empty_and_key_free_words(cg, gh):
    for c in (cg, gh):
        for w in (b"", b"x", b"xq", b"x" * 6, b"x" * 7, b"x" * 14, b"x" * 15, b"x" * 64):
            r = _check(c, w)
            assert r["code"] == EQUAL and r["units"] == 0 and r["ng"] == 0 and r["fast"], (w, r)
            assert r["np"] == (len(w) + 1 + 6) // 7 == r["literals"] and r["ne"] == r["np"], (w, r)


def test_overlapping_matches_are_not_this_path(cg):
    for w in (b"ss", b"strasse", b"xssx"):
        assert _check(cg, w)["code"] == NA
