"""k_keyspace_thread's count pass by unit index (psk_detect + psk_units) against the oracles.

The count pass finds every word's lone matches position by position, logs them (at most
KS_ULOG = 16 per word, match byte < 64, key index < 1024) and then runs the unit block
(lone_unit, mode_unit, count_unit, the planner) once per unit index.  A word the log does
not hold takes the fused position-synchronous walk instead, in the count pass and again in
the build pass; Context.keyspace_refit() counts those words, so that a test can tell the
two paths apart.

Default mode, czech + german: per-word count and bytes from a5x_keyspace_device (its
candidate / byte prefix arrays) and the order-independent digest {count, bytes, sum h,
sum h^2} of every word's expansion, against c_oracle.CTable.digest_batch.  The C oracle
runs once per distinct word of the module (WANT).  -r / -s / -s -r, greek-hebrew: sorted
candidate lists against the C oracle's, as tests/test_gpu_modes.py.

A word of more than 64 bytes never reaches the walk (k_keyspace_thread leaves it to the
wave kernel whatever it holds), and a word of at most 64 bytes has no match at byte >= 64:
the log's "q < 64" condition cannot fail, so a 100-byte word with a match past byte 64
counts as 0 refits here, and the only way into the fused walk with these tables is more
than 16 lone matches.
"""
import numpy as np
import pytest

from conftest import table_path

pytestmark = pytest.mark.gpu

TABS = ["czech", "german"]
KEYS2 = b"cdnrtz"          # one value each (R = 2); 's' too, but "ss" is a key of its own
KEYS = b"aeiouycdnrtz"     # (R = 3: a e o y i.., R = 4: u)
PLAIN = b"bfghjklmpqvwx"   # no key starts with these
WANT = {}                  # (word, mn, mx) -> the C oracle's digest row


@pytest.fixture(scope="module")
def ctab():
    from oracle import c_oracle as co
    return co.CTable([table_path(t) for t in TABS])


@pytest.fixture(scope="module")
def ctx():
    from hashcat_a5_table_generator_amd import Context
    c = Context(0)
    c.load_tables([table_path(t) for t in TABS])
    yield c
    c.close()


def _want(ctab, words, mn, mx):
    from oracle import c_oracle as co
    new = sorted({w for w in words if (w, mn, mx) not in WANT})
    if new:
        rows = ctab.digest_batch(*co.pack_words(new), 0, mn, mx)
        for w, r in zip(new, rows):
            WANT[(w, mn, mx)] = np.array(r, dtype=np.uint64)
    return np.stack([WANT[(w, mn, mx)] for w in words])


def _gpu(ctx, words, mn, mx):
    """(per-word count, bytes), digest rows of the expansion, refit count of the keyspace pass"""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    data, offs = pack_words(words)
    n = len(words)
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    coff, boff = DeviceBuffer(ctx, (n + 1) * 8), DeviceBuffer(ctx, (n + 1) * 8)
    tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, n, 0, mn, mx, d_cand_off=coff.ptr, d_byte_off=boff.ptr)
    refit = ctx.keyspace_refit()
    c, b = coff.to_array(np.uint64), boff.to_array(np.uint64)
    assert int(c[n]) == tc and int(b[n]) == tb
    out = DeviceBuffer(ctx, max(tb, 16))
    st = ctx.expand_device(dw.ptr, do.ptr, n, out.ptr, tb, 0, mn, mx, d_byte_off=boff.ptr)
    assert st["candidates"] == tc and st["bytes"] == tb
    dig = DeviceBuffer(ctx, n * 32)
    ctx.digest_device(out.ptr, boff.ptr, 0, n, dig.ptr)
    return np.diff(c), np.diff(b), dig.to_array(np.uint64).reshape(n, 4), refit


def _check(ctx, ctab, words, mn=0, mx=15):
    want = _want(ctab, words, mn, mx)
    cnt, byt, got, refit = _gpu(ctx, words, mn, mx)
    bad = np.nonzero((cnt != want[:, 0]) | (byt != want[:, 1]))[0]
    assert len(bad) == 0, [(i, words[i], int(cnt[i]), int(byt[i]), want[i][:2]) for i in bad[:5]]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(i, words[i], got[i], want[i]) for i in bad[:5]]
    return refit


def _word(rng, L, nkeys, keys=KEYS):
    """L bytes, nkeys of them key letters (no 's': "ss" is a key of its own)"""
    if L == 0:
        return b""
    w = rng.choice(np.frombuffer(PLAIN, dtype=np.uint8), size=L)
    at = rng.choice(L, size=min(nkeys, L), replace=False)
    w[at] = rng.choice(np.frombuffer(keys, dtype=np.uint8), size=len(at))
    return w.tobytes()


def _mixed_words(n, seed):
    """lengths 0..40, 0..8 key letters each; empty words, key-free words, an "ss" word mid-batch"""
    rng = np.random.default_rng(seed)
    ws = [_word(rng, int(rng.integers(0, 41)), int(rng.integers(0, 9))) for _ in range(n)]
    for i in range(0, n, 7):
        ws[i] = _word(rng, int(rng.integers(1, 41)), 0)
    for i in range(3, n, 11):
        ws[i] = b""
    ws[n // 2] = b"strasse" if n > 1 else ws[0]
    if n > 130:
        ws[130] = b"ss"
    return ws


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_batch_sizes(ctx, ctab, n):
    assert _check(ctx, ctab, _mixed_words(n, 0x5C0 + n)) == 0


def _unit_words():
    """256 words of 6..12 bytes with 0..10 two-choice units"""
    rng = np.random.default_rng(0x71E)
    return [_word(rng, L, int(rng.integers(0, min(L, 10) + 1)), KEYS2) for L in rng.integers(6, 13, size=256)]


def _nunits(w, keys=KEYS2):
    return sum(1 for b in w if b in keys)


LONG100 = b"q" * 70 + b"tet" + b"q" * 27  # 100 bytes, matches at bytes 70..72


def _orderings():
    ws = _unit_words()
    asc = sorted(ws, key=_nunits)
    mixed = list(ws)
    mixed[97] = LONG100
    return {"ascending": asc, "descending": asc[::-1], "equal": [b"dentritz"] * 256, "long_word": mixed}


@pytest.mark.parametrize("order", ["ascending", "descending", "equal", "long_word"])
def test_tile_orderings(ctx, ctab, order):
    """One 256-word tile: every word's ordered candidate list is its list in a 16-word batch
    (tests/test_gpu_numbering.py), and its multiset the C oracle's."""
    words = _orderings()[order]
    assert len(words) == 256
    big = ctx.expand_words(words, 0, 0, 15)
    small = []
    for i in range(0, 256, 16):
        small += ctx.expand_words(words[i:i + 16], 0, 0, 15)
    assert _check(ctx, ctab, words) == 0  # (LONG100 is the wave kernel's: no refit)
    for i, (w, b, s) in enumerate(zip(words, big, small)):
        assert b == s, (order, i, w, "candidate order differs between batches")
        assert len(b) == int(WANT[(w, 0, 15)][0]), (order, i, w)


U16 = b"cdnrtzscdnrtzcdn"    # 16 lone units of 2 choices: 65,536 combinations
U17 = b"cdnrtzscdnrtzcdnr"   # 17: one more than the unit log holds, 131,072


@pytest.mark.parametrize("lane", [0, 63, 255])
@pytest.mark.parametrize("word", [U16, U17])
def test_log_boundary(ctx, ctab, word, lane):
    words = _unit_words()
    words[lane] = word
    want = _want(ctab, [word], 0, 40)[0]
    assert int(want[0]) == (1 << len(word)) - 1
    assert _check(ctx, ctab, words, 0, 40) == (1 if word == U17 else 0)


def test_refit_count(ctx, ctab):
    """0 for C3-shaped words; else exactly the words with more than 16 lone matches."""
    from hashcat_a5_table_generator_amd import synth
    _, (data, offs) = synth.global_words("c3", 0, 256)
    c3 = [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(256)]
    assert _check(ctx, ctab, c3) == 0
    words = _unit_words() + _unit_words()[:100]
    over = {5: U17, 64: U17 + b"q", 200: b"x" + U17, 255: U17, 256: U17, 300: U17[::-1]}
    for i, w in over.items():
        words[i] = w
    words[7] = U16
    words[63] = LONG100
    # mx = 15: the 16- and 17-match words are outside the window (the DP kernel counts them),
    # but the walk meets their matches all the same
    assert _check(ctx, ctab, words, 0, 15) == len(over)
    assert _check(ctx, ctab, words[:5] + words[6:64], 0, 15) == 0


GREEK = "ςερτυθιοπασδφγηξκλζχψωβνμ"


def _greek_words():
    rng = np.random.default_rng(0x6E)
    alpha = list(GREEK) + list("xq7-")
    ws = []
    for _ in range(560):
        ws.append("".join(rng.choice(alpha, size=int(rng.integers(0, 10)))).encode())
    for _ in range(40):  # repeated letters: tied occurrences (-s / -s -r virtual words, the vocc rows)
        a, b = rng.choice(list(GREEK), size=2, replace=False)
        ws.append((a + "x" + b + a + "q" * int(rng.integers(0, 3)) + b + a).encode())
    ws += ["αβγδεζηθικλμνξο".encode(), b"", b"xq"]
    return ws


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("order", ["shuffled", "sorted"])
def test_greek_modes(mode, order):
    """-r / -s / -s -r (the same kernel is their FAST probe: mode_unit, the occurrence rows,
    rnseg), words shuffled and sorted by unit count."""
    from hashcat_a5_table_generator_amd import Context
    from oracle import c_oracle as co
    # 17 occurrences of one pattern: one tied digit for -s / -s -r (2 candidates), more than
    # the unit log holds; for -r they would be 2^17 candidates, so not there
    words = _greek_words() + ([("α" * 17).encode()] if mode != 1 else [])
    if order == "sorted":
        words = sorted(words, key=lambda w: sum(1 for ch in w.decode() if ch in GREEK))
    tab = [table_path("greek-hebrew")]
    key = ("greek", mode)
    if key not in WANT:
        t = co.CTable(tab)
        uniq = sorted(set(words))
        out, wb = t.expand_batch(*co.pack_words(uniq), mode, 0, 15)
        res, pos = {}, 0
        for w, b in zip(uniq, wb):
            seg = out[pos:pos + int(b)]
            pos += int(b)
            res[w] = sorted(seg.split(b"\n")[:-1]) if seg else []
        WANT[key] = res
    with Context(0) as c:
        c.load_tables(tab)
        got = c.expand_words(words, mode, 0, 15)
        refit = c.keyspace_refit()
    for w, g in zip(words, got):
        assert sorted(g) == WANT[key][w], (mode, order, w, len(g), len(WANT[key][w]))
    assert refit == (0 if mode == 1 else 1)
