"""The build pass of k_keyspace_thread for replayed words (PieceBuilder: the cuts per unit, a
group's entries once per piece) against the C oracle.

Records are checked through what reads them: per-word count and bytes of the keyspace pass
and the order-independent digest of every word's expansion against
c_oracle.CTable.digest_batch (default mode, czech + german), the helpers of
tests/test_gpu_keyspace_unit_sync.py; ordered candidate lists between batches; sorted lists
against the C oracle for -r / -s / -s -r on greek-hebrew.

What this file does not see: apart from the comparison between batches, every check here is
of a multiset (order-independent digests, sorted lists), so the order of a group's entries on
the device -- which candidate gets which rank -- is covered by tests/test_plan_piece_build.py
(the records themselves, entry by entry, against Planner<true> on the CPU; the device runs the
same a5x_plan.h code) and by tests/test_gpu_numbering.py, not here.
"""
import numpy as np
import pytest

import test_gpu_keyspace_unit_sync as us
from conftest import table_path

pytestmark = pytest.mark.gpu

FW_TILE_REC = 256 * 40  # csrc/a5x_plan.h
LARGE = 8192            # KS_WB


@pytest.fixture(scope="module")
def ctab():
    from oracle import c_oracle as co
    return co.CTable([table_path(t) for t in us.TABS])


@pytest.fixture(scope="module")
def ctx():
    from hashcat_a5_table_generator_amd import Context
    c = Context(0)
    c.load_tables([table_path(t) for t in us.TABS])
    yield c
    c.close()


def _piece_words(n, seed):
    """n words of 0..30 bytes: key letters of 2, 3 and 4 choices side by side (groups that
    close on 8 entries), apart by 1..3 bytes (groups that close on 7 bytes), apart by 8..16
    (literal pieces between groups), tails of 0..9 bytes; empty and key-free words."""
    rng = np.random.default_rng(seed)
    plain = np.frombuffer(us.PLAIN, dtype=np.uint8)

    def fill(k):
        return rng.choice(plain, size=k).tobytes()

    ws = []
    for i in range(n):
        style = i % 4
        keys = us.KEYS2 if style == 0 else us.KEYS
        w = b""
        for _ in range(int(rng.integers(0, 7))):
            gap = (0, int(rng.integers(0, 2)), int(rng.integers(1, 4)), int(rng.choice((0, 8, 9, 16))))[style]
            if len(w) + gap + 1 > 30:
                break
            w += fill(gap) + bytes((keys[int(rng.integers(0, len(keys)))],))
        ws.append(w + fill(int(rng.integers(0, 10))))
    for i in range(5, n, 13):
        ws[i] = b""
    for i in range(9, n, 17):
        ws[i] = fill(int(rng.integers(1, 31)))
    return ws


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_batch_sizes(ctx, ctab, n):
    assert us._check(ctx, ctab, _piece_words(n, 0x9B0 + n)) == 0


def _unit_ladder():
    """One tile: words of 0..16 two-choice units (most of them small), with words of 17 and 18
    units (the fused walk) in the first, a middle and the last lane of the word order."""
    rng = np.random.default_rng(0x1AD)
    ws = []
    for i in range(256):
        u = i % 11 if i % 32 else 11 + (i // 32) % 6  # 0..10, and 11..16 eight times
        L = max(u, int(rng.integers(6, 19)))
        ws.append(us._word(rng, L, u, us.KEYS2))
    ws[0] = us.U17
    ws[100] = us.U17 + b"c"
    ws[255] = b"q" + us.U17
    ws[32] = us.U16
    return ws


def test_units_0_to_16_beside_the_fused_walk(ctx, ctab):
    words = _unit_ladder()
    assert {us._nunits(w, us.KEYS2 + b"s") for w in words} >= set(range(0, 19))
    assert us._check(ctx, ctab, words, 0, 40) == 3


def _record_u64(words):
    """1 + np + ne of every word's record (a5x_debug_piece_build on a host-only context)"""
    import ctypes
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.a5x_create(-1, ctypes.byref(h)) == 0
    for t in us.TABS:
        assert L.a5x_load_table_file(h, table_path(t).encode()) == 0
    out = np.zeros(9, dtype=np.uint32)
    sizes = []
    for w in words:
        wb = np.frombuffer(w + b"\0", dtype=np.uint8)
        assert L.a5x_debug_piece_build(h, wb.ctypes.data, len(w), out.ctypes.data) == 0
        sizes.append(1 + int(out[2]) + int(out[4]) if out[0] == 0 and out[8] else 0)
    L.a5x_destroy(h)
    return sizes


def test_tile_record_budget(ctx, ctab):
    """Records of 41 u64 a word: the tile's budget runs out and its last FAST words are not
    built (the slow path expands them), between words that are."""
    u8 = b"uuuuuuuu"  # 8 groups of 4 entries
    words = [u8] * 120 + [b"tet"] + [u8] * 65 + [b"denu", b"e"] + [u8] * 65 + [b"cdn", u8, b"uc"] + _piece_words(40, 0xB0D)
    sizes = _record_u64(words)
    assert sum(sizes[:256]) > FW_TILE_REC and sizes[255] > 0 and sum(sizes[256:]) < FW_TILE_REC
    assert us._check(ctx, ctab, words) == 0


@pytest.mark.parametrize("batch", ["pieces", "ladder"])
def test_both_stages(ctx, batch):
    """The same batch with the small word stage and with the large one forced: equal prefix
    arrays and equal expansion digests."""
    import test_gpu_keyspace_stage as ks
    # (cut to fit the small stage; the ladder keeps its words of 16, 17 and 18 units whole, so both
    # stages see the fused walk beside replayed words in one wave)
    if batch == "pieces":
        words = [w[:9] for w in _piece_words(600, 0x57A)]
    else:
        words = [w if us._nunits(w, us.KEYS2 + b"s") >= 16 else w[:10] for w in _unit_ladder()]
        assert sum(us._nunits(w, us.KEYS2 + b"s") > 16 for w in words) == 3
    S = ctx.keyspace_small_stage()
    c0, b0, d0, stage0, refit0 = ks._run(ctx, words, 0, 40)
    ctx.keyspace_large_stage(True)
    try:
        c1, b1, d1, stage1, refit1 = ks._run(ctx, words, 0, 40)
    finally:
        ctx.keyspace_large_stage(False)
    assert stage0 == S and stage1 == LARGE
    assert refit0 == refit1 == (3 if batch == "ladder" else 0)
    assert np.array_equal(c0, c1) and np.array_equal(b0, b1) and np.array_equal(d0, d1)
    assert int(c0[-1]) > len(words)


def test_word_alone_and_in_a_large_batch(ctx):
    """Any word gives the same ordered candidates in a 1,000-word batch and in a 16-word one."""
    words = _piece_words(1000, 0xA10)
    big = ctx.expand_words(words, 0, 0, 15)
    for i in list(range(0, 1000, 16 * 7)) + [1000 - 16]:
        small = ctx.expand_words(words[i:i + 16], 0, 0, 15)
        for w, b, s in zip(words[i:i + 16], big[i:i + 16], small):
            assert b == s, (i, w, "candidate order differs between batches")
    assert sum(len(b) for b in big) > 10000


def _greek_words():
    rng = np.random.default_rng(0x9E)
    alpha = list(us.GREEK) + list("xq7-")
    ws = ["".join(rng.choice(alpha, size=int(rng.integers(0, 10)))).encode() for _ in range(1990)]
    ws += ["αβγδεζηθικλμνξο".encode(), b"", b"xq", "αxβ".encode(), "α".encode(), ("x" * 9 + "β" + "q" * 9 + "γ").encode()]
    ws += ["".join(rng.choice(list(us.GREEK), size=3)).encode() + b"-" * g + "δ".encode() for g in (0, 1, 5, 8)]
    return ws


@pytest.mark.parametrize("mn", [0, 1])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_greek_modes(mode, mn):
    """-r / -s / -s -r: the probe's records come from the same build pass (mode_unit's units)."""
    from hashcat_a5_table_generator_amd import Context
    from oracle import c_oracle as co
    words = _greek_words()
    tab = [table_path("greek-hebrew")]
    key = ("greek-pieces", mode, mn)
    if key not in us.WANT:
        t = co.CTable(tab)
        uniq = sorted(set(words))
        out, wb = t.expand_batch(*co.pack_words(uniq), mode, mn, 15)
        res, pos = {}, 0
        for w, b in zip(uniq, wb):
            seg = out[pos:pos + int(b)]
            pos += int(b)
            res[w] = sorted(seg.split(b"\n")[:-1]) if seg else []
        us.WANT[key] = res
    with Context(0) as c:
        c.load_tables(tab)
        got = c.expand_words(words, mode, mn, 15)
    for w, g in zip(words, got):
        assert sorted(g) == us.WANT[key][w], (mode, mn, w, len(g), len(us.WANT[key][w]))
    assert sum(len(g) for g in got) > len(words)
