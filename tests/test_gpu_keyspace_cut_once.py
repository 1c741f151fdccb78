"""k_keyspace_thread with every FAST word cut once: the count pass keeps one descriptor per
group (CutPlanner), the build pass writes the record from the descriptors alone -- literal
pieces from the gaps between groups, then the group's entries (PieceBuilder::place_cuts /
build_group / place_tail) -- against the C oracle.

Records are checked through what reads them, with the helpers of
tests/test_gpu_keyspace_unit_sync.py: per-word count and bytes of the keyspace pass and the
order-independent digest of every word's expansion against c_oracle.CTable.digest_batch
(default mode, czech + german); ordered candidate lists between batches; sorted lists against
the C oracle for -r / -s / -s -r on greek-hebrew.  The records themselves, u64 by u64, are
compared on the CPU (tests/test_plan_cut_once.py: the device runs the same a5x_plan.h code).
"""
import numpy as np
import pytest

import test_gpu_keyspace_unit_sync as us
from conftest import table_path

pytestmark = pytest.mark.gpu

FW_TILE_REC = 256 * 40  # csrc/a5x_plan.h
LARGE = 8192            # KS_WB
RUNS = (0, 6, 7, 8, 13, 14, 15)


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


def _fill(rng, k):
    return rng.choice(np.frombuffer(us.PLAIN, dtype=np.uint8), size=k).tobytes() if k else b""


def _cut_words(n, seed):
    """n words of 0..36 bytes: units side by side (groups that close on 8 entries), apart by
    1..3 bytes (groups that close on 7 bytes), apart by 6..15 (literal pieces between groups),
    leads and tails of 0..15 bytes; empty and key-free words."""
    rng = np.random.default_rng(seed)
    ws = []
    for i in range(n):
        style = i % 4
        keys = us.KEYS2 if style == 0 else us.KEYS
        w = _fill(rng, int(rng.choice((0, 0, 1, 6, 7, 8, 14))) if style == 3 else 0)
        for _ in range(int(rng.integers(0, 7))):
            gap = (0, int(rng.integers(0, 2)), int(rng.integers(1, 4)), int(rng.choice((0, 6, 7, 8, 13, 15))))[style]
            if len(w) + gap + 1 > 36:
                break
            w += _fill(rng, gap) + bytes((keys[int(rng.integers(0, len(keys)))],))
        ws.append(w + _fill(rng, int(rng.choice((0, 1, 3, 5, 6, 7, 8, 13, 14, 15)))))
    for i in range(5, n, 13):
        ws[i] = b""
    for i in range(9, n, 17):
        ws[i] = _fill(rng, int(rng.integers(1, 31)))
    return ws


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_batch_sizes(ctx, ctab, n):
    assert us._check(ctx, ctab, _cut_words(n, 0xC70 + n)) == 0


def _unit_ladder():
    """One tile: words of 0..16 units, with words of 17 and 18 units (the fused walk, whose
    count pass runs the same planner) in the first, a middle and the last lane."""
    rng = np.random.default_rng(0xC1D)
    ws = []
    for i in range(256):
        u = i % 11 if i % 32 else 11 + (i // 32) % 6  # 0..10, and 11..16 eight times
        L = max(u, int(rng.integers(6, 19)))
        ws.append(us._word(rng, L, u, us.KEYS2))
    ws[0] = us.U17 + b"c"
    ws[131] = us.U17
    ws[255] = b"q" + us.U17
    ws[33] = us.U16
    return ws


def test_units_0_to_16_beside_the_fused_walk(ctx, ctab):
    words = _unit_ladder()
    assert {us._nunits(w, us.KEYS2 + b"s") for w in words} >= set(range(0, 19))
    assert us._check(ctx, ctab, words, 0, 40) == 3


def _record_u64(words):
    """1 + np + ne of every FAST word's record (a5x_debug_cut_once on a host-only context)"""
    from hashcat_a5_table_generator_amd import Context
    sizes = []
    with Context(-1) as h:
        h.load_tables([table_path(t) for t in us.TABS])
        for w in words:
            out, _, _ = h.cut_once(w)
            sizes.append(int(out[9]) if out[0] == 0 and out[8] else 0)
    return sizes


def test_tile_record_budget(ctx, ctab):
    """Records of 41 u64 a word: the tile's budget runs out and its last FAST words are not
    built (the slow path expands them), between words that are."""
    u8 = b"uuuuuuuu"  # 8 groups of 4 entries
    words = ([u8] * 97 + [b"tet", b"xxxxxxxe"] + [u8] * 87 + [b"denu", b"e"] + [u8] * 64 + [b"cdn", u8, b"uc", b"bbbbbbbbbbbbbbc"] +
             _cut_words(40, 0xB0E))
    sizes = _record_u64(words)
    assert sizes[0] == 41 and sum(sizes[:256]) > FW_TILE_REC and sizes[255] > 0 and sum(sizes[256:]) < FW_TILE_REC
    # the first word past the budget: built words before it, FAST words from it on
    over = int(np.searchsorted(np.cumsum(sizes[:256]), FW_TILE_REC, side="right"))
    assert 200 < over < 255 and min(sizes[over:256]) > 0
    assert us._check(ctx, ctab, words) == 0


def _literal_words():
    """Literal runs of 0, 6, 7, 8, 13, 14, 15 bytes before the first unit, between units and in
    the tail (every combination around two units, and around one), tails that join the last
    group and tails that do not."""
    rng = np.random.default_rng(0x717)
    ws = []
    for a in RUNS:
        for b in RUNS:
            for t in RUNS:
                ws.append(_fill(rng, a) + b"c" + _fill(rng, b) + b"u" + _fill(rng, t))
    for a in RUNS:
        for t in RUNS + (1, 2, 3, 4, 5):
            ws.append(_fill(rng, a) + b"a" + _fill(rng, t))
    return ws


def test_literal_runs_and_tails_in_one_batch(ctx, ctab):
    words = _literal_words()
    assert len(words) == 343 + 84 and max(len(w) for w in words) == 47
    assert us._check(ctx, ctab, words) == 0


@pytest.mark.parametrize("batch", ["cuts", "ladder"])
def test_both_stages(ctx, batch):
    """The same batch with the small word stage and with the large one forced: equal prefix
    arrays and equal expansion digests."""
    import test_gpu_keyspace_stage as ks
    if batch == "cuts":
        words = [w[:9] for w in _cut_words(600, 0x57B)]
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
    words = (_literal_words() + _cut_words(1000, 0xA11))[:1000]
    big = ctx.expand_words(words, 0, 0, 15)
    for i in list(range(0, 1000, 16 * 7)) + [1000 - 16]:
        small = ctx.expand_words(words[i:i + 16], 0, 0, 15)
        for w, b, s in zip(words[i:i + 16], big[i:i + 16], small):
            assert b == s, (i, w, "candidate order differs between batches")
    assert sum(len(b) for b in big) > 10000


def _greek_words():
    rng = np.random.default_rng(0xC9E)
    alpha = list(us.GREEK) + list("xq7-")
    ws = ["".join(rng.choice(alpha, size=int(rng.integers(0, 10)))).encode() for _ in range(1500)]
    ws += ["αβγδεζηθικλμνξο".encode(), b"", b"xq", "αxβ".encode(), "α".encode(), ("x" * 9 + "β" + "q" * 9 + "γ").encode()]
    g = list(us.GREEK)
    for a in RUNS:  # the literal runs around two letters and in the tail
        for t in (0, 6, 7, 15):
            ws.append(("x" * a + g[a % 7] + "q" * t + g[7 + t % 5] + "-" * ((a + t) % 16)).encode())
    ws += ["".join(rng.choice(g, size=3)).encode() + b"-" * k + "δ".encode() for k in (0, 1, 5, 8)]
    return ws


@pytest.mark.parametrize("mn", [0, 1])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_greek_modes(mode, mn):
    """-r / -s / -s -r: the probe's records come from the same two passes (mode_unit's units)."""
    from hashcat_a5_table_generator_amd import Context
    from oracle import c_oracle as co
    words = _greek_words()
    tab = [table_path("greek-hebrew")]
    key = ("greek-cuts", mode, mn)
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
