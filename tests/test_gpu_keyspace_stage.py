"""k_keyspace_thread's word stage: the small one (five workgroups per CU) against the large one.

The byte walk stages a tile's words in LDS.  With the large stage (8192 B) four workgroups
share a CU; with the small one (Context.keyspace_small_stage(): what the loaded table leaves
of 32,000 B, 25 LDS allocation granules) five do.  A batch takes the small stage when every
one of its 256-word tiles fits it, woff[t1] - (woff[t0] & ~15) <= S, and the large one
otherwise: no word changes path inside a batch, and nothing per word may depend on the stage.
Context.keyspace_stage() names the stage the last pass used, Context.keyspace_large_stage()
stops the small one from being offered.

As tests/test_gpu_keyspace_unit_sync.py (whose word builders and oracle cache are used
here): czech + german, per-word count and bytes from the prefix arrays of
a5x_keyspace_device and the digest rows of the expansion, against the C oracle.
"""
import numpy as np
import pytest

from conftest import table_path
import test_gpu_keyspace_unit_sync as us

pytestmark = pytest.mark.gpu

LARGE = 8192  # KS_WB


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


def _run(ctx, words, mn=0, mx=15):
    """cand_off, byte_off, digest rows of the expansion, stage and refit count of the keyspace pass"""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    data, offs = pack_words(words)
    n = len(words)
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    coff, boff = DeviceBuffer(ctx, (n + 1) * 8), DeviceBuffer(ctx, (n + 1) * 8)
    tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, n, 0, mn, mx, d_cand_off=coff.ptr, d_byte_off=boff.ptr)
    stage, refit = ctx.keyspace_stage(), ctx.keyspace_refit()
    c, b = coff.to_array(np.uint64), boff.to_array(np.uint64)
    assert int(c[n]) == tc and int(b[n]) == tb
    out = DeviceBuffer(ctx, max(tb, 16))
    st = ctx.expand_device(dw.ptr, do.ptr, n, out.ptr, tb, 0, mn, mx, d_byte_off=boff.ptr)
    assert st["candidates"] == tc and st["bytes"] == tb
    dig = DeviceBuffer(ctx, n * 32)
    ctx.digest_device(out.ptr, boff.ptr, 0, n, dig.ptr)
    return c, b, dig.to_array(np.uint64).reshape(n, 4), stage, refit


def _check(ctx, ctab, words, mn=0, mx=15):
    """every word against the C oracle; returns (stage, refit)"""
    want = us._want(ctab, words, mn, mx)
    c, b, got, stage, refit = _run(ctx, words, mn, mx)
    cnt, byt = np.diff(c), np.diff(b)
    bad = np.nonzero((cnt != want[:, 0]) | (byt != want[:, 1]))[0]
    assert len(bad) == 0, [(i, words[i], int(cnt[i]), int(byt[i]), want[i][:2]) for i in bad[:5]]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(i, words[i], got[i], want[i]) for i in bad[:5]]
    return stage, refit


def _lengths(rng, n, total, lo):
    """n lengths of lo..lo + 2 bytes, shuffled, that sum to total"""
    extra = total - lo * n
    assert 0 <= extra <= 2 * n, (n, total, lo)
    ls = np.full(n, lo, dtype=np.int64)
    ls[: extra // 2] = lo + 2
    ls[extra // 2: extra // 2 + extra % 2] = lo + 1
    rng.shuffle(ls)
    return ls


def _boundary_words(tile, span, seed):
    """700 words in 3 tiles (the last one partial) of lo..lo + 2 bytes, lo + 1 the stage's bytes
    per word (10..12 for the 2928 B that czech + german leave); tile `tile` spans exactly `span`
    staged bytes.  tile 0 starts aligned; for tile 1, woff[256] % 16 == 15, so the span is 15
    bytes more than its words."""
    rng = np.random.default_rng(seed)
    lo = (span - 16) // 256 - 1
    assert lo >= 4
    if tile == 0:
        l0 = _lengths(rng, 256, span, lo)
        l1 = _lengths(rng, 256, lo * 256 + 37, lo)
    else:
        l0 = _lengths(rng, 256, lo * 256 + 15, lo)  # 256 lo is a multiple of 16
        l1 = _lengths(rng, 256, span - 15, lo)
    ls = np.concatenate([l0, l1, _lengths(rng, 188, lo * 188 + 20, lo)])
    offs = np.concatenate([[0], np.cumsum(ls)])
    spans = [int(offs[min(700, t + 256)] - (offs[t] & ~15)) for t in (0, 256, 512)]
    assert spans[tile] == span and (tile == 0 or offs[256] % 16 == 15)
    assert all(s < span for i, s in enumerate(spans) if i != tile)
    return [us._word(rng, int(L), int(rng.integers(0, 5))) for L in ls]


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("over", [0, 1])
def test_boundary(ctx, ctab, tile, over):
    """A tile of exactly S staged bytes takes the small stage, one of S + 1 the large one."""
    S = ctx.keyspace_small_stage()
    assert 2048 <= S < LARGE and S % 16 == 0
    words = _boundary_words(tile, S + over, 0x57A6E + 2 * tile + over)
    stage, refit = _check(ctx, ctab, words)
    assert stage == (LARGE if over else S)
    assert refit == 0


def _expected_stage(words, S):
    offs = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int64)
    n = len(words)
    span = max(int(offs[min(n, t + 256)] - (offs[t] & ~15)) for t in range(0, n, 256))
    return S if span <= S else LARGE


def _c3_words():
    from hashcat_a5_table_generator_amd import synth
    _, (data, offs) = synth.config_words("c3", 2000)
    return [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(2000)]


@pytest.mark.parametrize("batch", ["c3", "mixed", "mixed10"])
def test_equivalence(ctx, batch):
    """The same batch with the small stage and with the large one forced: equal prefix arrays
    and equal expansion digests.  mixed10: the mixed batch cut to 10 bytes a word, whose tiles
    fit the small stage."""
    words = _c3_words() if batch == "c3" else us._mixed_words(513, 0x5C0 + 513)
    if batch == "mixed10":
        words = [w[:10] for w in words]
    S = ctx.keyspace_small_stage()
    c0, b0, d0, stage0, _ = _run(ctx, words)
    ctx.keyspace_large_stage(True)
    try:
        c1, b1, d1, stage1, _ = _run(ctx, words)
    finally:
        ctx.keyspace_large_stage(False)
    # (C3 tiles are about 2.3 KB: small; the mixed batch of 0..40-byte words has tiles of
    # about 4.7 KB, so its normal run is the large stage chosen on the device)
    assert stage0 == _expected_stage(words, S) and stage1 == LARGE
    if batch != "mixed":
        assert stage0 == S
    assert np.array_equal(c0, c1) and np.array_equal(b0, b1)
    assert np.array_equal(d0, d1)
    assert int(c0[-1]) > len(words)


def test_one_long_tile(ctx, ctab):
    """512 short words, then a tile of 256 words of 40..64 bytes: the whole batch takes the
    large stage."""
    rng = np.random.default_rng(0x10E6)
    words = us._unit_words() + us._unit_words()
    words += [us._word(rng, int(L), int(rng.integers(0, 5))) for L in rng.integers(40, 65, size=256)]
    stage, _ = _check(ctx, ctab, words)
    assert stage == LARGE


def test_not_offered_utf8():
    """greek-hebrew, a UTF-8 batch: the walk by lead bytes keeps the large stage; -s candidates
    against the C oracle."""
    from hashcat_a5_table_generator_amd import Context
    from oracle import c_oracle as co
    words = us._greek_words()[:50]
    tab = [table_path("greek-hebrew")]
    t = co.CTable(tab)
    out, wb = t.expand_batch(*co.pack_words(words), 2, 0, 15)
    want, pos = [], 0
    for b in wb:
        seg = out[pos:pos + int(b)]
        pos += int(b)
        want.append(sorted(seg.split(b"\n")[:-1]) if seg else [])
    with Context(0) as c:
        c.load_tables(tab)
        got = c.expand_words(words, 2, 0, 15)
        stage = c.keyspace_stage()
    assert stage == LARGE
    for w, g, x in zip(words, got, want):
        assert sorted(g) == x, (w, len(g), len(x))


def test_refit_small_stage(ctx, ctab):
    """A word of 17 lone matches inside a small-stage batch still takes the fused walk."""
    words = us._unit_words()
    words[100] = us.U17
    stage, refit = _check(ctx, ctab, words, 0, 40)
    assert stage == ctx.keyspace_small_stage()
    assert refit == 1
