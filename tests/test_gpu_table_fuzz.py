"""GPU differential tests on the synthetic tables of tests/table_fuzz.py, through the C ABI.

The corpora put words on both sides of every limit that decides which kernel takes a word
(tests/test_table_fuzz.py asserts the census on the CPU); here the kernels themselves --
k_keyspace_thread / _cplx / _vsub, k_expand_fast, the per-word passes, the mode engines,
k_vwords_fill and the fused digest -- are compared with the C oracle per word: counts,
bytes, candidate multisets, the reference's -r panics, batch-independent numbering,
candidate ranges and digest hits.  Words no oracle can enumerate (2^24 .. 2^32 candidates)
are checked by windows against a decoder of the documented candidate numbering.
"""
import binascii
import collections
import functools
import hashlib
import os

import numpy as np
import pytest

import table_fuzz as tf

pytestmark = pytest.mark.gpu

RUNS = [(n, m) for n in tf.NAMES for m in tf.corpus(n).modes]


def _ctx(c, chunk=None):
    from hashcat_a5_table_generator_amd import Context
    if chunk is not None:
        os.environ["A5X_CHUNK"] = str(chunk)
    try:
        ctx = Context(0)
    finally:
        os.environ.pop("A5X_CHUNK", None)
    ctx.load_tables([c.path])
    return ctx


@functools.lru_cache(maxsize=2)
def _reference(name, mode, mn, mx, which):
    """(words the reference expands, their sorted candidate lists, the words it panics on)"""
    good, bad = tf.split_panics(name, which, mode, mn, mx)
    return good, tf.reference_lists(tf.corpus(name), good, mode, mn, mx, which), bad


M_LMAX, M_CMAX = 128, 127  # A5X_M_LMAX, A5X_M_CBUF - 1


def _runnable(name, mode, mn, mx, which="words"):
    """(words, sorted lists, refused words) of a run.  The -r / -s / -s -r LDS engines take
    words of <= 128 bytes whose candidates are <= 127 bytes (longer words go to mode pass G);
    a word on the far side makes its batch A5X_E_UNSUPPORTED, so it is run alone
    (test_mode_engine_refuses_long_candidates) and left out of the batches."""
    good, want, _ = _reference(name, mode, mn, mx, which)
    if mode == 0:
        return list(good), want, []
    far = [len(w) <= M_LMAX and max((len(x) for x in e), default=0) > M_CMAX for w, e in zip(good, want)]
    return ([w for w, f in zip(good, far) if not f], [e for e, f in zip(want, far) if not f],
            [w for w, f in zip(good, far) if f])


def _over_limit(c, w, mode):
    """past the documented -r / -s engine limit of 63 positions / patterns"""
    f = tf.tied_facts(c.table, w)
    return (f["occ"] if mode == 1 else f["patterns"]) > 63


def _expand_lists(ctx, words, mode, mn, mx):
    """(per-word ordered lists, per-word (count, bytes) of a5x_keyspace, stats)"""
    from hashcat_a5_table_generator_amd import pack_words
    data, offs = pack_words(list(words))
    cnt, byt = ctx.keyspace(data, offs, mode, mn, mx)
    out, st = ctx.expand(data, offs, mode, mn, mx)
    res, pos = [], 0
    for i in range(len(words)):
        seg = out[pos:pos + int(byt[i])]
        pos += int(byt[i])
        res.append(seg.split(b"\n")[:-1] if seg else [])
    assert pos == len(out)
    return res, list(zip(map(int, cnt), map(int, byt))), st


# ---------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", RUNS)
def test_parity(name, mode):
    """keyspace gives the oracle's count and bytes per word, expand_words its multiset, with
    the default chunk and with A5X_CHUNK=64."""
    c = tf.corpus(name)
    ctxs = [_ctx(c), _ctx(c, 64)]
    fast_seen = sum(r["fast"] and r["count"] > 0 for r in tf.census(name)) if mode == 0 else None
    for m, mn, mx, which in c.runs():
        if m != mode or which == "narrow":
            continue
        good, want, _ = _runnable(name, mode, mn, mx, which)
        sizes = [(len(e), sum(len(x) + 1 for x in e)) for e in want]
        for ctx in ctxs if good else []:
            got, ks, st = _expand_lists(ctx, good, mode, mn, mx)
            for w, g, k, e, sz in zip(good, got, ks, want, sizes):
                assert k == sz, (name, mode, mn, mx, w, k, sz)
                assert sorted(g) == e, (name, mode, mn, mx, w, len(g), len(e))
            if mode == 0 and (mn, mx) == (0, 15) and which == "words":
                assert fast_seen > 0 and st["words_slow"] > 0, (name, st)
                if name in ("pieces", "tied", "clusters"):
                    assert st["words_pass_b"] > 0, (name, st)
    for ctx in ctxs:
        ctx.close()


@pytest.mark.parametrize("name,mode", [(n, m) for n, m in RUNS if tf.corpus(n).word_list("narrow", m)])
def test_parity_narrow(name, mode):
    """The words with 62-65 patterns / positions (window (0, 3)), each alone in a batch: the
    reference's count, bytes and multiset up to the documented 63; past it a word may be
    refused (A5X_E_UNSUPPORTED), never answered wrongly.  Default mode has no such limit."""
    from hashcat_a5_table_generator_amd import A5xError
    c = tf.corpus(name)
    ctx = _ctx(c)
    for mn, mx in tf.NARROW:
        good, want, _ = _runnable(name, mode, mn, mx, "narrow")
        served = 0
        for w, e in zip(good, want):
            try:
                got, ks, _ = _expand_lists(ctx, [w], mode, mn, mx)
            except A5xError as err:
                assert mode and "UNSUPPORTED" in str(err) and _over_limit(c, w, mode), (name, mode, w, str(err))
                continue
            assert sorted(got[0]) == e and ks[0] == (len(e), sum(len(x) + 1 for x in e)), (name, mode, w)
            served += 1
        assert served >= sum(not _over_limit(c, w, mode) for w in good)
    ctx.close()


@pytest.mark.parametrize("name", ["lengths", "pieces", "tied"])
def test_mode_engine_refuses_long_candidates(name):
    """-r / -s / -s -r words of <= 128 bytes with a candidate of 128 bytes or more, alone in a
    batch: A5X_E_UNSUPPORTED (the documented limit of the LDS engines) or, where the FAST
    probe takes the word, the oracle's answer -- never a wrong one; candidates of 126 and 127
    bytes are in the parity runs."""
    from hashcat_a5_table_generator_amd import A5xError, pack_words
    c = tf.corpus(name)
    ctx = _ctx(c)
    n = served = 0
    for mode in (1, 2, 3):
        for mn, mx in ((0, 15), (0, 3)):
            good, want, far = _runnable(name, mode, mn, mx)
            assert any(max((len(x) for x in e), default=0) in (126, 127) for e in want) or name != "tied"
            ref = dict(zip(*_reference(name, mode, mn, mx, "words")[:2]))
            for w in far:
                try:
                    got, ks, _ = _expand_lists(ctx, [w], mode, mn, mx)
                except A5xError as err:
                    assert "UNSUPPORTED" in str(err), (name, mode, w, str(err))
                    n += 1
                    continue
                assert sorted(got[0]) == ref[w] and ks[0][0] == len(ref[w]), (name, mode, mn, mx, w)
                served += 1
    ctx.close()
    assert n >= 5 and n + served > 0


@pytest.mark.parametrize("name", [n for n in tf.NAMES if 1 in tf.corpus(n).modes])
def test_reverse_panics_are_reported(name):
    """Each word on which the reference panics under -r, alone in a batch: A5X_E_BOUNDS (the
    batches without them are the parity runs above)."""
    from hashcat_a5_table_generator_amd import A5xError, pack_words
    c = tf.corpus(name)
    ctx = _ctx(c)
    n = 0
    for m, mn, mx, which in c.runs():
        if m not in (1, 3):
            continue
        _, bad = tf.split_panics(name, which, m, mn, mx)
        for w in bad if mn >= 0 else bad[:8]:  # (min < 0: every word overflows the reference's stack)
            data, offs = pack_words([w])
            with pytest.raises(A5xError) as e:
                ctx.expand(data, offs, m, mn, mx)
            if "UNSUPPORTED" in str(e.value):  # past 63 positions / patterns: refused before the walk
                assert _over_limit(c, w, m), (name, m, mn, mx, w, str(e.value))
                continue
            assert "BOUNDS" in str(e.value), (name, m, mn, mx, w, str(e.value))
            n += 1
    ctx.close()
    assert n >= 8


# ---------------------------------------------------------------------------
# numbering and ranges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", RUNS)
def test_numbering_independent_of_batch(name, mode):
    """A word's ordered candidate list in one big batch == in 16-word batches."""
    c = tf.corpus(name)
    words, _, _ = _runnable(name, mode, 0, 15)
    ctx = _ctx(c)
    big, _, _ = _expand_lists(ctx, words, mode, 0, 15)
    pos = 0
    for i in range(0, len(words), 16):
        small, _, _ = _expand_lists(ctx, words[i:i + 16], mode, 0, 15)
        for w, s in zip(words[i:i + 16], small):
            assert big[pos] == s, (name, mode, w, "candidate order differs between batches")
            pos += 1
    ctx.close()


@pytest.mark.parametrize("name", tf.NAMES)
def test_candidate_ranges_concatenate(name):
    """expand_device over ~8 random candidate cuts == the full output, byte-exact, every mode."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    c = tf.corpus(name)
    ctx = _ctx(c)
    rng = np.random.default_rng(len(name) * 977)
    for mode in c.modes:
        mn, mx = (0, 15) if name not in ("tied", "choices") or mode else (0, 3)
        words, _, _ = _runnable(name, mode, mn, mx)
        data, offs = pack_words(list(words))
        dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
        tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, len(words), mode, mn, mx)
        full = DeviceBuffer(ctx, tb)
        st = ctx.expand_device(dw.ptr, do.ptr, len(words), full.ptr, tb, mode, mn, mx)
        assert (st["candidates"], st["bytes"]) == (tc, tb)
        ref = full.to_array()
        cuts = sorted(set([0, tc] + [int(x) for x in rng.integers(0, tc, size=7)]))
        buf = DeviceBuffer(ctx, tb)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            st = ctx.expand_device(dw.ptr, do.ptr, len(words), buf.ptr, tb, mode, mn, mx, cand_begin=a, cand_end=b)
            assert st["candidates"] == b - a, (name, mode, a, b)
            parts.append(buf.to_array(count=st["bytes"]))
        assert np.array_equal(np.concatenate(parts), ref), (name, mode, cuts)
        for x in (dw, do, full, buf):
            x.free()
    ctx.close()


# ---------------------------------------------------------------------------
# fused digest
# ---------------------------------------------------------------------------
def _digest_fn(algo):
    from oracle import c_oracle as co
    return {0: lambda b: hashlib.md5(b).digest(), 1: lambda b: co.digest(1, b),
            2: lambda b: hashlib.sha1(b).digest()}[algo]


@pytest.mark.parametrize("name,algo", [(n, a) for n in ("choices", "lengths", "clusters", "tied") for a in (0, 1)] +
                         [("clusters", 2)])
def test_fused_digest_hits_are_exhaustive(name, algo):
    """~200 planted targets among 5000 random ones: the hits equal the exhaustive set over the
    oracle's candidates (by word and digest: the oracle has no order), and every hit
    regenerates its plain through format_hits.  SHA-1 takes the two-pass route."""
    from hashcat_a5_table_generator_amd import pack_words
    from oracle import digest_oracle
    c = tf.corpus(name)
    dg = _digest_fn(algo)
    size = {0: 16, 1: 16, 2: 20}[algo]
    ctx = _ctx(c)
    rng = np.random.default_rng(1000 + algo)
    for mode in c.modes:
        mn, mx = 0, 3
        words, want, _ = _runnable(name, mode, mn, mx)
        flat = [(i, x) for i, e in enumerate(want) for x in e]
        planted = [flat[int(j)][1] for j in rng.choice(len(flat), size=min(200, len(flat)), replace=False)]
        if algo == 1:  # the C digest used for the exhaustive set is the oracle's NTLM
            assert all(dg(p) == digest_oracle.ntlm(p) for p in planted[:50])
        targets = {dg(p) for p in planted} | {bytes(rng.integers(0, 256, size=size, dtype=np.uint8)) for _ in range(5000)}
        ctx.set_targets(algo, b"".join(sorted(targets)))
        expect = collections.Counter((i, d) for i, x in flat for d in (dg(x),) if d in targets)
        data, offs = pack_words(list(words))
        hits, _ = ctx.expand_digest(data, offs, mode, mn, mx, hit_cap=1 << 16)
        assert collections.Counter((w, d) for w, _, d in hits) == expect, (name, algo, mode)
        text = ctx.format_hits(data, offs, hits, mode, mn, mx)
        lines = text.split(b"\n")[:-1]
        assert len(lines) == len(hits)
        seen = set()
        for line in lines:
            hx, plain = line.split(b":", 1)
            if plain.startswith(b"$HEX[") and plain.endswith(b"]"):
                plain = binascii.unhexlify(plain[5:-1])
            assert dg(plain).hex().encode() == hx, line
            seen.add(plain)
        assert set(planted) <= seen
    ctx.close()


# ---------------------------------------------------------------------------
# huge words, checked by windows
# ---------------------------------------------------------------------------
WIN = 4096


def _windows(count, seed):
    rng = np.random.default_rng(seed)
    ws = [0] + [int(x) for x in rng.integers(0, count - WIN, size=3)] + [count - WIN]
    if count > (1 << 24) + WIN:
        ws.append((1 << 24) - 1 - WIN // 2)  # across rank 2^24 - 1
    if count > (1 << 32) + WIN:
        ws.append((1 << 32) - 1 - WIN // 2)  # across rank 2^32 - 1 (the 32-bit candidate index ends)
    return ws


@pytest.mark.parametrize("word,P,fast,defer,nbig,bent", tf.HUGE, ids=[h[0].decode() for h in tf.HUGE])
def test_huge_word_windows(word, P, fast, defer, nbig, bent):
    """Closed-form count and bytes, then windows of 4096 candidates compared IN ORDER with
    table_fuzz.decode_rank (the documented numbering); the FAST word and its non-FAST
    neighbour also through the fused MD5 route over the same windows.

    The word past the 2^32 deferral (P = 4299816960) is a radix word with 64-bit digits
    (wave_setup wide, slot_digit): same numbering, one more window across rank 2^32 - 1."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    c = tf.corpus("choices")
    ctx = _ctx(c)
    mn, mx = 0, tf.HUGE_MAX
    data, offs = pack_words([word])
    cnt, byt = ctx.keyspace(data, offs, 0, mn, mx)
    assert (int(cnt[0]), int(byt[0])) == tf.huge_closed_form(c.table, word) == (P - 1, int(byt[0]))
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    cap = WIN * (len(word) + 1)
    buf = DeviceBuffer(ctx, cap)
    for a in _windows(P - 1, len(word)):
        st = ctx.expand_device(dw.ptr, do.ptr, 1, buf.ptr, cap, 0, mn, mx, cand_begin=a, cand_end=a + WIN)
        assert st["candidates"] == WIN
        got = buf.to_array(count=st["bytes"]).tobytes().split(b"\n")[:-1]
        want = [tf.decode_rank(c.table, word, r) for r in range(a, a + WIN)]
        assert got == want, (word, a, next((i, g, e) for i, (g, e) in enumerate(zip(got, want)) if g != e))
        if word in (b"fcfcjiji", b"fcfcfcji"):
            planted = {hashlib.md5(want[i]).digest(): a + i for i in (0, 1, 777, WIN - 1)}
            outside = hashlib.md5(tf.decode_rank(c.table, word, a + WIN if a + WIN < P - 1 else a - 1)).digest()
            ctx.set_targets(0, b"".join(planted) + outside)
            hits, _ = ctx.expand_digest_device(dw.ptr, do.ptr, 1, 0, mn, mx, cand_begin=a, cand_end=a + WIN)
            assert sorted((cand, d) for _, cand, d in hits) == sorted((r, d) for d, r in planted.items()), (word, a)
    ctx.close()


def test_wide_word_with_length_deltas():
    """A radix word past 2^32 candidates whose values are shorter and longer than their keys
    (lengths table: a -> "", "X"; b -> 6 bytes; h -> 1 byte): P = 3^21 * 2 * 2, count and bytes
    in closed form, windows in order against decode_rank, and a5x_locate_device's byte
    offsets of the window starts (radix_prefix_bytes with 64-bit ranks)."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    c = tf.corpus("lengths")
    ctx = _ctx(c)
    word, mn, mx = b"a" * 21 + b".hb", 0, tf.HUGE_MAX
    P = 3 ** 21 * 4
    data, offs = pack_words([word])
    cnt, byt = ctx.keyspace(data, offs, 0, mn, mx)
    assert (int(cnt[0]), int(byt[0])) == tf.huge_closed_form(c.table, word) and int(cnt[0]) == P - 1
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    cap = WIN * (len(word) + 8)
    buf = DeviceBuffer(ctx, cap)
    starts = _windows(P - 1, 21)
    for a in starts:
        st = ctx.expand_device(dw.ptr, do.ptr, 1, buf.ptr, cap, 0, mn, mx, cand_begin=a, cand_end=a + WIN)
        assert st["candidates"] == WIN
        got = buf.to_array(count=st["bytes"]).tobytes().split(b"\n")[:-1]
        want = [tf.decode_rank(c.table, word, r) for r in range(a, a + WIN)]
        assert got == want, (a, next((i, g, e) for i, (g, e) in enumerate(zip(got, want)) if g != e))
    # byte offset of rank r = bytes of the candidates before it: exact for the last window's
    # start from the total, and increasing by the window's bytes
    last = P - 1 - WIN
    off = ctx.locate_device(dw.ptr, do.ptr, 1, [last, last + WIN], 0, mn, mx)
    tail = sum(len(tf.decode_rank(c.table, word, r)) + 1 for r in range(last, P - 1))
    assert int(off[1]) == int(byt[0]) and int(off[0]) == int(byt[0]) - tail
    ctx.close()


def test_huge_word_overflow_is_reported():
    from hashcat_a5_table_generator_amd import A5xError, pack_words
    c = tf.corpus("choices")
    ctx = _ctx(c)
    data, offs = pack_words([tf.HUGE_OVERFLOW])
    with pytest.raises(A5xError) as e:
        ctx.keyspace(data, offs, 0, 0, tf.HUGE_MAX)
    assert "OVERFLOW" in str(e.value)
    ctx.close()


def test_default_engine_refuses_the_1144_key_table():
    """A key index >= 1024 never reaches the default engine's kernels: its table is refused."""
    from hashcat_a5_table_generator_amd import A5xError, pack_words
    ctx = _ctx(tf.corpus("manykeys"))
    data, offs = pack_words([b"aa.ab"])
    with pytest.raises(A5xError) as e:
        ctx.keyspace(data, offs, 0, 0, 15)
    assert "UNSUPPORTED" in str(e.value)
    ctx.close()
