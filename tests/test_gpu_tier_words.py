"""GPU differential tests at the limits that route a non-FAST word to pass A, B or G.

The words are the pairs of tests/tier_words.py (census: tests/test_tier_words.py): for every
limit of csrc/a5x_format.h one word with the deciding fact at the limit and one at the next
reachable value.  Checked here: the per-word flags that the keyspace leaves (a5x_debug_word_flags)
against the tier facts() derives, count and bytes against the closed form, and the candidates
against reference() (disjoint single-key words, any window) or the C oracle (windows of at most
one substitution).  One test function per tier boundary, pass A upward, so a failure names it.
"""
import functools
import os

import numpy as np
import pytest

import tier_words as tw

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# expected outputs: computed once per (word, window), shared by every test
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _facts(word, mn, mx):
    return tw.facts(word, mn, mx)


@functools.lru_cache(maxsize=None)
def _expected(word, mn, mx):
    """Sorted candidates: reference() where the matches are disjoint and single-key, the C
    oracle in windows of at most three substitutions otherwise."""
    f = _facts(word, mn, mx)
    if f["tier"] == "none":
        return ()
    if not f["conflict"] and not f["multi"] and (mx > 3 or f["nev"] <= 16):
        return tuple(sorted(tw.reference(word, mn, mx)))
    assert mx <= 3, "the C oracle walks every smaller subset first"
    from oracle import c_oracle as co
    return tuple(sorted(co.CTable([tw.table_file()]).expand_word(word, 0, mn, mx)))


@functools.lru_cache(maxsize=None)
def _host():
    from hashcat_a5_table_generator_amd import Context
    return Context(-1).load_tables([tw.table_file()])


@functools.lru_cache(maxsize=None)
def _host_plan(word, mn, mx):
    """(count, bytes, flags) of the host replay of the thread-level classifier"""
    c = _host()
    info = np.zeros(4, dtype=np.uint64)
    wb = np.frombuffer(word + b"\0", dtype=np.uint8)
    assert c._L.a5x_debug_plan_word(c.h, wb.ctypes.data, len(word), mn, mx, None, 0, info.ctypes.data) == 0
    return int(info[0]), int(info[1]), int(info[2]) & 0xFFFFFFFF


def _closed_form(word, mn, mx):
    from oracle import a5_oracle as o
    return o.keyspace_default(word, _sub(), mn, mx)


@functools.lru_cache(maxsize=None)
def _sub():
    from oracle import a5_oracle as o
    return o.load_tables([tw.table_file()])


# ---------------------------------------------------------------------------
# contexts and runs
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    gpu_ctx.clear_table()
    gpu_ctx.load_tables([tw.table_file()])
    return gpu_ctx


@pytest.fixture(scope="module")
def ctx64():
    """A context with chunks of 64 candidates: a tier word spans many chunks."""
    from hashcat_a5_table_generator_amd import Context
    os.environ["A5X_CHUNK"] = "64"
    try:
        c = Context(0)
    finally:
        os.environ.pop("A5X_CHUNK", None)
    c.load_tables([tw.table_file()])
    yield c
    c.close()


class Batch:
    """words on the device and what keyspace_device leaves: totals, per-word offsets, flags."""

    def __init__(self, c, words, mn, mx):
        from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
        self.c, self.words, self.mn, self.mx, self.n = c, list(words), mn, mx, len(words)
        data, offs = pack_words(self.words)
        self.dw, self.do = DeviceBuffer.from_array(c, data), DeviceBuffer.from_array(c, offs)
        self.dco, self.dbo = DeviceBuffer(c, 8 * (self.n + 1)), DeviceBuffer(c, 8 * (self.n + 1))

    def keyspace(self):
        self.tc, self.tb = self.c.keyspace_device(self.dw.ptr, self.do.ptr, self.n, 0, self.mn, self.mx, self.dco.ptr,
                                                  self.dbo.ptr)
        self.cand_off = self.dco.to_array(np.uint64).astype(object)
        self.byte_off = self.dbo.to_array(np.uint64).astype(object)
        self.flags = [int(x) for x in self.c.word_flags(self.n)]
        return self

    def expand(self, cand_begin=0, cand_end=(1 << 64) - 1, nbytes=None):
        from hashcat_a5_table_generator_amd import DeviceBuffer
        cap = self.tb if nbytes is None else nbytes
        out = DeviceBuffer(self.c, cap)
        st = self.c.expand_device(self.dw.ptr, self.do.ptr, self.n, out.ptr, cap, 0, self.mn, self.mx,
                                  cand_begin=cand_begin, cand_end=cand_end)
        buf = bytes(out.to_array()[:st["bytes"]])
        out.free()
        return buf, st

    def lists(self):
        """The ordered candidate list of every word, from one expansion of the whole batch."""
        buf, st = self.expand()
        assert (st["candidates"], st["bytes"]) == (self.tc, self.tb)
        res = []
        for i in range(self.n):
            seg = buf[self.byte_off[i]:self.byte_off[i + 1]]
            lines = seg.split(b"\n")
            assert lines[-1] == b"" and len(lines) - 1 == self.cand_off[i + 1] - self.cand_off[i] or not seg
            res.append(lines[:-1] if seg else [])
        return res

    def free(self):
        for b in (self.dw, self.do, self.dco, self.dbo):
            b.free()


def _check_flags(b, tier_idx=None):
    """flags, count and bytes of every word of a sized batch against facts() in its window;
    tier_idx: the tier words' indices (default: all), the others are the short FAST words"""
    for i, w in enumerate(b.words):
        f = _facts(w, b.mn, b.mx)
        cnt, byt = b.cand_off[i + 1] - b.cand_off[i], b.byte_off[i + 1] - b.byte_off[i]
        if f["tier"] == "none":
            assert (cnt, byt) == (0, 0), (i, len(w))
            continue
        # FAST or not is the host replay's word (a5x_debug_plan_word: the classifier the thread
        # kernel runs), never the flags under test: the short words beside the tier words, and a
        # tier word that is plain radix in this window, must be FAST exactly where it says so
        hcnt, hbyt, hfl = _host_plan(w, b.mn, b.mx)
        if hfl & tw.FAST:
            assert b.flags[i] & tw.FAST and not b.flags[i] & (tw.BIG | tw.GLOB | tw.ERR_BIG | tw.ERR_OVF), \
                (i, w[:40], hex(b.flags[i]), hex(hfl))
            assert (cnt, byt) == (f["count"], f["bytes"]) == (hcnt, hbyt), (i, w[:40])
            continue
        assert not b.flags[i] & tw.FAST, (i, w[:40], hex(b.flags[i]), hex(hfl))
        if tier_idx is not None and i not in tier_idx:  # a short word in a window that is not free
            assert (cnt, byt) == (f["count"], f["bytes"]), (i, w[:40], hex(b.flags[i]))
            continue
        mask, val = tw.tier_flags(f)
        assert b.flags[i] & mask == val, (i, len(w), b.mn, b.mx, f["tier"], hex(b.flags[i]))
        assert (cnt, byt) == (f["count"], f["bytes"]), (i, len(w), b.mn, b.mx, f["tier"])


def _check_alone(c, word, mn, mx, expand=True):
    """One word as a batch of its own: tier flags, closed-form keyspace, candidate multiset."""
    b = Batch(c, [word], mn, mx).keyspace()
    try:
        _check_flags(b)
        assert (b.tc, b.tb) == _closed_form(word, mn, mx)
        got = None
        if expand:
            got = b.lists()[0]
            want = _expected(word, mn, mx)
            assert len(got) == len(want) and tuple(sorted(got)) == want, (len(word), mn, mx, len(got), len(want))
        return got
    finally:
        b.free()


def _check_pair(name, c, c64):
    p = tw.pair(name)
    for i, side in enumerate(("at", "over")):
        if p.err[i] is not None:
            continue
        w, mn, mx = p.sides[side]
        assert _facts(w, mn, mx)["tier"] == p.tier[side]
        a = _check_alone(c, w, mn, mx, p.expand[i])
        if p.expand[i]:
            assert _check_alone(c64, w, mn, mx) == a, (name, side, "the chunk size changed a word's order")


# ---------------------------------------------------------------------------
# one test per boundary, pass A upward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A.L", "A.nmatch", "A.dp", "A.maxlen", "A.thread_maxl"])
def test_pass_a_to_b(name, ctx, ctx64):
    _check_pair(name, ctx, ctx64)


@pytest.mark.parametrize("name", ["B.L", "B.nmatch", "B.dp_square", "B.dp_events", "B.maxlen"])
def test_pass_b_to_g(name, ctx, ctx64):
    _check_pair(name, ctx, ctx64)


def test_count_columns_64(ctx, ctx64):
    """W = 64 count columns is the most any pass takes: 'c' * 64 in the window (63, 63) has 64
    candidates and a DP of 65 x 64 entries (pass G)."""
    _check_pair("W", ctx, ctx64)


@pytest.mark.parametrize("name", ["G.L", "G.maxlen"])
def test_pass_g_limits(name, ctx, ctx64):
    _check_pair(name, ctx, ctx64)


def test_pass_g_65536_matches(ctx):
    """The word of 65536 matches (1.4 GB if expanded) is never expanded whole: its keyspace is the
    closed form, and three windows of at most 64 candidates hold distinct lines that are the
    word with one substitution, whose lengths add up to the byte offsets locate_device gives."""
    w, mn, mx = tw.pair("G.nmatch").sides["at"]
    b = Batch(ctx, [w], mn, mx).keyspace()
    try:
        _check_flags(b)
        assert (b.tc, b.tb) == _closed_form(w, mn, mx) and b.tc == 65536
        one_sub = None
        seen = set()
        for lo, hi in ((0, 64), (32741, 32800), (65536 - 40, 65536)):
            offs = [int(x) for x in ctx.locate_device(b.dw.ptr, b.do.ptr, 1, [lo, hi], 0, mn, mx)]
            buf, st = b.expand(lo, hi, offs[1] - offs[0])
            lines = buf.split(b"\n")
            assert lines[-1] == b"" and st["candidates"] == hi - lo == len(lines) - 1
            assert sum(len(x) + 1 for x in lines[:-1]) == offs[1] - offs[0] == st["bytes"]
            if one_sub is None:
                one_sub = set()
                for p, ks in tw._positions(w):
                    for k in ks:
                        one_sub.add(w[:p] + tw.TABLE[k][0] + w[p + len(k):])
                assert len(one_sub) == 65536
            for x in lines[:-1]:
                assert x in one_sub and x not in seen
                seen.add(x)
        assert len(seen) == 64 + 59 + 40
    finally:
        b.free()


# ---------------------------------------------------------------------------
# mixed batches
# ---------------------------------------------------------------------------
def _mixed(mn, mx, cap=8 << 20, total=56 << 20):
    """Every pair word that the engine takes in the window (mn, mx) with at most cap output
    bytes, tiers mixed, in census order."""
    out, seen, tot = [], set(), 0
    for r in tw.census():
        w = r["word"]
        if w in seen:
            continue
        if (w.count(b"c") + w.count(b"a") + 1) * (min(mx, len(w)) + 1) > 100000:  # (seconds of Python DP)
            continue
        f = _facts(w, mn, mx)
        if (f["conflict"] or f["multi"]) and mx > 3:  # (no reference for it: see _expected)
            continue
        if f["tier"] in ("A", "B", "G") and f["bytes"] <= cap and tot + f["bytes"] <= total:
            out.append(w)
            seen.add(w)
            tot += f["bytes"]
    return out


@pytest.mark.parametrize("mn,mx", [(0, 1), (12, 12), (63, 63), (0, 15)])
def test_mixed_batch(mn, mx, ctx, ctx64):
    """The tier words in one batch, alone and interleaved with 200 short FAST words, at the
    default chunk and at 64 candidates per chunk: flags, keyspace, per-word multisets, and the
    same ordered list of a word in every batch."""
    words = _mixed(mn, mx)
    tiers = {_facts(w, mn, mx)["tier"] for w in words}
    assert tiers == {"A", "B", "G"}, tiers
    inter, where = _interleave(words, tw.short_fast_words())
    ordered = None
    for c in (ctx, ctx64):
        for batch, idx in ((words, range(len(words))), (inter, where)):
            b = Batch(c, batch, mn, mx).keyspace()
            try:
                _check_flags(b, set(idx))
                got = b.lists()
                for j, s in enumerate(batch):
                    want = _expected(s, mn, mx)
                    assert len(got[j]) == len(want) and tuple(sorted(got[j])) == want, (j, len(s), mn, mx)
                mine = [got[j] for j in idx]
                assert ordered is None or mine == ordered, "a word's order depends on its batch or the chunk size"
                ordered = mine
            finally:
                b.free()


def test_ranges_cut_inside_pass_b_and_g_words(ctx):
    """expand_device over candidate windows whose cuts fall inside a pass B word and a pass G
    word: the pieces concatenate to the stream of the whole batch."""
    mn, mx = 0, 1
    pb, pg = tw.pair("B.nmatch").sides["at"][0], tw.pair("B.dp_events").sides["over"][0]
    words = [b"c.c", pb, b"..c", pg, b"c-"]
    assert (_facts(pb, mn, mx)["tier"], _facts(pg, mn, mx)["tier"]) == ("B", "G")
    b = Batch(ctx, words, mn, mx).keyspace()
    try:
        _check_flags(b)
        full, _ = b.expand()
        co = [int(x) for x in b.cand_off]
        cuts = sorted({0, b.tc, co[1] + 1, co[1] + 777, co[2] - 1, co[3], co[3] + 63, co[3] + 64, co[3] + 1500, co[4] - 1})
        offs = [int(x) for x in ctx.locate_device(b.dw.ptr, b.do.ptr, b.n, cuts, 0, mn, mx)]
        parts = []
        for k in range(len(cuts) - 1):
            buf, st = b.expand(cuts[k], cuts[k + 1], offs[k + 1] - offs[k])
            assert st["candidates"] == cuts[k + 1] - cuts[k] and st["bytes"] == offs[k + 1] - offs[k]
            parts.append(buf)
        assert b"".join(parts) == full
    finally:
        b.free()


def _interleave(words, short):
    inter, where = [], []
    for i, s in enumerate(short):
        if i % (len(short) // len(words)) == 0 and len(where) < len(words):
            where.append(len(inter))
            inter.append(words[len(where) - 1])
        inter.append(s)
    assert len(where) == len(words)
    return inter, where


@pytest.mark.parametrize("algo", [0, 2])
def test_digest_hits_on_the_longest_candidates(algo, ctx):
    """expand_digest over the interleaved batch (MD5: fused kernel for the FAST words, hybrid
    sub-batch for the tier words; SHA-1: two-pass) with targets planted on the longest candidate
    of each tier among random ones: the hits are exactly the candidates whose digest is in the
    Python set, each at the index where the expansion writes it."""
    import collections
    import hashlib
    from hashcat_a5_table_generator_amd import pack_words
    dg = {0: lambda x: hashlib.md5(x).digest(), 2: lambda x: hashlib.sha1(x).digest()}[algo]
    mn, mx = 0, 1
    batch, where = _interleave(_mixed(mn, mx), tw.short_fast_words())
    b = Batch(ctx, batch, mn, mx).keyspace()
    try:
        lists = b.lists()
    finally:
        b.free()
    planted = {}
    for j in where:
        t = _facts(batch[j], mn, mx)["tier"]
        long = max(lists[j], key=len)
        if len(long) > len(planted.get(t, b"")):
            planted[t] = long
    assert set(planted) == {"A", "B", "G"} and len(planted["G"]) >= 65535
    planted = list(planted.values()) + [lists[where[0] + 1][0], lists[-1][-1]]
    rng = np.random.default_rng(77 + algo)
    size = {0: 16, 2: 20}[algo]
    targets = {dg(x) for x in planted} | {bytes(rng.integers(0, 256, size=size, dtype=np.uint8)) for _ in range(2000)}
    expect = collections.Counter((w, i) for w, cs in enumerate(lists) for i, x in enumerate(cs) if dg(x) in targets)
    assert len(expect) >= len(planted)
    try:
        ctx.set_targets(algo, b"".join(sorted(targets)))
        hits, _ = ctx.expand_digest(*pack_words(batch), 0, mn, mx, hit_cap=1 << 12)
    finally:
        ctx.set_targets(algo, b"")
    assert collections.Counter((w, c) for w, c, _ in hits) == expect
    for w, c, d in hits:
        assert dg(lists[w][c]) == d, (w, c)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def _refused():
    return [(p.name, side, p.sides[side], p.err[i]) for p in tw.pairs() for i, side in enumerate(("at", "over"))
            if p.err[i] is not None]


@pytest.mark.parametrize("name,side", [(n, s) for n, s, _, _ in _refused()])
def test_refusals(name, side, ctx):
    """A word past pass G, past 64 count columns or past 64 bits gives its error code alone and
    inside a batch, the flags name the reason, the error text names the word, and the next call
    on the context succeeds."""
    from hashcat_a5_table_generator_amd import A5xError
    (w, mn, mx), code = next((sw, e) for n, s, sw, e in _refused() if (n, s) == (name, side))
    f = _facts(w, mn, mx)
    for batch, at in (([w], 0), ([b"c.c", b"gc", w, b"..c"], 2)):
        b = Batch(ctx, batch, mn, mx)
        try:
            with pytest.raises(A5xError) as ei:
                b.keyspace()
            assert ei.value.code == code, str(ei.value)
            assert "[word %d len %d " % (at, len(w)) in str(ei.value), str(ei.value)
            fl = int(ctx.word_flags(len(batch))[at])
            mask, val = tw.tier_flags(f)
            assert fl & mask == val, (hex(fl), f["tier"], f["why"])
            if f["tier"] == "refused" and f["why"] != "W":
                assert fl & (tw.BIG | tw.GLOB) == tw.BIG | tw.GLOB
            with pytest.raises(A5xError):  # no layout was left to expand from
                b.expand(nbytes=1 << 16)
        finally:
            b.free()
        ok = Batch(ctx, [b"c.c", b"gc"], 0, 15).keyspace()
        try:
            assert (ok.tc, ok.tb) == (3 + 35, 3 * 4 + 35 * 3)
            assert sorted(ok.lists()[0]) == [b"C.C", b"C.c", b"c.C"]
        finally:
            ok.free()


# ---------------------------------------------------------------------------
# -r / -s / -s -r: the LDS engines' 128-byte word limit and mode pass G's limits
# ---------------------------------------------------------------------------
def _mode_ctx(table_path):
    from hashcat_a5_table_generator_amd import Context
    c = Context(0)
    c.load_tables([table_path])
    return c


def _mode_run(c, word, mode, mn, mx):
    """(sorted candidates, count, bytes, flags) of one word alone"""
    from hashcat_a5_table_generator_amd import pack_words
    data, offs = pack_words([word])
    cnt, byt = c.keyspace(data, offs, mode, mn, mx)
    fl = int(c.word_flags(1)[0])
    out, _ = c.expand(data, offs, mode, mn, mx)
    lines = out.split(b"\n")
    assert lines[-1] == b"" and len(out) == int(byt[0]) and len(lines) - 1 == int(cnt[0])
    return sorted(lines[:-1]), fl


def _mode_refused(c, word, mode, mn, mx, flag=True, at_keyspace=True):
    """A5X_E_UNSUPPORTED from the keyspace (at_keyspace) and in any case from the expansion:
    no output is ever written for the word; the context works afterwards."""
    from hashcat_a5_table_generator_amd import A5xError, pack_words
    data, offs = pack_words([word])
    if at_keyspace:
        with pytest.raises(A5xError) as ei:
            c.keyspace(data, offs, mode, mn, mx)
        assert ei.value.code == tw.E_UNSUPPORTED, str(ei.value)
        assert not flag or int(c.word_flags(1)[0]) & tw.ERR_BIG
    with pytest.raises(A5xError) as ei:
        c.expand(data, offs, mode, mn, mx)
    assert ei.value.code == tw.E_UNSUPPORTED, str(ei.value)
    ok, _ = _mode_run(c, b"c.c", mode, 0, 15)  # the context still works
    assert len(ok) >= 1


def _c_oracle(path, word, mode, mn, mx):
    from oracle import c_oracle as co
    return sorted(co.CTable([path]).expand_word(word, mode, mn, mx))


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_mode_word_128_129(mode):
    """The same word at 128 bytes (LDS engines) and 129 bytes (mode pass G) == the C oracle."""
    import table_fuzz as tf
    # -s: the LDS engines hold candidates of at most 127 bytes, so the 128-byte word's must shrink
    # (the tied table's d -> "" and c -> "<<" beside one-byte values)
    path = tf.corpus("tied").path if mode == 2 else tw.table_file()
    c = _mode_ctx(path)
    try:
        for n, glob in ((128, 0), (129, tw.GLOB)):
            w, win = b"c.gc" + tw.FILL * (n - 5) + b"c", (0, 15)
            if mode == 2:
                w = b"dd.e" + tw.FILL * (n - 5) + b"d"
                win = (2, 2) if n == 128 else (0, 15)   # d and e together: 125 or 126 bytes
            got, fl = _mode_run(c, w, mode, *win)
            assert fl & tw.GLOB == glob, (n, hex(fl))
            assert got == _c_oracle(path, w, mode, *win) and len(got) >= 2, (mode, n)
    finally:
        c.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_mode_pass_g_63_64(mode):
    """A mode pass G word with 63 patterns (-s, -s -r) or positions (-r) is expanded, with 64 it
    is refused with A5X_E_UNSUPPORTED."""
    import table_fuzz as tf
    if mode == 1:
        path, keys = tw.table_file(), [b"c"] * 64
    else:
        path, keys = tf.corpus("tied").path, [bytes((k,)) for k in tf.TIED_KEYS[:64]]
    c = _mode_ctx(path)
    try:
        w = b"".join(keys[:63]) + b"~" * 70
        got, fl = _mode_run(c, w, mode, 1, 1)
        assert fl & tw.GLOB
        if mode == 1:
            want = _c_oracle(path, w, mode, 1, 1)
        else:
            want = sorted(tf.suball_pruned(w, tf.corpus("tied").table, 1, 1, mode == 3))
        assert got == want and len(got) >= 63
        _mode_refused(c, b"".join(keys[:64]) + b"~" * 70, mode, 1, 1)
    finally:
        c.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_mode_pass_g_candidate_length(mode):
    """A mode pass G candidate of 2^17 - 1 bytes is written, one of 2^17 bytes is refused with
    A5X_E_UNSUPPORTED (-s, -s -r: by the keyspace; -r: by the expansion, after a keyspace that
    states the oracle's count and bytes), never written.  -s, -s -r: the word with every occurrence of its one pattern replaced (closed form); -r: the C
    oracle's one candidate of the window of all nine positions."""
    c = _mode_ctx(tw.table_file())
    try:
        for extra, ok in ((0, True), (1, False)):
            if mode == 1:   # 9 positions, all replaced: 5 * 24000 + 2 * 4070 + 2 * 1000 + filler
                w, win = b"v" * 5 + b"u" * 2 + b"w" * 2 + tw.FILL * (931 + extra), (9, 9)
            else:           # one pattern occurring 1310 times with a 100-byte value
                w, win = b"x" * 1310 + tw.FILL * (71 + extra), (1, 1)
            if mode == 1:   # (-r places by its running offset, main.go:255: the C oracle has the bytes)
                want = _c_oracle(tw.table_file(), w, mode, *win)[0]
            else:
                want = w.replace(b"x", tw.TABLE[b"x"][0])
            assert len(want) == (1 << 17) - 1 + extra and len(w) > 128
            if ok:
                got, fl = _mode_run(c, w, mode, *win)
                assert got == [want] and fl & tw.GLOB
            else:
                # -s, -s -r: the length pass of the keyspace builds every candidate and refuses
                # there (no ERR bit in the word's flags: the count pass had nothing to refuse).
                # -r: the length pass takes a candidate's length from its positions without
                # building it, so the keyspace answers -- with the oracle's count and bytes --
                # and the refusal comes from the expansion, which builds it in the lane buffer
                if mode == 1:
                    from hashcat_a5_table_generator_amd import pack_words
                    cnt, byt = c.keyspace(*pack_words([w]), mode, *win)
                    assert (int(cnt[0]), int(byt[0])) == (1, len(want) + 1)
                _mode_refused(c, w, mode, *win, flag=False, at_keyspace=mode != 1)
    finally:
        c.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_mode_dp_entries(mode):
    """A5X_M_DPMAX: (n + 1) * (min(max, n) + 1) <= 1024 -- 31 patterns or positions in the
    window (31, 31) fit (1024 entries, one candidate), 32 in (32, 32) are refused."""
    import table_fuzz as tf
    if mode == 1:
        path, keys, table = tw.table_file(), [b"c"] * 32, tw.TABLE
    else:
        path, keys, table = tf.corpus("tied").path, [bytes((k,)) for k in tf.TIED_KEYS[20:52]], tf.corpus("tied").table
    c = _mode_ctx(path)
    try:
        w = b"~".join(keys[:31])
        got, _ = _mode_run(c, w, mode, 31, 31)
        want = b"~".join(table[k][0] for k in keys[:31])
        assert got == [want]
        _mode_refused(c, b"~".join(keys[:32]), mode, 32, 32)
    finally:
        c.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_mode_dp_entries_63(mode, tmp_path):
    """A5X_M_DPMAX where the columns decide, not n: 63 patterns or positions with max = 16 are
    64 x 17 = 1088 entries and refused by the count pass (min = 2 keeps the FAST probe out), with
    max = 15 they are 64 x 16 = 1024 and fit.  -r: 63 overlapping positions of one 4-byte key in
    a run of 66 bytes, window (15, 15): the C(21, 15) = 54264 ways to place 15 disjoint keys,
    against reverse_pruned.  -s / -s -r have no near side that can be run: 63 distinct patterns
    in any window with max = 15 are at least C(63, 15) = 1.2e14 candidates, and the keyspace of
    these engines walks every candidate for its length."""
    import math
    import table_fuzz as tf
    if mode == 1:
        p = tmp_path / "dp63.table"
        p.write_bytes(b"".join(k + b"=" + v + b"\n" for k, vs in tw.DP63_TABLE.items() for v in vs))
        path, w = str(p), tw.DP63_WORD
    else:
        path, w = tf.corpus("tied").path, bytes(tf.TIED_KEYS[:63])
    c = _mode_ctx(path)
    try:
        if mode == 1:
            got, _ = _mode_run(c, w, mode, 15, 15)
            assert len(got) == math.comb(21, 15) and got == sorted(tw.reverse_pruned(w, tw.DP63_TABLE, 15, 15))
        from hashcat_a5_table_generator_amd import A5xError, pack_words
        data, offs = pack_words([w])
        with pytest.raises(A5xError) as ei:
            c.keyspace(data, offs, mode, 2, 16)
        assert ei.value.code == tw.E_UNSUPPORTED, str(ei.value)
        assert int(c.word_flags(1)[0]) & tw.ERR_BIG
        ok, _ = _mode_run(c, w[:8], mode, 0, 15)  # the context still works
        assert len(ok) >= 1
    finally:
        c.close()
