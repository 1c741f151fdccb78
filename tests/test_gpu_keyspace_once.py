"""GPU keyspace paths of the complex-word kernel (one unit walk per word, cached units)
and of the count pass (count-mode planner), czech+german, against the oracles.

Per word: count and bytes against the oracle (the C oracle's enumeration where the word
can be enumerated, the Python oracle's DP, oracle/a5_oracle.py keyspace_default, for every
word), and the order-independent digest {count, bytes, sum h, sum h^2} of its expansion
against c_oracle.CTable.digest_batch, as tests/test_gpu_parity.py does.  A word with more
than DIGEST_MAX candidates (only the 'e' * 17.. words of the default window, 10^8 and
more candidates each) is compared on count and bytes alone: nothing can enumerate it.
"""
import ctypes
import itertools

import numpy as np
import pytest

from conftest import table_path

pytestmark = pytest.mark.gpu

TABS = ["czech", "german"]
DIGEST_MAX = 1 << 25
FW_TILE_REC = 256 * 40  # csrc/a5x_plan.h


def _alphabet_words():
    # every word over {s, e, t, q} of length 1..7: s / ss / sss.. clusters at the start, middle
    # and end, several per word, next to cluster-free words in the same tiles
    return [bytes(w) for L in range(1, 8) for w in itertools.product(b"setq", repeat=L)]


def _slot_limit_words():
    # complex words on both sides of the lane-slot limit of k_keyspace_cplx (36 bytes)
    ws = []
    for L in (35, 36, 37, 64):
        ws += [b"ss" + b"x" * (L - 4) + b"ss", b"ss" + b"x" * (L - 2), b"x" * (L - 2) + b"ss",
               b"sse" + b"q" * (L - 6) + b"tss", b"sss" + b"x" * (L - 5) + b"ss"]
    return ws


def _cache_overflow_words():
    # more units (8) or clusters (2) than the unit cache of k_keyspace_cplx holds, and words at the limit
    return [b"ss" + b"tx" * 8, b"ss" + b"tx" * 7, b"tx" * 8 + b"ss", b"ssxssxssx", b"ssxssx", b"ssxssxssxssx",
            b"sstetetetete", b"tetetetetess", b"sss" + b"t" * 9, b"ssessesse"]


def _many_unit_words(e_words=True):
    # more than KS_ULOG = 16 lone units: the build pass of k_keyspace_thread walks the word again
    # (e_words: 'e' * 17..40, 3^17.. candidates without a cap on the substitutions)
    ws = [b"t" * k for k in range(15, 22)] + [b"tx" * 17, b"t" * 17 + b"x" * 8, b"xt" * 18]
    return ([b"e" * k for k in range(17, 41)] if e_words else []) + ws


def _tile_edge_words(n):
    base = [b"strasse", b"tet", b"qqqq", b"ss", b"use", b"sss", b"e", b"tessst"]
    return [base[i % len(base)] + bytes([97 + i % 26]) * (i % 5) for i in range(n)]


def _tile_budget_words():
    # 256 words whose records (41 u64 each) overrun the tile's record budget: the last words
    # of the tile fall back to the slow path
    return [b"uuuuuuuu"] * 250 + [b"uu", b"ss", b"uuuuuuuu", b"tet", b"uuuuuuuu", b"e"]


CASES = {
    "alphabet": (_alphabet_words, [(0, 15), (1, 2)]),
    "slot_limit": (_slot_limit_words, [(0, 15), (1, 2)]),
    "cache_overflow": (_cache_overflow_words, [(0, 15), (1, 2)]),
    "many_units": (_many_unit_words, [(0, 15), (1, 2)]),
    # 17+ units inside the window, so the words are FAST and the build pass re-walks them
    "many_units_free": (lambda: _many_unit_words(False), [(0, 40)]),
    "tile_257": (lambda: _tile_edge_words(257), [(0, 15), (1, 2)]),
    "tile_513": (lambda: _tile_edge_words(513), [(0, 15), (1, 2)]),
    "tile_budget": (_tile_budget_words, [(0, 15), (1, 2)]),
}
PARAMS = [(name, mn, mx) for name, (_, wins) in CASES.items() for mn, mx in wins]


@pytest.fixture(scope="module")
def oracles():
    from oracle import a5_oracle as o
    from oracle import c_oracle as co
    paths = [table_path(t) for t in TABS]
    return o, co, o.load_tables(paths), co.CTable(paths)


@pytest.fixture(scope="module")
def ctx():
    from hashcat_a5_table_generator_amd import Context
    c = Context(0)
    c.load_tables([table_path(t) for t in TABS])
    yield c
    c.close()


def _gpu_digests(ctx, data, offs, mn, mx):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    n = len(offs) - 1
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, n, 0, mn, mx)
    out = DeviceBuffer(ctx, max(tb, 16))
    boff = DeviceBuffer(ctx, (n + 1) * 8)
    st = ctx.expand_device(dw.ptr, do.ptr, n, out.ptr, tb, 0, mn, mx, d_byte_off=boff.ptr)
    assert st["candidates"] == tc and st["bytes"] == tb
    dig = DeviceBuffer(ctx, n * 32)
    ctx.digest_device(out.ptr, boff.ptr, 0, n, dig.ptr)
    return dig.to_array(np.uint64).reshape(n, 4)


@pytest.mark.parametrize("name,mn,mx", PARAMS)
def test_keyspace_once(ctx, oracles, name, mn, mx):
    from hashcat_a5_table_generator_amd import pack_words
    o, co, sub, ctab = oracles
    words = CASES[name][0]()
    data, offs = pack_words(words)
    cnt, byt = ctx.keyspace(data, offs, 0, mn, mx)
    for i, w in enumerate(words):  # the DP of the Python oracle
        assert (int(cnt[i]), int(byt[i])) == o.keyspace_default(w, sub, mn, mx), (name, w, mn, mx)
    keep = [i for i in range(len(words)) if int(cnt[i]) <= DIGEST_MAX]
    assert len(keep) == len(words) or (name == "many_units" and (mn, mx) == (0, 15))
    if len(keep) != len(words):
        data, offs = pack_words([words[i] for i in keep])
    want = ctab.digest_batch(data, offs, 0, mn, mx)
    assert np.array_equal(want[:, 0], cnt[keep]) and np.array_equal(want[:, 1], byt[keep])
    got = _gpu_digests(ctx, data, offs, mn, mx)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(words[keep[i]], got[i], want[i]) for i in bad[:5]]


def test_tile_budget_case_overruns_the_tile():
    """(CPU part of the tile_budget case: its records do not fit one tile's budget.)"""
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.a5x_create(-1, ctypes.byref(h)) == 0
    for t in TABS:
        assert L.a5x_load_table_file(h, table_path(t).encode()) == 0
    out = np.zeros(40, dtype=np.uint32)
    total = 0
    for w in _tile_budget_words()[:256]:
        wb = np.frombuffer(w + b"\0", dtype=np.uint8)
        assert L.a5x_debug_plan_sizes(h, wb.ctypes.data, len(w), out.ctypes.data) == 0
        if out[16]:  # groups of <= 8 entries (k_keyspace_thread): 1 + np + ne
            total += 1 + int(out[17]) + int(out[19])
    L.a5x_destroy(h)
    assert total > FW_TILE_REC
