"""The count-mode planner of the keyspace count pass (csrc/a5x_plan.h CountPlanner) against
the build-mode planner, on the CPU.

k_keyspace_thread sizes a word's record with CountPlanner (np, ng, ne and the FAST
decision's maxl, minl, nbig, bent) and builds it with Planner<true>; the two must cut
every word into the same pieces.  a5x_debug_plan_sizes runs both over the same unit walk,
with groups of <= 16 entries (the general planner) and of <= 8 (k_keyspace_thread), and
also plans the word from the cached units of one walk (k_keyspace_cplx) against the
two-walk record.
"""
import ctypes
import itertools
import random

import numpy as np
import pytest

from conftest import table_path

FIELDS = ("ok", "np", "ng", "ne", "maxl", "minl", "nbig", "bent")
SHIPPED = [("czech", "german"), ("qwerty-cyrillic",), ("qwerty-azerty",), ("qwerty-greek",), ("greek-hebrew",),
           ("czech",), ("german",)]


class Sizes:
    def __init__(self, tables=None, table_map=None):
        from hashcat_a5_table_generator_amd import _lib
        self.L = _lib.load()
        self.h = ctypes.c_void_p()
        assert self.L.a5x_create(-1, ctypes.byref(self.h)) == 0
        if tables:
            for t in tables:
                assert self.L.a5x_load_table_file(self.h, table_path(t).encode()) == 0
        else:
            txt = b"".join(k + b"=" + v + b"\n" for k, vs in table_map.items() for v in vs)
            assert self.L.a5x_parse_table(self.h, txt, len(txt)) == 0, self.L.a5x_last_error(self.h)
        self.out = np.zeros(40, dtype=np.uint32)

    def check(self, word: bytes):
        """Both planners agree on the word; returns (ok with 16-entry groups, cached-walk verdict)."""
        wb = np.frombuffer(word + b"\0", dtype=np.uint8)
        rc = self.L.a5x_debug_plan_sizes(self.h, wb.ctypes.data, len(word), self.out.ctypes.data)
        assert rc == 0, self.L.a5x_last_error(self.h)
        o = [int(x) for x in self.out]
        for cap, r in ((16, 0), (8, 16)):
            cnt, bld = o[r:r + 8], o[r + 8:r + 16]
            assert cnt[0] == bld[0], (word, cap, dict(zip(FIELDS, cnt)), dict(zip(FIELDS, bld)))
            if cnt[0]:
                assert cnt == bld, (word, cap, dict(zip(FIELDS, cnt)), dict(zip(FIELDS, bld)))
        assert o[32] in (1, 2, 3), (word, "record from the cached units differs from the two-walk record")
        return o[0], o[32]

    def close(self):
        self.L.a5x_destroy(self.h)


def test_count_mode_small_alphabet_exhaustive():
    """Every word over {s, e, u, t, q} of length 1..6 on czech+german (19,530 words)."""
    c = Sizes(("czech", "german"))
    n = ok = cached = 0
    for L in range(1, 7):
        for w in itertools.product(b"seutq", repeat=L):
            a, b = c.check(bytes(w))
            n += 1
            ok += a
            cached += b == 1
    c.close()
    assert n == sum(5 ** k for k in range(1, 7))
    assert ok > n // 2 and cached > n // 2


@pytest.mark.parametrize("tables", SHIPPED)
def test_count_mode_shipped_tables_random_words(tables):
    from oracle import a5_oracle as o
    c = Sizes(tables)
    sub = o.load_tables([table_path(t) for t in tables])
    rng = random.Random(",".join(tables))
    alpha = [k for k in sub if len(k) <= 2] + [b"a", b"b", b"q", b"x", b"1", b" ", b"s", b"e"]
    ok = 0
    for i in range(2000):
        # (short words merge units into groups; long ones split literal runs and fill big pieces)
        n = rng.randint(0, 12) if i % 4 else rng.randint(13, 40)
        w = b"".join(rng.choice(alpha) if rng.random() < 0.5 else b"x" for _ in range(n))[:64]
        ok += c.check(w)[0]
    c.close()
    assert ok > 500


def test_count_mode_literal_runs():
    """Literal runs of every length before, between and after units (the closed-form splitting)."""
    c = Sizes(("czech", "german"))
    for a in range(0, 24):
        for b in range(0, 24):
            if a + b + 3 <= 64:
                for u in (b"e", b"ss", b"t"):
                    c.check(b"x" * a + u + b"x" * b)
                    c.check(u + b"x" * a + u + b"x" * b)
    c.close()
    # a one-byte unit with one-byte values: the open big piece takes two 7-byte literal pieces
    c = Sizes(table_map={b"a": [b"b"], b"c": [b"d", b""]})
    for a in range(0, 30):
        for b in range(0, 30):
            c.check(b"a" + b"x" * a + b"c" + b"x" * b)
            c.check(b"x" * a + b"ac" + b"x" * b + b"a")
    c.close()


def test_count_mode_random_tables_with_overlaps():
    """The random overlapping tables of tests/test_plan.py."""
    rng = random.Random(7)
    ok = 0
    for _ in range(150):
        m = {}
        for _ in range(rng.randint(1, 5)):
            k = bytes(rng.choice(b"abs") for _ in range(rng.randint(1, 3)))
            m.setdefault(k, []).append(bytes(rng.choice(b"absxyz") for _ in range(rng.randint(0, 3))))
        c = Sizes(table_map=m)
        for _ in range(12):
            w = bytes(rng.choice(b"abs") for _ in range(rng.randint(0, 10)))
            ok += c.check(w)[0]
        for _ in range(6):
            w = bytes(rng.choice(b"absxxxxx") for _ in range(rng.randint(10, 40)))
            ok += c.check(w)[0]
        c.close()
    assert ok > 500


def test_cached_walk_paths():
    """One-walk records: resident cluster choices, two clusters, more clusters or units than the cache holds."""
    c = Sizes(("czech", "german"))
    assert c.check(b"strasse")[1] == 1       # one cluster: its choices stay in the buffer
    assert c.check(b"ssxssx")[1] == 1        # two clusters: the first is enumerated again
    assert c.check(b"ssxssxssx")[1] == 2     # three clusters: not cached
    assert c.check(b"txtxtxtxtxtxtxtxtx")[1] == 2  # nine units: not cached
    assert c.check(b"txtxtxtxtxtxtxtx")[1] == 1    # eight units
    assert c.check(b"qqq")[1] == 3           # no units, no record
    c.close()
