"""The target set as the host builds it (build_target_set through a5x_debug_target_set) against
a plain reference lookup, without a GPU: sizing, slot and bitmap contents of random sets from
0 to 100 000 targets, and the claims of the adversarial constructors of target_sets.py (near
misses inside a real digest's probe chain, displaced targets behind chains that wrap from the
last slot to slot 0, wide chains with shared prefixes, zero digests, degenerate sets).  The GPU
suite (test_gpu_target_set.py) runs every route over the same constructed sets."""
import numpy as np
import pytest

import target_sets as ts

WIDTHS = pytest.mark.parametrize("W", [16, 20, 32, 64])
E_ARG, E_CAPACITY = -1, -8

_cache = {}


def _digests(W, tag, n):
    """n distinct real digests of short strings (hashlib), W bytes each"""
    key = (W, tag, n)
    if key not in _cache:
        f = ts.WIDTHS[W]
        _cache[key] = [f(b"%s-%d" % (tag, i)).digest() for i in range(n)]
        assert len(set(_cache[key])) == n
    return _cache[key]


def _others(W):
    return _digests(W, b"other", 10_000)


def _random_set(W, n):
    """n targets, the largest size with 10 % duplicates mixed in"""
    if n < 100_000:
        return _digests(W, b"target", n)
    distinct = _digests(W, b"target", n - n // 10)
    rng = np.random.default_rng(n + W)
    out = distinct + [distinct[int(i)] for i in rng.integers(0, len(distinct), size=n // 10)]
    return [out[int(i)] for i in rng.permutation(len(out))]


def _expected_bitmap(S, targets):
    arr = np.frombuffer(b"".join(t[:16] for t in targets), dtype="<u4").reshape(-1, 4)
    arr = arr[arr.any(axis=1)]
    exp = np.zeros((1 << S.bm_log2) // 64, dtype=np.uint64)
    d0, d3 = arr[:, 0].astype(np.uint64), arr[:, 3].astype(np.uint64)
    one = np.uint64(1)
    bits = (one << (d3 & np.uint64(63))) | (one << ((d3 >> np.uint64(6)) & np.uint64(63)))
    np.bitwise_or.at(exp, ((d0 & np.uint64((1 << S.bm_log2) - 1)) >> np.uint64(6)).astype(np.int64), bits)
    return exp


def _check_layout(S, targets):
    """sizing, slots and bitmap of the set S built from targets"""
    n, tset = len(targets), set(targets)
    assert S.size == ts.table_size(n) and S.size >= 16 and S.size >= 2 * n and (S.size == 16 or S.size // 2 < 2 * n)
    assert S.bm_log2 == ts.prefilter_log2(n) and (S.bm_log2 == 16 or (1 << (S.bm_log2 - 1)) < 64 * n)
    ent = S.entries()
    nonzero = {t for t in tset if any(t[:16])}
    assert len(ent) == len(set(ent))      # no (prefix, tail) pair twice
    assert set(ent) == nonzero            # every slot holds a target, every target has a slot
    assert set(S.zero_entries()) == ({t for t in tset if not any(t[:16])} if S.TW else set())
    assert S.has_zero == (1 if len(nonzero) < len(tset) else 0)
    assert np.array_equal(S.bitmap, _expected_bitmap(S, targets))
    pre = [t[:16] for t in nonzero]
    assert S.shared == (1 if S.TW and len(set(pre)) < len(pre) else 0)


@WIDTHS
@pytest.mark.parametrize("n", [0, 1, 8, 9, 1000, 100_000])
def test_random_sets(W, n):
    targets = _random_set(W, n)
    tset = set(targets)
    S = ts.Dump(W, targets)
    _check_layout(S, targets)
    assert {0: 16, 1: 16, 8: 16, 9: 32, 1000: 2048, 100_000: 262144}[n] == S.size
    assert {0: 16, 1: 16, 8: 16, 9: 16, 1000: 16, 100_000: 23}[n] == S.bm_log2
    missed = [t.hex() for t in tset if not ts.lookup(S, t)[0]]
    assert not missed, missed[:3]
    false = [o.hex() for o in _others(W) if ts.lookup(S, o)[0]]
    assert not false, false[:3]
    # single-bit neighbours of 64 targets, 128 flips each over the whole width
    rng = np.random.default_rng(W + n)
    some = sorted(tset)[:: max(1, len(tset) // 64)][:64]
    for t in some:
        for bit in rng.choice(8 * W, size=min(128, 8 * W), replace=False):
            x = ts.flip(t, int(bit))
            assert ts.lookup(S, x)[0] == (x in tset), (t.hex(), int(bit))
    assert not ts.lookup(S, bytes(W))[0]


def _real(W):
    return _digests(W, b"real", 400)


@WIDTHS
def test_near_misses_sit_in_the_chain_and_never_hit(W):
    real = _real(W)
    N, D = real[0], real[1]
    forged = ts.near_misses(N, 8)
    assert len(forged) == {16: 4, 20: 5}.get(W, 6)
    for targets in (forged + [D], forged, forged + real[1:9 - len(forged)]):  # 16 slots, the last at load 1/2
        assert len(targets) <= 8
        S = ts.Dump(W, targets)
        assert S.size == 16
        _check_layout(S, targets)
        ts.check_near_misses(S, N, forged)
        assert all(ts.lookup(S, t)[0] for t in targets)
        assert not ts.lookup(S, N)[0]
    # the same at a table of another size: the word 1 / word 2 bits are searched for it
    more = real[1:300]
    forged = ts.near_misses(N, 6 + len(more))
    S = ts.Dump(W, forged + more)
    assert S.size == 1024
    ts.check_near_misses(S, N, forged)


@WIDTHS
@pytest.mark.parametrize("wraps", [True, False], ids=["wrapped", "straight"])
def test_chain_displaces_the_target(W, wraps):
    real = _real(W)
    k = 7
    D = ts.pick_home(real, 16, 9, 15) if wraps else ts.pick_home(real, 16, 0, 8)
    targets = ts.chain(D, k)
    assert len(targets) == 8
    S = ts.Dump(W, targets)
    assert S.size == 16
    _check_layout(S, targets)
    ts.check_chain(S, D, k, wraps)
    assert all(ts.lookup(S, t) == (True, j) for j, t in enumerate(targets))
    # without D the walk passes the whole chain and ends on the empty slot behind it
    S2 = ts.Dump(W, targets[:-1])
    assert ts.lookup(S2, D) == (False, k)
    # how scarce such digests are is no accident of these 400: about half have a high home slot
    high = sum(1 for d in real if ts.home_slot(d, 16) >= 9)
    assert 100 < high < 300


@pytest.mark.parametrize("W", [20, 32, 64])
@pytest.mark.parametrize("wraps", [True, False], ids=["wrapped", "straight"])
def test_wide_chain(W, wraps):
    real = _real(W)
    k = 5
    D = ts.pick_home(real, 16, 11, 15) if wraps else ts.pick_home(real, 16, 0, 10)
    targets = ts.wide_chain(D, k)
    assert len(targets) == 8
    S = ts.Dump(W, targets)
    assert S.size == 16 and S.shared == 1 and S.has_zero == 1 and len(S.ztails) == 2
    _check_layout(S, targets)
    ts.check_chain(S, D, k, wraps)
    for j, t in enumerate(targets[:k + 1]):
        assert ts.lookup(S, t) == (True, j)
    # the entries with D's prefix and another tail are displaced themselves
    assert [ts.lookup(S, t)[1] for t in targets if t[:16] == D[:16]] == list(range(k // 2, k + 1))
    assert ts.lookup(S, targets[-2])[0] and ts.lookup(S, targets[-1])[0]
    # D's prefix with a tail that is not listed: the walk goes past every equal prefix
    assert ts.lookup(S, D[:16] + bytes(W - 16)) == (False, k + 1)
    S2 = ts.Dump(W, [t for t in targets if t != D])
    assert ts.lookup(S2, D) == (False, k)


@WIDTHS
def test_degenerate_sets(W):
    real = _real(W)
    D = real[5]
    sets = ts.degenerate(D, real[10:30])
    sizes = {"empty": 16, "one": 16, "nine_copies": 32, "eight": 16, "nine": 32, "with_zero": 16}
    assert set(sets) == set(sizes)
    for name, targets in sets.items():
        S = ts.Dump(W, targets)
        assert S.size == sizes[name], name
        _check_layout(S, targets)
        assert len(S.entries()) == len({t for t in targets if any(t[:16])})
        assert ts.lookup(S, D)[0] == (name != "empty")
        assert all(ts.lookup(S, t)[0] for t in targets)
        assert not any(ts.lookup(S, o)[0] for o in real[40:] if o not in targets)
        assert ts.lookup(S, bytes(W))[0] == (name == "with_zero")
    S = ts.Dump(W, [])
    assert not S.bitmap.any() and not S.table.any() and S.has_zero == 0


@WIDTHS
def test_zero_targets(W):
    real = _real(W)
    zero = bytes(W)
    S = ts.Dump(W, real[:5])
    assert S.has_zero == 0 and not ts.lookup(S, zero)[0]
    S = ts.Dump(W, real[:5] + [zero])
    assert S.has_zero == 1 and ts.lookup(S, zero)[0]
    assert len(S.entries()) == 5  # the zero digest takes no slot and sets no bit
    assert np.array_equal(S.bitmap, ts.Dump(W, real[:5]).bitmap)
    if W == 16:
        assert S.ztails.size == 0
        return
    # a zero-prefix target is in the side list, not in the table; the all-zero digest is found
    # only when its tail is listed
    zp = bytes(16) + real[7][16:]
    S = ts.Dump(W, real[:5] + [zp])
    assert S.has_zero == 1 and len(S.entries()) == 5 and S.zero_entries() == [zp]
    assert ts.lookup(S, zp)[0] and not ts.lookup(S, zero)[0]
    assert not ts.lookup(S, bytes(16) + real[8][16:])[0]
    S = ts.Dump(W, [zp, zero] + real[:5] + [zp])
    assert S.zero_entries() == [zp, zero, zp] and ts.lookup(S, zero)[0] and ts.lookup(S, zp)[0]


def test_prefilter_size_hook(monkeypatch):
    """A5X_TARGET_BM_LOG2 is honoured (clamped to 16..32), as a5x_set_targets honours it."""
    real = _real(16)
    for env, want in (("20", 20), ("3", 16), ("24", 24)):
        monkeypatch.setenv("A5X_TARGET_BM_LOG2", env)
        S = ts.Dump(16, real[:50])
        assert S.bm_log2 == want and S.size == 128
        assert np.array_equal(S.bitmap, _expected_bitmap(S, real[:50]))
        assert all(ts.lookup(S, t)[0] for t in real[:50]) and not any(ts.lookup(S, t)[0] for t in real[50:])


def test_hook_arguments():
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    real = _real(32)
    dig = np.frombuffer(b"".join(real[:9]) + bytes([0] * 32), dtype=np.uint8)
    info = np.zeros(8, dtype=np.uint64)
    bufs = [np.zeros(k, dtype=np.uint32) for k in (32 * 4, 32 * 4, 4, (1 << 16) // 32)]

    def call(width=32, d=dig.ctypes.data, n=9, inf=info.ctypes.data, caps=None, ptrs=None):
        caps = caps or [len(b) for b in bufs]
        ptrs = ptrs or [b.ctypes.data for b in bufs]
        args = [x for pc in zip(ptrs, caps) for x in pc]
        return L.a5x_debug_target_set(width, d, n, inf, *args)

    for bad in (0, 4, 15, 17, 24, 40, 65, 128):
        assert call(width=bad) == E_ARG, bad
    assert call(d=None) == E_ARG and call(inf=None) == E_ARG
    assert call(d=None, n=0) == 0 and list(info[:4]) == [16, 16, 0, 0]
    # the size query: no buffer at all
    assert call(ptrs=[None] * 4, caps=[0] * 4) == 0
    assert list(info) == [16, 32, 0, 0, 128, 128, 0, 2048]
    # a needed buffer missing: the table, the bitmap, the tails of a wide set
    for k in (0, 1, 3):
        ptrs = [b.ctypes.data for b in bufs]
        ptrs[k] = None
        assert call(ptrs=ptrs) == E_ARG, k
    ptrs = [b.ctypes.data for b in bufs]
    ptrs[2] = None  # (no zero-prefix target: the side list is empty and needs no buffer)
    assert call(ptrs=ptrs) == 0
    for k in (0, 1, 3):
        caps = [len(b) for b in bufs]
        caps[k] -= 1
        for b in bufs:
            b[:] = 0
        assert call(caps=caps) == E_CAPACITY, k
        assert not any(b.any() for b in bufs)  # nothing written
        assert list(info) == [16, 32, 0, 0, 128, 128, 0, 2048]
    assert call() == 0 and bufs[0].any() and bufs[1].any() and bufs[3].any()
    # a side list that does not fit
    zp = np.frombuffer(bytes(16) + real[0][16:] + bytes(32), dtype=np.uint8)
    assert call(d=zp.ctypes.data, n=1, caps=[128, 128, 3, 2048]) == E_CAPACITY and info[6] == 4
    ptrs = [b.ctypes.data for b in bufs]
    ptrs[2] = None
    assert call(d=zp.ctypes.data, n=1, ptrs=ptrs) == E_ARG
    assert call(d=zp.ctypes.data, n=1) == 0 and bufs[2].tobytes() == real[0][16:]
    # every width the library has
    for W in (16, 20, 28, 32, 48, 64):
        S = ts.Dump(W, [bytes(range(1, W + 1))])
        assert S.size == 16 and S.tails.shape == (16, W // 4 - 4) and ts.lookup(S, bytes(range(1, W + 1))) == (True, 0)
    with pytest.raises(_lib.A5xError):
        _lib.debug_target_set(32, bytes(33))
