"""k_keyspace_cplx's lean path on the GPU: small batches of complex words at the lean path's
limits mixed with plain words, czech+german and the "clusters" fuzz table.

Per word: count and bytes against the C oracle's, the order-independent digest {count, bytes,
sum h, sum h^2} of its expansion against c_oracle.CTable.digest_batch (the pattern of
tests/test_gpu_keyspace_once.py), and through a5x_debug_keyspace_cplx_lean the number of words
the kernel took by its lean path and by the generic one against the CPU hook's prediction
(a5x_debug_cplx_build, tests/test_plan_cplx_build.py): the words k_keyspace_thread hands over
are those with a cluster, a lone unit of more than 8 choices or a key longer than 4 bytes.
"""
import numpy as np
import pytest

import table_fuzz as tf
import test_plan_cplx_build as cb
from conftest import table_path

pytestmark = pytest.mark.gpu

TABS = ["czech", "german"]


def _cg_words():
    ws = []
    for run in (b"ss", b"sss", b"ssss", b"sssss"):
        ws += [run, run + b"xyz", b"xyz" + run, b"xy" + run + b"zw", b"q" + run, run + b"q"]
    ws += [b"ssxss", b"ssxxxxxxxxss", b"ssxssxss", b"ssxssxssxss", b"sst", b"tss", b"ess", b"sse", b"tsst", b"usssu",
           b"strasse", b"wasserschloss", b"x" * 34 + b"ss", b"x" * 35 + b"ss", b"ss" + b"x" * 35, b"ss" + b"x" * 60 + b"ss",
           b"sstetetetete", b"tetetetetess", b"ss" + b"tx" * 8, b"ss" + b"t" * 15, b"ss" + b"t" * 16, b"ssqssq"]
    plain = [b"tet", b"qqqq", b"use", b"e", b"haus", b"x", b"strom", b"", b"zluty", b"kun"]
    out = []
    for i in range(900):  # four tiles: every complex word next to plain ones, at changing lanes
        out.append(ws[i % len(ws)] if i % 3 == 0 else plain[i % len(plain)] + bytes([97 + i % 26]) * (i % 4))
    return out


def _predict(hook, table, words, mn, mx):
    """(lean, generic) words of k_keyspace_cplx by the CPU hook"""
    lean = gen = 0
    for w in words:
        f = tf.facts(table, w)
        longkey = any(len(k) > 4 and k[0] == w[q] and q + len(k) <= len(w) for q in range(len(w)) for k in table)
        if not (f["clusters"] or f["maxR_lone"] > 8 or longkey):
            continue
        r = hook.check(w, mn, mx)
        assert r["agree"] == 1, (w, r)
        lean += r["why"] == 0
        gen += r["why"] != 0
    return lean, gen


def _gpu_digests(ctx, data, offs, mn, mx):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    n = len(offs) - 1
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, n, 0, mn, mx)
    lean = ctx.keyspace_cplx_lean()
    out = DeviceBuffer(ctx, max(tb, 16))
    boff = DeviceBuffer(ctx, (n + 1) * 8)
    st = ctx.expand_device(dw.ptr, do.ptr, n, out.ptr, tb, 0, mn, mx, d_byte_off=boff.ptr)
    assert st["candidates"] == tc and st["bytes"] == tb
    dig = DeviceBuffer(ctx, n * 32)
    ctx.digest_device(out.ptr, boff.ptr, 0, n, dig.ptr)
    return dig.to_array(np.uint64).reshape(n, 4), lean


def _check(ctx, ctab, hook, table, words, mn, mx):
    from hashcat_a5_table_generator_amd import pack_words
    assert len(words) <= 2048
    data, offs = pack_words(words)
    want = ctab.digest_batch(data, offs, 0, mn, mx)
    cnt, byt = ctx.keyspace(data, offs, 0, mn, mx)
    assert np.array_equal(want[:, 0], cnt) and np.array_equal(want[:, 1], byt)
    got, lean = _gpu_digests(ctx, data, offs, mn, mx)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(words[i], got[i], want[i]) for i in bad[:5]]
    assert lean == _predict(hook, table, words, mn, mx), lean
    assert lean[0] > 0 and lean[1] > 0, lean


@pytest.mark.parametrize("mn,mx", [(0, 15), (1, 2)])
def test_czech_german(mn, mx):
    from hashcat_a5_table_generator_amd import Context
    from oracle import a5_oracle as o
    from oracle import c_oracle as co
    paths = [table_path(t) for t in TABS]
    ctx = Context(0)
    ctx.load_tables(paths)
    hook = cb.Hook(tables=TABS)
    try:
        _check(ctx, co.CTable(paths), hook, o.load_tables(paths), _cg_words(), mn, mx)
    finally:
        hook.close()
        ctx.close()


def test_clusters_table():
    from hashcat_a5_table_generator_amd import Context
    c = tf.corpus("clusters")
    words = [w for w in c.words if len(w) <= 64]
    words = (words + [b"k.k", b"...", b"xyz"] * 40)[:2048]
    ctx = Context(0)
    ctx.load_tables([c.path])
    hook = cb.Hook(path=c.path)
    try:
        _check(ctx, tf.c_table(c), hook, c.table, words, 0, 15)
    finally:
        hook.close()
        ctx.close()
