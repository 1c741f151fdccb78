"""Iterated target lists on the GPU (k_pbkdf2_init / _loop / _compare, a5x_pbkdf2.hip) against
hashlib.pbkdf2_hmac: the 16 compared bytes of every (line, index) pair of a hand-built stream
under six (salt, iterations) pairs that mix counts in one pass; the same with the pass and
launch budgets forced small (several passes, the salt table cut mid-way, the loop sliced), with
the loop launch count the budgets imply; planted targets end to end in two modes with a near miss
on the count; more hits than the device hit buffer's first size, the iterations run once; the
host's check of the whole key in format_hits_iterated; and the CLI."""
import base64
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, table_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "hashcat_a5_table_generator_amd", "_build", "a5x_generator")
MD5 = 0
BLOCK = 4096  # STREAM_BLK of a5x_stream.h
LMAX = 128
HASH = {72: "md5", 73: "sha1", 74: "sha256", 75: "sha512"}
HLEN = {72: 16, 73: 20, 74: 32, 75: 64}
NAME = {a: "pbkdf2-hmac-" + HASH[a] for a in HASH}
ALGOS = pytest.mark.parametrize("algo", sorted(NAME), ids=[NAME[a] for a in sorted(NAME)])


def ref(algo, p, s, c, dklen=16):
    return hashlib.pbkdf2_hmac(HASH[algo], p, s, c, dklen)


def line_of(algo, s, c, dk):
    return b"%s:%d:%s:%s" % (HASH[algo].encode(), c, base64.b64encode(s), base64.b64encode(dk))


@pytest.fixture(autouse=True)
def _no_salts_left_behind(gpu_ctx):
    yield
    gpu_ctx.iter_budget(0, 0)
    gpu_ctx.set_targets(MD5, hashlib.md5(b"").digest())
    assert gpu_ctx.salt_count() == 0


def _salt(n, seed):
    return bytes((1 + (i * 37 + seed * 101 + n * 7) % 255) for i in range(n))


# salt . INT(1) is one block up to 51 bytes and two from 52 (SHA-512: one); the counts mix in one
# pass; the records are sorted by salt length, which is this order
SALTS = [_salt(n, 7) for n in (0, 1, 51, 52, 60, 64)]
ITERS = [1, 2, 3, 17, 1000, 1]
CAND_LENS = [0, 1, 55, 56, 63, 64, 65, 111, 112, 127, 128]

_cache = {}


def _stream(ctx):
    """The hand-built "cand\\n" stream: lines of the candidate lengths (the empty line among them),
    a 129-byte line, filler up to a line that straddles the 4096-byte block edge, and a last line
    with no newline; on the device once.  -> (buffer, bytes, lines, lines per block)"""
    from hashcat_a5_table_generator_amd import DeviceBuffer
    if "stream" in _cache:
        return _cache["stream"]
    body = lambda n, k: bytes(1 + (i * 29 + n * 13 + k * 7 + 3) % 255 for i in range(n)).replace(b"\n", b"\x0b")
    lines = [body(n, 0) for n in CAND_LENS] + [body(129, 0)]
    pos = sum(len(x) + 1 for x in lines)
    k = 0
    while pos + 41 < BLOCK - 20:
        k += 1
        lines.append(body(40, k))
        pos += 41
    assert BLOCK - 100 < pos < BLOCK
    lines.append(body(100, 99))  # starts before the edge, ends behind it
    lines += [body(7, 1), b"", body(128, 5), body(200, 1), body(33, 2)]
    stream = b"".join(x + b"\n" for x in lines)[:-1]  # the last line has no newline
    starts = np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])[:-1]
    assert BLOCK < len(stream) < 2 * BLOCK and any(s < BLOCK < s + len(x) for s, x in zip(starts, lines))
    per_block = [int(((starts >= b) & (starts < b + BLOCK)).sum()) for b in (0, BLOCK)]
    assert sum(per_block) == len(lines) and 64 < per_block[0] <= 128 and 0 < per_block[1] <= 64
    buf = DeviceBuffer.from_array(ctx, np.frombuffer(stream + b"\0" * 64, dtype=np.uint8))
    _cache["stream"] = (buf, len(stream), lines, per_block)
    return _cache["stream"]


def _expected(algo, lines):
    if ("exp", algo) not in _cache:
        _cache[("exp", algo)] = [[ref(algo, ln, s, c) if len(ln) <= LMAX else bytes(16) for s, c in zip(SALTS, ITERS)]
                                 for ln in lines]
    return _cache[("exp", algo)]


def _digests(ctx, algo):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    buf, nbytes, lines, _ = _stream(ctx)
    S = len(SALTS)
    ctx.set_iterated_targets(algo, b"".join(ref(algo, b"", s, c) for s, c in zip(SALTS, ITERS)), SALTS, ITERS)
    assert ctx.salt_count() == S
    assert [(ctx.salt(i), ctx.salt_iterations(i)) for i in range(S)] == list(zip(SALTS, ITERS))
    dig = DeviceBuffer(ctx, 16 * len(lines) * S + 16)
    n = ctx.digest_lines_salted_device(algo, 0, buf.ptr, nbytes, dig.ptr, len(lines) * S)
    assert n == len(lines)
    return dig.to_array(count=16 * n * S).reshape(n, S, 16).copy(), lines


def _check(algo, got, lines):
    exp = _expected(algo, lines)
    bad = [(len(ln), s, bytes(got[i, s]).hex(), exp[i][s].hex())
           for i, ln in enumerate(lines) for s in range(len(SALTS)) if bytes(got[i, s]) != exp[i][s]]
    assert not bad, (len(bad), bad[:5])


@ALGOS
def test_every_pair(gpu_ctx, algo):
    gpu_ctx.iter_budget(0, 0)
    got, lines = _digests(gpu_ctx, algo)
    _check(algo, got, lines)
    S = len(SALTS)
    over = sum(1 for ln in lines if len(ln) > LMAX)
    assert over == 2 and gpu_ctx.salts_last() == ((len(lines) - over) * S, over * S)
    # one pass of both blocks under every record, one loop launch up to the largest count
    assert gpu_ctx.iter_budget(0, 0) == 1


def _plan(per_block, iters, P, B):
    """The passes the budgets imply (DESIGN "Iterated target lists"): blocks are taken while their
    lines, rounded up to 64, fit P slots under every record; else one run of blocks under a slice
    of the records at a time; a pass's loop runs in slices of max(1, B // pairs) iterations up to
    its largest count.  -> [((b0, b1, s0, s1), loop launches)]"""
    S, nblk = len(iters), len(per_block)
    pre = [0]
    for n in per_block:
        pre.append(pre[-1] + n)
    slots = lambda n: (n + 63) // 64 * 64
    out, b0 = [], 0
    while b0 < nblk:
        b1 = b0 + 1
        while b1 < nblk and slots(pre[b1 + 1] - pre[b0]) * S <= P:
            b1 += 1
        n = pre[b1] - pre[b0]
        if n:
            ns = min(S, max(1, P // slots(n)))
            for s0 in range(0, S, ns):
                s1 = min(S, s0 + ns)
                pairs, cmax = (s1 - s0) * slots(n), max(iters[s0:s1])
                out.append(((b0, b1, s0, s1), -(-(cmax - 1) // max(1, B // pairs))))
        b0 = b1
    return out


@ALGOS
def test_sliced_passes_give_the_same(gpu_ctx, algo):
    _, _, lines, per_block = _stream(gpu_ctx)
    P, B = 300, 1024
    plan = _plan(per_block, ITERS, P, B)
    assert P < len(lines) * len(SALTS)
    # block 0 under two records at a time, block 1 under four and two: the table is cut mid-way
    assert [p for p, _ in plan] == [(0, 1, 0, 2), (0, 1, 2, 4), (0, 1, 4, 6), (1, 2, 0, 4), (1, 2, 4, 6)]
    assert plan[1][1] == 4  # c = 17 (with c = 3 beside it): 16 iterations in four launches of four
    assert [n for _, n in plan] == [1, 4, 250, 4, 125]
    gpu_ctx.iter_budget(P, B)
    got, lines = _digests(gpu_ctx, algo)
    assert gpu_ctx.iter_budget(0, 0) == sum(n for _, n in plan)
    _check(algo, got, lines)
    S = len(SALTS)
    assert gpu_ctx.salts_last() == ((len(lines) - 2) * S, 2 * S)
    # the unsliced run again: identical bytes
    again, _ = _digests(gpu_ctx, algo)
    assert gpu_ctx.iter_budget(0, 0) == 1 and np.array_equal(again, got)


def test_digest_lines_wants_the_sets_own_algorithm(gpu_ctx):
    from hashcat_a5_table_generator_amd import A5xError, DeviceBuffer
    buf, nbytes, lines, _ = _stream(gpu_ctx)
    dig = DeviceBuffer(gpu_ctx, 64 * len(lines) + 16)
    gpu_ctx.set_iterated_targets(73, ref(73, b"x", b"s", 2), [b"s"], [2])
    for algo, order in ((72, 0), (74, 0), (73, 1), (50, 0), (MD5, 0)):
        with pytest.raises(A5xError) as e:
            gpu_ctx.digest_lines_salted_device(algo, order, buf.ptr, nbytes, dig.ptr, len(lines))
        assert e.value.code == -1, (algo, order)
    gpu_ctx.set_salted_targets(50, 0, bytes(20), [b"s"])
    with pytest.raises(A5xError) as e:  # 72..75 on another kind of set
        gpu_ctx.digest_lines_salted_device(73, 0, buf.ptr, nbytes, dig.ptr, len(lines))
    assert e.value.code == -1


FILLER = list(b"bfghjklmpqvwxBFGH 19-")  # no key or value of the czech table
TOKENS = [b"a", b"e", b"s", b"A", b"S", b"z", "á".encode(), "š".encode(), "é".encode()]


def _words(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        parts = [bytes([int(c)]) for c in rng.choice(FILLER, size=int(rng.integers(3, 12)))]
        for _ in range(int(rng.integers(1, 4))):
            parts.insert(int(rng.integers(0, len(parts) + 1)), TOKENS[int(rng.integers(0, len(TOKENS)))])
        out.append(b"".join(parts))
    return out + [b"", b"a", b"a" + b"x" * 139]


def _per_word(ctx, mode):
    ctx.clear_table()
    ctx.load_tables([table_path("czech")])
    if ("pw", mode) not in _cache:
        words = _words(40 + mode, 40)
        _cache[("pw", mode)] = (words, ctx.expand_words(words, mode, 0, 15))
    return _cache[("pw", mode)]


E2E = [(72, 0), (73, 3), (74, 0), (75, 3), (75, 0)]


@pytest.mark.parametrize("algo,mode", E2E, ids=[f"{NAME[a]}-mode{m}" for a, m in E2E])
def test_end_to_end_planted(gpu_ctx, algo, mode):
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    words, per_word = _per_word(gpu_ctx, mode)
    flat = [(w, c) for w, cs in enumerate(per_word) for c, x in enumerate(cs) if len(x) <= LMAX]
    ncand = sum(len(cs) for cs in per_word)
    over = ncand - len(flat)
    assert over >= 1 and len(flat) > 60
    A, B = (b"NaCl", 5), (b"0123456789abcdef" * 4, 64)  # two salts with different counts
    near = (A[0], A[1] + 1)                              # the right salt, the count off by one
    digs, salts, iters = [], [], []
    planted = flat[:: max(1, len(flat) // 24)][:30]
    for k, (w, c) in enumerate(planted):
        s, n = A if k % 2 else B
        if k % 6 == 5:  # the near miss: the key of count c listed under c + 1
            s, n = near
            digs.append(ref(algo, per_word[w][c], s, n - 1))
        else:
            digs.append(ref(algo, per_word[w][c], s, n))
        salts.append(s)
        iters.append(n)
    rng = np.random.default_rng(algo)
    for _ in range(500):
        digs.append(bytes(rng.integers(0, 256, size=16, dtype=np.uint8)))
        s, n = (A, B, near)[int(rng.integers(0, 3))]
        salts.append(s)
        iters.append(n)
    gpu_ctx.iter_budget(0, 0)
    gpu_ctx.set_iterated_targets(algo, b"".join(digs), salts, iters)
    index = [B, A, near]  # first appearance: k = 0 is B, k = 1 is A, k = 5 the near miss
    S = gpu_ctx.salt_count()
    assert S == 3 and [(gpu_ctx.salt(i), gpu_ctx.salt_iterations(i)) for i in range(S)] == index
    reg = set(zip(digs, zip(salts, iters)))
    want = {(w, c, i) for w, c in flat for i, (s, n) in enumerate(index) if (ref(algo, per_word[w][c], s, n), (s, n)) in reg}
    assert len(want) >= 12 and not any(i == 2 for _, _, i in want)
    data, offs = pack_words(words)
    hits, st = gpu_ctx.expand_digest(data, offs, mode, 0, 15)
    hs = gpu_ctx.last_hit_salts()
    assert len(hs) == len(hits) and st["candidates"] == ncand
    got = {(int(w), int(c), int(i)) for (w, c, _), i in zip(hits, hs)}
    assert len(got) == len(hits) and got == want
    assert all(d == ref(algo, per_word[w][c], *index[i]) for (w, c, d), i in zip(hits, hs))
    assert gpu_ctx.salts_last() == ((ncand - over) * S, over * S)
    assert gpu_ctx.iter_budget(0, 0) == 1
    # the same through a small scratch and the smallest budgets: 64 slots hold one block's lines
    # (rounded up to a wave) under one index, 64 pair-iterations one iteration of them, so every
    # block of every range costs the 63 + 4 + 5 launches of the three counts
    gpu_ctx.iter_budget(64, 64)
    dw, do = DeviceBuffer.from_array(gpu_ctx, data), DeviceBuffer.from_array(gpu_ctx, offs)
    hits2, st2 = gpu_ctx.expand_digest_device(dw.ptr, do.ptr, len(words), mode, 0, 15, scratch_bytes=4096)
    hs2 = gpu_ctx.last_hit_salts()
    launches = gpu_ctx.iter_budget(0, 0)
    assert launches >= 72 * st2["expand_launches"] and launches % 72 == 0
    assert {(int(w), int(c), int(i)) for (w, c, _), i in zip(hits2, hs2)} == want and len(hits2) == len(want)
    assert gpu_ctx.salts_last() == ((ncand - over) * S, over * S)


def test_more_hits_than_the_device_buffer_iterate_once():
    """An identity table makes the 2047 candidates of a*11 equal: one target under (salt, c = 1)
    is hit 2047 times, more than the 1024 entries the iterated route's device buffer starts with;
    a second index of c = 5 gives every pass one loop launch.  The compare step runs again with
    room, the loop does not: its launch count is that of a run whose target nobody hits."""
    from hashcat_a5_table_generator_amd import Context, pack_words
    word = b"a" * 11
    with Context(0) as ctx:
        ctx.parse_table(b"a=a\n")
        data, offs = pack_words([word])
        total = int(ctx.keyspace(data, offs, 0, 0, 15)[0][0])
        assert total == 2047
        for algo in (72, 75):
            d = ref(algo, word, b"salt", 1)
            ctx.set_iterated_targets(algo, d + bytes(range(16, 32)), [b"salt", b"other"], [1, 5])
            hits, _ = ctx.expand_digest(data, offs, 0, 0, 15, hit_cap=4096)
            launches = ctx.iter_budget(0, 0)
            assert len(hits) == total and sorted(c for _, c, _ in hits) == list(range(total))
            assert all(w == 0 and x == d for w, _, x in hits) and ctx.last_hit_salts() == [0] * total
            ctx.set_iterated_targets(algo, bytes(range(16)) + bytes(range(16, 32)), [b"salt", b"other"], [1, 5])
            none, _ = ctx.expand_digest(data, offs, 0, 0, 15, hit_cap=4096)
            assert none == [] and ctx.iter_budget(0, 0) == launches == 1


@pytest.mark.parametrize("algo", [73, 75], ids=[NAME[73], NAME[75]])
def test_format_checks_the_whole_key(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import format_plain, pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    (w1, c1), (w2, c2), (w3, c3) = [(w, len(cs) // 2) for w, cs in enumerate(per_word) if len(cs) > 2][:3]
    h = HLEN[algo]
    true_key = ref(algo, per_word[w1][c1], b"NaCl", 7, 2 * h)           # two blocks of T
    k2 = ref(algo, per_word[w2][c2], b"pepper", 3, h + 4)
    false_key = k2[:16] + bytes([k2[16] ^ 1]) + k2[17:]                  # byte 17 is wrong
    k3 = ref(algo, per_word[w3][c3], b"NaCl", 7, h + 4)
    false_tail = k3[:-1] + bytes([k3[-1] ^ 0x80])                        # the last byte, in T2
    lines = [line_of(algo, b"NaCl", 7, true_key), line_of(algo, b"pepper", 3, false_key), line_of(algo, b"NaCl", 7, false_tail)]
    assert gpu_ctx.load_pbkdf2_hashes(algo, b"\n".join(lines) + b"\n") == (3, 2, 0)
    data, offs = pack_words(words)
    hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
    hs = gpu_ctx.last_hit_salts()
    assert {(w1, c1, 0), (w2, c2, 1), (w3, c3, 0)} <= {(w, c, i) for (w, c, _), i in zip(hits, hs)}
    out, dropped = gpu_ctx.format_hits_iterated(data, offs, hits, hs)
    # (two words may share a candidate: every hit on the true target prints its line)
    assert set(out.split(b"\n")[:-1]) == {lines[0] + b":" + format_plain(per_word[w1][c1])}
    assert dropped == len(hits) - out.count(b"\n") >= 2
    # a set given without lines prints the line it stands for
    gpu_ctx.set_iterated_targets(algo, true_key[:16], [b"NaCl"], [7])
    hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
    out, dropped = gpu_ctx.format_hits_iterated(data, offs, hits, gpu_ctx.last_hit_salts())
    assert dropped == 0 and set(out.split(b"\n")[:-1]) == {line_of(algo, b"NaCl", 7, true_key[:16]) + b":" +
                                                           format_plain(per_word[w1][c1])}


def test_cli(tmp_path):
    from hashcat_a5_table_generator_amd import Context, format_plain
    words = [b"strasse", b"hello", b"s\xffa", b"a" + b"x" * 139]
    (tmp_path / "d.txt").write_bytes(b"\n".join(words) + b"\n")
    with Context(0) as c:
        c.load_tables([table_path("czech")])
        per_word = c.expand_words(words, 0, 0, 15)
    assert all(per_word[:3])
    over = sum(1 for cs in per_word for x in cs if len(x) > LMAX)
    plan = [(0, len(per_word[0]) - 1, b"NaCl", 1000), (1, 0, b"", 3), (2, len(per_word[2]) - 1, b"NaCl", 999)]

    def run(algo, name):
        h = HLEN[algo]
        lines = [line_of(algo, s, n, ref(algo, per_word[w][c], s, n, h)) for w, c, s, n in plan]
        k = ref(algo, per_word[1][0], b"NaCl", 1000, h + 1)
        lines.append(line_of(algo, b"NaCl", 1000, k[:-1] + bytes([k[-1] ^ 1])))  # 16 bytes right, the last wrong
        lines.append(line_of(72 if algo != 72 else 73, b"NaCl", 10, bytes(16)))  # another algorithm's name
        lines.append(b"not a hash")
        (tmp_path / "h.txt").write_bytes(b"\n".join(lines) + b"\n")
        r = subprocess.run([CLI, str(tmp_path / "d.txt"), "-t", table_path("czech"), "--hashes", str(tmp_path / "h.txt"),
                            "--algo", name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        want = sorted(lines[k] + b":" + format_plain(per_word[w][c]) for k, (w, c, _, _) in enumerate(plan))
        assert sorted(r.stdout.split(b"\n")[:-1]) == want and b":$HEX[" in r.stdout
        assert b"4 target(s), 3 distinct (salt, iterations) pair(s), 2 line(s) skipped" in r.stderr
        assert b"%d (candidate, salt) pair(s) longer than 128 bytes skipped" % (over * 3) in r.stderr
        assert b"1 hit(s) on the first 16 bytes dropped" in r.stderr

    assert over > 0
    run(73, "pbkdf2-hmac-sha1")
    run(74, "10900")
    run(75, "12100")
    run(72, "pbkdf2-hmac-md5")
