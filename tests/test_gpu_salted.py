"""Salted target lists on the GPU (k_salt_stream, a5x_salt.hip): every (line, salt) digest
against hashlib of the concatenation for the six algorithms and both orders, over a stream
whose lines straddle and end exactly on the 4 KiB block edges and run over the 128-byte
limit; planted (word, candidate, salt) triples through every mode with decoys registered
under another salt; small scratch, candidate ranges and the hit cap; the empty salt; the
unsalted route restored by set_targets; and the hash:salt:plain output of format_hits_salted
and the CLI."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, table_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "hashcat_a5_table_generator_amd", "_build", "a5x_generator")
MD5, NTLM, SHA1, SHA256, SHA224, SHA384, SHA512 = 0, 1, 2, 3, 5, 6, 7
REF = {MD5: hashlib.md5, SHA1: hashlib.sha1, SHA256: hashlib.sha256, SHA224: hashlib.sha224, SHA384: hashlib.sha384,
       SHA512: hashlib.sha512}
SIZE = {MD5: 16, SHA1: 20, SHA256: 32, SHA224: 28, SHA384: 48, SHA512: 64}
IDS = {MD5: "md5", SHA1: "sha1", SHA256: "sha256", SHA224: "sha224", SHA384: "sha384", SHA512: "sha512"}
ALGOS = pytest.mark.parametrize("algo", sorted(REF), ids=[IDS[a] for a in sorted(REF)])
TWO_ALGOS = pytest.mark.parametrize("algo", [MD5, SHA512], ids=["md5", "sha512"])
ORDERS = pytest.mark.parametrize("order", [0, 1], ids=["pass.salt", "salt.pass"])
BLOCK = 4096  # STREAM_BLK of a5x_stream.h
LMAX = 128
E_CAPACITY = -8

FILLER = list(b"bfghjklmpqvwxBFGH 19-")  # no key or value of the czech / german tables
TOKENS = [b"a", b"e", b"s", b"A", b"S", b"z", "á".encode(), "š".encode(), "ä".encode(), "é".encode()]


def _digest(algo, b):
    return REF[algo](b).digest()


def _msg(order, cand, salt):
    return cand + salt if order == 0 else salt + cand


def _words(seed, n, max_tokens=2, lo=1, hi=13):
    """n words of filler bytes with 1..max_tokens substitutable tokens (as test_gpu_rules._words)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        parts = [bytes([int(c)]) for c in rng.choice(FILLER, size=int(rng.integers(lo, hi)))]
        for _ in range(int(rng.integers(1, max_tokens + 1))):
            parts.insert(int(rng.integers(0, len(parts) + 1)), TOKENS[int(rng.integers(0, len(TOKENS)))])
        out.append(b"".join(parts))
    return out + [b"", b"a", b"strasse", b"\xff\xfe", "😀ab".encode()]


def _load(ctx, tabs):
    ctx.clear_table()
    ctx.load_tables([table_path(t) for t in tabs])


@pytest.fixture(autouse=True)
def _no_salts_left_behind(gpu_ctx):
    yield
    gpu_ctx.set_targets(MD5, hashlib.md5(b"").digest())
    assert gpu_ctx.salt_count() == 0


def _salt(n, seed):
    return bytes((1 + (i * 37 + seed * 101 + n * 7) % 255) for i in range(n))


# 13 distinct salts in this unsorted order, the 8-byte one given twice
SALT_LENS = [16, 0, 64, 3, 1, 55, 8, 2, 31, 8, 4, 63, 32, 5]
GIVEN = [_salt(n, 7) for n in SALT_LENS]
SALTS = [s for k, s in enumerate(GIVEN) if s not in GIVEN[:k]]  # first-appearance order

_cache = {}


def _stream(ctx):
    """The shared "cand\\n" stream: the candidates of 360 filler-and-token words and of fixed
    words at the padding edges and around the 128-byte limit, with pad lines so that one line
    ends exactly on a block edge; on the device once, for every case."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    if "stream" in _cache:
        return _cache["stream"]
    _load(ctx, ["czech", "german"])
    fixed = [54, 55, 56, 63, 64, 100, 119, 120, 127, 128, 129, 200]
    words = _words(2, 360) + [b"1" * (n - 1) + b"a" for n in fixed]
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, len(words))
    out = DeviceBuffer(ctx, tb + 64)
    ctx.expand_device(dw.ptr, do.ptr, len(words), out.ptr, tb)
    lines = bytes(out.to_array(count=tb)).split(b"\n")[:-1]
    assert len(lines) == tc
    lens = {len(x) for x in lines}  # (a fixed word's candidates are its length or a byte or two longer)
    assert all(lens & {n, n + 1, n + 2} for n in fixed) and max(lens) > LMAX
    # pad lines in front of the line that reaches the first block edge: the last pad ends on it
    pos, k = 0, 0
    while pos + len(lines[k]) + 1 <= BLOCK:
        pos += len(lines[k]) + 1
        k += 1
    gap = BLOCK - pos
    pads = []
    while gap > 0:
        n = min(gap, 100)
        pads.append(b"p" * (n - 1))
        gap -= n
    lines = lines[:k] + pads + lines[k:]
    stream = b"".join(x + b"\n" for x in lines)
    starts = np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])
    assert len(stream) >= 3 * BLOCK
    edges = range(BLOCK, len(stream), BLOCK)
    assert any(int(e) in set(starts.tolist()) for e in edges)  # a line ends exactly on a block edge
    assert any(starts[i] < e < starts[i + 1] - 1 for e in edges for i in [int(np.searchsorted(starts, e)) - 1])  # one straddles
    buf = DeviceBuffer.from_array(ctx, np.frombuffer(stream + b"\0" * 64, dtype=np.uint8))
    _cache["stream"] = (buf, len(stream), lines)
    return _cache["stream"]


@ALGOS
@ORDERS
def test_every_digest(gpu_ctx, algo, order):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    buf, nbytes, lines = _stream(gpu_ctx)
    S, W = len(SALTS), SIZE[algo]
    assert S == 13 and len(GIVEN) == 14
    # the salts come from the target set; the digests of this set play no part here
    gpu_ctx.set_salted_targets(MD5, 0, b"".join(hashlib.md5(s).digest() for s in GIVEN), GIVEN)
    assert gpu_ctx.salt_count() == S and [gpu_ctx.salt(i) for i in range(S)] == SALTS
    dig = DeviceBuffer(gpu_ctx, W * len(lines) * S + 16)
    n = gpu_ctx.digest_lines_salted_device(algo, order, buf.ptr, nbytes, dig.ptr, len(lines) * S)
    assert n == len(lines)
    got = dig.to_array(count=W * n * S).reshape(n, S, W)
    bad, skipped = [], 0
    for i, ln in enumerate(lines):
        for s, salt in enumerate(SALTS):
            fits = len(ln) + len(salt) <= LMAX
            skipped += 0 if fits else 1
            exp = _digest(algo, _msg(order, ln, salt)) if fits else bytes(W)
            if bytes(got[i, s]) != exp:
                bad.append((len(ln), len(salt), ln[:16], bytes(got[i, s]).hex()[:16], exp.hex()[:16]))
    assert not bad, (len(bad), bad[:5])
    assert gpu_ctx.salts_last() == (len(lines) * S - skipped, skipped)
    # one line with both kinds of pair: the 100-byte word's candidate under the 16- and the 31-byte salt
    i100 = next(i for i, ln in enumerate(lines) if 100 <= len(ln) <= 102)
    assert any(got[i100, SALTS.index(GIVEN[0])]) and not any(got[i100, SALTS.index(GIVEN[8])])
    assert skipped > 0 and any(len(ln) > LMAX for ln in lines)


LOOKUP_SALTS = [b"NaCl", b"", b"0123456789abcdef!", b"x", b"pepper:", b"\x00\xff\x80"]


def _per_word(ctx, mode):
    _load(ctx, ["czech", "german"])
    key = ("pw", mode)
    if key not in _cache:
        words = _words(100 + mode, 150, max_tokens=4, lo=4, hi=17)
        _cache[key] = (words, ctx.expand_words(words, mode, 0, 15))
    return _cache[key]


def _planted_set(algo, order, per_word, seed, planted=60):
    """Salted targets: one random digest per salt (fixing the salt indices), planted (candidate,
    salt) pairs, decoys -- H(cand . salt A) registered with salt B -- and random filler.
    Returns (digests, salts, the (word, cand, salt) triples that must hit, the decoy triples)."""
    rng = np.random.default_rng(seed)
    W, S = SIZE[algo], len(LOOKUP_SALTS)
    digs = [bytes(rng.integers(0, 256, size=W, dtype=np.uint8)) for _ in range(S)]
    sidx = list(range(S))
    flat = [(w, c) for w, cs in enumerate(per_word) for c in range(len(cs))]
    decoys = []
    planted = max(8, min(planted, len(flat) // 4))
    for k, g in enumerate(range(0, len(flat), len(flat) // planted)):
        w, c = flat[g]
        a = k % S
        digs.append(_digest(algo, _msg(order, per_word[w][c], LOOKUP_SALTS[a])))
        if k % 4 == 3:  # registered with another salt: must not hit
            sidx.append((a + 1 + k % (S - 1)) % S)
            assert sidx[-1] != a
            decoys.append((w, c, a))
        else:
            sidx.append(a)
    for _ in range(2000):
        digs.append(bytes(rng.integers(0, 256, size=W, dtype=np.uint8)))
        sidx.append(int(rng.integers(0, S)))
    reg = set(zip(digs, sidx))
    want = {(w, c, s) for w, cs in enumerate(per_word) for c, x in enumerate(cs) for s, salt in enumerate(LOOKUP_SALTS)
            if (_digest(algo, _msg(order, x, salt)), s) in reg}
    decoys = [t for t in decoys if t not in want]  # (two words may share a candidate, planted under the decoy's salt)
    assert len(decoys) >= 1 and len(want) > 5
    return b"".join(digs), [LOOKUP_SALTS[s] for s in sidx], want, decoys


def _hits_with_salts(ctx, call):
    hits, st = call()
    salts = ctx.last_hit_salts()
    assert len(salts) == len(hits)
    return [(int(w), int(c), int(s), d) for (w, c, d), s in zip(hits, salts)], st


@TWO_ALGOS
@ORDERS
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_lookup_planted_triples(gpu_ctx, algo, order, mode):
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word = _per_word(gpu_ctx, mode)
    digs, salts, want, decoys = _planted_set(algo, order, per_word, 9 + algo + mode)
    gpu_ctx.set_salted_targets(algo, order, digs, salts)
    S = len(LOOKUP_SALTS)
    assert gpu_ctx.salt_count() == S
    data, offs = pack_words(words)
    hits, st = _hits_with_salts(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, mode, 0, 15))
    ncand = sum(len(cs) for cs in per_word)
    assert st["candidates"] == ncand  # not multiplied by S
    skipped = sum(1 for cs in per_word for x in cs for s in LOOKUP_SALTS if len(x) + len(s) > LMAX)
    assert gpu_ctx.salts_last() == (ncand * S - skipped, skipped)
    got = {(w, c, s) for w, c, s, _ in hits}
    assert len(hits) == len(got) and got == want
    assert not (got & set(decoys))  # a digest under salt A registered with salt B is no hit
    assert all(len(d) == SIZE[algo] and d == _digest(algo, _msg(order, per_word[w][c], LOOKUP_SALTS[s]))
               for w, c, s, d in hits)


@TWO_ALGOS
@ORDERS
def test_small_scratch_ranges_and_hit_cap(gpu_ctx, algo, order):
    from hashcat_a5_table_generator_amd import A5xError, DeviceBuffer, _lib, pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    digs, salts, want, _ = _planted_set(algo, order, per_word, 77 + algo, planted=200)
    gpu_ctx.set_salted_targets(algo, order, digs, salts)
    cnt = np.array([len(x) for x in per_word], dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum(cnt)])
    tc = int(coff[-1])
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(gpu_ctx, data), DeviceBuffer.from_array(gpu_ctx, offs)

    def hits(cb=0, ce=None, scratch=0):
        h, st = _hits_with_salts(gpu_ctx, lambda: gpu_ctx.expand_digest_device(
            dw.ptr, do.ptr, len(words), 0, 0, 15, scratch_bytes=scratch, cand_begin=cb, cand_end=ce))
        assert st["candidates"] == (tc if ce is None else ce) - cb
        got = {(w, c, s) for w, c, s, _ in h}
        assert len(got) == len(h)  # no duplicates
        return got, st

    full, _ = hits()
    assert full == want
    small, st = hits(scratch=4096)
    assert st["expand_launches"] > 3 and small == want
    inner = [w for w in range(len(words)) if cnt[w] >= 3]
    cuts = [int(coff[w]) + int(cnt[w]) // 2 for w in (inner[len(inner) // 4], inner[len(inner) // 2], inner[3 * len(inner) // 4])]
    cuts = [0] + cuts + [tc]
    assert cuts == sorted(set(cuts))
    union = set()
    for a, b in zip(cuts, cuts[1:]):
        part, _ = hits(a, b)
        assert all(a <= coff[w] + c < b for w, c, _ in part), (a, b)
        assert not (part & union)
        union |= part
    assert union == want
    # the hit cap: 0 and one below the total give A5X_E_CAPACITY with the total; entries past
    # the cap keep the caller's bytes
    total = len(want)
    for cap in (0, total - 1):
        arr = (_lib.Hit * (cap + 2))()
        ctypes.memset(arr, 0xAB, ctypes.sizeof(arr))
        nh = ctypes.c_uint64()
        rc = gpu_ctx._L.a5x_expand_digest_device(gpu_ctx.h, dw.ptr, do.ptr, len(words), 0, 0, 15, 0, arr, cap,
                                                 ctypes.byref(nh), None, None)
        assert rc == E_CAPACITY and nh.value == total
        assert bytes(arr)[cap * ctypes.sizeof(_lib.Hit):] == b"\xab" * (2 * ctypes.sizeof(_lib.Hit))
        assert len(gpu_ctx.last_hit_salts()) == cap
    with pytest.raises(A5xError) as e:
        gpu_ctx.expand_digest_device(dw.ptr, do.ptr, len(words), 0, 0, 15, hit_cap=total - 1)
    assert e.value.code == E_CAPACITY and f"{total} hits" in str(e.value)


@TWO_ALGOS
def test_empty_salt_and_route_restored(gpu_ctx, algo):
    """A set whose only salt is empty finds what the unsalted set finds; set_targets after a
    salted run restores the unsalted hits and stats."""
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    tg = sorted({_digest(algo, cs[len(cs) // 2]) for cs in per_word[::7] if cs})
    data, offs = pack_words(words)
    keys = ("candidates", "bytes", "words", "expand_launches", "words_slow", "words_pass_b")

    def plain_run():
        gpu_ctx.set_targets(algo, b"".join(tg))
        assert gpu_ctx.salt_count() == 0
        hits, st = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
        assert gpu_ctx.last_hit_salts() == [] and gpu_ctx.salts_last() == (0, 0)
        return sorted(hits), {k: st[k] for k in keys}

    before = plain_run()
    assert len(before[0]) >= len(tg)
    for order in (0, 1):
        gpu_ctx.set_salted_targets(algo, order, b"".join(tg), [b""] * len(tg))
        assert gpu_ctx.salt_count() == 1 and gpu_ctx.salt(0) == b""
        hits, st = _hits_with_salts(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, 0, 0, 15))
        assert sorted((w, c, d) for w, c, _, d in hits) == before[0] and all(s == 0 for _, _, s, _ in hits)
        assert st["candidates"] == before[1]["candidates"]
    assert plain_run() == before


def test_format_hits_salted(gpu_ctx):
    from hashcat_a5_table_generator_amd import format_plain, pack_words
    gpu_ctx.clear_table()
    gpu_ctx.set_table({b"a": [b"b", b"\x01"], b"e": [b"3"]})
    try:
        words = [b"banana", b"zaq", b"tee"]
        salts = [b"NaCl", b"a:b", b"\x00\xff"]
        per_word = gpu_ctx.expand_words(words, 0, 0, 15)
        assert all(per_word)
        triples = [(w, c, s) for w in range(3) for c in (0, len(per_word[w]) - 1) for s in (w, (w + 1) % 3)]
        sha1 = lambda b: hashlib.sha1(b).digest()
        gpu_ctx.set_salted_targets(SHA1, 1, b"".join(sha1(salts[s] + per_word[w][c]) for w, c, s in triples),
                                   [salts[s] for _, _, s in triples])
        idx = {gpu_ctx.salt(i): i for i in range(gpu_ctx.salt_count())}
        assert set(idx) == set(salts)
        data, offs = pack_words(words)
        hits, _ = _hits_with_salts(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, 0, 0, 15))
        assert {(w, c, idx[salts[s]]) for w, c, s in triples} <= {(w, c, s) for w, c, s, _ in hits}
        by = {i: s for s, i in idx.items()}
        for hx in (False, True):
            enc = (lambda s: s.hex().encode()) if hx else (lambda s: s)
            want = sorted(sha1(by[s] + per_word[w][c]).hex().encode() + b":" + enc(by[s]) + b":" +
                          format_plain(per_word[w][c]) + b"\n" for w, c, s, _ in hits)
            out = gpu_ctx.format_hits_salted(data, offs, [(w, c, d) for w, c, _, d in hits], [s for _, _, s, _ in hits],
                                             hex_salt=hx)
            got = [ln + b"\n" for ln in out.split(b"\n")[:-1]] if hx else None
            if hx:
                assert sorted(got) == want
            else:  # raw salts may hold any byte but '\n' here: compare the whole output as a multiset of lines
                assert sorted(out.split(b"\n")) == sorted(b"".join(want).split(b"\n"))
        assert b":$HEX[" in out
    finally:
        gpu_ctx.clear_table()


def _cli(tmp_path, args, timeout=120):
    return subprocess.run([CLI, str(tmp_path / "d.txt"), "-t", ",".join([table_path("czech"), table_path("german")])] + args,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def test_cli_salted(tmp_path):
    from hashcat_a5_table_generator_amd import Context, format_plain
    words = [b"strasse", b"hello", b"zuerich", b"a" + b"x" * 139]
    (tmp_path / "d.txt").write_bytes(b"\n".join(words) + b"\n")
    with Context(0) as c:
        c.load_tables([table_path("czech"), table_path("german")])
        per_word = c.expand_words(words, 0, 0, 15)
    assert all(per_word[:3])
    salts = [b"NaCl", b"pe:pper", b""]
    plan = [(0, len(per_word[0]) - 1, 0), (1, 0, 1), (2, len(per_word[2]) // 2, 2), (1, 0, 0)]
    sha1 = lambda b: hashlib.sha1(b).hexdigest().encode()

    def run(order, args, hex_salt=False, repeat=False):
        msg = lambda w, c, s: _msg(order, per_word[w][c], salts[s])
        enc = (lambda s: s.hex().encode()) if hex_salt else (lambda s: s)
        lines = [sha1(msg(w, c, s)) + b":" + enc(salts[s]) for w, c, s in plan]
        lines.append(sha1(msg(0, 0, 0)) + b":" + enc(salts[1]))  # decoy: salt 0's digest listed with salt 1
        if repeat:
            lines.append(lines[0])
        lines.append(b"not a hash")
        (tmp_path / "h.txt").write_bytes(b"\n".join(lines) + b"\n")
        r = _cli(tmp_path, ["--hashes", str(tmp_path / "h.txt")] + args)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        want = sorted(sha1(msg(w, c, s)) + b":" + enc(salts[s]) + b":" + format_plain(per_word[w][c]) for w, c, s in plan)
        assert sorted(r.stdout.split(b"\n")[:-1]) == want  # each (hash, salt) target once, the decoy never
        ntg = len(plan) + 1 + (1 if repeat else 0)
        assert b"%d target(s), 3 distinct salt(s), 1 line(s) skipped" % ntg in r.stderr
        skipped = sum(1 for cs in per_word for x in cs for s in salts if len(x) + len(s) > LMAX)
        assert skipped > 0 and b"%d (candidate, salt) pair(s) longer than 128 bytes skipped" % skipped in r.stderr

    run(0, ["--algo", "sha1", "--salted=pass.salt"])
    run(1, ["--algo", "120"])
    run(0, ["--algo", "110", "--hex-salt"], hex_salt=True)
    run(1, ["--algo", "sha1", "--salted", "salt.pass"], repeat=True)


def test_cli_salted_usage_errors(tmp_path):
    (tmp_path / "d.txt").write_bytes(b"word\n")
    (tmp_path / "h.txt").write_bytes(hashlib.md5(b"x").hexdigest().encode() + b":s\n")
    h = ["--hashes", str(tmp_path / "h.txt")]
    for args in (h + ["--salted=pass.salt", "--rules", str(tmp_path / "h.txt")], h + ["--salted=salt.pass", "--algo", "ntlm"],
                 h + ["--algo", "20", "--rules", str(tmp_path / "h.txt")], h + ["--salted=both"], ["--salted=pass.salt"],
                 h + ["--hex-salt"], h + ["--algo", "120", "--salted=pass.salt"]):
        r = _cli(tmp_path, args, timeout=30)
        assert r.returncode == 80 and b"error:" in r.stderr and r.stdout == b"", args
