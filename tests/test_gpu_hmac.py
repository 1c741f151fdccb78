"""HMAC target lists on the GPU (k_hmac_stream, a5x_hmac.hip): every (line, salt) digest of the
eight algorithms 48..55 against Python's hmac, over a stream whose lines straddle and end exactly
on the 4 KiB block edges, sit on the key's and the message's block edges and run over the
128-byte limit, under sixteen salts on the inner message's block and dword edges; planted (word,
candidate, salt) triples with decoys that must not hit; small scratch, candidate ranges and the
hit cap; the adversarial target sets of target_sets.py; the hash:salt:plain output of
format_hits_salted and the CLI; and switching between plain salted, HMAC, salted nested and
unsalted sets."""
import ctypes
import hashlib
import hmac
import os
import subprocess

import numpy as np
import pytest

import target_sets as ts
from conftest import ROOT, table_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "hashcat_a5_table_generator_amd", "_build", "a5x_generator")
MD5, MD5_MD5_SALT = 0, 32
BLOCK = 4096  # STREAM_BLK of a5x_stream.h
LMAX = 128
E_CAPACITY = -8

HASH = {48: "md5", 49: "md5", 50: "sha1", 51: "sha1", 52: "sha256", 53: "sha256", 54: "sha512", 55: "sha512"}
SIZE = {48: 16, 49: 16, 50: 20, 51: 20, 52: 32, 53: 32, 54: 64, 55: 64}
ORDER = {a: a & 1 for a in range(48, 56)}  # 0: key = pass, 1: key = salt
NAME = {a: "hmac-%s-key-%s" % (HASH[a], "salt" if ORDER[a] else "pass") for a in range(48, 56)}
ALGOS = pytest.mark.parametrize("algo", sorted(NAME), ids=[NAME[a] for a in sorted(NAME)])
TWO_ALGOS = pytest.mark.parametrize("algo", [48, 55], ids=[NAME[48], NAME[55]])


def ref(algo, p, s):
    """The definition: HMAC with the candidate as the key (even values) or the salt (odd)."""
    return hmac.new(s, p, HASH[algo]).digest() if ORDER[algo] else hmac.new(p, s, HASH[algo]).digest()


def _h(algo, b):
    return hashlib.new(HASH[algo], b).digest()


FILLER = list(b"bfghjklmpqvwxBFGH 19-")  # no key or value of the czech / german tables
TOKENS = [b"a", b"e", b"s", b"A", b"S", b"z", "á".encode(), "š".encode(), "ä".encode(), "é".encode()]


def _words(seed, n, max_tokens=2, lo=1, hi=13):
    """n words of filler bytes with 1..max_tokens substitutable tokens (as test_gpu_salted._words)."""
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


# sixteen distinct salts in this unsorted order, the 5-byte one given twice: 55 / 56 are the one /
# two block edge of key = pass's inner message, 63 / 64 fill the second block's words, 0 is the
# empty message / the all-zero key, lengths = 1, 2, 3 mod 4 end in a partial word
SALT_LENS = [16, 0, 64, 3, 1, 55, 5, 2, 31, 24, 5, 4, 63, 32, 15, 56, 30]
GIVEN = [_salt(n, 7) for n in SALT_LENS]
SALTS = [s for k, s in enumerate(GIVEN) if s not in GIVEN[:k]]  # first-appearance order
# candidate bytes: 64 / 65 the key as it is / pre-hashed, 119 / 120 the pre-hash's own blocks (key =
# pass); 55 / 56 and 119 / 120 the message's blocks, SHA-512 111 / 112 (key = salt); 128 / 129 the limit
FIXED = [0, 1, 54, 55, 56, 63, 64, 65, 66, 111, 112, 119, 120, 127, 128, 129, 200]

_cache = {}


def _stream(ctx):
    """The shared "cand\\n" stream (built as test_gpu_salted_nested._stream builds its own): the
    candidates of 440 filler-and-token words, lines of the fixed lengths spread among them, and
    pad lines so that one line ends exactly on a block edge; on the device once, for every case."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    if "stream" in _cache:
        return _cache["stream"]
    _load(ctx, ["czech", "german"])
    words = _words(2, 440)
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, len(words))
    out = DeviceBuffer(ctx, tb + 64)
    ctx.expand_device(dw.ptr, do.ptr, len(words), out.ptr, tb)
    lines = bytes(out.to_array(count=tb)).split(b"\n")[:-1]
    assert len(lines) == tc
    step = len(lines) // (len(FIXED) + 1)
    for k, n in enumerate(FIXED):  # (bytes 1..255 but '\n', each line its own)
        lines.insert((k + 1) * step + k, bytes(1 + (i * 29 + n * 13 + 3) % 255 for i in range(n)).replace(b"\n", b"\x0b"))
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
    lens = {len(x) for x in lines}
    assert all(n in lens for n in FIXED)
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
def test_every_digest(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    buf, nbytes, lines = _stream(gpu_ctx)
    S, W, o = len(SALTS), SIZE[algo], ORDER[algo]
    assert S == 16 and len(GIVEN) == 17
    # the salt records come from the target set (built for this algorithm); its digests play no part here
    gpu_ctx.set_salted_targets(algo, o, b"".join(ref(algo, b"", s) for s in GIVEN), GIVEN)
    assert gpu_ctx.salt_count() == S and [gpu_ctx.salt(i) for i in range(S)] == SALTS
    dig = DeviceBuffer(gpu_ctx, W * len(lines) * S + 16)
    n = gpu_ctx.digest_lines_salted_device(algo, o, buf.ptr, nbytes, dig.ptr, len(lines) * S)
    assert n == len(lines)
    got = dig.to_array(count=W * n * S).reshape(n, S, W)
    bad, over = [], 0
    for i, ln in enumerate(lines):
        fits = len(ln) <= LMAX  # no pair is skipped for its salt
        over += 0 if fits else 1
        for s, salt in enumerate(SALTS):
            exp = ref(algo, ln, salt) if fits else bytes(W)
            if bytes(got[i, s]) != exp:
                bad.append((len(ln), len(salt), ln[:16], bytes(got[i, s]).hex()[:16], exp.hex()[:16]))
    assert not bad, (len(bad), bad[:5])
    assert over >= 2 and gpu_ctx.salts_last() == ((len(lines) - over) * S, over * S)


def test_digest_lines_wants_the_sets_own_algorithm(gpu_ctx):
    from hashcat_a5_table_generator_amd import A5xError, DeviceBuffer
    buf, nbytes, lines = _stream(gpu_ctx)
    dig = DeviceBuffer(gpu_ctx, 64 * len(lines) + 16)
    gpu_ctx.set_salted_targets(48, 0, ref(48, b"x", b"s"), [b"s"])
    # another HMAC, the other key, a salted nested and a plain algorithm, the wrong order
    for algo, order in ((50, 0), (49, 1), (MD5_MD5_SALT, 0), (MD5, 0), (48, 1)):
        with pytest.raises(A5xError) as e:
            gpu_ctx.digest_lines_salted_device(algo, order, buf.ptr, nbytes, dig.ptr, len(lines))
        assert e.value.code == -1, (algo, order)
    for other, o, d in ((MD5, 0, hashlib.md5(b"xs").digest()), (MD5_MD5_SALT, 0, bytes(range(16)))):
        gpu_ctx.set_salted_targets(other, o, d, [b"s"])
        with pytest.raises(A5xError) as e:  # 48..55 on another kind of set
            gpu_ctx.digest_lines_salted_device(48, 0, buf.ptr, nbytes, dig.ptr, len(lines))
        assert e.value.code == -1
    with pytest.raises(A5xError) as e:  # the unsalted hook has no salt to give
        gpu_ctx.digest_lines_device(48, buf.ptr, nbytes, dig.ptr, len(lines))
    assert e.value.code == -1


LOOKUP_SALTS = [b"NaCl", b"", b"0123456789abcdef!", b"x", b"pepper:", b"\x00\xff\x80", b"s" * 24]


def _per_word(ctx, mode):
    _load(ctx, ["czech", "german"])
    key = ("pw", mode)
    if key not in _cache:
        words = _words(100 + mode, 150, max_tokens=4, lo=4, hi=17)
        _cache[key] = (words, ctx.expand_words(words, mode, 0, 15))
    return _cache[key]


def _planted_set(algo, per_word, seed, planted=60):
    """Salted targets: one random digest per salt (fixing the salt indices), planted (candidate,
    salt) pairs, decoys and random filler.  The decoys, by k % 8: 2 -- the HMAC with key and
    message swapped; 3 -- the right digest registered with another salt; 4 -- H(pass . salt);
    5 -- H(salt . pass); 6 -- the inner hash alone, H((K0 ^ ipad) . message).
    Returns (digests, salts, the (word, cand, salt) triples that must hit, the decoy triples)."""
    rng = np.random.default_rng(seed)
    W, S, o = SIZE[algo], len(LOOKUP_SALTS), ORDER[algo]
    B = 128 if W == 64 else 64
    digs = [bytes(rng.integers(0, 256, size=W, dtype=np.uint8)) for _ in range(S)]
    sidx = list(range(S))
    flat = [(w, c) for w, cs in enumerate(per_word) for c in range(len(cs))]
    decoys = []
    planted = max(16, min(planted, len(flat) // 4))
    for k, g in enumerate(range(0, len(flat), len(flat) // planted)):
        w, c = flat[g]
        p = per_word[w][c]
        a = k % S
        salt = LOOKUP_SALTS[a]
        if k % 8 == 3:
            digs.append(ref(algo, p, salt))
            sidx.append((a + 1 + k % (S - 1)) % S)
            assert sidx[-1] != a
            decoys.append((w, c, a))
            decoys.append((w, c, sidx[-1]))
            continue
        if k % 8 == 2:
            digs.append(ref(algo ^ 1, p, salt))
        elif k % 8 == 4:
            digs.append(_h(algo, p + salt))
        elif k % 8 == 5:
            digs.append(_h(algo, salt + p))
        elif k % 8 == 6:
            key, msg = (salt, p) if o else (p, salt)
            k0 = (_h(algo, key) if len(key) > B else key).ljust(B, b"\0")
            digs.append(_h(algo, bytes(x ^ 0x36 for x in k0) + msg))
        else:
            digs.append(ref(algo, p, salt))
            sidx.append(a)
            continue
        sidx.append(a)
        decoys.append((w, c, a))
    for _ in range(2000):
        digs.append(bytes(rng.integers(0, 256, size=W, dtype=np.uint8)))
        sidx.append(int(rng.integers(0, S)))
    reg = set(zip(digs, sidx))
    want = {(w, c, s) for w, cs in enumerate(per_word) for c, x in enumerate(cs) for s, salt in enumerate(LOOKUP_SALTS)
            if (ref(algo, x, salt), s) in reg}
    decoys = [t for t in decoys if t not in want]  # (two words may share a candidate, planted under the decoy's salt)
    assert len(decoys) >= 10 and len(want) > 5
    return b"".join(digs), [LOOKUP_SALTS[s] for s in sidx], want, decoys


def _hits_with_salts(ctx, call):
    hits, st = call()
    salts = ctx.last_hit_salts()
    assert len(salts) == len(hits)
    return [(int(w), int(c), int(s), d) for (w, c, d), s in zip(hits, salts)], st


LOOKUPS = [(a, 0) for a in sorted(NAME)] + [(a, m) for a in (48, 55) for m in (1, 2, 3)]


@pytest.mark.parametrize("algo,mode", LOOKUPS, ids=[f"{NAME[a]}-mode{m}" for a, m in LOOKUPS])
def test_lookup_planted_triples(gpu_ctx, algo, mode):
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word = _per_word(gpu_ctx, mode)
    digs, salts, want, decoys = _planted_set(algo, per_word, 9 + algo + mode)
    gpu_ctx.set_salted_targets(algo, ORDER[algo], digs, salts)
    S = len(LOOKUP_SALTS)
    assert gpu_ctx.salt_count() == S and [gpu_ctx.salt(i) for i in range(S)] == LOOKUP_SALTS
    data, offs = pack_words(words)
    hits, st = _hits_with_salts(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, mode, 0, 15))
    ncand = sum(len(cs) for cs in per_word)
    assert st["candidates"] == ncand  # not multiplied by S
    over = sum(1 for cs in per_word for x in cs if len(x) > LMAX)
    assert gpu_ctx.salts_last() == ((ncand - over) * S, over * S)
    got = {(w, c, s) for w, c, s, _ in hits}
    assert len(hits) == len(got) and got == want
    assert not (got & set(decoys))
    # the public salt index, and the whole digest (20 / 32 / 64 bytes: a5x_hit_digest)
    assert all(len(d) == SIZE[algo] and d == ref(algo, per_word[w][c], LOOKUP_SALTS[s]) for w, c, s, d in hits)


@TWO_ALGOS
def test_small_scratch_ranges_and_hit_cap(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import A5xError, DeviceBuffer, _lib, pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    digs, salts, want, _ = _planted_set(algo, per_word, 77 + algo, planted=200)
    gpu_ctx.set_salted_targets(algo, ORDER[algo], digs, salts)
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
    for a, b in zip(cuts, cuts[1:]):  # every cut is inside a word
        part, _ = hits(a, b)
        assert all(a <= coff[w] + c < b for w, c, _ in part), (a, b)
        assert not (part & union)
        union |= part
    assert union == want
    # the hit cap one below the total: A5X_E_CAPACITY with the total, the entries past the cap keep
    # the caller's bytes
    total = len(want)
    cap = total - 1
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


ADV_SALTS = [b"NaCl", b"", b"0123456789abcdef!"]


def _unique(seq):
    seen, out = set(), []
    for d in seq:
        if d not in seen and any(d[:16]):
            seen.add(d)
            out.append(d)
    return out


@TWO_ALGOS
def test_target_set_adversaries(gpu_ctx, algo):
    """As test_gpu_target_set.test_salts: a displaced probe chain before D (55: the wide chain,
    through entries with D's own 16-byte prefix, beside a zero-prefix target and the all-zero
    digest) and the near misses of N, all registered with salt 0 and built from digests under salt
    0; the forged targets once more under salt 1; a planted digest under salt 2.  The table's key
    is the digest XOR the salt's mask, so the layout claims hold for the unmasked lists (asserted);
    the exhaustive equality of the (word, candidate, salt) hits is asserted."""
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    data, offs = pack_words(words)
    W = SIZE[algo]
    flat = [(w, c, x) for w, cs in enumerate(per_word) for c, x in enumerate(cs)]
    salted = [[ref(algo, x, s) for s in ADV_SALTS] for _, _, x in flat]
    pool = _unique(r[0] for r in salted)
    N = pool[0]
    forged = ts.near_misses(N, 8)
    ts.check_near_misses(ts.Dump(W, forged), N, forged)
    if W == 16:
        D = ts.pick_home(pool[2:], 16, 9, 15)
        chain = ts.chain(D, 7)
        ts.check_chain(ts.Dump(W, chain), D, 7, True)
    else:
        D = ts.pick_home(pool[2:], 16, 11, 15)
        chain = ts.wide_chain(D, 5)
        S = ts.Dump(W, chain)
        assert S.size == 16 and S.shared == 1 and S.has_zero == 1 and len(S.ztails) == 2
        ts.check_chain(S, D, 5, True)
    D2 = next(r[2] for r in reversed(salted))
    reg = [(t, 0) for t in chain + forged] + [(t, 1) for t in forged] + [(D2, 2)]
    for pairs in (reg, [p for p in reg if p[0] not in (D, D2)]):
        gpu_ctx.set_salted_targets(algo, ORDER[algo], b"".join(t for t, _ in pairs), [ADV_SALTS[s] for _, s in pairs])
        assert gpu_ctx.salt_count() == (3 if pairs is reg else 2)
        hits, st = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
        which = gpu_ctx.last_hit_salts()
        assert len(which) == len(hits)
        S = gpu_ctx.salt_count()
        over = sum(1 for _, _, x in flat if len(x) > LMAX)
        assert gpu_ctx.salts_last() == (S * (len(flat) - over), S * over)
        pset = set(pairs)
        want = {(w, c, s) for (w, c, x), rs in zip(flat, salted) for s in range(S) if len(x) <= LMAX and (rs[s], s) in pset}
        got = [(w, c, s) for (w, c, _), s in zip(hits, which)]
        assert len(got) == len(set(got)) and set(got) == want
        at = {(w, c): rs for (w, c, _), rs in zip(flat, salted)}
        assert all(d == at[(w, c)][s] for (w, c, d), s in zip(hits, which))
        if pairs is reg:
            assert {s for _, _, s in want} == {0, 2}
        else:
            assert hits == []


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
        for algo in (49, 52, 54):
            gpu_ctx.set_salted_targets(algo, ORDER[algo], b"".join(ref(algo, per_word[w][c], salts[s]) for w, c, s in triples),
                                       [salts[s] for _, _, s in triples])
            idx = {gpu_ctx.salt(i): i for i in range(gpu_ctx.salt_count())}
            assert set(idx) == set(salts)
            data, offs = pack_words(words)
            hits, _ = _hits_with_salts(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, 0, 0, 15))
            assert {(w, c, idx[salts[s]]) for w, c, s in triples} <= {(w, c, s) for w, c, s, _ in hits}
            by = {i: s for s, i in idx.items()}
            for hx in (False, True):
                enc = (lambda s: s.hex().encode()) if hx else (lambda s: s)
                want = sorted(ref(algo, per_word[w][c], by[s]).hex().encode() + b":" + enc(by[s]) + b":" +
                              format_plain(per_word[w][c]) + b"\n" for w, c, s, _ in hits)
                out = gpu_ctx.format_hits_salted(data, offs, [(w, c, d) for w, c, _, d in hits], [s for _, _, s, _ in hits],
                                                 hex_salt=hx)
                if hx:
                    assert sorted(ln + b"\n" for ln in out.split(b"\n")[:-1]) == want
                else:  # raw salts may hold any byte but '\n' here: compare the whole output as a multiset of lines
                    assert sorted(out.split(b"\n")) == sorted(b"".join(want).split(b"\n"))
            assert b":$HEX[" in out
    finally:
        gpu_ctx.clear_table()


def _cli(tmp_path, args, timeout=120):
    return subprocess.run([CLI, str(tmp_path / "d.txt"), "-t", ",".join([table_path("czech"), table_path("german")])] + args,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def test_cli_hmac(tmp_path):
    from hashcat_a5_table_generator_amd import Context, format_plain
    words = [b"strasse", b"hello", b"zuerich", b"a" + b"x" * 139]
    (tmp_path / "d.txt").write_bytes(b"\n".join(words) + b"\n")
    with Context(0) as c:
        c.load_tables([table_path("czech"), table_path("german")])
        per_word = c.expand_words(words, 0, 0, 15)
    assert all(per_word[:3])
    salts = [b"NaCl", b"pe:pper", b""]
    plan = [(0, len(per_word[0]) - 1, 0), (1, 0, 1), (2, len(per_word[2]) // 2, 2), (1, 0, 0)]

    def run(algo, args, hex_salt=False):
        hx = lambda w, c, s: ref(algo, per_word[w][c], salts[s]).hex().encode()
        enc = (lambda s: s.hex().encode()) if hex_salt else (lambda s: s)
        lines = [hx(w, c, s) + b":" + enc(salts[s]) for w, c, s in plan]
        lines.append(hx(0, 0, 0) + b":" + enc(salts[1]))  # decoy: salt 0's digest listed with salt 1
        lines.append(b"not a hash")
        (tmp_path / "h.txt").write_bytes(b"\n".join(lines) + b"\n")
        r = _cli(tmp_path, ["--hashes", str(tmp_path / "h.txt")] + args)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        want = sorted(hx(w, c, s) + b":" + enc(salts[s]) + b":" + format_plain(per_word[w][c]) for w, c, s in plan)
        assert sorted(r.stdout.split(b"\n")[:-1]) == want  # each (hash, salt) target once, the decoy never
        assert b"%d target(s), 3 distinct salt(s), 1 line(s) skipped" % (len(plan) + 1) in r.stderr
        over = sum(1 for cs in per_word for x in cs if len(x) > LMAX)
        assert over > 0 and b"%d (candidate, salt) pair(s) longer than 128 bytes skipped" % (over * len(salts)) in r.stderr

    run(50, ["--algo", "150"])
    run(53, ["--algo", "hmac-sha256-key-salt", "--hex-salt"], hex_salt=True)
    run(55, ["--algo", "1760", "--salted=salt.pass"])


def test_set_switching(gpu_ctx):
    """Plain salted MD5 -> HMAC-MD5 key = pass -> md5-md5.salt -> set_targets(md5) -> HMAC-SHA512
    key = salt -> plain salted: each finds what its own kind plants and nothing of the previous
    one (the salt table is re-uploaded in the layout of the set's kind)."""
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    data, offs = pack_words(words)
    picks = [(w, len(cs) // 2) for w, cs in enumerate(per_word) if cs][::9]
    salts = [b"NaCl", b"0123456789abcdef!", b"xyz"]
    sof = lambda k: salts[k % len(salts)]
    md5 = lambda b: hashlib.md5(b).digest()
    nest = lambda p, s: md5(md5(p).hex().encode() + s)
    plain = [md5(per_word[w][c] + sof(k)) for k, (w, c) in enumerate(picks)]               # md5(p . salt)
    h48 = [ref(48, per_word[w][c], sof(k)) for k, (w, c) in enumerate(picks)]
    n32 = [nest(per_word[w][c], sof(k)) for k, (w, c) in enumerate(picks)]
    h55 = [ref(55, per_word[w][c], sof(k)) for k, (w, c) in enumerate(picks)]
    unsalted = [md5(per_word[w][c]) for w, c in picks]
    allsalts = [sof(k) for k in range(len(picks))]
    want = {(w, c, k % len(salts)) for k, (w, c) in enumerate(picks)}

    def run():
        hits, _ = _hits_with_salts(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, 0, 0, 15))
        return hits

    def planted(hits):  # (two words may share a candidate: at least what was planted, each with its own digest)
        return want <= {(w, c, s) for w, c, s, _ in hits}

    # 1: a plain salted MD5 set holding its own digests and the HMAC-MD5 ones
    gpu_ctx.set_salted_targets(MD5, 0, b"".join(plain + h48), allsalts * 2)
    h = run()
    assert planted(h) and all(d == md5(per_word[w][c] + salts[s]) for w, c, s, d in h)
    # 2: an HMAC-MD5 key = pass set holding its own digests, the plain salted and the nested ones
    gpu_ctx.set_salted_targets(48, 0, b"".join(h48 + plain + n32), allsalts * 3)
    h = run()
    assert planted(h) and all(d == ref(48, per_word[w][c], salts[s]) for w, c, s, d in h)
    # 3: a salted nested set holding its own digests and the HMAC ones
    gpu_ctx.set_salted_targets(MD5_MD5_SALT, 0, b"".join(n32 + h48), allsalts * 2)
    h = run()
    assert planted(h) and all(d == nest(per_word[w][c], salts[s]) for w, c, s, d in h)
    # 4: the unsalted MD5 set: no salts, no salt indices
    gpu_ctx.set_targets(MD5, b"".join(unsalted + h48))
    assert gpu_ctx.salt_count() == 0
    hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
    assert set(picks) <= {(w, c) for w, c, _ in hits} and all(d == md5(per_word[w][c]) for w, c, d in hits)
    assert gpu_ctx.last_hit_salts() == [] and gpu_ctx.salts_last() == (0, 0)
    # 5: an HMAC set of the other layout (key = salt, SHA-512, wide) holding its own digests only
    gpu_ctx.set_salted_targets(55, 1, b"".join(h55), allsalts)
    h = run()
    assert planted(h) and all(d == ref(55, per_word[w][c], salts[s]) for w, c, s, d in h)
    # 6: and back to the first kind
    gpu_ctx.set_salted_targets(MD5, 0, b"".join(plain), allsalts)
    h = run()
    assert planted(h) and all(d == md5(per_word[w][c] + salts[s]) for w, c, s, d in h)
