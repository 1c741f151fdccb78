"""Nested digests on the GPU (a5x_nest.h in k_digest_stream and k_rules_stream): every line's
digest against hashlib compositions for the seven algorithms over a stream with the inner
digests' padding edges, a line ending exactly on a 4 KiB block edge, one straddling it and
one read from HBM past the staged margin; the same under rules; planted candidates through
every mode with decoys (the plain inner-less digests, the other hex case) that must not hit;
small scratch, candidate ranges and the hit cap; hits with rules and the outerhex:plain
output; the CLI; and the fused route restored by a plain MD5 set."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import rule_oracle as ro
from conftest import ROOT, table_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "hashcat_a5_table_generator_amd", "_build", "a5x_generator")
MD5 = 0
MD5_MD5, MD5_MD5_MD5, MD5_MD5UP, MD5_SHA1, SHA1_SHA1, SHA1_MD5, SHA256_MD5 = range(16, 23)
E_ARG, E_CAPACITY = -1, -8
BLOCK = 4096   # DCfg<nested>::BLK of a5x_digest.hip, STREAM_BLK of a5x_stream.h
MARGIN = 256   # STREAM_MARGIN of a5x_stream.h: next-block bytes staged in LDS
LMAX = 128


def _md5(b):
    return hashlib.md5(b).digest()


def _sha1(b):
    return hashlib.sha1(b).digest()


def _hex(d):
    return d.hex().encode()


REF = {
    MD5_MD5: lambda p: _md5(_hex(_md5(p))),
    MD5_MD5_MD5: lambda p: _md5(_hex(_md5(_hex(_md5(p))))),
    MD5_MD5UP: lambda p: _md5(_hex(_md5(p)).upper()),
    MD5_SHA1: lambda p: _md5(_hex(_sha1(p))),
    SHA1_SHA1: lambda p: _sha1(_hex(_sha1(p))),
    SHA1_MD5: lambda p: _sha1(_hex(_md5(p))),
    SHA256_MD5: lambda p: hashlib.sha256(_hex(_md5(p))).digest(),
}
SIZE = {MD5_MD5: 16, MD5_MD5_MD5: 16, MD5_MD5UP: 16, MD5_SHA1: 16, SHA1_SHA1: 20, SHA1_MD5: 20, SHA256_MD5: 32}
NAME = {MD5_MD5: "md5-md5", MD5_MD5_MD5: "md5-md5-md5", MD5_MD5UP: "md5-md5up", MD5_SHA1: "md5-sha1",
        SHA1_SHA1: "sha1-sha1", SHA1_MD5: "sha1-md5", SHA256_MD5: "sha256-md5"}
ALGOS = pytest.mark.parametrize("algo", sorted(REF), ids=[NAME[a] for a in sorted(REF)])
# what a confused route would compute instead: the plain digests of the candidate at the set's
# width, and for the 16-byte forms the other hex case
DECOY = {
    MD5_MD5: [_md5, REF[MD5_MD5UP], REF[MD5_MD5_MD5], REF[MD5_SHA1]],
    MD5_MD5_MD5: [_md5, REF[MD5_MD5]],
    MD5_MD5UP: [_md5, REF[MD5_MD5]],
    MD5_SHA1: [_md5, REF[MD5_MD5], lambda p: _sha1(p)[:16]],
    SHA1_SHA1: [_sha1, REF[SHA1_MD5]],
    SHA1_MD5: [_sha1, REF[SHA1_SHA1]],
    SHA256_MD5: [lambda p: hashlib.sha256(p).digest(), lambda p: hashlib.sha256(_hex(_sha1(p))).digest()],
}

FILLER = list(b"bfghjklmpqvwxBFGH 19-")  # no key or value of the czech / german tables
TOKENS = [b"a", b"e", b"s", b"A", b"S", b"z", "á".encode(), "š".encode(), "ä".encode(), "é".encode()]
FIXED = (55, 56, 63, 64, 119, 120, 128, 200)  # the inner digests' padding edges, the rules' cap, a long line
LONG = 310  # read from HBM: placed to end past the staged margin


def _words(seed, n, max_tokens=2, lo=1, hi=13):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        parts = [bytes([int(c)]) for c in rng.choice(FILLER, size=int(rng.integers(lo, hi)))]
        for _ in range(int(rng.integers(1, max_tokens + 1))):
            parts.insert(int(rng.integers(0, len(parts) + 1)), TOKENS[int(rng.integers(0, len(TOKENS)))])
        out.append(b"".join(parts))
    return out + [b"a", b"strasse", b"\xff\xfea", "😀ab".encode()]


def _load(ctx, tabs=("czech", "german")):
    ctx.clear_table()
    ctx.load_tables([table_path(t) for t in tabs])


@pytest.fixture(autouse=True)
def _plain_set_left_behind(gpu_ctx):
    yield
    gpu_ctx.clear_rules()
    gpu_ctx.set_targets(MD5, _md5(b""))


_cache = {}


def _pads(gap):
    """Lines that take exactly gap stream bytes (each at most 100 with its newline)."""
    out = []
    while gap > 0:
        n = min(gap, 100)
        out.append(b"p" * (n - 1))
        gap -= n
    return out


def _stream(ctx):
    """The shared "cand\\n" stream, on the device once for every case: candidates of 400
    filler-and-token words and of fixed words, lines of exactly the FIXED lengths, the empty
    line, pad lines so that one line ends exactly on the first block edge, and the LONG line
    placed 20 bytes before the second edge so that it straddles it and ends past the margin."""
    from hashcat_a5_table_generator_amd import DeviceBuffer
    if "stream" in _cache:
        return _cache["stream"]
    _load(ctx)
    cands = [x for cs in ctx.expand_words(_words(5, 400), 0, 0, 15) for x in cs][:1200]
    assert len(cands) > 300 and sum(len(x) + 1 for x in cands) > 2 * BLOCK + 1024
    rest = iter(cands)
    lines, pos = [], 0

    def fill_to(limit):  # candidates while they fit below limit, then pads to reach it exactly
        nonlocal pos
        for x in rest:
            if pos + len(x) + 1 > limit:
                rest_first.append(x)
                break
            lines.append(x)
            pos += len(x) + 1
        for p in _pads(limit - pos):
            lines.append(p)
            pos += len(p) + 1
        assert pos == limit

    rest_first = []
    fill_to(BLOCK)                      # a line ends exactly on the first edge
    lines.append(rest_first.pop())
    pos += len(lines[-1]) + 1
    fill_to(2 * BLOCK - 20)
    long_at = len(lines)
    lines.append(bytes(33 + (7 * i) % 90 for i in range(LONG)))
    lines += [b""] + [bytes(33 + (11 * i + n) % 90 for i in range(n)) for n in FIXED] + rest_first + list(rest)
    stream = b"".join(x + b"\n" for x in lines)
    starts = np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])
    assert len(stream) >= 3 * BLOCK + 1 and len(lines) >= 300
    assert int(starts[long_at]) == 2 * BLOCK - 20 and starts[long_at] + LONG > 2 * BLOCK + MARGIN  # the HBM source
    assert BLOCK in set(starts.tolist())  # a line ends exactly on a block edge
    assert {len(x) for x in lines} >= set(FIXED) | {0, LONG}
    buf = DeviceBuffer.from_array(ctx, np.frombuffer(stream + b"\0" * 64, dtype=np.uint8))
    _cache["stream"] = (buf, len(stream), lines)
    return _cache["stream"]


@ALGOS
def test_every_digest(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    buf, nbytes, lines = _stream(gpu_ctx)
    W, f = SIZE[algo], REF[algo]
    dig = DeviceBuffer(gpu_ctx, W * len(lines) + 16)
    n = gpu_ctx.digest_lines_device(algo, buf.ptr, nbytes, dig.ptr, len(lines))
    assert n == len(lines)
    got = dig.to_array(count=W * n).reshape(n, W)
    bad = [(i, len(ln), ln[:16], bytes(got[i]).hex(), f(ln).hex()) for i, ln in enumerate(lines) if bytes(got[i]) != f(ln)]
    assert not bad, (len(bad), bad[:5])


RULES = [b":", b"u", b"c", b"r", b"d", b"$1", b"^!", b"]", b"T0"]


@pytest.mark.parametrize("algo", [MD5_MD5, MD5_MD5UP, SHA1_SHA1, SHA1_MD5, SHA256_MD5],
                         ids=["md5-md5", "md5-md5up", "sha1-sha1", "sha1-md5", "sha256-md5"])
def test_every_ruled_digest(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    buf, nbytes, lines = _stream(gpu_ctx)
    if "ruled" not in _cache:
        _cache["ruled"] = [None if len(ln) > LMAX else [ro.apply_rule(r, ln) for r in RULES] for ln in lines]
    ruled = _cache["ruled"]
    W, f, R = SIZE[algo], REF[algo], len(RULES)
    assert gpu_ctx.set_rules(RULES) == (R, 0)
    dig = DeviceBuffer(gpu_ctx, W * len(lines) * R + 16)
    n = gpu_ctx.digest_lines_rules_device(algo, buf.ptr, nbytes, dig.ptr, len(lines) * R)
    assert n == len(lines)
    got = dig.to_array(count=W * n * R).reshape(n, R, W)
    bad = []
    for i, ln in enumerate(lines):
        for r in range(R):
            exp = bytes(W) if ruled[i] is None else f(ruled[i][r])  # a rejected line: all-zero digests
            if bytes(got[i, r]) != exp:
                bad.append((len(ln), RULES[r], bytes(got[i, r]).hex(), exp.hex()))
    assert not bad, (len(bad), bad[:5])
    over = sum(1 for rs in ruled if rs is None)
    assert over >= 2 and gpu_ctx.rules_last() == ((len(lines) - over) * R, over)
    # the doubled 64-byte line fills the 128-byte cap, and the 128-byte line passes under ':'
    assert any(rs and len(rs[4]) == LMAX for rs in ruled) and any(rs and len(rs[0]) == LMAX for rs in ruled)


def _per_word(ctx, mode):
    _load(ctx)
    key = ("pw", mode)
    if key not in _cache:
        words = _words(100 + mode, 150, max_tokens=4, lo=4, hi=17)
        _cache[key] = (words, ctx.expand_words(words, mode, 0, 15))
    return _cache[key]


def _planted_set(algo, per_word, seed, planted=60):
    """The outer digests of ~planted candidates among 2000 random ones, and decoys -- what
    another route would compute for planted candidates.  Returns (digests, the (word, cand)
    pairs that must hit)."""
    rng = np.random.default_rng(seed)
    W, f = SIZE[algo], REF[algo]
    flat = [(w, c) for w, cs in enumerate(per_word) for c in range(len(cs))]
    planted = max(8, min(planted, len(flat) // 4))
    picks = [flat[g] for g in range(0, len(flat), len(flat) // planted)]
    digs = [f(per_word[w][c]) for w, c in picks]
    decoys = [g(per_word[w][c]) for w, c in picks[::3] for g in DECOY[algo]]
    assert all(len(d) == W for d in decoys)
    digs += decoys + [bytes(rng.integers(0, 256, size=W, dtype=np.uint8)) for _ in range(2000)]
    reg = set(digs)
    want = {(w, c) for w, cs in enumerate(per_word) for c, x in enumerate(cs) if f(x) in reg}
    assert len(want) >= len(set(picks)) > 5
    return b"".join(digs), want


LOOKUP = [(a, m) for a in (MD5_MD5, SHA1_MD5) for m in (0, 1, 2, 3)] + \
         [(a, 0) for a in (MD5_MD5_MD5, MD5_MD5UP, MD5_SHA1, SHA1_SHA1, SHA256_MD5)]


@pytest.mark.parametrize("algo,mode", LOOKUP, ids=[f"{NAME[a]}-mode{m}" for a, m in LOOKUP])
def test_lookup_planted(gpu_ctx, algo, mode):
    """(md5-md5 in the default mode is the case that goes wrong if a nested set reaches the
    fused MD5 kernel: the planted digests are missed and the md5(p) decoys hit.)"""
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word = _per_word(gpu_ctx, mode)
    digs, want = _planted_set(algo, per_word, 31 + algo + mode)
    gpu_ctx.set_targets(algo, digs)
    data, offs = pack_words(words)
    hits, st = gpu_ctx.expand_digest(data, offs, mode, 0, 15)
    assert st["candidates"] == sum(len(cs) for cs in per_word)
    got = {(int(w), int(c)) for w, c, _ in hits}
    assert len(got) == len(hits) and got == want
    assert all(len(d) == SIZE[algo] and d == REF[algo](per_word[w][c]) for w, c, d in hits)
    for w, c, d in hits[:5]:  # hit_digest: the full outer digest from the hit's first 16 bytes
        assert gpu_ctx.hit_digest((w, c, d[:16])) == d


@pytest.mark.parametrize("algo", [MD5_MD5, SHA1_SHA1], ids=["md5-md5", "sha1-sha1"])
def test_small_scratch_ranges_and_hit_cap(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import A5xError, DeviceBuffer, _lib, pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    digs, want = _planted_set(algo, per_word, 77 + algo, planted=200)
    gpu_ctx.set_targets(algo, digs)
    cnt = np.array([len(x) for x in per_word], dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum(cnt)])
    tc = int(coff[-1])
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(gpu_ctx, data), DeviceBuffer.from_array(gpu_ctx, offs)

    def hits(cb=0, ce=None, scratch=0):
        h, st = gpu_ctx.expand_digest_device(dw.ptr, do.ptr, len(words), 0, 0, 15, scratch_bytes=scratch, cand_begin=cb,
                                             cand_end=ce)
        assert st["candidates"] == (tc if ce is None else ce) - cb
        got = {(int(w), int(c)) for w, c, _ in h}
        assert len(got) == len(h)  # no duplicates
        assert all(d == REF[algo](per_word[w][c]) for w, c, d in h)
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
        part, _ = hits(a, b, scratch=8192)
        assert all(a <= coff[w] + c < b for w, c in part), (a, b)
        assert not (part & union)
        union |= part
    assert union == want
    total = len(want)
    for cap in (0, total - 1):  # A5X_E_CAPACITY with the true count; entries past the cap keep the caller's bytes
        arr = (_lib.Hit * (cap + 2))()
        ctypes.memset(arr, 0xAB, ctypes.sizeof(arr))
        nh = ctypes.c_uint64()
        rc = gpu_ctx._L.a5x_expand_digest_device(gpu_ctx.h, dw.ptr, do.ptr, len(words), 0, 0, 15, 0, arr, cap,
                                                 ctypes.byref(nh), None, None)
        assert rc == E_CAPACITY and nh.value == total
        assert bytes(arr)[cap * ctypes.sizeof(_lib.Hit):] == b"\xab" * (2 * ctypes.sizeof(_lib.Hit))
    with pytest.raises(A5xError) as e:
        gpu_ctx.expand_digest_device(dw.ptr, do.ptr, len(words), 0, 0, 15, hit_cap=total - 1)
    assert e.value.code == E_CAPACITY and f"{total} hits" in str(e.value)


LOOKUP_RULES = [b":", b"u", b"c$1", b"r", b"d", b"^!", b"]"]


@pytest.mark.parametrize("algo", [MD5_MD5, SHA1_SHA1, SHA256_MD5], ids=["md5-md5", "sha1-sha1", "sha256-md5"])
def test_hits_with_rules_and_format(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import format_plain, pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    f, W, R = REF[algo], SIZE[algo], len(LOOKUP_RULES)
    rng = np.random.default_rng(5 + algo)
    picks = []
    for w in rng.choice([w for w in range(len(words)) if per_word[w]], size=30, replace=False):
        c, r = int(rng.integers(0, len(per_word[w]))), int(rng.integers(0, R))
        picks.append((int(w), c, r, ro.apply_rule(LOOKUP_RULES[r], per_word[w][c])))
    targets = {f(p) for _, _, _, p in picks}
    decoys = [hashlib.md5(p).digest() + bytes(W - 16) for _, _, _, p in picks]  # (the ruled plain's own MD5)
    tl = sorted(targets) + decoys + [bytes(rng.integers(0, 256, size=W, dtype=np.uint8)) for _ in range(2000)]
    gpu_ctx.set_targets(algo, b"".join(tl))
    data, offs = pack_words(words)
    # without rules: the ':' picks (and whatever shares their plain)
    plain_hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
    assert {(w, c) for w, c, r, _ in picks if r == 0} <= {(w, c) for w, c, _ in plain_hits}
    assert all(d == f(per_word[w][c]) and d in targets for w, c, d in plain_hits)
    lines = gpu_ctx.format_hits(data, offs, plain_hits, 0, 0, 15).split(b"\n")[:-1]
    assert sorted(lines) == sorted(d.hex().encode() + b":" + format_plain(per_word[w][c]) for w, c, d in plain_hits)
    # with rules
    assert gpu_ctx.set_rules(LOOKUP_RULES) == (R, 0)
    hits, st = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
    rules = gpu_ctx.last_hit_rules()
    assert len(rules) == len(hits)
    ncand = sum(len(cs) for cs in per_word)
    assert st["candidates"] == ncand and gpu_ctx.rules_last() == (ncand * R, 0)
    got = {(int(w), int(c), int(r)): d for (w, c, d), r in zip(hits, rules)}
    assert len(got) == len(hits)
    for w, c, r, p in picks:
        assert got.get((w, c, r)) == f(p), (w, c, LOOKUP_RULES[r], p)
    for (w, c, r), d in got.items():
        assert len(d) == W and d in targets and d == f(ro.apply_rule(LOOKUP_RULES[r], per_word[w][c]))
    lines = gpu_ctx.format_hits(data, offs, hits, 0, 0, 15, rules=rules).split(b"\n")[:-1]
    want = sorted(d.hex().encode() + b":" + format_plain(ro.apply_rule(LOOKUP_RULES[r], per_word[w][c]))
                  for (w, c, r), d in got.items())
    assert sorted(lines) == want and all(len(ln.split(b":", 1)[0]) == 2 * W for ln in lines)


def test_fused_route_restored_by_a_plain_set(gpu_ctx):
    """After a nested set, set_targets(MD5) on the same context finds a planted default-mode
    candidate again, and the nested digest of it no longer hits."""
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    w = next(w for w in range(len(words)) if len(per_word[w]) >= 2)
    p = per_word[w][1]
    data, offs = pack_words(words)
    gpu_ctx.set_targets(MD5_MD5, REF[MD5_MD5](p) + _md5(p))
    hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
    assert (w, 1) in {(a, b) for a, b, _ in hits} and {d for _, _, d in hits} == {REF[MD5_MD5](p)}
    gpu_ctx.set_targets(MD5, REF[MD5_MD5](p) + _md5(p))
    hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
    assert (w, 1) in {(a, b) for a, b, _ in hits} and {d for _, _, d in hits} == {_md5(p)}


def test_salted_device_entry_point_refuses(gpu_ctx):
    from hashcat_a5_table_generator_amd import A5xError, DeviceBuffer
    buf, nbytes, lines = _stream(gpu_ctx)
    dig = DeviceBuffer(gpu_ctx, 64 * len(lines))
    for algo in sorted(REF):
        with pytest.raises(A5xError, match="no salted mode") as e:
            gpu_ctx.digest_lines_salted_device(algo, 0, buf.ptr, nbytes, dig.ptr, len(lines))
        assert e.value.code == E_ARG
    for algo in (8, 9, 15, 23):  # unassigned values have no kernel and no size
        with pytest.raises(A5xError) as e:
            gpu_ctx.digest_lines_device(algo, buf.ptr, nbytes, dig.ptr, len(lines))
        assert e.value.code == E_ARG


def test_cli(tmp_path):
    from hashcat_a5_table_generator_amd import Context, format_plain
    words = [b"strasse", b"hello", b"zuerich", b"a" + b"x" * 139]
    (tmp_path / "d.txt").write_bytes(b"\n".join(words) + b"\n")
    (tmp_path / "r.rule").write_bytes(b":\nc$1\nu\n")
    rules = [b":", b"c$1", b"u"]
    tabs = [table_path("czech"), table_path("german")]
    with Context(0) as c:
        c.load_tables(tabs)
        per_word = c.expand_words(words, 0, 0, 15)
    assert all(per_word[:3])
    picks = [per_word[0][-1], per_word[1][0], per_word[2][len(per_word[2]) // 2]]

    def run(algo, args, plains):
        f = REF[algo]
        listed = [f(p).hex() for p in plains] + [hashlib.md5(p).hexdigest() + "0" * (2 * SIZE[algo] - 32) for p in plains]
        (tmp_path / "h.txt").write_text("\n".join(listed) + "\nnot a hash\n")
        r = subprocess.run([CLI, str(tmp_path / "d.txt"), "-t", ",".join(tabs), "--hashes", str(tmp_path / "h.txt")] + args,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        assert sorted(r.stdout.split(b"\n")[:-1]) == sorted(f(p).hex().encode() + b":" + format_plain(p) for p in set(plains))

    run(MD5_MD5, ["--algo", "md5-md5"], picks)
    run(SHA1_SHA1, ["--algo", "4500"], picks)
    run(SHA256_MD5, ["--algo", "sha256-md5", "--rules", str(tmp_path / "r.rule")],
        [ro.apply_rule(rules[1], picks[0]), ro.apply_rule(rules[2], picks[1]), ro.apply_rule(rules[0], picks[2])])
