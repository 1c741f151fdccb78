"""GPU parity of SHA-224 (hashcat -m 1300), SHA-384 (-m 10800) and SHA-512 (-m 1700) in the
digest + lookup stage: k_digest_stream's digests bit-exact against hashlib at the
algorithm's width and stride, and lookups against target sets whose tails are 3 / 8 / 12
words (first 16 bytes in the table, the rest in the parallel tail array and in the per-hit
tail record) through every entry point: all four modes, small scratch, candidate ranges,
a5x_hit_digest, a5x_format_hits and the CLI's --hashes / --algo."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, table_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "hashcat_a5_table_generator_amd", "_build", "a5x_generator")
SHA224, SHA384, SHA512 = 5, 6, 7
REF = {SHA224: lambda b: hashlib.sha224(b).digest(), SHA384: lambda b: hashlib.sha384(b).digest(),
       SHA512: lambda b: hashlib.sha512(b).digest()}
SIZE = {SHA224: 28, SHA384: 48, SHA512: 64}
NAME = {SHA224: "sha224", SHA384: "sha384", SHA512: "sha512"}
HASHCAT_MODE = {SHA224: "1300", SHA384: "10800", SHA512: "1700"}
STREAM_BLOCK = 4096  # DCfg<SHA224 / SHA384 / SHA512>::BLK of a5x_digest.hip
ALGOS = pytest.mark.parametrize("algo", [SHA224, SHA384, SHA512], ids=["sha224", "sha384", "sha512"])
# one substitutable letter at SHA-224's block edges (55/56, 63/64), at SHA-384 / SHA-512's
# one-to-two and two-to-three block edges (111/112, 127/128, 239/240, 255/256) and their
# length-field edges (119/120), at the end of the 256 B staging margin, and past it (HBM)
EDGE_LENGTHS = (54, 55, 56, 63, 64, 110, 111, 112, 119, 120, 127, 128, 239, 240, 255, 256, 600, 3000)


def _rw(rng, alpha, n):
    return np.asarray(rng.choice(alpha, size=int(n)), dtype=np.uint8).tobytes()


def _words(seed, n, greek=False):  # (as test_gpu_digest_sha.py builds them)
    rng = np.random.default_rng(seed)
    alpha = list("αβγδεζηθικλμνξοπρστυφχψω".encode()) if greek else list(b"abcdefghijklmnopqrstuvwxyzs")
    out = [_rw(rng, alpha, rng.integers(1, 13)) for _ in range(n)]
    return out + [b"", b"a", b"strasse", b"\xff\xfe", "😀ab".encode()]


def _load(ctx, tabs):
    ctx.clear_table()
    ctx.load_tables([table_path(t) for t in tabs])


def _expanded_lines(ctx, words):
    """The batch's "cand\\n" stream on the device and its lines."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, len(words))
    out = DeviceBuffer(ctx, tb + 64)
    ctx.expand_device(dw.ptr, do.ptr, len(words), out.ptr, tb)
    lines = bytes(out.to_array(count=tb)).split(b"\n")[:-1]
    assert len(lines) == tc
    return out, tb, lines


def _check_every_line(ctx, algo, out, tb, lines):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    W, f = SIZE[algo], REF[algo]
    dig = DeviceBuffer(ctx, W * len(lines) + 16)
    n = ctx.digest_lines_device(algo, out.ptr, tb, dig.ptr, len(lines))
    assert n == len(lines)
    got = dig.to_array(count=W * n).reshape(n, W)
    bad = [i for i, ln in enumerate(lines) if bytes(got[i]) != f(ln)]
    assert not bad, [(len(lines[i]), lines[i][:40], bytes(got[i]).hex(), f(lines[i]).hex()) for i in bad[:5]]


_stream_cache = {}


@ALGOS
@pytest.mark.parametrize("tabs", [["czech", "german"], ["greek-hebrew"]], ids=["cz-de", "el-he"])
def test_digest_every_line(gpu_ctx, algo, tabs):
    """Every line of an expanded batch, at the algorithm's width and stride."""
    _load(gpu_ctx, tabs)
    key = tuple(tabs)
    if key not in _stream_cache:  # one expansion per table set, shared by the three algorithms
        words = _words(len(tabs), 300, greek=tabs == ["greek-hebrew"])
        words += [b"1" * (n - 1) + b"a" for n in EDGE_LENGTHS]
        _stream_cache[key] = _expanded_lines(gpu_ctx, words)
    out, tb, lines = _stream_cache[key]
    if tabs == ["czech", "german"]:  # ("a" becomes a two-byte letter there: the lines are one byte longer)
        assert {55, 56, 111, 112, 120, 128, 240, 256} <= {len(ln) for ln in lines}
    _check_every_line(gpu_ctx, algo, out, tb, lines)


@ALGOS
def test_digest_lines_straddle_stream_blocks(gpu_ctx, algo):
    """250-300 B lines that straddle the stream's block edges at many offsets."""
    _load(gpu_ctx, ["czech"])
    if "edges" not in _stream_cache:
        rng = np.random.default_rng(11)
        _stream_cache["edges"] = _expanded_lines(gpu_ctx, [b"1" * int(k) + b"a" for k in rng.integers(250, 300, size=200)])
    out, tb, lines = _stream_cache["edges"]
    assert tb > 3 * STREAM_BLOCK
    _check_every_line(gpu_ctx, algo, out, tb, lines)


_per_word_cache = {}


def _per_word(ctx, mode):
    """400 words under czech + german and the library's per-word candidates, per mode."""
    _load(ctx, ["czech", "german"])
    if mode not in _per_word_cache:
        words = _words(100 + mode, 400)
        _per_word_cache[mode] = (words, ctx.expand_words(words, mode, 0, 15))
    return _per_word_cache[mode]


@ALGOS
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_lookup_planted_targets(gpu_ctx, algo, mode):
    """Planted digests are found at their (word, candidate), at full width, and 5000
    random digests never hit; the candidate count is the oracle's."""
    from hashcat_a5_table_generator_amd import pack_words
    from oracle import c_oracle as co
    words, per_word = _per_word(gpu_ctx, mode)
    f, W = REF[algo], SIZE[algo]
    rng = np.random.default_rng(9 + algo)
    planted = {}
    for w in rng.choice(len(words), size=40, replace=False):
        if per_word[w]:
            c = int(rng.integers(0, len(per_word[w])))
            planted[f(per_word[w][c])] = (int(w), c)
    assert len(planted) > 20
    targets = list(planted) + [bytes(rng.integers(0, 256, size=W, dtype=np.uint8)) for _ in range(5000)]
    gpu_ctx.set_targets(algo, b"".join(targets))
    data, offs = pack_words(words)
    hits, st = gpu_ctx.expand_digest(data, offs, mode, 0, 15)
    oracle_out, _ = co.CTable([table_path("czech"), table_path("german")]).expand_batch(data, offs, mode, 0, 15)
    assert st["candidates"] == oracle_out.count(b"\n")
    got = {}
    for w, c, d in hits:
        assert len(d) == W and f(per_word[w][c]) == d  # the reported candidate really has that digest
        got.setdefault(d, set()).add((w, c))
    for d, (w, c) in planted.items():
        assert (w, c) in got.get(d, set()), (per_word[w][c], d.hex())
    assert set(got) == set(planted)


def _one_real_digest(ctx, algo):
    words, per_word = _per_word(ctx, 0)
    w0 = next(w for w in range(len(words)) if len(per_word[w]) > 3)
    plain = per_word[w0][2]
    where = {(w, c) for w, cs in enumerate(per_word) for c, x in enumerate(cs) if x == plain}
    return words, w0, REF[algo](plain), where


def _flip(b):
    return bytes(x ^ 0x5A for x in b)


@ALGOS
def test_the_tail_is_compared_whole(gpu_ctx, algo):
    """Targets equal to a real digest D except in the first tail word, or in the last 4
    bytes only, or with a zero 16-byte prefix, must not hit; D hits exactly where its plain
    occurs."""
    from hashcat_a5_table_generator_amd import pack_words
    words, w0, D, where = _one_real_digest(gpu_ctx, algo)
    W = SIZE[algo]
    rng = np.random.default_rng(3)
    forged_first = D[:16] + _flip(D[16:20]) + D[20:]
    forged_last = D[:-4] + _flip(D[-4:])
    zero = bytes(16) + bytes(rng.integers(0, 256, size=W - 16, dtype=np.uint8))
    forged = forged_first + forged_last + zero
    assert len(forged) == 3 * W
    data, offs = pack_words(words)
    gpu_ctx.set_targets(algo, forged + D)
    hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
    assert {(w, c) for w, c, _ in hits} == where and len(hits) == len(where)
    assert all(d == D for _, _, d in hits)
    gpu_ctx.set_targets(algo, forged)
    hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
    assert hits == []


@ALGOS
def test_shared_prefix_reports_the_digest_that_matched(gpu_ctx, algo):
    """D and a target that differs from it in the last 4 bytes only share every byte a 4-word
    tail record holds (SHA-384, SHA-512): hit_digest and format_hits must still name D."""
    from hashcat_a5_table_generator_amd import pack_words
    words, w0, D, where = _one_real_digest(gpu_ctx, algo)
    forged_last = D[:-4] + _flip(D[-4:])
    data, offs = pack_words(words)
    for targets in (forged_last + D, D + forged_last):
        gpu_ctx.set_targets(algo, targets)
        hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
        assert {(w, c) for w, c, _ in hits} == where and len(hits) == len(where)
        assert all(d == D for _, _, d in hits)
        assert gpu_ctx.hit_digest((w0, 2, D[:16])) == D
        lines = gpu_ctx.format_hits(data, offs, [(w, c, d[:16]) for w, c, d in hits]).split(b"\n")[:-1]
        assert len(lines) == len(hits)
        assert all(ln.split(b":", 1)[0] == D.hex().encode() for ln in lines)


@ALGOS
def test_lookup_small_scratch_ranges(gpu_ctx, algo):
    """A scratch far smaller than the batch's output: many expand + digest ranges, the
    same hits as the full enumeration."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    _load(gpu_ctx, ["czech", "german"])
    if "small" not in _per_word_cache:
        words = _words(5, 1500)
        _per_word_cache["small"] = (words, gpu_ctx.expand_words(words, 0, 0, 15))
    words, per_word = _per_word_cache["small"]
    f = REF[algo]
    pl = [(w, len(per_word[w]) - 1) for w in range(0, len(words), 97) if per_word[w]]
    tg = {f(per_word[w][c]) for w, c in pl}
    gpu_ctx.set_targets(algo, b"".join(sorted(tg)))
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(gpu_ctx, data), DeviceBuffer.from_array(gpu_ctx, offs)
    hits, st = gpu_ctx.expand_digest_device(dw.ptr, do.ptr, len(words), 0, 0, 15, scratch_bytes=50_000)
    assert st["expand_launches"] > 3
    want = sorted((w, c) for w, cs in enumerate(per_word) for c, x in enumerate(cs) if f(x) in tg)
    assert sorted((w, c) for w, c, _ in hits) == want  # every candidate with a target digest, once


@ALGOS
@pytest.mark.parametrize("mode", [0, 3])
def test_digest_ranges_partition_the_hits(gpu_ctx, algo, mode):
    """[0, total) cut at three candidates inside words: the four ranges' hits are disjoint
    and their union is the whole batch's (every 7th candidate is a target)."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    words, per_word = _per_word(gpu_ctx, mode)
    f = REF[algo]
    cnt = np.array([len(x) for x in per_word], dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum(cnt)])
    tc = int(coff[-1])
    flat = [c for w in per_word for c in w]
    targets = {f(flat[g]) for g in range(0, tc, 7)}
    gpu_ctx.set_targets(algo, b"".join(sorted(targets)))
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(gpu_ctx, data), DeviceBuffer.from_array(gpu_ctx, offs)

    def hits(cb=0, ce=None):
        h, st = gpu_ctx.expand_digest_device(dw.ptr, do.ptr, len(words), mode, 0, 15, hit_cap=1 << 18,
                                             cand_begin=cb, cand_end=ce)
        assert st["candidates"] == (tc if ce is None else ce) - cb
        assert len({(w, c) for w, c, _ in h}) == len(h)  # no duplicates
        return {(int(w), int(c)) for w, c, _ in h}

    full = hits()
    assert full == {(w, c) for w, cs in enumerate(per_word) for c, x in enumerate(cs) if f(x) in targets}
    inner = [w for w in range(len(words)) if cnt[w] >= 3]  # words a cut can fall inside
    cuts = [int(coff[w]) + int(cnt[w]) // 2 for w in (inner[len(inner) // 4], inner[len(inner) // 2], inner[3 * len(inner) // 4])]
    cuts = [0] + cuts + [tc]
    assert cuts == sorted(set(cuts))
    union = set()
    for a, b in zip(cuts, cuts[1:]):
        part = hits(a, b)
        assert all(a <= coff[w] + c < b for w, c in part), (a, b)
        assert not (part & union)
        union |= part
    assert union == full


@ALGOS
def test_format_hits_prints_the_full_width_digest(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import format_plain, pack_words
    f, W = REF[algo], SIZE[algo]
    gpu_ctx.clear_table()
    gpu_ctx.set_table({b"a": [b"b", b"4"], b"e": [b"3"]})
    try:
        words = [b"banana", b"za\x01q", b"tee"]  # (the second word's plains need $HEX[])
        per_word = gpu_ctx.expand_words(words, 0, 0, 15)
        assert all(per_word)
        plains = {(w, c): per_word[w][c] for w in range(3) for c in (0, len(per_word[w]) - 1)}
        gpu_ctx.set_targets(algo, b"".join(f(p) for p in plains.values()))
        data, offs = pack_words(words)
        hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
        assert {(w, c) for w, c, _ in hits} == set(plains)
        want = sorted(f(p).hex().encode() + b":" + format_plain(p) for p in plains.values())
        for hs in (hits, [(w, c, d[:16]) for w, c, d in hits]):  # the full digest or its first 16 bytes
            lines = gpu_ctx.format_hits(data, offs, hs).split(b"\n")[:-1]
            assert sorted(lines) == want
            assert all(len(ln.split(b":", 1)[0]) == 2 * W for ln in lines)  # 56 / 96 / 128 hex digits
        assert any(b":$HEX[" in ln for ln in want)
    finally:
        gpu_ctx.clear_table()


@ALGOS
def test_cli_hashes_mode(tmp_path, algo):
    """--hashes with --algo by name and by hashcat mode number: full-width hex targets, a
    potfile-style line, and a 32-digit line that is counted as skipped."""
    from hashcat_a5_table_generator_amd import Context, format_plain
    f, W = REF[algo], SIZE[algo]
    words = [b"strasse", b"hello", b"zuerich"]
    (tmp_path / "d.txt").write_bytes(b"\n".join(words) + b"\n")
    tabs = [table_path("czech"), table_path("german")]
    with Context(0) as c:
        c.load_tables(tabs)
        per_word = c.expand_words(words, 0, 0, 15)
    assert all(per_word)
    plains = [per_word[0][-1], per_word[1][0], per_word[2][len(per_word[2]) // 2]]
    lines = [f(plains[0]).hex(), f(plains[1]).hex(), f(plains[2]).hex().upper() + ":potfile-plain",
             hashlib.md5(b"x").hexdigest()]
    (tmp_path / "h.txt").write_text("\n".join(lines) + "\n")
    for how in (NAME[algo], HASHCAT_MODE[algo]):
        r = subprocess.run([CLI, str(tmp_path / "d.txt"), "-t", ",".join(tabs), "--hashes", str(tmp_path / "h.txt"),
                            "--algo", how], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        got = r.stdout.split(b"\n")[:-1]
        assert sorted(got) == sorted(f(p).hex().encode() + b":" + format_plain(p) for p in set(plains))
        assert b"1 line(s)" in r.stderr and b"%d-hex-digit" % (2 * W) in r.stderr


def test_switching_target_sets_leaves_no_stale_tails(gpu_ctx):
    """The same context: SHA-512 targets, then MD5, then SHA-224."""
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word = _per_word(gpu_ctx, 0)
    data, offs = pack_words(words)
    pl = [(w, 0) for w in range(0, len(words), 37) if per_word[w]]
    for algo, f in ((SHA512, REF[SHA512]), (0, lambda b: hashlib.md5(b).digest()), (SHA224, REF[SHA224])):
        tg = {f(per_word[w][c]) for w, c in pl}
        gpu_ctx.set_targets(algo, b"".join(sorted(tg)))
        hits, _ = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
        want = {(w, c): f(x) for w, cs in enumerate(per_word) for c, x in enumerate(cs) if f(x) in tg}
        assert {(w, c): d for w, c, d in hits} == want and len(hits) == len(want)
        assert all(gpu_ctx.hit_digest(h) == h[2] for h in hits)
