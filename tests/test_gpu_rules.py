"""hashcat rules in the digest + lookup stage on the GPU (k_rules_stream, a5x_rules.hip): every
(line, rule) digest against hashlib / RFC MD4 of the Python rule oracle's output for all four
algorithms, lines at the stream-block edges and over the 128-byte cap, planted (word,
candidate, rule) triples through every mode, small scratch, candidate ranges, the hit cap,
no change without rules, and the ruled hash:plain output of format_hits and the CLI."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import rule_oracle as ro
from conftest import ROOT, table_path
from oracle import digest_oracle

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "hashcat_a5_table_generator_amd", "_build", "a5x_generator")
MD5, NTLM, SHA1, SHA256 = 0, 1, 2, 3
REF = {MD5: lambda b: hashlib.md5(b).digest(), NTLM: functools.lru_cache(maxsize=None)(digest_oracle.ntlm),
       SHA1: lambda b: hashlib.sha1(b).digest(), SHA256: lambda b: hashlib.sha256(b).digest()}
SIZE = {MD5: 16, NTLM: 16, SHA1: 20, SHA256: 32}
ALGOS = pytest.mark.parametrize("algo", [MD5, NTLM, SHA1, SHA256], ids=["md5", "ntlm", "sha1", "sha256"])
RULES_BLOCK = 4096  # STREAM_BLK of a5x_stream.h
LMAX = 128

# every function at least once; growth rules that carry the long lines (53..128 bytes) across
# the padding edges 55/56, 63/64, 119/120 and up to / over the 128 cap
EVERY = [b":", b"l", b"u", b"c", b"C", b"t", b"T0", b"r", b"d", b"p2", b"f", b"{", b"}", b"$1", b"^1", b"[", b"]",
         b"D3", b"x04", b"O12", b"i4!", b"o3$", b"'6", b"sa4", b"@a", b"z2", b"Z2", b"q", b"k", b"K", b"*03", b"L2",
         b"R2", b"+2", b"-1", b".1", b",1", b"y2", b"Y2", b"E", b"ea", b"$1$2", b"$1$2$3$4$5$6$7$8$9", b"y1",
         b"y5Y4", b"^a^b^c", b"dp1", b"$ "]


@pytest.fixture(autouse=True)
def _no_rules_left_behind(gpu_ctx):
    yield
    gpu_ctx.clear_rules()


FILLER = list(b"bfghjklmpqvwxBFGH 19-")  # no key or value of the czech / german tables
TOKENS = [b"a", b"e", b"s", b"A", b"S", b"z", "á".encode(), "š".encode(), "ä".encode(), "é".encode()]


def _words(seed, n, max_tokens=2, lo=1, hi=13):
    """n words of filler bytes with 1..max_tokens substitutable tokens (keys for the default
    and -s modes, values for -r): a few candidates per word, so that the pure-Python
    references stay cheap."""
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


def _expanded_lines(ctx, words):
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
    tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, len(words))
    out = DeviceBuffer(ctx, tb + 64)
    ctx.expand_device(dw.ptr, do.ptr, len(words), out.ptr, tb)
    lines = bytes(out.to_array(count=tb)).split(b"\n")[:-1]
    assert len(lines) == tc
    return out, tb, lines


_cache = {}


def _ruled(lines, rules):
    """oracle output of every (line, rule); None for a line over the cap"""
    ops = [ro.parse_line(r) for r in rules]
    return [None if len(ln) > LMAX else [ro.apply_ops(ln, o) for o in ops] for ln in lines]


def _check_every_digest(ctx, algo, out, tb, lines, rules, want):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    W, f, R = SIZE[algo], REF[algo], len(rules)
    assert ctx.set_rules(rules) == (R, 0)
    dig = DeviceBuffer(ctx, W * len(lines) * R + 16)
    n = ctx.digest_lines_rules_device(algo, out.ptr, tb, dig.ptr, len(lines) * R)
    assert n == len(lines)
    got = dig.to_array(count=W * n * R).reshape(n, R, W)
    bad = []
    for i, ln in enumerate(lines):
        for r in range(R):
            exp = bytes(W) if want[i] is None else f(want[i][r])
            if bytes(got[i, r]) != exp:
                bad.append((len(ln), ln[:24], rules[r], bytes(got[i, r]).hex(), exp.hex()))
    assert not bad, (len(bad), bad[:5])
    over = sum(1 for ln in lines if len(ln) > LMAX)
    assert ctx.rules_last() == ((len(lines) - over) * R, over)
    return over


@ALGOS
def test_every_digest_under_every_function(gpu_ctx, algo):
    _load(gpu_ctx, ["czech", "german"])
    if "every" not in _cache:  # one expansion and one oracle pass, shared by the four algorithms
        words = _words(2, 300) + [b"1" * (n - 1) + b"a" for n in (54, 55, 56, 63, 64, 119, 120, 127, 128, 129, 200)]
        out, tb, lines = _expanded_lines(gpu_ctx, words)
        _cache["every"] = (out, tb, lines, _ruled(lines, EVERY))
    out, tb, lines, want = _cache["every"]
    used = {op[0] for r in EVERY for op in ro.parse_line(r)}
    assert used == set(ro.KINDS)
    lens = {len(x) for w in want if w for x in w}
    assert {55, 56, 63, 64, 119, 120, 128} <= lens  # the padding edges are reached by ruled words
    over = _check_every_digest(gpu_ctx, algo, out, tb, lines, EVERY, want)
    assert over >= 2  # the 129- and 200-byte words' candidates


@ALGOS
def test_lines_straddle_the_stream_blocks(gpu_ctx, algo):
    """100-128 B lines (a 99-126 byte run + "a", whose substitutes are two bytes) at random
    offsets: every block edge cut at another phase."""
    _load(gpu_ctx, ["czech"])
    rules = [b":", b"r", b"$1", b"^1", b"]", b"u"]
    if "edges" not in _cache:
        rng = np.random.default_rng(11)
        out, tb, lines = _expanded_lines(gpu_ctx, [b"1" * int(k) + b"a" for k in rng.integers(99, 127, size=200)])
        _cache["edges"] = (out, tb, lines, _ruled(lines, rules))
    out, tb, lines, want = _cache["edges"]
    assert tb > 3 * RULES_BLOCK and all(100 <= len(ln) <= 128 for ln in lines)
    _check_every_digest(gpu_ctx, algo, out, tb, lines, rules, want)


LOOKUP_RULES = [b":", b"l", b"u", b"c", b"$1", b"^1", b"sa@", b"r", b"d", b"T0", b"]", b"[", b"c$1", b"$1$2$3", b"t",
                b"se3", b"f", b"{", b"k", b"'4"]


def _per_word(ctx, mode):
    """400 words under czech + german, the library's per-word candidates and the oracle's
    output of every (candidate, rule), per mode."""
    _load(ctx, ["czech", "german"])
    key = ("pw", mode)
    if key not in _cache:
        words = _words(100 + mode, 400, max_tokens=4, lo=4, hi=17)
        per_word = ctx.expand_words(words, mode, 0, 15)
        ops = [ro.parse_line(r) for r in LOOKUP_RULES]
        ruled = [[[ro.apply_ops(x, o) for o in ops] for x in cs] for cs in per_word]
        _cache[key] = (words, per_word, ruled)
    return _cache[key]


def _hits_with_rules(ctx, call):
    hits, st = call()
    rules = ctx.last_hit_rules()
    assert len(rules) == len(hits)
    return [(int(w), int(c), int(r), d) for (w, c, d), r in zip(hits, rules)], st


@ALGOS
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_lookup_planted_triples(gpu_ctx, algo, mode):
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word, ruled = _per_word(gpu_ctx, mode)
    f, W, R = REF[algo], SIZE[algo], len(LOOKUP_RULES)
    rng = np.random.default_rng(9 + algo)
    targets = set()
    for w in rng.choice([w for w in range(len(words)) if per_word[w]], size=30, replace=False):
        c, r = int(rng.integers(0, len(per_word[w]))), int(rng.integers(0, R))
        targets.add(f(ruled[w][c][r]))
    assert len(targets) > 20
    tl = sorted(targets) + [bytes(rng.integers(0, 256, size=W, dtype=np.uint8)) for _ in range(5000)]
    gpu_ctx.set_targets(algo, b"".join(tl))
    assert gpu_ctx.set_rules(LOOKUP_RULES) == (R, 0)
    data, offs = pack_words(words)
    hits, st = _hits_with_rules(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, mode, 0, 15))
    ncand = sum(len(cs) for cs in per_word)
    assert st["candidates"] == ncand  # not multiplied by R
    assert gpu_ctx.rules_last() == (ncand * R, 0)
    # exhaustively: every (word, cand, rule) whose ruled plain hashes to a target
    want = {(w, c, r) for w, cs in enumerate(ruled) for c, rs in enumerate(cs) for r, x in enumerate(rs)
            if f(x) in targets}
    assert len(hits) == len(want) and {(w, c, r) for w, c, r, _ in hits} == want
    assert all(len(d) == W and d == f(ruled[w][c][r]) for w, c, r, d in hits)


def test_two_rules_one_output_give_two_hits(gpu_ctx):
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word, _ = _per_word(gpu_ctx, 0)
    pl = [(w, len(per_word[w]) - 1) for w in range(0, len(words), 41) if per_word[w]]
    tg = {hashlib.md5(per_word[w][c]).digest() for w, c in pl}
    gpu_ctx.set_targets(MD5, b"".join(sorted(tg)))
    assert gpu_ctx.set_rules([b":", b"T0T0"]) == (2, 0)
    data, offs = pack_words(words)
    hits, _ = _hits_with_rules(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, 0, 0, 15))
    where = {(w, c) for w, cs in enumerate(per_word) for c, x in enumerate(cs) if hashlib.md5(x).digest() in tg}
    assert set(pl) <= where
    assert sorted((w, c, r) for w, c, r, _ in hits) == sorted((w, c, r) for w, c in where for r in (0, 1))


@ALGOS
def test_small_scratch_and_candidate_ranges(gpu_ctx, algo):
    """Many expand + digest ranges give the same hit set; [0, total) cut at three candidates
    inside words partitions it."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
    words, per_word, ruled = _per_word(gpu_ctx, 0)
    f, R = REF[algo], len(LOOKUP_RULES)
    cnt = np.array([len(x) for x in per_word], dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum(cnt)])
    tc = int(coff[-1])
    flat = [rs for cs in ruled for rs in cs]
    targets = {f(flat[g][g % R]) for g in range(0, tc, 7)}
    want = {(w, c, r) for w, cs in enumerate(ruled) for c, rs in enumerate(cs) for r, x in enumerate(rs)
            if f(x) in targets}
    gpu_ctx.set_targets(algo, b"".join(sorted(targets)))
    assert gpu_ctx.set_rules(LOOKUP_RULES) == (R, 0)
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(gpu_ctx, data), DeviceBuffer.from_array(gpu_ctx, offs)

    def hits(cb=0, ce=None, scratch=0):
        h, st = _hits_with_rules(gpu_ctx, lambda: gpu_ctx.expand_digest_device(
            dw.ptr, do.ptr, len(words), 0, 0, 15, scratch_bytes=scratch, hit_cap=1 << 18, cand_begin=cb, cand_end=ce))
        assert st["candidates"] == (tc if ce is None else ce) - cb
        got = {(w, c, r) for w, c, r, _ in h}
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


def test_hit_cap(gpu_ctx):
    from hashcat_a5_table_generator_amd import A5xError, DeviceBuffer, pack_words
    words, per_word, _ = _per_word(gpu_ctx, 0)
    flat = [x for cs in per_word for x in cs]
    tg = {hashlib.md5(x).digest() for x in flat[::3]}
    total = 2 * sum(1 for x in flat if hashlib.md5(x).digest() in tg)
    assert total > 64
    gpu_ctx.set_targets(MD5, b"".join(sorted(tg)))
    gpu_ctx.set_rules([b":", b"T0T0"])
    data, offs = pack_words(words)
    dw, do = DeviceBuffer.from_array(gpu_ctx, data), DeviceBuffer.from_array(gpu_ctx, offs)
    with pytest.raises(A5xError) as e:
        gpu_ctx.expand_digest_device(dw.ptr, do.ptr, len(words), 0, 0, 15, hit_cap=64)
    assert e.value.code == -8 and f"{total} hits" in str(e.value)  # A5X_E_CAPACITY, the total reported
    assert len(gpu_ctx.last_hit_rules()) == 64
    hits, _ = gpu_ctx.expand_digest_device(dw.ptr, do.ptr, len(words), 0, 0, 15, hit_cap=total)
    assert len(hits) == total


@ALGOS
def test_no_rules_no_change(gpu_ctx, algo):
    """clear_rules() restores the hits and stats taken before any rules were set; the rule
    set ':' alone finds the same (word, cand) set, with rule 0."""
    from hashcat_a5_table_generator_amd import pack_words
    words, per_word, _ = _per_word(gpu_ctx, 0)
    f = REF[algo]
    tg = {f(cs[len(cs) // 2]) for cs in per_word[::13] if cs}
    gpu_ctx.set_targets(algo, b"".join(sorted(tg)))
    data, offs = pack_words(words)
    keys = ("candidates", "bytes", "words", "expand_launches", "words_slow", "words_pass_b")

    def plain_run():
        hits, st = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
        assert gpu_ctx.last_hit_rules() == []
        return sorted(hits), {k: st[k] for k in keys}

    before = plain_run()
    assert gpu_ctx.set_rules([b":"]) == (1, 0)
    hits, st = _hits_with_rules(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, 0, 0, 15))
    assert sorted((w, c, d) for w, c, _, d in hits) == before[0] and all(r == 0 for _, _, r, _ in hits)
    assert st["candidates"] == before[1]["candidates"]
    gpu_ctx.clear_rules()
    assert gpu_ctx.rule_count() == 0
    assert plain_run() == before


def test_format_hits_prints_the_ruled_plain(gpu_ctx):
    from hashcat_a5_table_generator_amd import format_plain, pack_words
    gpu_ctx.clear_table()
    gpu_ctx.set_table({b"a": [b"b", b"4"], b"e": [b"3"]})
    try:
        words = [b"banana", b"zaq", b"tee"]
        rules = [b"c$1", b"i1\x01", b"r"]  # (the second rule's plains need $HEX[])
        per_word = gpu_ctx.expand_words(words, 0, 0, 15)
        assert all(per_word)
        triples = [(w, c, r) for w in range(3) for c in (0, len(per_word[w]) - 1) for r in (w, (w + 1) % 3)]
        plains = {t: ro.apply_rule(rules[t[2]], per_word[t[0]][t[1]]) for t in triples}
        sha1 = lambda b: hashlib.sha1(b).digest()
        gpu_ctx.set_targets(SHA1, b"".join(sha1(p) for p in plains.values()))
        assert gpu_ctx.set_rules(rules) == (3, 0)
        data, offs = pack_words(words)
        hits, _ = _hits_with_rules(gpu_ctx, lambda: gpu_ctx.expand_digest(data, offs, 0, 0, 15))
        assert set(plains) <= {(w, c, r) for w, c, r, _ in hits}
        want = sorted(sha1(ro.apply_rule(rules[r], per_word[w][c])).hex().encode() + b":" +
                      format_plain(ro.apply_rule(rules[r], per_word[w][c])) for w, c, r, _ in hits)
        lines = gpu_ctx.format_hits(data, offs, [(w, c, d) for w, c, _, d in hits],
                                    rules=[r for _, _, r, _ in hits]).split(b"\n")[:-1]
        assert sorted(lines) == want
        assert any(b":$HEX[" in ln for ln in lines) and any(b":$HEX[" not in ln for ln in lines)
    finally:
        gpu_ctx.clear_table()


def test_cli_hashes_with_rules(tmp_path):
    from hashcat_a5_table_generator_amd import Context, format_plain
    words = [b"strasse", b"hello", b"zuerich", b"a" + b"x" * 139]
    (tmp_path / "d.txt").write_bytes(b"\n".join(words) + b"\n")
    (tmp_path / "r.rule").write_bytes(b"# best of\r\n:\r\nc$1\r\nM\r\nu\n")
    rules = [b":", b"c$1", b"u"]
    tabs = [table_path("czech"), table_path("german")]
    with Context(0) as c:
        c.load_tables(tabs)
        per_word = c.expand_words(words, 0, 0, 15)
    assert all(per_word[:3])
    over = sum(1 for x in per_word[3] if len(x) > 128)
    assert over >= 1
    plains = [ro.apply_rule(rules[1], per_word[0][-1]), ro.apply_rule(rules[2], per_word[1][0]),
              ro.apply_rule(rules[0], per_word[2][len(per_word[2]) // 2])]
    (tmp_path / "h.txt").write_text("\n".join(hashlib.sha1(p).hexdigest() for p in plains) + "\n")
    r = subprocess.run([CLI, str(tmp_path / "d.txt"), "-t", ",".join(tabs), "--hashes", str(tmp_path / "h.txt"),
                        "--algo", "sha1", "--rules", str(tmp_path / "r.rule")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    got = r.stdout.split(b"\n")[:-1]
    assert sorted(got) == sorted(hashlib.sha1(p).hexdigest().encode() + b":" + format_plain(p) for p in set(plains))
    assert b"3 accepted, 1 line(s) skipped" in r.stderr
    assert b"%d candidate(s) longer than 128 bytes rejected" % over in r.stderr
