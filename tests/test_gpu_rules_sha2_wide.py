"""hashcat rules with SHA-224 / SHA-384 / SHA-512 on the GPU (k_rules_stream): every (line,
rule) digest against hashlib of the host rule interpreter's output, with ruled words on the
padding edges of both block sizes and a line over the 128-byte cap, and lookups of planted
(word, candidate, rule) triples whose hits name the rule and print at full width."""
import hashlib

import numpy as np
import pytest

from conftest import table_path

pytestmark = pytest.mark.gpu

SHA224, SHA384, SHA512 = 5, 6, 7
REF = {SHA224: lambda b: hashlib.sha224(b).digest(), SHA384: lambda b: hashlib.sha384(b).digest(),
       SHA512: lambda b: hashlib.sha512(b).digest()}
SIZE = {SHA224: 28, SHA384: 48, SHA512: 64}
ALGOS = pytest.mark.parametrize("algo", [SHA224, SHA384, SHA512], ids=["sha224", "sha384", "sha512"])
LMAX = 128
RULES = [b":", b"l", b"u", b"c", b"r", b"d", b"$1", b"^!", b"$1$2$3$4$5$6$7$8$9"]
# line lengths (a word of filler bytes and one final "a", which the czech / german tables turn
# into a two-byte letter).  With the rules above the ruled words have 55 / 56 (SHA-224's edge;
# 28 doubled), 111 / 112 and 127 / 128 bytes (SHA-384 / SHA-512's edges and the cap; 64
# doubled, 118 / 119 + 9)
LINE_LENGTHS = (3, 7, 28, 54, 55, 56, 64, 103, 110, 111, 112, 118, 119, 126, 127, 128)
OVER = 131  # rejected: hashed under no rule


@pytest.fixture(autouse=True)
def _no_rules_left_behind(gpu_ctx):
    yield
    gpu_ctx.clear_rules()


def _load(ctx, tabs):
    ctx.clear_table()
    ctx.load_tables([table_path(t) for t in tabs])


_cache = {}


def _lines(ctx):
    """The expanded stream of the fixed-length lines and the host's ruled words."""
    from hashcat_a5_table_generator_amd import DeviceBuffer, apply_rule, pack_words
    _load(ctx, ["czech", "german"])
    if "lines" not in _cache:
        words = [(b"bH" + b"1" * n)[:n - 2] + b"a" for n in LINE_LENGTHS + (OVER,)]
        data, offs = pack_words(words)
        dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
        tc, tb = ctx.keyspace_device(dw.ptr, do.ptr, len(words))
        out = DeviceBuffer(ctx, tb + 64)
        ctx.expand_device(dw.ptr, do.ptr, len(words), out.ptr, tb)
        lines = bytes(out.to_array(count=tb)).split(b"\n")[:-1]
        assert {len(ln) for ln in lines} == set(LINE_LENGTHS + (OVER,))
        ruled = [None if len(ln) > LMAX else [apply_rule(r, ln) for r in RULES] for ln in lines]
        _cache["lines"] = (out, tb, lines, ruled)
    return _cache["lines"]


@ALGOS
def test_every_ruled_digest(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    out, tb, lines, ruled = _lines(gpu_ctx)
    lens = {len(x) for rs in ruled if rs for x in rs}
    assert {55, 56, 111, 112, 127, 128} <= lens and max(lens) == LMAX
    W, f, R = SIZE[algo], REF[algo], len(RULES)
    assert gpu_ctx.set_rules(RULES) == (R, 0)
    dig = DeviceBuffer(gpu_ctx, W * len(lines) * R + 16)
    n = gpu_ctx.digest_lines_rules_device(algo, out.ptr, tb, dig.ptr, len(lines) * R)
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
    assert over >= 1 and gpu_ctx.rules_last() == ((len(lines) - over) * R, over)


LOOKUP_RULES = [b":", b"u", b"c$1", b"r", b"d", b"^!", b"$1$2$3"]


def _per_word(ctx, mode):
    from hashcat_a5_table_generator_amd import apply_rule
    _load(ctx, ["czech", "german"])
    if mode not in _cache:
        rng = np.random.default_rng(70 + mode)
        alpha = list(b"abcdefghijklmnopqrstuvwxyzs")
        words = [np.asarray(rng.choice(alpha, size=int(rng.integers(1, 13))), dtype=np.uint8).tobytes() for _ in range(400)]
        per_word = ctx.expand_words(words, mode, 0, 15)
        picks = []  # 30 (word, cand, rule) triples and their ruled plains
        for w in rng.choice([w for w in range(len(words)) if per_word[w]], size=30, replace=False):
            c, r = int(rng.integers(0, len(per_word[w]))), int(rng.integers(0, len(LOOKUP_RULES)))
            picks.append((int(w), c, r, apply_rule(LOOKUP_RULES[r], per_word[w][c])))
        _cache[mode] = (words, per_word, picks)
    return _cache[mode]


@ALGOS
@pytest.mark.parametrize("mode", [0, 3])
def test_lookup_planted_triples(gpu_ctx, algo, mode):
    from hashcat_a5_table_generator_amd import apply_rule, format_plain, pack_words
    words, per_word, picks = _per_word(gpu_ctx, mode)
    f, W, R = REF[algo], SIZE[algo], len(LOOKUP_RULES)
    rng = np.random.default_rng(9 + algo)
    targets = {f(p) for _, _, _, p in picks}
    tl = sorted(targets) + [bytes(rng.integers(0, 256, size=W, dtype=np.uint8)) for _ in range(5000)]
    gpu_ctx.set_targets(algo, b"".join(tl))
    assert gpu_ctx.set_rules(LOOKUP_RULES) == (R, 0)
    data, offs = pack_words(words)
    hits, st = gpu_ctx.expand_digest(data, offs, mode, 0, 15)
    rules = gpu_ctx.last_hit_rules()
    assert len(rules) == len(hits)
    ncand = sum(len(cs) for cs in per_word)
    assert st["candidates"] == ncand and gpu_ctx.rules_last() == (ncand * R, 0)
    got = {(int(w), int(c), int(r)): d for (w, c, d), r in zip(hits, rules)}
    assert len(got) == len(hits)
    for w, c, r, p in picks:  # every planted triple, under its rule
        assert got.get((w, c, r)) == f(p), (w, c, LOOKUP_RULES[r], p)
    for (w, c, r), d in got.items():  # and nothing that is not a target's plain
        assert len(d) == W and d in targets and d == f(apply_rule(LOOKUP_RULES[r], per_word[w][c]))
    lines = gpu_ctx.format_hits(data, offs, hits, mode, 0, 15, rules=rules).split(b"\n")[:-1]
    want = sorted(d.hex().encode() + b":" + format_plain(apply_rule(LOOKUP_RULES[r], per_word[w][c]))
                  for (w, c, r), d in got.items())
    assert sorted(lines) == want
    assert all(len(ln.split(b":", 1)[0]) == 2 * W for ln in lines)
