"""The rule corpus of tests/rule_fuzz.py on the GPU (k_rules_stream in its three translation
units, a5x_rules.hip / a5x_rules_wide.hip / a5x_rules_nest.hip): every (line, rule) digest of
a hand-built stream of arbitrary bytes against hashlib / RFC MD4 of the Python oracle's ruled
word, for every function at every position and for chains of up to 31 functions; the same
digests whatever rule ran before on the lane (reversed order, a grower or an emptying rule
in front of every rule); and a lookup whose hits name rules past index 255.  The host build of
the interpreter passes this corpus on the CPU (test_rule_fuzz.py), so a mismatch here is in
device-only code: the v_perm / v_alignbyte branches, the lane buffer, the candidate load, the
`dirty` zeroing between rules."""
import functools
import hashlib

import numpy as np
import pytest

import rule_fuzz as rf
import rule_oracle as ro
from oracle import digest_oracle

pytestmark = pytest.mark.gpu

MD5, NTLM, SHA1, SHA512, MD5_MD5, MD5_SHA1 = 0, 1, 2, 7, 16, 19


def _md5(b):
    return hashlib.md5(b).digest()


REF = {MD5: _md5, NTLM: functools.lru_cache(maxsize=None)(digest_oracle.ntlm),
       SHA1: lambda b: hashlib.sha1(b).digest(), SHA512: lambda b: hashlib.sha512(b).digest(),
       MD5_MD5: lambda b: _md5(_md5(b).hex().encode()),
       MD5_SHA1: lambda b: _md5(hashlib.sha1(b).hexdigest().encode())}
SIZE = {MD5: 16, NTLM: 16, SHA1: 20, SHA512: 64, MD5_MD5: 16, MD5_SHA1: 16}
NAME = {MD5: "md5", NTLM: "ntlm", SHA1: "sha1", SHA512: "sha512", MD5_MD5: "md5-md5", MD5_SHA1: "md5-sha1"}
# one algorithm or more of each translation unit; SHA-1 has the big-endian source, the two
# nested ones both inner digests
EVERY_UNIT = [MD5, SHA1, SHA512, MD5_MD5, MD5_SHA1]
# NTLM's reference is pure Python (~160 us a word): every 3rd chain x every 2nd line, a cap
NTLM_CHAIN_STRIDE, NTLM_LINE_STRIDE, NTLM_WORDS_MAX = 3, 2, 30_000


def _ids(algos):
    return [NAME[a] for a in algos]


@pytest.fixture(autouse=True)
def _no_rules_left_behind(gpu_ctx):
    yield
    gpu_ctx.clear_rules()


_cache = {}


def _stream(ctx):
    """The corpus' lines as one "cand\\n" stream on the device (the last line without newline)."""
    from hashcat_a5_table_generator_amd import DeviceBuffer
    if "stream" not in _cache:
        ls = rf.lines()
        s = rf.stream(ls)
        buf = DeviceBuffer.from_array(ctx, np.frombuffer(s + b"\0" * 64, dtype=np.uint8))
        _cache["stream"] = (buf, len(s), ls)
    return _cache["stream"]


def _digests(ctx, algo, rules):
    """(lines, rules, width) digest bytes of the stream under the rules, and the counters."""
    from hashcat_a5_table_generator_amd import DeviceBuffer
    buf, nbytes, ls = _stream(ctx)
    W, R = SIZE[algo], len(rules)
    assert ctx.set_rules(rules) == (R, 0)
    dig = DeviceBuffer(ctx, W * len(ls) * R + 16)
    try:
        n = ctx.digest_lines_rules_device(algo, buf.ptr, nbytes, dig.ptr, len(ls) * R)
        assert n == len(ls)
        got = dig.to_array(count=W * n * R).reshape(n, R, W)
    finally:
        dig.free()
    over = sum(1 for ln in ls if len(ln) > rf.LMAX)
    assert over == len(rf.OVER) and ctx.rules_last() == ((len(ls) - over) * R, over)
    return got


def _index(kind):
    """The corpus' distinct ruled words and, per (line, rule), the index of its word (the
    last index, one past the words, for a line over the cap): once per session."""
    if ("index", kind) not in _cache:
        rules, ls, ruled, _ = rf.corpus(kind)
        ids = {}
        idx = np.empty((len(ls), len(rules)), dtype=np.int32)
        for i, row in enumerate(ruled):
            idx[i] = -1 if row is None else [ids.setdefault(w, len(ids)) for w in row]
        idx[idx < 0] = len(ids)
        _cache[("index", kind)] = (list(ids), idx)
    return _cache[("index", kind)]


def _expected(kind, algo, rows=slice(None), cols=slice(None)):
    """The expected (lines, rules, width) byte block: the reference digest of every distinct
    ruled word once, gathered by index; all-zero digests for a line over the cap."""
    words, idx = _index(kind)
    idx = idx[rows, cols]
    W, f = SIZE[algo], REF[algo]
    need = np.unique(idx)
    table = np.zeros((len(words) + 1, W), dtype=np.uint8)
    used = need[need < len(words)]
    table[used] = np.frombuffer(b"".join(f(words[j]) for j in used), dtype=np.uint8).reshape(-1, W)
    return table[idx], len(used)


def _host_agrees(rule, line):
    from hashcat_a5_table_generator_amd import apply_rule
    try:
        return apply_rule(rule, line) == ro.apply_rule(rule, line)
    except Exception as e:  # (the zero-tail check of the host hook, a refused line)
        return repr(e)


def _compare(kind, got, exp, rows=slice(None), cols=slice(None)):
    rules, ls, ruled, _ = rf.corpus(kind)
    assert got.shape == exp.shape
    bad = np.argwhere((got != exp).any(axis=2))
    if len(bad):
        rsel, lsel = np.arange(len(rules))[cols], np.arange(len(ls))[rows]
        st = rf.starts(ls)
        report = []
        for i, r in bad[:5]:
            i, r = int(lsel[i]), int(rsel[r])
            report.append({"rule": rules[r], "rule_index": r, "line_len": len(ls[i]), "start_mod_4": int(st[i]) & 3,
                           "ruled_len": None if ruled[i] is None else len(ruled[i][r]),
                           "host_agrees_with_oracle": None if ruled[i] is None else _host_agrees(rules[r], ls[i])})
        pytest.fail(f"{len(bad)} of {got.shape[0] * got.shape[1]} (line, rule) digests differ; first: {report}")


@pytest.mark.parametrize("algo", EVERY_UNIT, ids=_ids(EVERY_UNIT))
def test_grid_every_digest(gpu_ctx, algo):
    """Every function at every position, a shrinking rule behind every growing one."""
    rules, ls, _, _ = rf.corpus("grid")
    got = _digests(gpu_ctx, algo, rules)
    exp, nwords = _expected("grid", algo)
    print(f"grid {NAME[algo]}: {got.shape[0] * got.shape[1]} digests, {nwords} distinct ruled words")
    _compare("grid", got, exp)


@pytest.mark.parametrize("algo", EVERY_UNIT + [NTLM], ids=_ids(EVERY_UNIT + [NTLM]))
def test_chains_every_digest(gpu_ctx, algo):
    """Chains of 1..31 functions.  Under NTLM the device runs every pair as well, and the
    pure-Python MD4 checks every NTLM_CHAIN_STRIDE-th chain on every NTLM_LINE_STRIDE-th line:
    at most NTLM_WORDS_MAX distinct ruled words."""
    rules, ls, _, _ = rf.corpus("chains")
    rows = cols = slice(None)
    if algo == NTLM:
        rows, cols = slice(None, None, NTLM_LINE_STRIDE), slice(None, None, NTLM_CHAIN_STRIDE)
        assert sum(1 for r in rules[cols] if len(rf.functions(r)) == rf.OPS_MAX) >= 10
    got = _digests(gpu_ctx, algo, rules)[rows, cols]
    exp, nwords = _expected("chains", algo, rows, cols)
    if algo == NTLM:
        assert 5_000 <= nwords <= NTLM_WORDS_MAX
    print(f"chains {NAME[algo]}: {got.shape[0] * got.shape[1]} digests, {nwords} distinct ruled words")
    _compare("chains", got, exp, rows, cols)


@pytest.mark.parametrize("algo", [MD5, SHA512], ids=_ids([MD5, SHA512]))
def test_rule_order_does_not_matter(gpu_ctx, algo):
    """A (line, rule) digest is the same whatever ran before it on the lane: the chains in the
    given and in the reversed order, and with a grower ('d') or a rule that empties the word
    ("'0") in front of every rule.  What the lane buffer holds between two rules is the
    kernel's business (`dirty`), not the interpreter's."""
    rules, ls, _, _ = rf.corpus("chains")
    R = len(rules)
    base = _digests(gpu_ctx, algo, rules)
    rev = _digests(gpu_ctx, algo, rules[::-1])
    assert np.array_equal(rev[:, ::-1], base)
    for pre in (b"d", b"'0"):
        both = _digests(gpu_ctx, algo, [x for r in rules for x in (pre, r)])
        bad = np.argwhere((both[:, 1::2] != base).any(axis=2))
        assert not len(bad), (pre, len(bad), [(len(ls[i]), rules[r]) for i, r in bad[:5].tolist()])
        assert (both[:, 0::2] == both[:, :1]).all()  # and the rule in front gives one digest a line
    assert R > 255


LOOKUP_WORDS = [b"banana", b"tea", b"a", b"e", b"", b"zebra", b"Area51", b"eagle", b"xyz", b"aaaa", b"sea!", b"e a"]


@pytest.mark.parametrize("algo", [MD5, SHA512], ids=_ids([MD5, SHA512]))
def test_lookup_names_rules_past_255(gpu_ctx, algo):
    from hashcat_a5_table_generator_amd import pack_words
    rules = rf.chain_rules()
    R, W, f = len(rules), SIZE[algo], REF[algo]
    assert R > 255 + 10
    gpu_ctx.clear_table()
    gpu_ctx.set_table({b"a": [b"b", b"\x01"], b"e": [b"3"]})
    try:
        if "lookup" not in _cache:
            per_word = gpu_ctx.expand_words(LOOKUP_WORDS, 0, 0, 15)
            ops = [ro.parse_line(r) for r in rules]
            _cache["lookup"] = (per_word, [[[ro.apply_ops(x, o) for o in ops] for x in cs] for cs in per_word])
        per_word, ruled = _cache["lookup"]
        assert sum(len(cs) for cs in per_word) >= 100
        rng = np.random.default_rng(77 + algo)
        flat = [(w, c) for w, cs in enumerate(per_word) for c in range(len(cs))]
        planted = []
        for k in range(40):  # every third one under a rule past index 255
            w, c = flat[int(rng.integers(0, len(flat)))]
            planted.append((w, c, int(rng.integers(256, R)) if k % 3 == 0 else int(rng.integers(0, 256))))
        assert sum(1 for _, _, r in planted if r > 255) >= 10
        targets = {f(ruled[w][c][r]) for w, c, r in planted}
        tl = sorted(targets) + [bytes(rng.integers(0, 256, size=W, dtype=np.uint8)) for _ in range(3000)]
        gpu_ctx.set_targets(algo, b"".join(tl))
        assert gpu_ctx.set_rules(rules) == (R, 0)
        data, offs = pack_words(LOOKUP_WORDS)
        hits, st = gpu_ctx.expand_digest(data, offs, 0, 0, 15, hit_cap=1 << 17)
        hit_rules = gpu_ctx.last_hit_rules()
        assert len(hit_rules) == len(hits) and st["candidates"] == len(flat)
        assert gpu_ctx.rules_last() == (len(flat) * R, 0)
        # exhaustively: every (word, candidate, rule) whose ruled word hashes to a target
        want = {(w, c, r): f(x) for w, cs in enumerate(ruled) for c, rs in enumerate(cs) for r, x in enumerate(rs)
                if f(x) in targets}
        got = {(int(w), int(c), int(r)): d for (w, c, d), r in zip(hits, hit_rules)}
        assert len(got) == len(hits) and set(planted) <= set(want)
        assert got == want  # the triples and their full-width digests
        assert sum(1 for _, _, r in got if r > 255) >= 10
    finally:
        gpu_ctx.clear_rules()
        gpu_ctx.clear_table()
