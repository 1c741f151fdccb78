"""Every route of the digest + lookup stage over the adversarial target sets of target_sets.py.

The routes end in the same probe (md_prefilter / md_probe / md_probe_wide / md_block_probe,
a5x_md.h), each call site with its own copy of the table arguments; the suite's other sets
are friendly (load 0.3, targets in their home slots, no decoy that resembles a digest).  Here
each route gets, built against digests of its own candidates: near misses of a real non-target
digest N in each of the four prefix words (and the tail), inside N's probe chain; a real
target D seven slots past its home slot, once with the chain wrapped from the last slot to
slot 0; for wide digests a chain through entries with D's own 16-byte prefix, beside a
zero-prefix target and the all-zero digest; and the degenerate sets.  The host builds every
set once through a5x_debug_target_set and the constructors' claims are asserted on it
(target_sets.check_*) before the device sees the list.  For every set the hits must equal
{(word, candidate) : digest(candidate) in set(targets)} computed exhaustively in Python, once
each, with the candidate's digest, and the same list without its real digests must give [].

Routes: the fused default-mode kernels on the slot path (md_block_probe) and, NTLM, the general
path (md_probe on the run layout, taken by a window with a candidate past 27 UTF-16 units; an
MD5 window never leaves the slots, see LONG_FAST), the two-pass stream, the hybrid sub-batch of the
non-FAST words, the mode engines, rules, salts and one nested form.  Which words are FAST is
asserted with the statistics of a plain expansion of the same words."""
import functools
import hashlib

import numpy as np
import pytest

import rule_oracle as ro
import target_sets as ts
from conftest import table_path
from oracle import digest_oracle as dg

pytestmark = pytest.mark.gpu

MD5, NTLM, SHA1, SHA256, SHA512, MD5_MD5 = 0, 1, 2, 3, 7, 16
_ntlm = functools.lru_cache(maxsize=None)(dg.ntlm)
REF = {MD5: lambda b: hashlib.md5(b).digest(), NTLM: _ntlm, SHA1: lambda b: hashlib.sha1(b).digest(),
       SHA256: lambda b: hashlib.sha256(b).digest(), SHA512: lambda b: hashlib.sha512(b).digest(),
       MD5_MD5: lambda b: hashlib.md5(hashlib.md5(b).hexdigest().encode()).digest()}
SIZE = {MD5: 16, NTLM: 16, SHA1: 20, SHA256: 32, SHA512: 64, MD5_MD5: 16}
IDS = {MD5: "md5", NTLM: "ntlm", SHA1: "sha1", SHA256: "sha256", SHA512: "sha512", MD5_MD5: "md5-md5"}

FILLER = list(b"bfghjklmpqvwxBFGH 19-")  # no key or value of the czech / german tables
TOKENS = [b"a", b"e", b"s", b"A", b"S", b"z", "á".encode(), "š".encode(), "ä".encode(), "é".encode()]
# FAST words with long candidates.  A FAST word is at most 8 pieces of 7 bytes with its '\n', so
# its candidates have at most 55 bytes: every MD5 window of the fused kernel fits one message
# block and takes the slots (the 53-byte words below reach the 14-word slot rounds with 54- and
# 55-byte candidates; with 8 or more candidates a word of this length is slow on the device, so
# these have 3 to 7); an NTLM window leaves them for the general path, the UTF-8 walk over the
# run layout, as soon as a candidate has more than 27 UTF-16 units.  The last three are the long
# words of test_fused_slot_path_every_candidate_mixed_utf8.
LONG_FAST = [b"1" * 51 + b"uy", b"2" * 51 + b"us", b"3" * 51 + b"ey", b"4" * 51 + b"ie", b"6" * 51 + b"sy",
             b"7" * 51 + b"iz", b"q" * 40 + b"ao", ("β" * 20 + "eo").encode(), ("日本語" * 3 + "ae").encode()]
# the 20-letter word of test_digest_ranges_partition_the_hits (FAST under these tables), then words
# the fused kernel skips (the hybrid sub-batch): that test's two words past 64 bytes (BIG) and two
# words past the FAST length limit (slow)
NON_FAST = [b"abcdefghijklmnopqrst", b"q" * 64 + b"abcdes", b"qq" * 40 + b"strasse", b"7" * 58 + b"as",
            b"1" * 56 + b"ae"]
LETTERS = "αβγδεζηθικλμνξοπρστυφχψω"


def _words(seed, n, max_tokens=2, lo=1, hi=13):
    """n words of filler bytes with 1..max_tokens substitutable tokens (as test_gpu_rules._words)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        parts = [bytes([int(c)]) for c in rng.choice(FILLER, size=int(rng.integers(lo, hi)))]
        for _ in range(int(rng.integers(1, max_tokens + 1))):
            parts.insert(int(rng.integers(0, len(parts) + 1)), TOKENS[int(rng.integers(0, len(TOKENS)))])
        out.append(b"".join(parts))
    return out + [b"", b"a", b"strasse", b"\xff\xfe", "😀ab".encode()]


def _greek_words(seed, n):
    rng = np.random.default_rng(seed)
    return ["".join(LETTERS[int(x)] for x in rng.integers(0, 24, size=int(rng.integers(2, 7)))).encode()
            for _ in range(n)] + ["αλφα".encode() * 2, "ααααα".encode()]


def _load(ctx, tabs):
    ctx.clear_table()
    ctx.load_tables([table_path(t) for t in tabs])


@pytest.fixture(autouse=True)
def _plain_state_left_behind(gpu_ctx):
    yield
    gpu_ctx.clear_rules()
    gpu_ctx.set_targets(MD5, hashlib.md5(b"").digest())
    assert gpu_ctx.salt_count() == 0


class _Batch:
    """words under tables in one mode: the library's per-word candidates, once"""

    def __init__(self, ctx, tabs, words, mode):
        from hashcat_a5_table_generator_amd import pack_words
        self.tabs, self.words, self.mode = tabs, words, mode
        _load(ctx, tabs)
        self.per_word = ctx.expand_words(words, mode, 0, 15)
        self.packed = pack_words(words)
        self.flat = [(w, c, x) for w, cs in enumerate(self.per_word) for c, x in enumerate(cs)]
        self._dig = {}

    def digests(self, algo):
        """digest of every candidate, in the order of flat"""
        if algo not in self._dig:
            f = REF[algo]
            self._dig[algo] = [f(x) for _, _, x in self.flat]
        return self._dig[algo]

    def not_fast(self, ctx, words=None):
        """(slow, BIG) words among words (default: the batch's) as the device classifies them: the
        statistics of a plain expansion"""
        from hashcat_a5_table_generator_amd import DeviceBuffer, pack_words
        data, offs = self.packed if words is None else pack_words(words)
        dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
        n = len(offs) - 1
        _, tb = ctx.keyspace_device(dw.ptr, do.ptr, n)
        out = DeviceBuffer(ctx, tb + 64)
        st = ctx.expand_device(dw.ptr, do.ptr, n, out.ptr, tb)
        return st["words_slow"], st["words_pass_b"]


_cache = {}
N_FILL = 305  # the filler-and-token words come first in every czech + german batch


def _fill():
    return _words(3, 300)


def _fast_fill():
    """(the one-letter word is below the FAST minimum: it would go to the hybrid sub-batch)"""
    return [w if w != b"a" else b"ah" for w in _fill()]


def _batch(ctx, key):
    if key not in _cache:
        if key == "fast":       # every candidate-bearing word FAST: the fused kernels alone
            _cache[key] = _Batch(ctx, ["czech", "german"], _fast_fill() + LONG_FAST, 0)
        elif key == "short":    # words of at most 6 characters: every window can take the NTLM slots
            _cache[key] = _Batch(ctx, ["czech", "german"], [w for w in _words(5, 300, lo=1, hi=5) if 1 < len(w) <= 6], 0)
        elif key == "hybrid":   # the same with words the fused kernels leave to the sub-batch
            _cache[key] = _Batch(ctx, ["czech", "german"], _fill() + LONG_FAST + NON_FAST, 0)
        else:                   # ("mode", m): greek words for the -r / -s / -s -r engines
            _cache[key] = _Batch(ctx, ["greek-hebrew"], _greek_words(40 + key[1], 300), key[1])
    b = _cache[key]
    _load(ctx, b.tabs)
    return b


def _unique(seq):
    seen, out = set(), []
    for d in seq:
        if d not in seen and any(d[:16]):
            seen.add(d)
            out.append(d)
    return out


def _sets(W, pool, wide=False):
    """The constructed sets over the real digests in pool as (name, targets, real digests among
    them); each claim asserted on the set as the host builds it."""
    pool = _unique(pool)
    assert len(pool) >= 12, len(pool)
    out = []
    N, D = pool[0], pool[1]
    forged = ts.near_misses(N, 8)
    targets = forged + [D]
    S = ts.Dump(W, targets)
    assert S.size == 16
    ts.check_near_misses(S, N, forged)
    assert ts.lookup(S, D)[0]
    out.append(("near", targets, {D}))
    for name, lo, hi, wraps in (("wrapped", 9, 15, True), ("straight", 0, 8, False)):
        D = ts.pick_home(pool[2:], 16, lo, hi)
        targets = ts.chain(D, 7)
        S = ts.Dump(W, targets)
        assert S.size == 16
        ts.check_chain(S, D, 7, wraps)
        out.append((name, targets, {D}))
    if wide:
        D = ts.pick_home(pool[2:], 16, 11, 15)
        targets = ts.wide_chain(D, 5)
        S = ts.Dump(W, targets)
        assert S.size == 16 and S.shared == 1 and S.has_zero == 1 and len(S.ztails) == 2
        ts.check_chain(S, D, 5, True)
        out.append(("wide", targets, {D}))
    return out


def _fused_ran(st):
    assert st["ms_total"] - st["ms_keyspace"] - st["ms_expand"] < 1e-3 and st["expand_launches"] == 1


def _two_pass_ran(st):
    assert st["ms_total"] - st["ms_keyspace"] - st["ms_expand"] > 0  # the digest stream's own time


def _check(ctx, algo, batch, sets, route_ran):
    """every set, then the set without its real digests: the hits against the exhaustive truth"""
    data, offs = batch.packed
    dig = batch.digests(algo)
    at = {(w, c): d for (w, c, _), d in zip(batch.flat, dig)}
    for name, targets, reals in sets:
        for tl in (targets, [t for t in targets if t not in reals]):
            tset = set(tl)
            ctx.set_targets(algo, b"".join(tl))
            hits, st = ctx.expand_digest(data, offs, batch.mode, 0, 15)
            assert st["candidates"] == len(batch.flat)
            if len(batch.flat):
                route_ran(st)
            want = {(w, c) for (w, c, _), d in zip(batch.flat, dig) if d in tset}
            got = [(w, c) for w, c, _ in hits]
            assert len(got) == len(set(got)), (name, "a hit twice")
            assert set(got) == want, (name, sorted(set(got) - want)[:5], sorted(want - set(got))[:5])
            assert all(d == at[(w, c)] for w, c, d in hits), name
            if tl is targets:
                assert want or not reals, (name, "the real digest has no candidate")
            else:
                assert hits == [] and not want, name


# ---- fused default mode ---------------------------------------------------------------------
def _units(x):
    return len(dg.utf16le_go(x)) // 2


@pytest.mark.parametrize("algo,path", [(MD5, "slot"), (MD5, "long"), (NTLM, "slot"), (NTLM, "general"), (NTLM, "long")],
                         ids=["md5-slot", "md5-long", "ntlm-slot", "ntlm-general", "ntlm-long"])
def test_fused_default_mode(gpu_ctx, algo, path):
    """k_expand_fast_md5 / _ntlm, every word of the batch FAST.
    slot: md_block_probe on one candidate per 64-byte slot; MD5 with N and D among candidates of
    at most 20 bytes, NTLM on a batch of words of at most 6 characters (an NTLM window takes the
    slots only when each of its big entries is at most 7 UTF-16 units, the '\\n' included).
    long, MD5: N and D among the 54- and 55-byte candidates, the longest a FAST word has (the
    14-word slot rounds).
    general, NTLM: the same short candidates as MD5's slot case, in windows that hold an entry of
    more than 7 units: the UTF-8 walk and md_probe on the run layout.  long, NTLM: candidates
    of more than 27 UTF-16 units, whose windows are past the slots by length."""
    b = _batch(gpu_ctx, "short" if (algo, path) == (NTLM, "slot") else "fast")
    assert b.not_fast(gpu_ctx) == (0, 0)  # no sub-batch: the fused kernels hash everything
    dig = b.digests(algo)
    if (algo, path) == (NTLM, "slot"):
        assert max(_units(x) for _, _, x in b.flat) <= 6
        pool = dig
    elif path in ("slot", "general"):
        assert max(_units(x) for w, _, x in b.flat if w < N_FILL) > 8
        pool = [d for (w, _, x), d in zip(b.flat, dig) if w < N_FILL and len(x) <= 20]
    elif algo == MD5:
        assert max(len(x) for _, _, x in b.flat) == 55
        pool = [d for (w, _, x), d in zip(b.flat, dig) if w >= N_FILL and len(x) >= 54]
    else:
        pool = [d for (w, _, x), d in zip(b.flat, dig) if w >= N_FILL and _units(x) > 27]
    assert len(_unique(pool)) >= 20
    _check(gpu_ctx, algo, b, _sets(16, pool), _fused_ran)


# ---- two-pass, hybrid ------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [MD5, SHA1, SHA512], ids=["md5", "sha1", "sha512"])
def test_two_pass(gpu_ctx, monkeypatch, algo):
    """k_digest_stream behind the expansion (A5X_NO_FUSED_DIGEST): md_probe, md_probe_wide."""
    monkeypatch.setenv("A5X_NO_FUSED_DIGEST", "1")
    b = _batch(gpu_ctx, "hybrid")
    pool = [d for (w, _, x), d in zip(b.flat, b.digests(algo)) if w < N_FILL]
    _check(gpu_ctx, algo, b, _sets(SIZE[algo], pool, wide=SIZE[algo] > 16), _two_pass_ran)


@pytest.mark.parametrize("algo", [MD5, NTLM], ids=["md5", "ntlm"])
def test_hybrid_sub_batch(gpu_ctx, algo):
    """The fused route with non-FAST words in the batch: N and D among the candidates of two
    slow and two BIG words, which the fused kernel skips and which reach the probe through the
    two-pass sub-batch."""
    b = _batch(gpu_ctx, "hybrid")
    skipped = NON_FAST[1:]
    slow, big = b.not_fast(gpu_ctx, skipped)
    assert slow >= 1 and big >= 1 and slow + big == len(skipped)
    first = len(b.words) - len(skipped)
    assert b.words[first:] == skipped and all(b.per_word[first:])
    by_word = {w: [d for (v, _, _), d in zip(b.flat, b.digests(algo)) if v == w] for w in range(first, len(b.words))}
    pool, k = [], 0
    while any(k < len(v) for v in by_word.values()):  # the words' candidates in turn
        pool += [v[k] for v in by_word.values() if k < len(v)]
        k += 1
    elsewhere = {d for (w, _, _), d in zip(b.flat, b.digests(algo)) if w not in by_word}
    _check(gpu_ctx, algo, b, _sets(16, [d for d in pool if d not in elsewhere]), _fused_ran)


# ---- mode engines ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [MD5, NTLM], ids=["md5", "ntlm"])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_mode_engines(gpu_ctx, algo, mode):
    """-r / -s / -s -r: MD5 with every leaf of at most 47 bytes (m_slot_md5_probe, whose
    md_block_probe skips the last steps on a wave without a prefilter pass) and NTLM
    (m_digest_probe)."""
    b = _batch(gpu_ctx, ("mode", mode))
    assert len(b.flat) > 1000 and max(len(x) for _, _, x in b.flat) <= 47
    dig = b.digests(algo)
    for start in (0, len(dig) // 2):  # two choices of N and D, in different words
        _check(gpu_ctx, algo, b, _sets(16, dig[start:] + dig[:start]), _fused_ran)


# ---- rules -----------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [MD5, SHA256], ids=["md5", "sha256"])
def test_rules(gpu_ctx, algo):
    """k_rules_stream under the rules ':' and 'u': D is the digest of a candidate upper-cased
    by rule 1 (and of no candidate as it stands), the near misses are forged from another such
    ruled plain."""
    b = _batch(gpu_ctx, "fast")
    f, W = REF[algo], SIZE[algo]
    rules = [b":", b"u"]
    ops = [ro.parse_line(r) for r in rules]
    data, offs = b.packed
    ruled = [[f(ro.apply_ops(x, o)) for o in ops] for _, _, x in b.flat]
    plain = {r[0] for r in ruled}
    pool = [r[1] for (w, _, _), r in zip(b.flat, ruled) if w < N_FILL and r[1] not in plain]
    for name, targets, reals in _sets(W, pool, wide=W > 16):
        for tl in (targets, [t for t in targets if t not in reals]):
            tset = set(tl)
            gpu_ctx.set_targets(algo, b"".join(tl))
            assert gpu_ctx.set_rules(rules) == (2, 0)
            hits, st = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
            which = gpu_ctx.last_hit_rules()
            assert len(which) == len(hits)
            assert gpu_ctx.rules_last() == (2 * len(b.flat), 0)  # the rules stream hashed every pair
            want = {(w, c, r) for (w, c, _), rs in zip(b.flat, ruled) for r, d in enumerate(rs) if d in tset}
            got = [(w, c, r) for (w, c, _), r in zip(hits, which)]
            assert len(got) == len(set(got)) and set(got) == want, name
            at = {(w, c): rs for (w, c, _), rs in zip(b.flat, ruled)}
            assert all(d == at[(w, c)][r] for (w, c, d), r in zip(hits, which)), name
            if tl is targets:
                assert want and all(r == 1 for _, _, r in want), name
            else:
                assert hits == [], name


# ---- salts -----------------------------------------------------------------------------------
SALTS = [b"NaCl", b"", b"0123456789abcdef!"]


@pytest.mark.parametrize("algo", [MD5, SHA512], ids=["md5", "sha512"])
@pytest.mark.parametrize("order", [0, 1], ids=["pass.salt", "salt.pass"])
def test_salts(gpu_ctx, algo, order):
    """k_salt_stream: a chain of seven decoys before D and the near misses of N, all registered
    with salt 0 and built from digests under salt 0; the forged targets once more under salt 1; a
    planted digest under salt 2.  The table's key is the digest XOR the salt's mask and the
    host hook dumps unmasked sets only, so where the masked entries lie -- the chain, the
    displacement, the forged entries inside N's chain -- cannot be asserted for this route;
    the layout claims hold for the unmasked lists (asserted), and the exhaustive equality of
    the (word, candidate, salt) hits is asserted as on every other route."""
    b = _batch(gpu_ctx, "fast")
    f, W = REF[algo], SIZE[algo]
    data, offs = b.packed
    msg = (lambda x, s: x + s) if order == 0 else (lambda x, s: s + x)
    salted = [[f(msg(x, s)) for s in SALTS] for _, _, x in b.flat]
    pool = _unique(r[0] for (w, _, _), r in zip(b.flat, salted) if w < N_FILL)
    N = pool[0]
    D = ts.pick_home(pool[2:], 16, 9, 15)
    chain = ts.chain(D, 7)
    forged = ts.near_misses(N, 8)
    ts.check_chain(ts.Dump(W, chain), D, 7, True)
    ts.check_near_misses(ts.Dump(W, forged), N, forged)
    D2 = next(r[2] for r in reversed(salted))
    reg = [(t, 0) for t in chain + forged] + [(t, 1) for t in forged] + [(D2, 2)]
    for pairs in (reg, [p for p in reg if p[0] not in (D, D2)]):
        gpu_ctx.set_salted_targets(algo, order, b"".join(t for t, _ in pairs), [SALTS[s] for _, s in pairs])
        assert gpu_ctx.salt_count() == (3 if pairs is reg else 2)
        hits, st = gpu_ctx.expand_digest(data, offs, 0, 0, 15)
        which = gpu_ctx.last_hit_salts()
        assert len(which) == len(hits)
        S = gpu_ctx.salt_count()
        assert gpu_ctx.salts_last() == (S * len(b.flat), 0)  # the salt stream hashed every pair
        pset = set(pairs)
        want = {(w, c, s) for (w, c, _), rs in zip(b.flat, salted) for s in range(S) if (rs[s], s) in pset}
        got = [(w, c, s) for (w, c, _), s in zip(hits, which)]
        assert len(got) == len(set(got)) and set(got) == want
        at = {(w, c): rs for (w, c, _), rs in zip(b.flat, salted)}
        assert all(d == at[(w, c)][s] for (w, c, d), s in zip(hits, which))
        if pairs is reg:
            assert {s for _, _, s in want} == {0, 2}
        else:
            assert hits == []


# ---- nested ----------------------------------------------------------------------------------
def test_nested_md5_md5(gpu_ctx):
    """md5(hex(md5(p))) through the nested two-pass route, on the near-miss and wrapped-chain sets."""
    b = _batch(gpu_ctx, "fast")
    pool = [d for (w, _, _), d in zip(b.flat, b.digests(MD5_MD5)) if w < N_FILL]
    sets = [s for s in _sets(16, pool) if s[0] in ("near", "wrapped")]
    assert len(sets) == 2
    _check(gpu_ctx, MD5_MD5, b, sets, _two_pass_ran)


# ---- degenerate sets -------------------------------------------------------------------------
@pytest.mark.parametrize("route,algo", [("fused", MD5), ("fused", NTLM), ("two-pass", MD5), ("two-pass", SHA1)],
                         ids=["fused-md5", "fused-ntlm", "two-pass-md5", "two-pass-sha1"])
def test_degenerate_sets(gpu_ctx, monkeypatch, route, algo):
    """The empty set (accepted by a5x_set_targets and by the binding: zero hits, no error), one
    target, nine copies of it (32 slots, one entry), 8 and 9 distinct targets (16 slots at load
    1/2, 32 slots), and a set with the all-zero digest, which gives the hits of the set without
    it."""
    if route == "two-pass":
        monkeypatch.setenv("A5X_NO_FUSED_DIGEST", "1")
    b = _batch(gpu_ctx, "fast")
    W = SIZE[algo]
    pool = _unique(d for (w, _, _), d in zip(b.flat, b.digests(algo)) if w < N_FILL)
    sets = ts.degenerate(pool[3], pool[10:30])
    sizes = {"empty": 16, "one": 16, "nine_copies": 32, "eight": 16, "nine": 32, "with_zero": 16}
    for name, targets in sets.items():
        S = ts.Dump(W, targets)
        assert S.size == sizes[name] and S.has_zero == (1 if name == "with_zero" else 0)
    ran = _fused_ran if route == "fused" else _two_pass_ran
    _check(gpu_ctx, algo, b, [(name, t, {x for x in t if any(x)}) for name, t in sets.items()], ran)
    gpu_ctx.set_targets(algo, b"")
    hits, st = gpu_ctx.expand_digest(*b.packed, 0, 0, 15)
    assert hits == [] and st["candidates"] == len(b.flat)
