"""The rule corpus of tests/rule_fuzz.py on the CPU: the host build of the interpreter
(csrc/a5x_rules.h through a5x_debug_apply_rule, whose A5X_E_BOUNDS is the zero-tail check)
against the Python oracle on every (line, rule) pair the GPU suite runs, and the conditions on
the corpus itself -- what the census says it reaches, what the stream puts at the block edges,
and the order that puts a shrinking rule behind every growing one.  The conditions are on the
inputs: they hold by construction and say what test_gpu_rule_fuzz.py then pins down."""
import ctypes

import numpy as np
import pytest

import rule_fuzz as rf
import rule_oracle as ro

E_BOUNDS = -6
POSITIONAL = "TpD'zZLR+-.,yYxO*io"


def _host_against_oracle(kind):
    from hashcat_a5_table_generator_amd import _lib
    rules, ls, ruled, _ = rf.corpus(kind)
    fn = _lib.load().a5x_debug_apply_rule
    out = ctypes.create_string_buffer(136)  # one buffer for every call
    n = ctypes.c_size_t()
    nref = ctypes.byref(n)
    pairs, bad, tails = 0, [], []
    for ln, row in zip(ls, ruled):
        if row is None:
            continue
        for r, want in zip(rules, row):
            rc = fn(r, len(r), ln, len(ln), out, 136, nref)
            pairs += 1
            if rc == E_BOUNDS:
                tails.append((r, ln))
            elif rc != 0 or out[:n.value] != want:
                bad.append((r, ln, rc, out[:n.value], want))
    assert not tails, (len(tails), tails[:5])  # a non-zero byte at or past the ruled length
    assert not bad, (len(bad), bad[:5])
    return pairs


def test_host_interpreter_equals_the_oracle_on_the_grid():
    rules, ls, _, cen = rf.corpus("grid")
    assert len(rules) == len(set(rules)) == 4511 and sorted(rules) == sorted(rf.grid_rules())
    pairs = _host_against_oracle("grid")
    assert pairs == cen["pairs"] == len(rules) * sum(1 for ln in ls if len(ln) <= rf.LMAX)


def test_host_interpreter_equals_the_oracle_on_the_chains():
    rules, ls, _, cen = rf.corpus("chains")
    assert _host_against_oracle("chains") == cen["pairs"] == len(rules) * sum(1 for ln in ls if len(ln) <= rf.LMAX)


def test_grid_names_every_function_at_every_position():
    rules = rf.grid_rules()
    seen = {}
    for r in rules:
        (f, a, b), = ro.parse_line(r)
        seen.setdefault(f, set()).add((a, b))
    assert set(seen) == set(ro.KINDS)
    for f, kind in ro.KINDS.items():
        if kind == "N":
            assert seen[f] == {(p, 0) for p in range(36)}, f
        elif kind == "NM":
            assert seen[f] == {(p, q) for p in range(36) for q in range(36)}, f
        elif kind == "NX":
            assert {p for p, _ in seen[f]} == set(range(36)) and {c for _, c in seen[f]} == set(rf.CHARS), f
        elif kind == "X":
            assert seen[f] == {(c, 0) for c in rf.CHARS}, f
        elif kind == "XY":
            assert {c for c, _ in seen[f]} == {c for _, c in seen[f]} == set(rf.CHARS)
    assert all(b"\n" not in r and not r.endswith(b"\r") for r in rules + rf.chain_rules())


def test_grid_census():
    _, _, _, cen = rf.corpus("grid")
    phases = {(p, n) for p in range(4) for n in range(4)}
    for f in POSITIONAL:  # changed a word at every (p0 & 3, length & 3)
        assert set(cen["changed"][f]) == phases, (f, sorted(phases - set(cen["changed"][f])))
    for f in rf.AMOUNT_P0 + rf.AMOUNT_P1:  # and at every byte count & 3
        assert set(cen["amount"][f]) == {0, 1, 2, 3}, (f, cen["amount"][f])
    for f in ro.KINDS:  # no function is a no-op on the whole corpus
        assert f == ":" or sum(cen["changed"][f].values()) > 0, f
    for f in rf.GROW:  # accepted up to exactly the cap, refused over it
        assert cen["full"][f] >= 1 and cen["refused"][f] >= 1, (f, cen["full"][f], cen["refused"][f])


def test_chain_census():
    rules, _, ruled, cen = rf.corpus("chains")
    nfn = [len(rf.functions(r)) for r in rules]
    assert max(nfn) == rf.OPS_MAX and min(nfn) == 1 and len(rules) >= 200
    assert cen["chains_31"] == sum(1 for k in nfn if k == 31) >= 50
    assert cen["chains_16"] == sum(1 for k in nfn if k >= 16) >= 100
    for r, k in zip(rules, nfn):
        fns = rf.functions(r)
        assert k < 8 or (any(f in rf.GROW for f in fns) and any(f in rf.SHRINK for f in fns)), r
    assert rules == rf.chain_rules(rf.SEED, len(rules))  # deterministic
    # the chains reach the cap from below, are refused at it, and use every function to some effect
    assert cen["full_words"] > 0 and sum(cen["refused"].values()) > 0
    assert all(f == ":" or sum(cen["changed"][f].values()) > 0 for f in ro.KINDS)
    # the 31-function chains do not all collapse: some end in words of more than one dword
    long_ = [j for j, k in enumerate(nfn) if k == 31]
    assert sum(1 for row in ruled if row for j in long_ if len(row[j]) > 4) > 1000


def test_ordered_puts_a_shrinking_rule_behind_every_growing_one():
    for rules in (rf.grid_rules(), rf.grid_rules() + [r for r in rf.chain_rules() if not rf.can_grow(r)]):
        o = rf.ordered(rules)
        assert sorted(o) == sorted(rules) and o != rules and o == rf.ordered(rules)
        grow = [rf.can_grow(r) for r in o]
        assert sum(grow) >= 200 and not grow[-1]
        assert all(not grow[j + 1] for j in range(len(o) - 1) if grow[j])
    with pytest.raises(ValueError):
        rf.ordered([b"d", b"$1", b"l"])
    assert rf.can_grow(b"l $1") and rf.can_grow(b"lzA") and not rf.can_grow(b"sa$ o1^ '5")


def test_stream_claims():
    B = rf.BLOCK
    ls = rf.lines()
    assert ls == rf.lines(rf.SEED)
    s = rf.stream(ls)
    st = rf.starts(ls)
    assert s.split(b"\n") == ls and not s.endswith(b"\n") and len(ls[-1]) > 0  # the last line has no newline
    assert len(s) >= 4 * B
    lens = np.array([len(x) for x in ls])
    # every length 0..128 twice: once over letters and boundary bytes, once over arbitrary bytes
    for n in range(rf.LMAX + 1):
        assert int((lens == n).sum()) >= 2, n
    alpha = set(rf.WORD_ALPHA) | {0xc1, 0xe1}
    for n in range(1, rf.LMAX + 1):
        kinds = {set(x) <= alpha for x in ls if len(x) == n}
        assert True in kinds and (n < 8 or False in kinds), n
    assert set(b"".join(ls)) == set(range(256)) - {0x0a}
    # neighbours in a round of 64 differ in length (outside the short run, too)
    assert all(len(set(lens[i:i + 64].tolist())) >= 8 for i in range(0, len(ls) - 64, 64))
    # one block with more than 128 line starts, all of a run of lines of 0..8 bytes
    per_block = np.bincount(st // B)
    assert per_block.max() > 128 and len(per_block) >= 4
    short = lens <= 8
    run = max(len(r) for r in "".join("s" if x else " " for x in short).split())
    assert run >= 200
    # a line ends exactly on a block edge (the next starts on it); others straddle one
    assert any(x > 0 and x % B == 0 for x in st.tolist())
    ends = st + lens  # the newline's offset
    straddle = [(int(a), int(n)) for a, n, e in zip(st, lens, ends) if a // B != (e - 1) // B and n <= rf.LMAX]
    assert len(straddle) >= 2
    # the lines over the cap: in the middle, two of them past the staged margin, one of those
    # as the last line of its block
    over = [i for i, n in enumerate(lens) if n > rf.LMAX]
    assert sorted(lens[over].tolist()) == sorted(rf.OVER) and max(over) < len(ls) - 20 and min(over) > 20
    i400 = int(np.flatnonzero(lens == 400)[0])
    assert st[i400] // B != st[i400 + 1] // B and ends[i400] > (st[i400] // B + 1) * B + rf.MARGIN
    # every start phase meets every length phase
    assert {(int(a) & 3, int(n) & 3) for a, n in zip(st, lens) if n <= rf.LMAX} == {(a, n) for a in range(4) for n in range(4)}
