"""The rule language of the digest + lookup stage on the CPU: hashcat's documented examples
through the library's interpreter (csrc/a5x_rules.h, the code k_rules_stream runs) and
through the plain-Python statement of the specification (tests/rule_oracle.py), the two
against each other on random rules x random words, the rule-file parser, and the CLI's
--rules argument check."""
import os
import subprocess

import numpy as np
import pytest

import rule_oracle as ro
# the grammar of the random rules and words, shared with the rule corpus
from rule_fuzz import random_rule as _random_rule, random_word as _random_word

W =b"p@ssW0rd"
KAT = [
    (b"l", b"p@ssw0rd"), (b"u", b"P@SSW0RD"), (b"c", b"P@ssw0rd"), (b"C", b"p@SSW0RD"), (b"t", b"P@SSw0RD"),
    (b"T3", b"p@sSW0rd"), (b"r", b"dr0Wss@p"), (b"d", b"p@ssW0rdp@ssW0rd"), (b"p2", W * 3),
    (b"f", b"p@ssW0rddr0Wss@p"), (b"{", b"@ssW0rdp"), (b"}", b"dp@ssW0r"), (b"$1", b"p@ssW0rd1"),
    (b"^1", b"1p@ssW0rd"), (b"[", b"@ssW0rd"), (b"]", b"p@ssW0r"), (b"D3", b"p@sW0rd"), (b"x04", b"p@ss"),
    (b"O12", b"psW0rd"), (b"i4!", b"p@ss!W0rd"), (b"o3$", b"p@s$W0rd"), (b"'6", b"p@ssW0"), (b"ss$", b"p@$$W0rd"),
    (b"@s", b"p@W0rd"), (b"z2", b"ppp@ssW0rd"), (b"Z2", b"p@ssW0rddd"), (b"q", b"pp@@ssssWW00rrdd"),
    (b"k", b"@pssW0rd"), (b"K", b"p@ssW0dr"), (b"*34", b"p@sWs0rd"), (b"L2", b"p@\xe6sW0rd"), (b"R2", b"p@9sW0rd"),
    (b"+2", b"p@tsW0rd"), (b"-1", b"p?ssW0rd"), (b".1", b"psssW0rd"), (b",1", b"ppssW0rd"), (b"y2", b"p@p@ssW0rd"),
    (b"Y2", b"p@ssW0rdrd"), (b":", W),
]
KAT_OTHER = [
    (b"E", b"p@ssW0rd w0rld", b"P@ssw0rd W0rld"),
    (b"e-", b"p@ssW0rd-w0rld", b"P@ssw0rd-W0rld"),
]
UNSUPPORTED = b"<>_!/()=%QM46X"


def _lib_apply(rule, word):
    from hashcat_a5_table_generator_amd import apply_rule
    return apply_rule(rule, word)


@pytest.mark.parametrize("rule,want", KAT, ids=[r.decode() for r, _ in KAT])
def test_known_answers(rule, want):
    assert ro.apply_rule(rule, W) == want
    assert _lib_apply(rule, W) == want


@pytest.mark.parametrize("rule,word,want", KAT_OTHER, ids=["E", "e-"])
def test_known_answers_title_case(rule, word, want):
    assert ro.apply_rule(rule, word) == want
    assert _lib_apply(rule, word) == want


def test_interpreter_agrees_with_the_python_statement():
    """~2000 random rule lines (1-6 functions, every function >= 50 times) x random byte words
    of lengths 0, 1, 2, random up to 128 and the dword / overflow edges 63, 64, 65, 127, 128."""
    rng = np.random.default_rng(2024)
    fns_all = sorted(ro.KINDS)
    used = {f: 0 for f in fns_all}
    rules = []
    for i in range(2000):
        k = int(rng.integers(1, 7))
        fns = [fns_all[(i + j * 7) % len(fns_all)] if j == 0 else str(rng.choice(fns_all)) for j in range(k)]
        for f in fns:
            used[f] += 1
        rules.append(_random_rule(rng, fns))
    assert min(used.values()) >= 50, used
    lengths = [0, 1, 2, 63, 64, 65, 127, 128]
    bad = []
    for i, r in enumerate(rules):
        ops = ro.parse_line(r)
        assert isinstance(ops, list), r
        for n in lengths + [int(x) for x in rng.integers(0, 129, size=4)] + [int(x) for x in rng.integers(0, 20, size=3)]:
            w = _random_word(rng, n)
            want = ro.apply_ops(w, ops)
            got = _lib_apply(r, w)
            if got != want:
                bad.append((r, w, got, want))
    assert not bad, bad[:5]


def test_growth_functions_stop_at_the_cap():
    for rule, n_ok, n_no in ((b"d", 64, 65), (b"p1", 64, 65), (b"p3", 32, 33), (b"f", 64, 65), (b"q", 64, 65),
                             (b"$x", 127, 128), (b"^x", 127, 128), (b"i0x", 127, 128), (b"z5", 123, 124),
                             (b"Z5", 123, 124), (b"y5", 123, 124), (b"Y5", 123, 124)):
        for n, grows in ((n_ok, True), (n_no, False)):
            w = bytes((i * 7 + 33) % 90 + 33 for i in range(n))
            got = _lib_apply(rule, w)
            assert got == ro.apply_rule(rule, w)
            assert (len(got) > n) == grows and len(got) <= 128, (rule, n)


def test_word_over_the_cap_is_refused():
    with pytest.raises(ValueError):
        _lib_apply(b":", b"a" * 129)


# ---- parser -------------------------------------------------------------------
def _ctx():
    from hashcat_a5_table_generator_amd import Context
    return Context(-1)


def test_parser_comments_blanks_crlf_and_counts():
    text = b"# comment\n\n   \n  # indented comment\nl\r\n  u\n\t c\n$1 $2\r\n: \n"
    with _ctx() as c:
        assert c.set_rules(text) == (5, 0)
        assert c.rule_count() == 5
    rules, skipped = ro.parse_rules(text)
    assert len(rules) == 5 and skipped == 0
    assert rules[3] == [("$", 0x31, 0), ("$", 0x32, 0)]


def test_parser_spaces_and_literal_space_parameter():
    assert _lib_apply(b"$ ", b"ab") == b"ab "
    assert _lib_apply(b"l   $1  ^2", b"Ab") == b"2ab1"
    assert _lib_apply(b"s a", b"x y") == b"xay"       # s, X = ' ', Y = 'a'
    assert _lib_apply(b"  $ $ ", b"") == b"  "        # leading blanks, then "$ " twice
    assert ro.apply_rule(b"$ ", b"ab") == b"ab "
    assert ro.apply_rule(b"  $ $ ", b"") == b"  "


def test_parser_positions_up_to_Z():
    w = bytes(range(0x41, 0x41 + 40))
    assert _lib_apply(b"TA", w) == w[:10] + b"k" + w[11:]
    assert _lib_apply(b"DZ", w) == w[:35] + w[36:]
    assert _lib_apply(b"'A", w) == w[:10]
    for bad in (b"Ta", b"D:", b"x1a", b"Oz1"):  # lower-case / punctuation are no positions
        assert ro.parse_line(bad) == "skipped"
        with pytest.raises(ValueError):
            _lib_apply(bad, w)


def test_parser_function_limit():
    ok, over = b"$a" * 31, b"$a" * 32
    assert _lib_apply(ok, b"") == b"a" * 31
    assert ro.parse_line(over) == "skipped"
    with pytest.raises(ValueError):
        _lib_apply(over, b"")
    with _ctx() as c:
        assert c.set_rules(ok + b"\n" + over + b"\n" + b": " * 31 + b"\n" + b":" * 32) == (2, 2)


def test_parser_truncated_parameters_and_unsupported_functions():
    lines = [b"s", b"sa", b"i", b"i1", b"x", b"x1", b"$", b"T", b"l$", b"lx1"]
    lines += [bytes([f]) for f in UNSUPPORTED] + [b"l" + bytes([f]) + b"1" for f in UNSUPPORTED]
    for ln in lines:
        assert ro.parse_line(ln) == "skipped", ln
        with pytest.raises(ValueError):
            _lib_apply(ln, b"word")
    with _ctx() as c:
        assert c.set_rules(b"\n".join(lines)) == (0, len(lines))
        assert c.rule_count() == 0


def test_rule_numbering_skips_skipped_lines():
    """Accepted rules are numbered from 0 in file order: set_rules' count is the oracle's."""
    text = b"l\nM\n# x\nu\n<5\n\nsa\nc\n"
    rules, skipped = ro.parse_rules(text)
    assert [r[0][0] for r in rules] == ["l", "u", "c"] and skipped == 3
    with _ctx() as c:
        assert c.set_rules(text) == (3, 3)
        assert c.set_rules([b"l", "u", b"Q", b"c"]) == (3, 1)  # a sequence of lines


def test_set_rules_count_and_clear_on_a_host_context():
    with _ctx() as c:
        assert c.rule_count() == 0
        assert c.set_rules(b"l\nu\n") == (2, 0)
        assert c.rule_count() == 2
        c.clear_rules()
        assert c.rule_count() == 0
        assert c.set_rules(b"") == (0, 0)
        assert c.last_hit_rules() == [] and c.rules_last() == (0, 0)


def test_load_rules_file(tmp_path):
    p = tmp_path / "r.rule"
    p.write_bytes(b":\r\nl\r\n$1\r\nX\r\n")
    with _ctx() as c:
        assert c.load_rules_file(str(p)) == (3, 1)
        from hashcat_a5_table_generator_amd import A5xError
        with pytest.raises(A5xError):
            c.load_rules_file(str(tmp_path / "missing.rule"))


def test_cli_rules_needs_hashes(tmp_path):
    from hashcat_a5_table_generator_amd import build
    from conftest import table_path
    if not os.path.exists(build.CLI):
        build.build()
    (tmp_path / "d.txt").write_bytes(b"word\n")
    (tmp_path / "r.rule").write_bytes(b"l\n")
    r = subprocess.run([build.CLI, str(tmp_path / "d.txt"), "-t", table_path("czech"), "--rules",
                        str(tmp_path / "r.rule")], capture_output=True, timeout=60)
    assert r.returncode == 80
    assert b"--rules" in r.stderr and b"--hashes" in r.stderr and r.stdout == b""
