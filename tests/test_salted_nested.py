"""Salted nested digests on the CPU: csrc/a5x_salt_nest.h (the code the salted-nested stream
kernel runs, record preparation included) through a5x_debug_digest_salted against hashlib
compositions for the seven algorithms 32..38; the constants, sizes and salt orders; the
refusals; what a host-only context keeps of such a set; the CLI's names and mode numbers; and
the stand-alone selftest's build line."""
import ctypes
import hashlib
import os
import subprocess

import pytest

from conftest import ROOT, table_path

E_ARG, E_HIP, E_UNSUPPORTED = -1, -2, -9
MD5_MD5_SALT, MD5_SALT_MD5, MD5_MD5_MD5SALT, MD5_MD5SALT_MD5, SHA1_SHA1_SALT, SHA1_SALT_SHA1, SHA1_MD5_SALT = range(32, 39)


def _md5(b):
    return hashlib.md5(b).digest()


def _sha1(b):
    return hashlib.sha1(b).digest()


def _hex(d):
    return d.hex().encode()


# the definitions: hex is lower-case ASCII hex of a digest in its standard byte order
REF = {
    MD5_MD5_SALT: lambda p, s: _md5(_hex(_md5(p)) + s),
    MD5_SALT_MD5: lambda p, s: _md5(s + _hex(_md5(p))),
    MD5_MD5_MD5SALT: lambda p, s: _md5(_hex(_md5(p)) + _hex(_md5(s))),
    MD5_MD5SALT_MD5: lambda p, s: _md5(_hex(_md5(s)) + _hex(_md5(p))),
    SHA1_SHA1_SALT: lambda p, s: _sha1(_hex(_sha1(p)) + s),
    SHA1_SALT_SHA1: lambda p, s: _sha1(s + _hex(_sha1(p))),
    SHA1_MD5_SALT: lambda p, s: _sha1(_hex(_md5(p)) + s),
}
SIZE = {32: 16, 33: 16, 34: 16, 35: 16, 36: 20, 37: 20, 38: 20}
ORDER = {32: 0, 33: 1, 34: 0, 35: 1, 36: 0, 37: 1, 38: 0}
NAME = {32: "md5-md5.salt", 33: "md5-salt.md5", 34: "md5-md5.md5salt", 35: "md5-md5salt.md5", 36: "sha1-sha1.salt",
        37: "sha1-salt.sha1", 38: "sha1-md5.salt"}
MODES = {"2611": 32, "2711": 32, "3710": 33, "3910": 34, "2811": 35, "4510": 36, "4520": 37, "4710": 38}
ALGOS = pytest.mark.parametrize("algo", sorted(REF), ids=[NAME[a] for a in sorted(REF)])
# 15/16 and 23/24: the one / two block edges behind 40 and 32 characters; 24 and 32: the message
# ends on the block edge; lengths = 1, 2, 3 mod 4: the funnel shifts of salt . text
SALT_LENS = [0, 1, 2, 3, 4, 5, 15, 16, 23, 24, 30, 31, 32, 55, 63, 64]


def _bytes(n, seed):
    return bytes((i * 37 + seed * 101 + n * 11 + 5) % 256 for i in range(n))


def test_constants_sizes_and_orders():
    import hashcat_a5_table_generator_amd as a5x
    from hashcat_a5_table_generator_amd import A5xError, _lib, digest_size, salt_order
    L = _lib.load()
    assert (a5x.ALGO_MD5_MD5_SALT, a5x.ALGO_MD5_SALT_MD5, a5x.ALGO_MD5_MD5_MD5SALT, a5x.ALGO_MD5_MD5SALT_MD5,
            a5x.ALGO_SHA1_SHA1_SALT, a5x.ALGO_SHA1_SALT_SHA1, a5x.ALGO_SHA1_MD5_SALT) == tuple(range(32, 39))
    assert [L.a5x_digest_size(a) for a in range(32, 39)] == [16, 16, 16, 16, 20, 20, 20]
    assert [digest_size(a) for a in range(32, 39)] == [16, 16, 16, 16, 20, 20, 20]
    assert [L.a5x_digest_size(a) for a in list(range(23, 32)) + [39]] == [E_ARG] * 10
    assert [L.a5x_algo_salt_order(a) for a in range(32, 39)] == [0, 1, 0, 1, 0, 1, 0]
    assert [salt_order(a) for a in range(32, 39)] == [ORDER[a] for a in range(32, 39)]
    for a in (0, 2, 16, 22, 23, 31, 39, -1):
        assert L.a5x_algo_salt_order(a) == E_ARG
        with pytest.raises(A5xError):
            salt_order(a)
    assert L.a5x_abi_version() == 1


@ALGOS
def test_debug_digest_salted_matches_hashlib(algo):
    from hashcat_a5_table_generator_amd import debug_digest_salted
    bad = []
    for sl in SALT_LENS:
        salt = _bytes(sl, 3)
        for n in range(129):
            p = _bytes(n, sl)
            if debug_digest_salted(algo, ORDER[algo], salt, p) != REF[algo](p, salt):
                bad.append((n, sl))
    assert not bad, (len(bad), bad[:10])


def test_the_empty_salt_is_the_unsalted_nested_digest_or_the_salts_md5():
    from hashcat_a5_table_generator_amd import _lib, debug_digest_salted
    L = _lib.load()
    out = (ctypes.c_uint8 * 64)()
    for n in (0, 1, 55, 56, 64, 128):
        p = _bytes(n, 9)
        for algo, plain in ((32, 16), (33, 16), (36, 20), (37, 20), (38, 21)):
            assert L.a5x_debug_digest(plain, p, n, out, 64) == 0
            assert debug_digest_salted(algo, ORDER[algo], b"", p) == bytes(out[: SIZE[algo]])
        # 34 / 35 hash the salt: md5(b"")'s hex text, not the empty string
        e = _hex(_md5(b""))
        assert debug_digest_salted(34, 0, b"", p) == _md5(_hex(_md5(p)) + e) != _md5(_hex(_md5(p)))
        assert debug_digest_salted(35, 1, b"", p) == _md5(e + _hex(_md5(p))) != _md5(_hex(_md5(p)))


@ALGOS
def test_refusals(algo):
    from hashcat_a5_table_generator_amd import A5xError, Context, _lib, debug_digest_salted
    L = _lib.load()
    out = (ctypes.c_uint8 * 64)()
    o = ORDER[algo]
    assert debug_digest_salted(algo, o, b"s" * 64, b"p" * 128) == REF[algo](b"p" * 128, b"s" * 64)  # no pair skipped for its salt
    for salt, msg, order, code in ((b"s", b"p" * 129, o, E_UNSUPPORTED), (b"", b"p" * 129, o, E_UNSUPPORTED),
                                   (b"s", b"p", 1 - o, E_ARG), (b"s", b"p", 2, E_ARG), (b"s" * 65, b"p", o, E_ARG)):
        with pytest.raises(A5xError) as e:
            debug_digest_salted(algo, order, salt, msg)
        assert e.value.code == code, (len(salt), len(msg), order)
    assert L.a5x_debug_digest_salted(algo, o, b"s", 1, b"p", 1, out, SIZE[algo] - 1) == -8  # A5X_E_CAPACITY
    assert L.a5x_debug_digest(algo, b"abc", 3, out, 64) == E_ARG  # salted only
    dig = REF[algo](b"x", b"salt")
    with Context(-1) as c:
        with pytest.raises(A5xError, match="salted only") as e:
            c.set_targets(algo, dig)
        assert e.value.code == E_ARG
        with pytest.raises(A5xError) as e:
            c.set_salted_targets(algo, 1 - o, dig, [b"salt"])
        assert e.value.code == E_ARG and c.salt_count() == 0
        with pytest.raises(A5xError) as e:
            c.load_salted_hashes(algo, 1 - o, dig.hex().encode() + b":salt\n")
        assert e.value.code == E_ARG and c.salt_count() == 0
        with pytest.raises(A5xError) as e:
            c.set_salted_targets(algo, o, dig, [b"s" * 65])
        assert e.value.code == E_ARG and c.salt_count() == 0
        # rules on such a set, in both orders of setting
        c.set_salted_targets(algo, o, dig, [b"salt"])
        with pytest.raises(A5xError) as e:
            c.set_rules([b":"])
        assert e.value.code == E_UNSUPPORTED and c.rule_count() == 0 and c.salt_count() == 1
    with Context(-1) as c:
        assert c.set_rules([b":", b"u"]) == (2, 0)
        with pytest.raises(A5xError) as e:
            c.set_salted_targets(algo, o, dig, [b"salt"])
        assert e.value.code == E_UNSUPPORTED and c.salt_count() == 0 and c.rule_count() == 2


def test_the_nested_and_ntlm_values_stay_refused_by_the_salted_entry_points():
    from hashcat_a5_table_generator_amd import A5xError, Context
    with Context(-1) as c:
        for algo in (1, 16, 17, 18, 19, 20, 21, 22):
            with pytest.raises(A5xError, match="no salted mode") as e:
                c.set_salted_targets(algo, 0, bytes(32 if algo == 22 else 20 if algo in (20, 21) else 16), [b"salt"])
            assert e.value.code == E_ARG


@ALGOS
def test_host_only_context_keeps_the_original_salts(algo):
    from hashcat_a5_table_generator_amd import Context
    o, W = ORDER[algo], SIZE[algo]
    salts = [b"bb", b"", b"a", b"bb", b"cc:cc", b"", b"z" * 64, b"b"]
    want = [b"bb", b"", b"a", b"cc:cc", b"z" * 64, b"b"]
    with Context(-1) as c:
        c.set_salted_targets(algo, o, b"".join(REF[algo](bytes([i]), s) for i, s in enumerate(salts)), salts)
        assert c.salt_count() == len(want) and [c.salt(i) for i in range(len(want))] == want
        h = lambda i, s: REF[algo](bytes([i]), s).hex().encode()
        text = b"\n".join([
            h(1, b"na:cl") + b":na:cl",         # a literal salt with a ':'
            h(2, b"crlf") + b":crlf\r",
            h(3, b"") + b":",                   # an empty salt
            h(4, b"x"),                         # no colon: skipped
            h(5, b"x")[:-2] + b":short",        # a short digest: skipped
            h(6, b"x") + b":" + b"s" * 65,      # a 65-byte salt: skipped
            h(7, b"s" * 64) + b":" + b"s" * 64,
            h(8, b"na:cl") + b":na:cl",         # a repeated salt
        ]) + b"\n"
        assert c.load_salted_hashes(algo, o, text) == (5, 4, 3)
        assert [c.salt(i) for i in range(4)] == [b"na:cl", b"crlf", b"", b"s" * 64]
        hx = b"\n".join([h(1, b"na:\x00\xff") + b":6e613a00ff", h(2, b"na") + b":6E61", h(3, b"") + b":",
                         h(4, b"x") + b":abc", h(5, b"x") + b":zz", h(6, b"a" * 64) + b":" + b"61" * 64])
        assert c.load_salted_hashes(algo, o, hx, hex_salt=True) == (4, 4, 2)
        assert [c.salt(i) for i in range(4)] == [b"na:\x00\xff", b"na", b"", b"a" * 64]
        assert W == len(REF[algo](b"", b""))


def _cli(tmp_path, args):
    from hashcat_a5_table_generator_amd import build
    assert os.path.exists(build.CLI)
    d = tmp_path / "d.txt"
    d.write_bytes(b"abc\n")
    return subprocess.run([build.CLI, str(d)] + args, capture_output=True, text=True, timeout=60)


def test_cli_names_and_modes_parse(tmp_path):
    """A new --algo value gets past the parser to the next usage error (no table given); no
    device is opened."""
    unknown = _cli(tmp_path, ["--algo", "sha3"])
    assert unknown.returncode == 80 and "--algo:" in unknown.stderr
    helptext = _cli(tmp_path, ["--help"]).stdout
    for v in list(NAME.values()) + list(MODES):
        r = _cli(tmp_path, ["--algo", v])
        assert r.returncode == 80 and "--algo:" not in r.stderr and "--table-files" in r.stderr, v
        assert v in helptext, v
    for v in NAME.values():
        assert v in unknown.stderr.replace(",", " ").split(), v
    for v in ("md5-md5.pepper", "2612", "md5.md5-salt", "4511"):
        r = _cli(tmp_path, ["--algo", v])
        assert r.returncode == 80 and "--algo:" in r.stderr, v


def test_cli_order_must_agree(tmp_path):
    h = tmp_path / "h.txt"
    h.write_bytes(REF[32](b"x", b"salt").hex().encode() + b":salt\n")
    base = ["-t", table_path("czech"), "--hashes", str(h)]
    for args in (["--algo", "2611", "--salted=salt.pass"], ["--salted=pass.salt", "--algo", "md5-salt.md5"],
                 ["--algo", "4520", "--salted=pass.salt", "--hex-salt"], ["--algo", "sha1-md5.salt", "--salted=salt.pass"]):
        r = _cli(tmp_path, base + args)
        assert r.returncode == 80 and "contradicts" in r.stderr and r.stdout == "", args
    # without --hashes a salted nested algorithm is the usage error a salted mode number is
    r = _cli(tmp_path, ["-t", table_path("czech"), "--algo", "2611"])
    assert r.returncode == 80 and "--hashes" in r.stderr
    # rules stay refused with such a list; the unsalted nested names with --salted stay what they were
    r = _cli(tmp_path, base + ["--algo", "2611", "--rules", str(h)])
    assert r.returncode == 80 and "rules" in r.stderr
    r = _cli(tmp_path, base + ["--algo", "2600", "--salted=pass.salt"])
    assert r.returncode == 80 and "nested" in r.stderr


def test_selftest_build_line_is_in_its_header():
    src = open(os.path.join(ROOT, "tools", "salt_nest_selftest.cpp")).read()
    head = src[: src.index("#include")]
    assert "-fsanitize=address,undefined" in head and "tools/salt_nest_selftest.cpp" in head
    assert "int main()" in src and "a5x_salt_nest.h" in src
