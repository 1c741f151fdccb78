"""Iterated target lists on the CPU: csrc/a5x_pbkdf2.h (the code the iterated kernels run, record
preparation included) through a5x_debug_pbkdf2 against hashlib.pbkdf2_hmac for the four
algorithms 72..75; hashcat's example hashes; the constants, sizes and orders; the list parser;
what a host-only context keeps of such a set; the refusals; the CLI's names and usage errors;
and the stand-alone selftest, built with its header's line and run."""
import base64
import ctypes
import hashlib
import os
import shlex
import subprocess

import pytest

from conftest import ROOT, table_path

E_ARG, E_UNSUPPORTED = -1, -9
HASH = {72: "md5", 73: "sha1", 74: "sha256", 75: "sha512"}
HLEN = {72: 16, 73: 20, 74: 32, 75: 64}
NAME = {a: "pbkdf2-hmac-" + HASH[a] for a in HASH}
MODES = {"11900": 72, "12000": 73, "10900": 74, "12100": 75}
ALGOS = pytest.mark.parametrize("algo", sorted(NAME), ids=[NAME[a] for a in sorted(NAME)])
# the key used as it is / pre-hashed at 64 / 65 (64-byte blocks), its own blocks at 55 / 56 and
# 111 / 112, SHA-512's block at 127 / 128
CAND_LENS = [0, 1, 55, 56, 63, 64, 65, 111, 112, 127, 128]
# salt . INT(i) is one block up to 51 bytes, two from 52 (SHA-512: always one)
SALT_LENS = [0, 1, 3, 51, 52, 60, 64]
ITERS = [1, 2, 3, 1000]


def ref(algo, p, s, c, dklen=16):
    return hashlib.pbkdf2_hmac(HASH[algo], p, s, c, dklen)


def _bytes(n, seed):
    return bytes((i * 37 + seed * 101 + n * 11 + 5) % 256 for i in range(n))


def line(algo, p, s, c, dklen=None):
    dk = ref(algo, p, s, c, dklen or HLEN[algo])
    return b"%s:%d:%s:%s" % (HASH[algo].encode(), c, base64.b64encode(s), base64.b64encode(dk))


@ALGOS
def test_core_matches_hashlib(algo):
    from hashcat_a5_table_generator_amd import A5xError, debug_pbkdf2
    h = HLEN[algo]
    bad = []
    for c in ITERS:
        for sl in SALT_LENS:
            salt = _bytes(sl, 3)
            for n in CAND_LENS:
                p = _bytes(n, sl)
                want = ref(algo, p, salt, c, 2 * h)
                for dklen in (16, h, h + 1, 2 * h):
                    if debug_pbkdf2(algo, p, salt, c, dklen) != want[:dklen]:
                        bad.append((c, sl, n, dklen))
    assert not bad, (len(bad), bad[:10])
    with pytest.raises(A5xError) as e:
        debug_pbkdf2(algo, b"p" * 129, b"salt", 1, 16)
    assert e.value.code == E_UNSUPPORTED


EXAMPLES = [  # hashcat's example hashes of -m 11900 / 12000 / 10900, password "hashcat"
    (72, b"md5:1000:MTg1MzA=:Lz84VOcrXd699Edsj34PP98+f4f3S0rTZ4kHAIHoAjs="),   # 32 bytes: two blocks of T
    (73, b"sha1:1000:MzU4NTA4MzIzNzA1MDQ=:19ofiY+ahBXhvkDsp0j2ww=="),          # 16 bytes under SHA-1
    (74, b"sha256:1000:MTc3MTA0MTQwMjQxNzY=:PYjCU215Mi57AYPKva9j7mvF4Rc5bCnt"),  # 24 bytes
]


def test_hashcat_examples():
    from hashcat_a5_table_generator_amd import debug_pbkdf2
    for algo, text in EXAMPLES:
        name, c, salt, dk = text.split(b":")
        salt, dk = base64.b64decode(salt), base64.b64decode(dk)
        assert name.decode() == HASH[algo]
        assert ref(algo, b"hashcat", salt, int(c), len(dk)) == dk, algo
        assert debug_pbkdf2(algo, b"hashcat", salt, int(c), len(dk)) == dk, algo
    assert debug_pbkdf2(75, b"hashcat", b"1234", 1000, 64) == ref(75, b"hashcat", b"1234", 1000, 64)


def test_constants_sizes_and_orders():
    import hashcat_a5_table_generator_amd as a5x
    from hashcat_a5_table_generator_amd import A5xError, _lib, digest_size, salt_order
    L = _lib.load()
    assert (a5x.ALGO_PBKDF2_HMAC_MD5, a5x.ALGO_PBKDF2_HMAC_SHA1, a5x.ALGO_PBKDF2_HMAC_SHA256,
            a5x.ALGO_PBKDF2_HMAC_SHA512) == (72, 73, 74, 75)
    for n in ("ALGO_PBKDF2_HMAC_MD5", "ALGO_PBKDF2_HMAC_SHA1", "ALGO_PBKDF2_HMAC_SHA256", "ALGO_PBKDF2_HMAC_SHA512",
              "debug_pbkdf2"):
        assert n in a5x.__all__
    assert [L.a5x_digest_size(a) for a in range(72, 76)] == [16] * 4
    assert [digest_size(a) for a in range(72, 76)] == [16] * 4
    assert [L.a5x_algo_salt_order(a) for a in range(72, 76)] == [0] * 4
    assert [salt_order(a) for a in range(72, 76)] == [0] * 4
    for a in [4, 8, 9, 15, 23, 31, 39, 47, 100, 128] + list(range(56, 72)) + [76, 77]:
        assert L.a5x_digest_size(a) == E_ARG and L.a5x_algo_salt_order(a) == E_ARG, a
        with pytest.raises(A5xError):
            digest_size(a)
    assert L.a5x_abi_version() == 1


@ALGOS
def test_parser_counts_every_skip_reason(algo):
    from hashcat_a5_table_generator_amd import Context
    other = HASH[72 if algo != 72 else 73].encode()
    good = [line(algo, b"a", b"salt", 1000), line(algo, b"b", b"salt", 1000, 16), line(algo, b"c", b"salt", 999),
            line(algo, b"d", b"", 1), line(algo, b"e", b"s" * 64, 2, 2 * HLEN[algo] + 1), line(algo, b"f", b"other", 1000)]
    name = HASH[algo].encode()
    b64 = lambda b: base64.b64encode(b)
    dk = b64(b"k" * 16)
    bad = [
        other + b":1000:" + b64(b"salt") + b":" + dk,        # a wrong name
        name.upper() + b":1000:" + b64(b"salt") + b":" + dk,  # ... names are lower case
        name + b":1000:c2Fsd*==:" + dk,                       # bad base64 in the salt
        name + b":1000:c2FsdA:" + dk,                         # ... no padding
        name + b":1000:" + b64(b"salt") + b":a2tr=a==",       # ... a character behind padding
        name + b":0:" + b64(b"salt") + b":" + dk,             # iterations 0
        name + b":1e3:" + b64(b"salt") + b":" + dk,           # ... not a number
        name + b"::" + b64(b"salt") + b":" + dk,              # ... missing
        name + b":99999999999:" + b64(b"salt") + b":" + dk,   # ... beyond 32 bits
        name + b":1000:" + b64(b"s" * 65) + b":" + dk,        # a salt over 64 bytes
        name + b":1000:" + b64(b"salt") + b":" + b64(b"k" * 15),  # a key under 16 bytes
        name + b":1000:" + b64(b"salt"),                      # a field short
        name + b":1000:" + b64(b"salt") + b":" + dk + b":x",  # a field more
    ]
    text = b"\n".join([good[0], bad[0], good[1] + b"\r", b"", bad[1], bad[2], good[2], bad[3], bad[4], bad[5], good[3],
                       bad[6], bad[7], bad[8], good[4], bad[9], bad[10], bad[11], good[5], bad[12]])  # (no last newline)
    with Context(-1) as c:
        assert c.load_pbkdf2_hashes(algo, text) == (6, 5, len(bad))
        # (salt, iterations) pairs by first appearance: the same salt under another count is another pair
        assert [(c.salt(i), c.salt_iterations(i)) for i in range(5)] == [
            (b"salt", 1000), (b"salt", 999), (b"", 1), (b"s" * 64, 2), (b"other", 1000)]
        assert c.salt_count() == 5


@ALGOS
def test_host_only_context_keeps_the_set(algo):
    from hashcat_a5_table_generator_amd import A5xError, Context
    salts = [b"bb", b"", b"bb", b"bb", b"z" * 64, b""]
    iters = [5, 1, 6, 5, 1000, 1]
    want = [(b"bb", 5), (b"", 1), (b"bb", 6), (b"z" * 64, 1000)]
    with Context(-1) as c:
        c.set_iterated_targets(algo, b"".join(ref(algo, bytes([i]), s, n) for i, (s, n) in enumerate(zip(salts, iters))),
                               salts, iters)
        assert c.salt_count() == 4 and [(c.salt(i), c.salt_iterations(i)) for i in range(4)] == want
        with pytest.raises(A5xError) as e:
            c.salt_iterations(4)
        assert e.value.code == E_ARG
        c.set_iterated_targets(algo, b"", [], [])  # the empty set
        assert c.salt_count() == 0
        # a salted set of another kind has no iteration counts
        c.set_salted_targets(0, 0, hashlib.md5(b"xs").digest(), [b"s"])
        with pytest.raises(A5xError):
            c.salt_iterations(0)


@ALGOS
def test_refusals(algo):
    from hashcat_a5_table_generator_amd import A5xError, Context, _lib, debug_digest_salted, debug_pbkdf2
    L = _lib.load()
    out = (ctypes.c_uint8 * 64)()
    dig = ref(algo, b"x", b"salt", 3)
    assert debug_pbkdf2(algo, b"p" * 128, b"s" * 64, 1, 16) == ref(algo, b"p" * 128, b"s" * 64, 1)
    for p, s, c in ((b"p", b"s", 0), (b"p", b"s" * 65, 1)):
        with pytest.raises(A5xError) as e:
            debug_pbkdf2(algo, p, s, c, 16)
        assert e.value.code == E_ARG
    for a in (0, 2, 48, 54, 71, 76):
        assert L.a5x_debug_pbkdf2(a, b"p", 1, b"s", 1, 1, out, 16) == E_ARG, a
    with pytest.raises(A5xError) as e:  # the wrong entry points
        debug_digest_salted(algo, 0, b"salt", b"x")
    assert e.value.code == E_ARG
    assert L.a5x_debug_digest(algo, b"abc", 3, out, 64) == E_ARG
    with Context(-1) as c:
        with pytest.raises(A5xError) as e:
            c.set_targets(algo, dig)
        assert e.value.code == E_ARG
        for order in (0, 1):
            with pytest.raises(A5xError) as e:
                c.set_salted_targets(algo, order, dig, [b"salt"])
            assert e.value.code == E_ARG and c.salt_count() == 0
        with pytest.raises(A5xError) as e:
            c.load_salted_hashes(algo, 0, dig.hex().encode() + b":salt\n")
        assert e.value.code == E_ARG and c.salt_count() == 0
        for a in (0, 2, 48, 55, 71, 76):
            with pytest.raises(A5xError) as e:
                c.set_iterated_targets(a, dig, [b"salt"], [3])
            assert e.value.code == E_ARG and c.salt_count() == 0, a
            with pytest.raises(A5xError) as e:
                c.load_pbkdf2_hashes(a, line(algo, b"x", b"salt", 3))
            assert e.value.code == E_ARG, a
        for salts, iters in (([b"salt"], [0]), ([b"s" * 65], [1])):
            with pytest.raises(A5xError) as e:
                c.set_iterated_targets(algo, dig, salts, iters)
            assert e.value.code == E_ARG and c.salt_count() == 0
        # rules on such a set, in both orders of setting
        c.set_iterated_targets(algo, dig, [b"salt"], [3])
        with pytest.raises(A5xError) as e:
            c.set_rules([b":"])
        assert e.value.code == E_UNSUPPORTED and c.rule_count() == 0 and c.salt_count() == 1
    with Context(-1) as c:
        assert c.set_rules([b":", b"u"]) == (2, 0)
        with pytest.raises(A5xError) as e:
            c.set_iterated_targets(algo, dig, [b"salt"], [3])
        assert e.value.code == E_UNSUPPORTED and c.salt_count() == 0 and c.rule_count() == 2
        with pytest.raises(A5xError) as e:
            c.load_pbkdf2_hashes(algo, line(algo, b"x", b"salt", 3))
        assert e.value.code == E_UNSUPPORTED and c.salt_count() == 0


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
    for v in NAME.values():
        assert v in helptext.replace(",", " ").replace(";", " ").split(), v
        assert v in unknown.stderr.replace(",", " ").split(), v
    for v in MODES:
        assert "-m %s" % v in helptext, v
    src = open(os.path.join(ROOT, "hashcat_a5_table_generator_amd", "csrc", "a5x_cli.cpp")).read()
    assert "pbkdf2-hmac-{md5,sha1,sha256,sha512}" in src[: src.index("#include")]
    for v in ("pbkdf2", "pbkdf2-hmac-sha224", "pbkdf2-sha1", "11901"):
        r = _cli(tmp_path, ["--algo", v])
        assert r.returncode == 80 and "--algo:" in r.stderr, v


def test_cli_usage_errors(tmp_path):
    h = tmp_path / "h.txt"
    h.write_bytes(line(73, b"x", b"salt", 3) + b"\n")
    base = ["-t", table_path("czech"), "--hashes", str(h)]
    for algo in ("pbkdf2-hmac-sha1", "12000"):
        for extra, word in ((["--salted=pass.salt"], "--salted"), (["--salted=salt.pass"], "--salted"),
                            (["--hex-salt"], "--hex-salt"), (["--rules", str(h)], "--rules")):
            for args in (["--algo", algo] + extra, extra + ["--algo", algo]):
                r = _cli(tmp_path, base + args)
                assert r.returncode == 80 and word in r.stderr and "PBKDF2" in r.stderr and r.stdout == "", args
        r = _cli(tmp_path, ["-t", table_path("czech"), "--algo", algo])  # such a list needs --hashes
        assert r.returncode == 80 and "--hashes" in r.stderr, algo


def test_selftest_builds_by_its_header_line_and_runs_clean(tmp_path):
    """The line in the program's header, with its output moved to a scratch directory: host code
    under AddressSanitizer and UBSan as a program of its own, on the CPU."""
    src = open(os.path.join(ROOT, "tools", "pbkdf2_selftest.cpp")).read()
    head = src[: src.index("#include")]
    assert "-fsanitize=address,undefined" in head and "-fno-sanitize-recover=all" in head and "tools/pbkdf2_selftest.cpp" in head
    assert "int main()" in src and "a5x_pbkdf2.h" in src
    lines = [l[2:].strip() for l in head.splitlines() if l.startswith("//  ")]
    cmd = " ".join(l.rstrip("\\").strip() for l in lines)
    cmd = cmd[: cmd.index("&&")].strip()
    argv = shlex.split(cmd)
    assert argv[0] == "c++" and argv[-2] == "-o"
    exe = str(tmp_path / "pbkdf2_selftest")
    argv[-1] = exe
    subprocess.run(argv, cwd=ROOT, check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
