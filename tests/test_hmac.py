"""HMAC target lists on the CPU: csrc/a5x_hmac.h (the code the HMAC stream kernel runs, record
preparation included) through a5x_debug_digest_salted against Python's hmac for the eight
algorithms 48..55; the constants, sizes and salt orders; hashcat's and the RFCs' known answers;
the refusals; what a host-only context keeps of such a set; the CLI's names and mode numbers;
and the stand-alone selftest's build line."""
import ctypes
import hashlib
import hmac
import os
import subprocess

import pytest

from conftest import ROOT, table_path

E_ARG, E_HIP, E_CAPACITY, E_UNSUPPORTED = -1, -2, -8, -9
HASH = {48: "md5", 49: "md5", 50: "sha1", 51: "sha1", 52: "sha256", 53: "sha256", 54: "sha512", 55: "sha512"}
SIZE = {48: 16, 49: 16, 50: 20, 51: 20, 52: 32, 53: 32, 54: 64, 55: 64}
ORDER = {a: a & 1 for a in range(48, 56)}  # 0: key = pass, 1: key = salt
NAME = {a: "hmac-%s-key-%s" % (HASH[a], "salt" if ORDER[a] else "pass") for a in range(48, 56)}
MODES = {"50": 48, "60": 49, "150": 50, "160": 51, "1450": 52, "1460": 53, "1750": 54, "1760": 55}
ALGOS = pytest.mark.parametrize("algo", sorted(NAME), ids=[NAME[a] for a in sorted(NAME)])
# key = pass: the salt's message is one block up to 55 bytes, two from 56 (SHA-512: always one);
# lengths = 1, 2, 3 mod 4: the partial last word
SALT_LENS = [0, 1, 2, 3, 4, 5, 15, 16, 31, 32, 55, 56, 63, 64]


def ref(algo, p, s):
    """The definition: HMAC with the candidate as the key (even values) or the salt (odd)."""
    return hmac.new(s, p, HASH[algo]).digest() if ORDER[algo] else hmac.new(p, s, HASH[algo]).digest()


def _bytes(n, seed):
    return bytes((i * 37 + seed * 101 + n * 11 + 5) % 256 for i in range(n))


def test_constants_sizes_and_orders():
    import hashcat_a5_table_generator_amd as a5x
    from hashcat_a5_table_generator_amd import A5xError, _lib, digest_size, salt_order
    L = _lib.load()
    assert (a5x.ALGO_HMAC_MD5_KEY_PASS, a5x.ALGO_HMAC_MD5_KEY_SALT, a5x.ALGO_HMAC_SHA1_KEY_PASS, a5x.ALGO_HMAC_SHA1_KEY_SALT,
            a5x.ALGO_HMAC_SHA256_KEY_PASS, a5x.ALGO_HMAC_SHA256_KEY_SALT, a5x.ALGO_HMAC_SHA512_KEY_PASS,
            a5x.ALGO_HMAC_SHA512_KEY_SALT) == tuple(range(48, 56))
    for n in ("ALGO_HMAC_MD5_KEY_PASS", "ALGO_HMAC_SHA512_KEY_SALT"):
        assert n in a5x.__all__
    assert [L.a5x_digest_size(a) for a in range(48, 56)] == [16, 16, 20, 20, 32, 32, 64, 64]
    assert [digest_size(a) for a in range(48, 56)] == [SIZE[a] for a in range(48, 56)]
    assert [L.a5x_algo_salt_order(a) for a in range(48, 56)] == [0, 1, 0, 1, 0, 1, 0, 1]
    assert [salt_order(a) for a in range(48, 56)] == [ORDER[a] for a in range(48, 56)]
    for a in list(range(39, 48)) + [56]:
        assert L.a5x_digest_size(a) == E_ARG and L.a5x_algo_salt_order(a) == E_ARG, a
        with pytest.raises(A5xError):
            digest_size(a)
        with pytest.raises(A5xError):
            salt_order(a)
    assert L.a5x_abi_version() == 1


KNOWN = [  # password "hashcat", salt "1234": hashcat's example hashes of these modes
    (48, "fc741db0a2968c39d9c2a5cc75b05370"),
    (49, "bfd280436f45fa38eaacac3b00518f29"),
    (50, "c898896f3f70f61bc3fb19bef222aa860e5ea717"),
    (51, "d89c92b4400b15c39e462a8caa939ab40c3aeeea"),
    (52, "abaf88d66bf2334a4a8b207cc61a96fb46c3e38e882e6f6f886742f688b8588c"),
    (53, "8efbef4cec28f228fa948daaf4893ac3638fbae81358ff9020be1d7a9a509fc6"),
]
RFC = [  # RFC 2202 / 4231 test case 2: key "Jefe", data "what do ya want for nothing?"
    ("md5", 48, "750c783e6ab0b503eaa86e310a5db738"),
    ("sha1", 50, "effcdf6ae5eb2fa2d27416d5f184df9c259a7c79"),
    ("sha256", 52, "5bdcc146bf60754e6a042426089575c75a003f089d2739839dec58b964ec3843"),
]


def test_known_answers():
    from hashcat_a5_table_generator_amd import debug_digest_salted
    for algo, want in KNOWN:
        assert debug_digest_salted(algo, ORDER[algo], b"1234", b"hashcat").hex() == want, algo
        assert ref(algo, b"hashcat", b"1234").hex() == want, algo
    key, data = b"Jefe", b"what do ya want for nothing?"
    for _, kp, want in RFC:
        # key = pass: the candidate is the key; key = salt: the salt is
        assert debug_digest_salted(kp, 0, data, key).hex() == want, kp
        assert debug_digest_salted(kp + 1, 1, key, data).hex() == want, kp + 1
    want512 = hmac.new(key, data, "sha512").hexdigest()
    assert debug_digest_salted(54, 0, data, key).hex() == want512
    assert debug_digest_salted(55, 1, key, data).hex() == want512


@ALGOS
def test_debug_digest_salted_matches_hmac(algo):
    """Every candidate length 0..128: the key used as it is / pre-hashed at 64 / 65 and the
    pre-hash's own blocks at 119 / 120 (key = pass, 64-byte blocks); the message's blocks at 55 /
    56 and 119 / 120, SHA-512 111 / 112 (key = salt); the salt's blocks at 55 / 56 (key = pass)."""
    from hashcat_a5_table_generator_amd import debug_digest_salted
    bad = []
    for sl in SALT_LENS:
        salt = _bytes(sl, 3)
        for n in range(129):
            p = _bytes(n, sl)
            if debug_digest_salted(algo, ORDER[algo], salt, p) != ref(algo, p, salt):
                bad.append((n, sl))
    assert not bad, (len(bad), bad[:10])


@ALGOS
def test_refusals(algo):
    from hashcat_a5_table_generator_amd import A5xError, Context, _lib, debug_digest_salted
    L = _lib.load()
    out = (ctypes.c_uint8 * 64)()
    o = ORDER[algo]
    assert debug_digest_salted(algo, o, b"s" * 64, b"p" * 128) == ref(algo, b"p" * 128, b"s" * 64)  # no pair skipped for its salt
    for salt, msg, order, code in ((b"s", b"p" * 129, o, E_UNSUPPORTED), (b"", b"p" * 129, o, E_UNSUPPORTED),
                                   (b"s", b"p", 1 - o, E_ARG), (b"s", b"p", 2, E_ARG), (b"s" * 65, b"p", o, E_ARG)):
        with pytest.raises(A5xError) as e:
            debug_digest_salted(algo, order, salt, msg)
        assert e.value.code == code, (len(salt), len(msg), order)
    assert L.a5x_debug_digest_salted(algo, o, b"s", 1, b"p", 1, out, SIZE[algo] - 1) == E_CAPACITY
    assert L.a5x_debug_digest(algo, b"abc", 3, out, 64) == E_ARG  # salted only
    dig = ref(algo, b"x", b"salt")
    with Context(-1) as c:
        with pytest.raises(A5xError, match="salted only") as e:
            c.set_targets(algo, dig)
        assert e.value.code == E_ARG
        with pytest.raises(A5xError) as e:
            c.set_salted_targets(algo, 1 - o, dig, [b"salt"])
        assert e.value.code == E_ARG and c.salt_count() == 0
        with pytest.raises(A5xError) as e:
            c.set_salted_targets(algo, 2, dig, [b"salt"])
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


@ALGOS
def test_host_only_context_keeps_the_original_salts(algo):
    from hashcat_a5_table_generator_amd import Context
    o = ORDER[algo]
    salts = [b"bb", b"", b"a", b"bb", b"cc:cc", b"", b"z" * 64, b"b"]
    want = [b"bb", b"", b"a", b"cc:cc", b"z" * 64, b"b"]
    with Context(-1) as c:
        c.set_salted_targets(algo, o, b"".join(ref(algo, bytes([i]), s) for i, s in enumerate(salts)), salts)
        assert c.salt_count() == len(want) and [c.salt(i) for i in range(len(want))] == want
        h = lambda i, s: ref(algo, bytes([i]), s).hex().encode()
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
        assert SIZE[algo] == len(ref(algo, b"", b"")) == hashlib.new(HASH[algo]).digest_size


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
    for v in ("hmac-md5", "151", "hmac-sha1-key-pepper", "hmac-sha224-key-pass"):
        r = _cli(tmp_path, ["--algo", v])
        assert r.returncode == 80 and "--algo:" in r.stderr, v


def test_cli_order_must_agree(tmp_path):
    h = tmp_path / "h.txt"
    h.write_bytes(ref(48, b"x", b"salt").hex().encode() + b":salt\n")
    base = ["-t", table_path("czech"), "--hashes", str(h)]
    for args in (["--algo", "50", "--salted=salt.pass"], ["--salted=pass.salt", "--algo", "hmac-md5-key-salt"],
                 ["--algo", "1460", "--salted=pass.salt", "--hex-salt"], ["--algo", "hmac-sha512-key-pass", "--salted=salt.pass"]):
        r = _cli(tmp_path, base + args)
        assert r.returncode == 80 and "contradicts" in r.stderr and r.stdout == "", args
    # without --hashes an HMAC algorithm is the usage error a salted mode number is
    for v in ("150", "hmac-sha256-key-salt"):
        r = _cli(tmp_path, ["-t", table_path("czech"), "--algo", v])
        assert r.returncode == 80 and "--hashes" in r.stderr, v
    # rules stay refused with such a list
    for v in ("50", "hmac-sha512-key-salt"):
        r = _cli(tmp_path, base + ["--algo", v, "--rules", str(h)])
        assert r.returncode == 80 and "rules" in r.stderr, v


def test_selftest_build_line_is_in_its_header():
    src = open(os.path.join(ROOT, "tools", "hmac_selftest.cpp")).read()
    head = src[: src.index("#include")]
    assert "-fsanitize=address,undefined" in head and "-fno-sanitize-recover=all" in head and "tools/hmac_selftest.cpp" in head
    assert "int main()" in src and "a5x_hmac.h" in src
