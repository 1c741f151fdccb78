"""Nested digests on the CPU: csrc/a5x_nest.h (the code the stream kernels run) through
a5x_debug_digest against hashlib compositions for the seven algorithms, the published
"hashcat" vectors, the sizes and constants, the refusals (host-only contexts, salted entry
points, unassigned values), the CLI's names and the stand-alone selftest's build line."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, table_path

MD5_MD5, MD5_MD5_MD5, MD5_MD5UP, MD5_SHA1, SHA1_SHA1, SHA1_MD5, SHA256_MD5 = range(16, 23)
E_ARG, E_HIP = -1, -2


def _md5(b):
    return hashlib.md5(b).digest()


def _sha1(b):
    return hashlib.sha1(b).digest()


def _hex(d):
    return d.hex().encode()


REF = {
    MD5_MD5: lambda p: _md5(_hex(_md5(p))),
    MD5_MD5_MD5: lambda p: _md5(_hex(_md5(_hex(_md5(p))))),
    MD5_MD5UP: lambda p: _md5(_hex(_md5(p)).upper()),
    MD5_SHA1: lambda p: _md5(_hex(_sha1(p))),
    SHA1_SHA1: lambda p: _sha1(_hex(_sha1(p))),
    SHA1_MD5: lambda p: _sha1(_hex(_md5(p))),
    SHA256_MD5: lambda p: hashlib.sha256(_hex(_md5(p))).digest(),
}
SIZE = {MD5_MD5: 16, MD5_MD5_MD5: 16, MD5_MD5UP: 16, MD5_SHA1: 16, SHA1_SHA1: 20, SHA1_MD5: 20, SHA256_MD5: 32}
NAME = {MD5_MD5: "md5-md5", MD5_MD5_MD5: "md5-md5-md5", MD5_MD5UP: "md5-md5up", MD5_SHA1: "md5-sha1",
        SHA1_SHA1: "sha1-sha1", SHA1_MD5: "sha1-md5", SHA256_MD5: "sha256-md5"}
# each algorithm over b"hashcat": hashcat's published example hashes of -m 2600 / 3500 / 4300 /
# 4400 / 4500 / 4700 / 20800
HASHCAT = {
    MD5_MD5: "a936af92b0ae20b1ff6c3347a72e5fbe",
    MD5_MD5_MD5: "9882d0778518b095917eb589f6998441",
    MD5_MD5UP: "b8c385461bb9f9d733d3af832cf60b27",
    MD5_SHA1: "288496df99b33f8f75a7ce4837d1b480",
    SHA1_SHA1: "3db9184f5da4e463832b086211af8d2314919951",
    SHA1_MD5: "92d85978d884eb1d99a51652b1139c8279fa8663",
    SHA256_MD5: "74ee1fae245edd6f27bf36efc3604942479fceefbadab5dc5c0b538c196eb0f1",
}
ALGOS = pytest.mark.parametrize("algo", sorted(REF), ids=[NAME[a] for a in sorted(REF)])
# every length through the inner digests' padding edges (55/56, 63/64, 119/120), then many blocks
LENGTHS = list(range(0, 301)) + [1000, 65535]


def _debug_digest(algo, msg):
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    n = L.a5x_digest_size(algo)
    assert n > 0, (algo, n)
    out = (ctypes.c_uint8 * n)()
    assert L.a5x_debug_digest(algo, msg, len(msg), out, n) == 0
    return bytes(out)


def test_constants_and_sizes():
    import hashcat_a5_table_generator_amd as a5x
    from hashcat_a5_table_generator_amd import A5xError, _lib, digest_size
    assert (a5x.ALGO_MD5_MD5, a5x.ALGO_MD5_MD5_MD5, a5x.ALGO_MD5_MD5UP, a5x.ALGO_MD5_SHA1, a5x.ALGO_SHA1_SHA1,
            a5x.ALGO_SHA1_MD5, a5x.ALGO_SHA256_MD5) == (16, 17, 18, 19, 20, 21, 22)
    L = _lib.load()
    assert [L.a5x_digest_size(a) for a in range(16, 23)] == [16, 16, 16, 16, 20, 20, 32]
    assert [digest_size(a) for a in range(16, 23)] == [16, 16, 16, 16, 20, 20, 32]
    assert [L.a5x_digest_size(a) for a in (9, 15, 23)] == [E_ARG] * 3
    for a in (9, 15, 23):
        with pytest.raises(A5xError):
            digest_size(a)
    assert L.a5x_abi_version() == 1


def test_the_reference_compositions_give_the_published_vectors():
    for algo, hx in HASHCAT.items():
        assert REF[algo](b"hashcat").hex() == hx


@ALGOS
def test_hashcat_vector(algo):
    assert _debug_digest(algo, b"hashcat").hex() == HASHCAT[algo]


@ALGOS
def test_debug_digest_matches_hashlib(algo):
    rng = np.random.default_rng(2600 + algo)
    for n in LENGTHS:
        msg = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert _debug_digest(algo, msg) == REF[algo](msg), n


def test_every_hex_digit_value_in_both_cases():
    """Messages whose MD5 runs through every byte value are not to be had on purpose; 3000
    random ones carry each of the 256 values in an inner digest many times over."""
    rng = np.random.default_rng(4300)
    seen = set()
    for _ in range(3000):
        msg = rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        seen |= set(_md5(msg))
        assert _debug_digest(MD5_MD5, msg) == REF[MD5_MD5](msg)
        assert _debug_digest(MD5_MD5UP, msg) == REF[MD5_MD5UP](msg)
    assert len(seen) == 256


def test_debug_digest_arguments():
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    out = (ctypes.c_uint8 * 64)()
    for algo in (0, 1, 4, 8, 9, 10, 11, 12, 13, 14, 15, 23, 24, 100, -1):
        assert L.a5x_debug_digest(algo, b"abc", 3, out, 64) == E_ARG, algo
    for algo, size in SIZE.items():
        assert L.a5x_debug_digest(algo, b"abc", 3, out, size - 1) == -8  # A5X_E_CAPACITY
        assert L.a5x_debug_digest(algo, b"abc", 3, None, 64) == E_ARG
        assert L.a5x_debug_digest(algo, b"abc", 3, out, size) == 0


@ALGOS
def test_set_targets_on_a_host_only_context(algo):
    """No CPU fallback: a host-only context refuses, as for the plain algorithms."""
    from hashcat_a5_table_generator_amd import A5xError, Context
    with Context(-1) as c:
        with pytest.raises(ValueError, match=f"digests must be {SIZE[algo]} bytes each"):
            c.set_targets(algo, bytes(SIZE[algo] + 1))
        with pytest.raises(A5xError, match="host-only") as e:
            c.set_targets(algo, REF[algo](b"x"))
        assert e.value.code == E_HIP


@ALGOS
def test_salted_entry_points_refuse(algo):
    from hashcat_a5_table_generator_amd import A5xError, Context, debug_digest_salted
    dig = REF[algo](b"x")
    with Context(-1) as c:
        with pytest.raises(A5xError, match="no salted mode") as e:
            c.set_salted_targets(algo, 0, dig, [b"salt"])
        assert e.value.code == E_ARG and c.salt_count() == 0
        with pytest.raises(A5xError, match="no salted mode") as e:
            c.load_salted_hashes(algo, 1, dig.hex().encode() + b":salt\n")
        assert e.value.code == E_ARG and c.salt_count() == 0
    with pytest.raises(A5xError) as e:
        debug_digest_salted(algo, 0, b"salt", b"pass")
    assert e.value.code == E_ARG


def _cli(tmp_path, args):
    from hashcat_a5_table_generator_amd import build
    assert os.path.exists(build.CLI)
    d = tmp_path / "d.txt"
    d.write_bytes(b"abc\n")
    return subprocess.run([build.CLI, str(d)] + args, capture_output=True, text=True, timeout=60)


def test_cli_names_and_modes_parse(tmp_path):
    """A known --algo value gets past the parser to the next usage error (no table given), an
    unknown one stops at --algo; no device is opened either way."""
    unknown = _cli(tmp_path, ["--algo", "sha3"])
    assert unknown.returncode == 80 and "--algo:" in unknown.stderr
    for name in ("md5", "ntlm", "sha1", "sha224", "sha256", "sha384", "sha512"):
        assert name in unknown.stderr.replace(",", " ").split()
    for v in list(NAME.values()) + ["2600", "3500", "4300", "4400", "4500", "4700", "20800"]:
        r = _cli(tmp_path, ["--algo", v])
        assert r.returncode == 80 and "--algo:" not in r.stderr and "--table-files" in r.stderr, v
        assert v in unknown.stderr.replace(",", " ").split() or v.isdigit()
    for v in ("md5-md4", "2601", "md5_md5", "sha1-sha256"):
        r = _cli(tmp_path, ["--algo", v])
        assert r.returncode == 80 and "--algo:" in r.stderr, v
    helptext = _cli(tmp_path, ["--help"]).stdout
    for v in list(NAME.values()) + ["2600", "3500", "4300", "4400", "4500", "4700", "20800"]:
        assert v in helptext, v


def test_cli_refuses_salted_nested(tmp_path):
    h = tmp_path / "h.txt"
    h.write_bytes(HASHCAT[MD5_MD5].encode() + b":salt\n")
    base = ["-t", table_path("czech"), "--hashes", str(h)]
    for args in (["--algo", "2600", "--salted=pass.salt"], ["--algo", "md5-md5", "--salted=salt.pass"],
                 ["--algo", "sha256-md5", "--salted=pass.salt", "--hex-salt"], ["--salted=pass.salt", "--algo", "4500"]):
        r = _cli(tmp_path, base + args)
        assert r.returncode == 80 and "error:" in r.stderr and "nested" in r.stderr and r.stdout == "", args


def test_selftest_build_line_is_in_its_header():
    src = open(os.path.join(ROOT, "tools", "nest_selftest.cpp")).read()
    head = src[: src.index("#include")]
    assert "-fsanitize=address,undefined" in head and "tools/nest_selftest.cpp" in head
    assert "int main()" in src and "a5x_nest.h" in src
