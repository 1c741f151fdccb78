"""SHA-224 / SHA-384 / SHA-512 of the digest + lookup stage without a GPU: the
__host__ __device__ digest core the kernels run (csrc/a5x_sha.h, through the test hook
a5x_debug_digest) against hashlib, the digest widths, and the host-side argument handling
of the three algorithms."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import table_path

SHA224, SHA384, SHA512 = 5, 6, 7
REF = {SHA224: hashlib.sha224, SHA384: hashlib.sha384, SHA512: hashlib.sha512}
SIZE = {SHA224: 28, SHA384: 48, SHA512: 64}
ALGOS = pytest.mark.parametrize("algo", [SHA224, SHA384, SHA512])
# every length through two SHA-512 blocks and four SHA-256 blocks (all padding edges:
# 55/56, 111/112, 119/120, 127/128, 239/240, 255/256), then many blocks
LENGTHS = list(range(0, 301)) + [1000, 65535]


def _debug_digest(algo, msg):
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    n = L.a5x_digest_size(algo)
    out = (ctypes.c_uint8 * n)()
    assert L.a5x_debug_digest(algo, msg, len(msg), out, n) == 0
    return bytes(out)


def test_digest_size():
    from hashcat_a5_table_generator_amd import _lib, digest_size, A5xError
    from hashcat_a5_table_generator_amd import ALGO_SHA224, ALGO_SHA384, ALGO_SHA512
    L = _lib.load()
    assert (ALGO_SHA224, ALGO_SHA384, ALGO_SHA512) == (SHA224, SHA384, SHA512)
    assert [L.a5x_digest_size(a) for a in (5, 6, 7)] == [28, 48, 64]
    assert [L.a5x_digest_size(a) for a in (4, 8, -1)] == [-1, -1, -1]  # A5X_E_ARG: 4 stays unassigned
    assert [digest_size(a) for a in (5, 6, 7)] == [28, 48, 64]
    for a in (4, 8, -1):
        with pytest.raises(A5xError):
            digest_size(a)


@ALGOS
def test_debug_digest_matches_hashlib(algo):
    rng = np.random.default_rng(2209 + algo)
    for n in LENGTHS:
        msg = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert _debug_digest(algo, msg) == REF[algo](msg).digest(), n


def test_debug_digest_fips_abc():
    assert _debug_digest(SHA224, b"abc").hex() == "23097d223405d8228642a477bda255b32aadbce4bda0b3f7e36c9da7"
    assert _debug_digest(SHA384, b"abc").hex() == (
        "cb00753f45a35e8bb5a03d699ac65007272c32ab0eded1631a8b605a43ff5bed"
        "8086072ba1e7cc2358baeca134c825a7")
    assert _debug_digest(SHA512, b"abc").hex() == (
        "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a"
        "2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f")


@ALGOS
def test_debug_digest_arguments(algo):
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    out = (ctypes.c_uint8 * 64)()
    assert L.a5x_debug_digest(algo, b"abc", 3, out, SIZE[algo] - 1) == -8  # A5X_E_CAPACITY
    assert L.a5x_debug_digest(algo, b"abc", 3, None, 64) == -1            # A5X_E_ARG
    assert L.a5x_debug_digest(8, b"abc", 3, out, 64) == -1


@ALGOS
def test_set_targets_on_a_host_only_context(algo):
    """No CPU fallback: a host-only context refuses, as for SHA-1."""
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.a5x_create(-1, ctypes.byref(h)) == 0
    dig = REF[algo](b"x").digest()
    assert L.a5x_set_targets(h, algo, dig, 1) == -2  # A5X_E_HIP
    assert b"host-only" in L.a5x_last_error(h)
    L.a5x_destroy(h)


def test_python_set_targets_checks_the_length_per_algorithm():
    from hashcat_a5_table_generator_amd import A5xError, Context
    with Context(-1) as c:
        for algo, size in SIZE.items():
            with pytest.raises(ValueError, match=f"digests must be {size} bytes each"):
                c.set_targets(algo, bytes(size + 1))
            with pytest.raises(A5xError, match="host-only"):  # a whole number of digests reaches the library
                c.set_targets(algo, bytes(2 * size))


def test_cli_rejects_an_unknown_algo_naming_all_seven(tmp_path):
    from hashcat_a5_table_generator_amd import build
    assert os.path.exists(build.CLI)
    d = tmp_path / "d.txt"
    d.write_bytes(b"abc\n")
    r = subprocess.run([build.CLI, str(d), "-t", table_path("czech"), "--hashes", str(d), "--algo", "sha3"],
                       capture_output=True, text=True)
    assert r.returncode == 80
    for name in ("md5", "ntlm", "sha1", "sha224", "sha256", "sha384", "sha512"):
        assert name in r.stderr.replace(",", " ").split()
