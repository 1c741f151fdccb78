"""SHA-1 / SHA-256 of the fused digest stage without a GPU: the __host__ __device__ digest
core the kernels run (csrc/a5x_sha.h, through the test hook a5x_debug_digest) against
hashlib, the digest widths, and the host-side argument handling of the new algorithms."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import table_path

ALGO_SHA1, ALGO_SHA256 = 2, 3
REF = {ALGO_SHA1: hashlib.sha1, ALGO_SHA256: hashlib.sha256}
# 55/56 and 119/120: the padding spills into a second / third block; 63/64: block edges
LENGTHS = [0, 1, 3, 4, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 127, 128, 129, 1000]


def _debug_digest(algo, msg):
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    n = L.a5x_digest_size(algo)
    out = (ctypes.c_uint8 * n)()
    assert L.a5x_debug_digest(algo, msg, len(msg), out, n) == 0
    return bytes(out)


def test_digest_size():
    from hashcat_a5_table_generator_amd import _lib, digest_size, A5xError
    L = _lib.load()
    assert [L.a5x_digest_size(a) for a in range(4)] == [16, 16, 20, 32]
    assert L.a5x_digest_size(-1) == -1 and L.a5x_digest_size(4) == -1  # A5X_E_ARG
    assert [digest_size(a) for a in range(4)] == [16, 16, 20, 32]
    with pytest.raises(A5xError):
        digest_size(4)


@pytest.mark.parametrize("algo", [ALGO_SHA1, ALGO_SHA256])
def test_debug_digest_matches_hashlib(algo):
    rng = np.random.default_rng(1804 + algo)
    for n in LENGTHS:
        msg = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert _debug_digest(algo, msg) == REF[algo](msg).digest(), n


def test_debug_digest_fips_abc():
    assert _debug_digest(ALGO_SHA1, b"abc").hex() == "a9993e364706816aba3e25717850c26c9cd0d89d"
    assert _debug_digest(ALGO_SHA256, b"abc").hex() == \
        "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"


def test_debug_digest_arguments():
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    out = (ctypes.c_uint8 * 32)()
    assert L.a5x_debug_digest(ALGO_SHA256, b"abc", 3, out, 20) == -8  # A5X_E_CAPACITY
    assert L.a5x_debug_digest(4, b"abc", 3, out, 32) == -1            # A5X_E_ARG
    assert L.a5x_debug_digest(ALGO_SHA1, b"abc", 3, None, 32) == -1


def test_set_targets_sha1_on_a_host_only_context():
    """No CPU fallback for the new algorithms either: a host-only context refuses, as for MD5."""
    from hashcat_a5_table_generator_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.a5x_create(-1, ctypes.byref(h)) == 0
    dig = hashlib.sha1(b"x").digest()
    assert L.a5x_set_targets(h, ALGO_SHA1, dig, 1) == -2  # A5X_E_HIP
    assert b"host-only" in L.a5x_last_error(h)
    hit = _lib.Hit()
    n = ctypes.c_size_t()
    assert L.a5x_hit_digest(h, ctypes.byref(hit), None, 0, ctypes.byref(n)) == -1  # no target set
    L.a5x_destroy(h)


def test_python_set_targets_checks_the_length_per_algorithm():
    from hashcat_a5_table_generator_amd import A5xError, Context
    with Context(-1) as c:
        for algo, size in ((0, 16), (1, 16), (ALGO_SHA1, 20), (ALGO_SHA256, 32)):
            with pytest.raises(ValueError, match=f"digests must be {size} bytes each"):
                c.set_targets(algo, bytes(size + 1))
            with pytest.raises(A5xError, match="host-only"):  # a whole number of digests reaches the library
                c.set_targets(algo, bytes(2 * size))


def test_cli_rejects_an_unknown_algo_naming_all_four(tmp_path):
    from hashcat_a5_table_generator_amd import build
    assert os.path.exists(build.CLI)
    d = tmp_path / "d.txt"
    d.write_bytes(b"abc\n")
    r = subprocess.run([build.CLI, str(d), "-t", table_path("czech"), "--hashes", str(d), "--algo", "sha3"],
                       capture_output=True, text=True)
    assert r.returncode == 80
    for name in ("md5", "ntlm", "sha1", "sha256"):
        assert name in r.stderr
