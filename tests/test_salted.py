"""Salted target lists on the CPU: the message assembly of csrc/a5x_salt.h (the code
k_salt_stream runs) with the host digest cores against hashlib of the concatenation, the
validation of a5x_set_salted_targets, the hash:salt file reader, and the refusal of rules
and salts together -- all on a host-only context."""
import hashlib

import pytest

MD5, NTLM, SHA1, SHA256, SHA224, SHA384, SHA512 = 0, 1, 2, 3, 5, 6, 7
REF = {MD5: hashlib.md5, SHA1: hashlib.sha1, SHA256: hashlib.sha256, SHA224: hashlib.sha224, SHA384: hashlib.sha384,
       SHA512: hashlib.sha512}
ALGOS = pytest.mark.parametrize("algo", sorted(REF), ids=["md5", "sha1", "sha256", "sha224", "sha384", "sha512"])
ORDERS = pytest.mark.parametrize("order", [0, 1], ids=["pass.salt", "salt.pass"])
E_ARG, E_UNSUPPORTED = -1, -9


def _bytes(n, seed):
    return bytes((1 + (i * 37 + seed * 101 + n * 7) % 255) for i in range(n))


def _msg(order, cand, salt):
    return cand + salt if order == 0 else salt + cand


def _pairs():
    """(len, slen): every pair of len % 4 and slen % 4, message lengths on both sides of the
    padding edges, empty parts, the longest salt, the 128-byte limit."""
    out = {(ln, sl) for ln in (8, 9, 10, 11) for sl in (4, 5, 6, 7)}
    out |= {(ln, sl) for ln in (0, 1, 2, 3) for sl in (0, 1, 2, 3)}
    for edge in (55, 56, 63, 64, 111, 112, 119, 120, 127, 128):
        for sl in (0, 1, 7, 8, 33, 64):
            if edge - sl >= 0:
                out.add((edge - sl, sl))
    out |= {(0, 0), (0, 64), (64, 0), (17, 0), (0, 17), (64, 64), (1, 64), (63, 64), (128, 0)}
    assert all(ln + sl <= 128 and sl <= 64 for ln, sl in out)
    assert {(ln % 4, sl % 4) for ln, sl in out} == {(a, b) for a in range(4) for b in range(4)}
    return sorted(out)


@ALGOS
@ORDERS
def test_debug_digest_salted_matches_hashlib(algo, order):
    from hashcat_a5_table_generator_amd import debug_digest_salted
    f = REF[algo]
    bad = []
    for ln, sl in _pairs():
        cand, salt = _bytes(ln, 1), _bytes(sl, 2)
        got = debug_digest_salted(algo, order, salt, cand)
        if got != f(_msg(order, cand, salt)).digest():
            bad.append((ln, sl, got.hex()))
    assert not bad, bad[:5]


@ALGOS
@ORDERS
def test_the_128_byte_limit(algo, order):
    from hashcat_a5_table_generator_amd import A5xError, debug_digest_salted
    f = REF[algo]
    for ln, sl in ((128, 0), (64, 64), (127, 1), (96, 32)):
        cand, salt = _bytes(ln, 3), _bytes(sl, 4)
        assert debug_digest_salted(algo, order, salt, cand) == f(_msg(order, cand, salt)).digest()
    for ln, sl in ((129, 0), (65, 64), (128, 1), (97, 32)):
        with pytest.raises(A5xError) as e:
            debug_digest_salted(algo, order, _bytes(sl, 4), _bytes(ln, 3))
        assert e.value.code == E_UNSUPPORTED
    with pytest.raises(A5xError) as e:  # a salt over 64 bytes is no salt at all
        debug_digest_salted(algo, order, _bytes(65, 4), b"x")
    assert e.value.code == E_ARG


def test_debug_digest_salted_refuses_ntlm_and_bad_orders():
    from hashcat_a5_table_generator_amd import A5xError, debug_digest_salted
    for algo, order in ((NTLM, 0), (4, 0), (99, 1), (MD5, 2), (SHA1, -1)):
        with pytest.raises(A5xError) as e:
            debug_digest_salted(algo, order, b"salt", b"pass")
        assert e.value.code == E_ARG


@pytest.fixture
def host_ctx():
    from hashcat_a5_table_generator_amd import Context
    with Context(-1) as c:
        yield c


def test_validation(host_ctx):
    from hashcat_a5_table_generator_amd import A5xError
    c = host_ctx
    d = hashlib.md5(b"x").digest()
    for algo, order, dig, salts in ((NTLM, 0, d, [b"s"]), (4, 0, d, [b"s"]), (MD5, 2, d, [b"s"]), (MD5, -1, d, [b"s"]),
                                    (MD5, 0, d, [b"s" * 65]), (SHA1, 1, hashlib.sha1(b"x").digest(), [b"s" * 65])):
        with pytest.raises(A5xError) as e:
            c.set_salted_targets(algo, order, dig, salts)
        assert e.value.code == E_ARG, (algo, order)
        assert c.salt_count() == 0
    c.set_salted_targets(MD5, 0, d, [b"s" * 64])
    assert c.salt_count() == 1 and c.salt(0) == b"s" * 64


def test_salts_are_deduplicated_by_first_appearance(host_ctx):
    from hashcat_a5_table_generator_amd import A5xError
    c = host_ctx
    salts = [b"bb", b"", b"a", b"bb", b"cccc", b"", b"a", b"z" * 64, b"b"]
    digs = b"".join(hashlib.sha256(bytes([i])).digest() for i in range(len(salts)))
    c.set_salted_targets(SHA256, 1, digs, salts)
    want = [b"bb", b"", b"a", b"cccc", b"z" * 64, b"b"]
    assert c.salt_count() == len(want)
    assert [c.salt(i) for i in range(len(want))] == want
    with pytest.raises(A5xError) as e:
        c.salt(len(want))
    assert e.value.code == E_ARG
    # a5x_set_targets makes the set unsalted again (a host-only context cannot hold its
    # device tables: the call still fails there as it always did, and the salts are gone)
    with pytest.raises(A5xError) as e:
        c.set_targets(SHA256, digs)
    assert e.value.code == -2
    assert c.salt_count() == 0


def test_load_salted_hashes(host_ctx):
    c = host_ctx
    h = lambda b: hashlib.sha1(b).hexdigest().encode()
    text = b"\n".join([
        h(b"1") + b":na:cl",           # a literal salt with a ':'
        h(b"2") + b":crlf\r",          # "\r\n" line
        h(b"3") + b":",                # an empty salt
        b"",                           # (an empty line: no target, no error)
        h(b"4"),                       # no colon: skipped
        h(b"5")[:-2] + b":short",      # a short digest: skipped
        h(b"6") + b"0:long",           # a long digest: skipped
        b"zz" + h(b"7")[2:] + b":hex", # not hex: skipped
        h(b"8") + b":" + b"s" * 65,    # a 65-byte salt: skipped
        h(b"9") + b":" + b"s" * 64,
        h(b"10") + b":na:cl",          # a repeated salt
    ]) + b"\n"
    assert c.load_salted_hashes(SHA1, 0, text) == (5, 4, 5)
    assert [c.salt(i) for i in range(4)] == [b"na:cl", b"crlf", b"", b"s" * 64]
    hx = b"\n".join([
        h(b"1") + b":6e613a00ff",
        h(b"2") + b":6E61",            # upper-case hex
        h(b"3") + b":",                # an empty hex salt
        h(b"4") + b":abc",             # odd length: skipped
        h(b"5") + b":zz",              # not hex: skipped
        h(b"6") + b":" + b"61" * 65,   # 65 bytes: skipped
        h(b"7") + b":" + b"61" * 64,
    ])
    assert c.load_salted_hashes(SHA1, 1, hx, hex_salt=True) == (4, 4, 3)
    assert [c.salt(i) for i in range(4)] == [b"na:\x00\xff", b"na", b"", b"a" * 64]
    assert c.load_salted_hashes(SHA1, 0, b"") == (0, 0, 0) and c.salt_count() == 0


def test_rules_and_salts_refuse_each_other(host_ctx):
    from hashcat_a5_table_generator_amd import A5xError
    c = host_ctx
    d = hashlib.md5(b"x").digest()
    assert c.set_rules([b":", b"u"]) == (2, 0)
    with pytest.raises(A5xError) as e:
        c.set_salted_targets(MD5, 0, d, [b"salt"])
    assert e.value.code == E_UNSUPPORTED and "rules" in str(e.value) and "salt" in str(e.value)
    assert c.salt_count() == 0 and c.rule_count() == 2
    c.clear_rules()
    c.set_salted_targets(MD5, 0, d, [b"salt"])  # after clear_rules the salted set loads
    assert c.salt_count() == 1
    with pytest.raises(A5xError) as e:
        c.set_rules([b":"])
    assert e.value.code == E_UNSUPPORTED and "rules" in str(e.value) and "salt" in str(e.value)
    assert c.rule_count() == 0 and c.salt_count() == 1
    c.clear_rules()  # clearing rules is no rule set: allowed on a salted set
    assert c.set_rules([b"# only a comment"]) == (0, 0)
