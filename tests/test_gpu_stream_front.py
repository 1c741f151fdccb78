"""The line-stream front end (csrc/a5x_stream.h) agrees on the three routes that share it:
k_digest_stream, k_rules_stream under the single rule ':' and k_salt_stream under the single
empty salt digest one hand-built stream, whose lines sit on every edge the block staging and
the newline scan have: the same line count as the host's split, and every line's digest equal
to hashlib (oracle/digest_oracle.ntlm for NTLM).  On the rules and salt routes a line over
128 bytes is hashed under no rule / salt: all-zero digests, counted by rules_last() /
salts_last().

Line count: a line is what starts at byte 0 or behind a '\\n', inside the stream.  For a stream
that ends in '\\n' that is stream.split(b"\\n") without the empty piece behind the last '\\n';
for the unterminated variant it is stream.split(b"\\n") as it stands."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MD5, NTLM, SHA1, SHA512 = 0, 1, 2, 7
SIZE = {MD5: 16, NTLM: 16, SHA1: 20, SHA512: 64}
B, H, MARGIN, LMAX = 4096, 2048, 256, 128


def _filler(k, n):
    """n bytes without '\\n', different for every k"""
    return bytes(33 + (k * 31 + i * 7) % 90 for i in range(n))


def _build():
    """The stream with its final '\\n', and the positions the test asserts on."""
    out = bytearray()
    k = [0]

    def line(n):
        out.extend(_filler(k[0], n) + b"\n")
        k[0] += 1

    def pad_to(pos):  # filler lines of at most 100 bytes; the next line starts at pos
        assert pos >= len(out)
        while len(out) < pos:
            line(min(pos - len(out), 1 + (k[0] * 37) % 100) - 1)

    out += b"\n"                       # an empty first line
    out += "abc\n\n\nš1\n".encode()    # two consecutive '\n' in the middle
    pad_to(H - 18); line(40)           # straddles the odd 2 KiB edge at 2048 only
    pad_to(B - 61); line(60)           # its '\n' is the last byte of block 0
    pad_to(5000); line(129)            # one byte over the rules / salt limit
    pad_to(2 * B - 42); line(100)      # straddles the 4 KiB edge at 8192
    pad_to(3 * B - 20); line(20)       # its '\n' is the first byte of block 3
    pad_to(4 * B - 30); line(300)      # starts in the last 40 bytes of block 3, ends past its margin
    line(7); line(0); line(45)
    line(3 + (13 - (len(out) + 4) % 16) % 16)  # total length = 13 mod 16
    return bytes(out)


STREAM = _build()
VARIANTS = {"terminated": STREAM, "unterminated": STREAM[:-1]}


def _lines(stream):
    lines = stream.split(b"\n")
    return lines[:-1] if stream.endswith(b"\n") else lines


def _check_stream(stream):
    """What the stream is built for, asserted on the bytes themselves."""
    lines = _lines(stream)
    starts = np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])[:len(lines)]
    ends = starts + np.array([len(x) for x in lines])  # the '\n' positions (the stream's end for an unterminated line)
    span = lambda e: [(int(s), int(t)) for s, t in zip(starts, ends) if s < e <= t - 1]  # lines with bytes on both sides of e
    assert stream[0:1] == b"\n" and lines[0] == b""
    assert b"\n\n" in stream[1:-1]
    assert stream[B - 1:B] == b"\n" and (B - 1) % H == H - 1
    assert stream[3 * B:3 * B + 1] == b"\n" and stream[3 * B - 1:3 * B] != b"\n"
    assert span(2 * B) and all(t - s <= LMAX for s, t in span(2 * B))
    assert span(H) and all(s // B == (t) // B for s, t in span(H))  # crosses 2048, inside one 4 KiB block
    lens = sorted(len(x) for x in lines)
    assert lens[-2:] == [129, 300] and lens[-3] <= LMAX
    s300 = int(starts[[len(x) for x in lines].index(300)])
    assert B - 40 <= s300 % B < B and s300 + 300 > (s300 // B + 1) * B + MARGIN
    assert len(stream) % 16 != 0 and 4 * B < len(stream) < 5 * B
    assert stream.endswith(b"\n") == (stream is STREAM)
    return lines


_dev = {}


def _upload(ctx, name):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    if name not in _dev:
        _dev[name] = DeviceBuffer.from_array(ctx, np.frombuffer(VARIANTS[name] + b"\0" * 64, dtype=np.uint8))
    return _dev[name]


def _ref(algo, line):
    if algo == NTLM:
        from oracle import digest_oracle as dg
        return dg.ntlm(line)
    return {MD5: hashlib.md5, SHA1: hashlib.sha1, SHA512: hashlib.sha512}[algo](line).digest()


def _compare(got, algo, lines, long_is_zero):
    bad = []
    for i, ln in enumerate(lines):
        want = bytes(SIZE[algo]) if long_is_zero and len(ln) > LMAX else _ref(algo, ln)
        if bytes(got[i]) != want:
            bad.append((i, len(ln)))
    assert not bad, bad[:8]


@pytest.fixture
def _plain_after(gpu_ctx):
    yield
    gpu_ctx.clear_rules()
    gpu_ctx.set_targets(MD5, hashlib.md5(b"").digest())


VAR = pytest.mark.parametrize("variant", sorted(VARIANTS))


@VAR
@pytest.mark.parametrize("algo", [MD5, NTLM, SHA1, SHA512], ids=["md5", "ntlm", "sha1", "sha512"])
def test_plain_route(gpu_ctx, algo, variant):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    stream = VARIANTS[variant]
    lines = _check_stream(stream)
    buf, W = _upload(gpu_ctx, variant), SIZE[algo]
    dig = DeviceBuffer(gpu_ctx, W * len(lines) + 16)
    n = gpu_ctx.digest_lines_device(algo, buf.ptr, len(stream), dig.ptr, len(lines))
    assert n == len(lines)
    _compare(dig.to_array(count=W * n).reshape(n, W), algo, lines, False)


@VAR
@pytest.mark.parametrize("algo", [MD5, SHA1], ids=["md5", "sha1"])
def test_rules_route(gpu_ctx, _plain_after, algo, variant):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    stream = VARIANTS[variant]
    lines = _check_stream(stream)
    buf, W = _upload(gpu_ctx, variant), SIZE[algo]
    gpu_ctx.set_targets(MD5, hashlib.md5(b"").digest())
    assert gpu_ctx.set_rules(b":\n") == (1, 0)
    dig = DeviceBuffer(gpu_ctx, W * len(lines) + 16)
    n = gpu_ctx.digest_lines_rules_device(algo, buf.ptr, len(stream), dig.ptr, len(lines))
    assert n == len(lines)
    _compare(dig.to_array(count=W * n).reshape(n, W), algo, lines, True)
    assert gpu_ctx.rules_last() == (len(lines) - 2, 2)


@VAR
@pytest.mark.parametrize("order", [0, 1], ids=["pass.salt", "salt.pass"])
@pytest.mark.parametrize("algo", [MD5, SHA1], ids=["md5", "sha1"])
def test_salt_route(gpu_ctx, _plain_after, algo, order, variant):
    from hashcat_a5_table_generator_amd import DeviceBuffer
    stream = VARIANTS[variant]
    lines = _check_stream(stream)
    buf, W = _upload(gpu_ctx, variant), SIZE[algo]
    gpu_ctx.clear_rules()
    gpu_ctx.set_salted_targets(MD5, 0, hashlib.md5(b"").digest(), [b""])
    assert gpu_ctx.salt_count() == 1 and gpu_ctx.salt(0) == b""
    dig = DeviceBuffer(gpu_ctx, W * len(lines) + 16)
    n = gpu_ctx.digest_lines_salted_device(algo, order, buf.ptr, len(stream), dig.ptr, len(lines))
    assert n == len(lines)
    _compare(dig.to_array(count=W * n).reshape(n, W), algo, lines, True)
    assert gpu_ctx.salts_last() == (len(lines) - 2, 2)
