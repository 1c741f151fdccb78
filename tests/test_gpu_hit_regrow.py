"""The hit buffer's second run: one launch that finds more than 2^20 hits while the caller's
buffer is larger than that.  The device hit buffer starts at min(hit_cap, 2^20) entries, so
every digest route grows it and runs again only past that count -- the fused default route,
the fused -r route and the two-pass range loop (plain, wide, ruled, salted), the last with its
hit-tail and rule / salt side arrays.

An identity table makes every candidate of a word equal to the word, so the target set is the
one digest of the word and the truth is "every (word, cand) of the batch, exactly once": the
total and the per-word counts come from the keyspace, the comparison runs in numpy on the raw
hit buffer.

    table "a=a" x 3, word a*8,  default mode: 65 535 candidates   x 17 words = 1 114 095
    table "a=a",     word a*14, default mode: 16 383 candidates   x 65 words = 1 064 895
    table "a=a",     word a*14, -r:           16 384 candidates   x 65 words = 1 064 960
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HIT = np.dtype([("word", "<u8"), ("cand", "<u8"), ("digest", "u1", (16,))])  # a5x_hit
MD5, SHA1 = 0, 2
FLOOR = 1 << 20     # the device hit buffer's first size
CAP = 1 << 21       # 64 MiB of a5x_hit
E_CAPACITY = -8
GUARD = 0xDEADBEEF
WF_FAST = 1 << 5

TABLE3, WORD8, N8 = b"a=a\na=a\na=a\n", b"a" * 8, 17
TABLE1, WORD14, N14 = b"a=a\n", b"a" * 14, 65


class _Batch:
    """One context with the table loaded and n copies of the word staged on the device."""

    def __init__(self, table, word, n, mode=0):
        from hashcat_a5_table_generator_amd import Context, DeviceBuffer, pack_words
        self.word, self.n, self.mode = word, n, mode
        self.ctx = Context(0)
        self.ctx.parse_table(table)
        data, offs = pack_words([word] * n)
        self.cnt = self.ctx.keyspace(data, offs, mode, 0, 15)[0].astype(np.uint64)
        self.total = int(self.cnt.sum())
        self.dw, self.do = DeviceBuffer.from_array(self.ctx, data), DeviceBuffer.from_array(self.ctx, offs)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    def run(self, hit_cap, guard=0):
        """a5x_expand_digest_device into a numpy hit buffer -> (rc, n_hits, buffer)"""
        buf = np.zeros(hit_cap + guard, dtype=HIT)
        buf["word"][hit_cap:] = GUARD
        nh = ctypes.c_uint64()
        rc = self.ctx._L.a5x_expand_digest_device(self.ctx.h, self.dw.ptr, self.do.ptr, self.n, self.mode, 0, 15, 0,
                                                  buf.ctypes.data, hit_cap, ctypes.byref(nh), None, None)
        return rc, nh.value, buf

    def global_index(self, hits):
        """every hit valid; its index among the batch's candidates"""
        w, c = hits["word"], hits["cand"]
        assert (w < self.n).all()
        assert (c < self.cnt[w]).all()
        coff = np.concatenate([np.zeros(1, np.uint64), np.cumsum(self.cnt, dtype=np.uint64)])
        return coff[w] + c

    def check_all(self, rc, nh, buf, digest16=None):
        """every (word, cand) of the batch is a hit, exactly once"""
        assert rc == 0, self.ctx._L.a5x_last_error(self.ctx.h)
        assert nh == self.total
        hits = buf[:nh]
        g = np.sort(self.global_index(hits))
        assert np.array_equal(g, np.arange(self.total, dtype=np.uint64))
        assert np.array_equal(np.bincount(hits["word"].astype(np.int64), minlength=self.n).astype(np.uint64), self.cnt)
        if digest16 is not None:
            assert (hits["digest"] == np.frombuffer(digest16[:16], dtype=np.uint8)).all()


def _two_pass(fn):
    os.environ["A5X_NO_FUSED_DIGEST"] = "1"
    try:
        return fn()
    finally:
        os.environ.pop("A5X_NO_FUSED_DIGEST")


def _is_fast(ctx, word):
    info = np.zeros(4, dtype=np.uint64)
    wb = np.frombuffer(word + b"\0" * 16, dtype=np.uint8)
    assert ctx._L.a5x_debug_plan_word(ctx.h, wb.ctypes.data, len(word), 0, 15, None, 0, info.ctypes.data) == 0
    return bool(int(info[2]) & WF_FAST) and int(info[0]) > 0


def test_fused_default_md5():
    d = hashlib.md5(WORD8).digest()
    with _Batch(TABLE3, WORD8, N8) as b:
        assert _is_fast(b.ctx, WORD8)  # the fused kernel takes the words: no hybrid sub-batch
        assert b.total == N8 * 65535 > FLOOR
        b.ctx.set_targets(MD5, d)
        b.check_all(*b.run(CAP), digest16=d)
        # the caller's buffer between 2^20 and the hits: grown once to the cap, run again, full
        cap = FLOOR + 10
        rc, nh, buf = b.run(cap, guard=8)
        assert rc == E_CAPACITY
        assert nh == b.total
        assert (buf["word"][cap:] == GUARD).all() and (buf["cand"][cap:] == 0).all()
        assert len(np.unique(b.global_index(buf[:cap]))) == cap
        assert (buf["digest"][:cap] == np.frombuffer(d, dtype=np.uint8)).all()


def test_two_pass_plain_md5():
    d = hashlib.md5(WORD8).digest()
    with _Batch(TABLE3, WORD8, N8) as b:
        assert b.total > FLOOR
        b.ctx.set_targets(MD5, d)
        b.check_all(*_two_pass(lambda: b.run(CAP)), digest16=d)


def test_two_pass_sha1_wide():
    """the wide case: the per-hit tail words regrow with the hit buffer"""
    d = hashlib.sha1(WORD14).digest()
    with _Batch(TABLE1, WORD14, N14) as b:
        assert b.total == N14 * 16383 > FLOOR
        b.ctx.set_targets(SHA1, d)
        rc, nh, buf = _two_pass(lambda: b.run(CAP))
        b.check_all(rc, nh, buf, digest16=d)
        for h in (buf[0], buf[nh - 1]):
            assert b.ctx.hit_digest((h["word"], h["cand"], h["digest"].tobytes())) == d


def test_two_pass_one_rule():
    """the rule ':' alone: the per-hit rule array regrows with the hit buffer"""
    d = hashlib.md5(WORD8).digest()
    with _Batch(TABLE3, WORD8, N8) as b:
        assert b.total > FLOOR
        b.ctx.set_targets(MD5, d)
        assert b.ctx.set_rules([b":"]) == (1, 0)
        b.check_all(*b.run(CAP), digest16=d)
        n = ctypes.c_uint64()
        rules = np.full(b.total + 8, 0xFFFFFFFF, dtype=np.uint32)
        assert b.ctx._L.a5x_hit_rules(b.ctx.h, rules.ctypes.data, rules.size, ctypes.byref(n)) == 0
        assert n.value == b.total and not rules[:b.total].any()
        assert b.ctx.rules_last() == (b.total, 0)


def test_two_pass_one_salt():
    """a salted set of one salt: the per-hit salt array regrows with the hit buffer"""
    from hashcat_a5_table_generator_amd import ORDER_PASS_SALT
    salt = b"NaCl"
    with _Batch(TABLE3, WORD8, N8) as b:
        assert b.total > FLOOR
        b.ctx.set_salted_targets(MD5, ORDER_PASS_SALT, hashlib.md5(WORD8 + salt).digest(), [salt])
        b.check_all(*b.run(CAP))
        n = ctypes.c_uint64()
        salts = np.full(b.total + 8, 0xFFFFFFFF, dtype=np.uint32)
        assert b.ctx._L.a5x_hit_salts(b.ctx.h, salts.ctypes.data, salts.size, ctypes.byref(n)) == 0
        assert n.value == b.total and not salts[:b.total].any()
        assert b.ctx.salts_last() == (b.total, 0)


def test_fused_reverse_md5():
    d = hashlib.md5(WORD14).digest()
    with _Batch(TABLE1, WORD14, N14, mode=1) as b:
        assert b.total == N14 * 16384 > FLOOR
        b.ctx.set_targets(MD5, d)
        b.check_all(*b.run(CAP), digest16=d)
