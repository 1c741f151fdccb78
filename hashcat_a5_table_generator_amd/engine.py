"""Host-side mirror of the reference's operator interface, running on liba5x.

Reference functions (``/root/reference/main.go``) and their counterparts here:

=====================================  ==========================================
``readSubstitutionTable`` (108-144)    :func:`read_substitution_table`
``decodeHexNotation`` (147-162)        :func:`decode_hex_notation`
``-t`` merge loop (40-50)              :meth:`Context.load_tables`
``processWord`` (168-205)              :func:`process_word` / :meth:`Context.expand`
``processWordReverse`` (208-261)       :func:`process_word_reverse` (mode 1)
``processWordSubstituteAll`` (308)     :func:`process_word_substitute_all` (mode 2)
``...SubstituteAllReverse`` (369)      :func:`process_word_substitute_all_reverse`
word scanner (72-74)                   :func:`split_words`
channel + writer (58-68)               :meth:`Context.expand` sink / :func:`generate`
=====================================  ==========================================

Everything computes on the GPU through the C ABI (``include/a5x.h``); there is
no host fallback.
"""
from __future__ import annotations

import ctypes
import io
import os
import sys
from typing import BinaryIO, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import A5xError, Stats, check

MODE_DEFAULT = 0
MODE_REVERSE = 1
MODE_SUBALL = 2
MODE_SUBALL_REVERSE = 3
ALGO_MD5 = 0   # RFC 1321 (Go crypto/md5)
ALGO_NTLM = 1  # MD4 over UTF-16LE ([]rune + utf16.Encode)
ALGO_SHA1 = 2  # FIPS 180-4 over the candidate bytes (hashcat -m 100)
ALGO_SHA256 = 3  # FIPS 180-4 over the candidate bytes (hashcat -m 1400)
# (4 is unassigned)
ALGO_SHA224 = 5  # FIPS 180-4 over the candidate bytes (hashcat -m 1300)
ALGO_SHA384 = 6  # FIPS 180-4 over the candidate bytes (hashcat -m 10800)
ALGO_SHA512 = 7  # FIPS 180-4 over the candidate bytes (hashcat -m 1700)
# (8..15 are unassigned) nested: a digest of the lower-case (UP: upper-case) hex text of another
ALGO_MD5_MD5 = 16      # md5(hex(md5(p))) (hashcat -m 2600)
ALGO_MD5_MD5_MD5 = 17  # md5(hex(md5(hex(md5(p))))) (hashcat -m 3500)
ALGO_MD5_MD5UP = 18    # md5(HEX(md5(p))) (hashcat -m 4300)
ALGO_MD5_SHA1 = 19     # md5(hex(sha1(p))) (hashcat -m 4400)
ALGO_SHA1_SHA1 = 20    # sha1(hex(sha1(p))) (hashcat -m 4500)
ALGO_SHA1_MD5 = 21     # sha1(hex(md5(p))) (hashcat -m 4700)
ALGO_SHA256_MD5 = 22   # sha256(hex(md5(p))) (hashcat -m 20800)
# (23..31 are unassigned) salted nested: salted sets only, each with its own salt order (``salt_order``)
ALGO_MD5_MD5_SALT = 32     # md5(hex(md5(p)) + salt) (hashcat -m 2611 / 2711)
ALGO_MD5_SALT_MD5 = 33     # md5(salt + hex(md5(p))) (hashcat -m 3710)
ALGO_MD5_MD5_MD5SALT = 34  # md5(hex(md5(p)) + hex(md5(salt))) (hashcat -m 3910)
ALGO_MD5_MD5SALT_MD5 = 35  # md5(hex(md5(salt)) + hex(md5(p))) (hashcat -m 2811)
ALGO_SHA1_SHA1_SALT = 36   # sha1(hex(sha1(p)) + salt) (hashcat -m 4510)
ALGO_SHA1_SALT_SHA1 = 37   # sha1(salt + hex(sha1(p))) (hashcat -m 4520)
ALGO_SHA1_MD5_SALT = 38    # sha1(hex(md5(p)) + salt) (hashcat -m 4710)
# (39..47 are unassigned) HMAC (RFC 2104): salted sets only; key = pass has order 0, key = salt order 1 (``salt_order``)
ALGO_HMAC_MD5_KEY_PASS = 48     # HMAC-MD5(key = candidate, salt) (hashcat -m 50)
ALGO_HMAC_MD5_KEY_SALT = 49     # HMAC-MD5(key = salt, candidate) (hashcat -m 60)
ALGO_HMAC_SHA1_KEY_PASS = 50    # HMAC-SHA1(key = candidate, salt) (hashcat -m 150)
ALGO_HMAC_SHA1_KEY_SALT = 51    # HMAC-SHA1(key = salt, candidate) (hashcat -m 160)
ALGO_HMAC_SHA256_KEY_PASS = 52  # HMAC-SHA256(key = candidate, salt) (hashcat -m 1450)
ALGO_HMAC_SHA256_KEY_SALT = 53  # HMAC-SHA256(key = salt, candidate) (hashcat -m 1460)
ALGO_HMAC_SHA512_KEY_PASS = 54  # HMAC-SHA512(key = candidate, salt) (hashcat -m 1750)
ALGO_HMAC_SHA512_KEY_SALT = 55  # HMAC-SHA512(key = salt, candidate) (hashcat -m 1760)
# (56..71 are unassigned) PBKDF2 (RFC 8018) over HMAC, password = candidate: iterated sets only
# (``Context.set_iterated_targets``), matched on the first 16 bytes of the derived key
ALGO_PBKDF2_HMAC_MD5 = 72     # hashcat -m 11900
ALGO_PBKDF2_HMAC_SHA1 = 73    # hashcat -m 12000
ALGO_PBKDF2_HMAC_SHA256 = 74  # hashcat -m 10900
ALGO_PBKDF2_HMAC_SHA512 = 75  # hashcat -m 12100
ORDER_PASS_SALT = 0  # salted sets: hash(candidate + salt), hashcat -m 10 / 110 / 1310 / 1410 / 10810 / 1710
ORDER_SALT_PASS = 1  # hash(salt + candidate), hashcat -m 20 / 120 / 1320 / 1420 / 10820 / 1720

SubMap = Dict[bytes, List[bytes]]


def digest_size(algo: int) -> int:
    """Digest bytes of an algorithm (``a5x_digest_size``): 16, 16, 20, 32 for MD5, NTLM, SHA-1, SHA-256 and
    28, 48, 64 for SHA-224, SHA-384, SHA-512; the outer digest's 16, 20 or 32 for the nested algorithms; the
    hash's 16, 20, 32 or 64 for the HMAC algorithms."""
    n = _lib.load().a5x_digest_size(algo)
    if n < 0:
        raise A5xError(n, f"bad digest algorithm {algo}")
    return n


def salt_order(algo: int) -> int:
    """Where a salted nested algorithm (32..38) puts its salt (``a5x_algo_salt_order``): ``ORDER_PASS_SALT``
    for text + salt, ``ORDER_SALT_PASS`` for salt + text; an HMAC algorithm (48..55): ``ORDER_PASS_SALT`` for
    key = candidate, ``ORDER_SALT_PASS`` for key = salt -- the order its salted calls must be given."""
    o = _lib.load().a5x_algo_salt_order(algo)
    if o < 0:
        raise A5xError(o, f"digest algorithm {algo} has no salt order of its own")
    return o


def mode_of(substitute_all: bool, reverse_sub: bool) -> int:
    """The engine switch of ``main.go:80-92``."""
    return (MODE_SUBALL if substitute_all else MODE_DEFAULT) + (1 if reverse_sub else 0)


def pack_words(words: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """Contiguous word bytes + ``n+1`` u64 offsets (the batch layout of the ABI)."""
    offs = np.zeros(len(words) + 1, dtype=np.uint64)
    if len(words):
        offs[1:] = np.cumsum(np.fromiter((len(w) for w in words), dtype=np.uint64, count=len(words)))
    data = np.frombuffer(b"".join(words) + b"\0" * 16, dtype=np.uint8).copy()
    return data, offs


def split_words(data: bytes) -> Tuple[np.ndarray, np.ndarray]:
    """Dictionary bytes -> words exactly as ``bufio.Scanner`` yields them (``main.go:72-74``)."""
    L = _lib.load()
    n = ctypes.c_uint64()
    check(L.a5x_split_words(data, len(data), None, None, 0, ctypes.byref(n)))
    words = np.zeros(len(data) + 16, dtype=np.uint8)
    offs = np.zeros(n.value + 2, dtype=np.uint64)
    check(L.a5x_split_words(data, len(data), words.ctypes.data, offs.ctypes.data, offs.size, ctypes.byref(n)))
    return words, offs[: n.value + 1]


class Context:
    """One device context (``a5x_ctx``) with its merged substitution map."""

    def __init__(self, device: int = 0):
        self._L = _lib.load()
        h = ctypes.c_void_p()
        rc = self._L.a5x_create(device, ctypes.byref(h))
        if rc != 0:
            why = (self._L.a5x_create_error() or b"").decode(errors="replace")
            raise A5xError(rc, why or f"a5x_create(device={device}) failed")
        self.h = h
        self.device = device

    def close(self) -> None:
        if getattr(self, "h", None):
            self._L.a5x_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc: int) -> None:
        check(rc, self.h)

    @property
    def device_name(self) -> str:
        buf = ctypes.create_string_buffer(256)
        cu = ctypes.c_int()
        self._chk(self._L.a5x_device_info(self.h, buf, 256, ctypes.byref(cu)))
        return buf.value.decode()

    # ---- tables ------------------------------------------------------------
    def load_tables(self, paths: Iterable[str]) -> "Context":
        """``-t`` files merged in order (``main.go:40-50``)."""
        for p in paths:
            self._chk(self._L.a5x_load_table_file(self.h, os.fsencode(p)))
        return self

    def parse_table(self, data: bytes) -> "Context":
        self._chk(self._L.a5x_parse_table(self.h, data, len(data)))
        return self

    def set_table(self, sub: SubMap) -> "Context":
        keys = list(sub.keys())
        kb = b"".join(keys)
        koff = np.zeros(len(keys) + 1, dtype=np.uint64)
        koff[1:] = np.cumsum([len(k) for k in keys]) if keys else []
        vals, vkey = [], []
        for i, k in enumerate(keys):
            for v in sub[k]:
                vals.append(v)
                vkey.append(i)
        vb = b"".join(vals)
        voff = np.zeros(len(vals) + 1, dtype=np.uint64)
        if vals:
            voff[1:] = np.cumsum([len(v) for v in vals])
        vk = np.array(vkey, dtype=np.uint32)
        kbuf = np.frombuffer(kb + b"\0", dtype=np.uint8)
        vbuf = np.frombuffer(vb + b"\0", dtype=np.uint8)
        self._chk(self._L.a5x_set_table(self.h, kbuf.ctypes.data, koff.ctypes.data, len(keys), vbuf.ctypes.data,
                                        voff.ctypes.data, vk.ctypes.data if len(vk) else None, len(vals)))
        return self

    def clear_table(self) -> None:
        self._chk(self._L.a5x_clear_table(self.h))

    def table(self) -> SubMap:
        nk, nv, kb, vb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._L.a5x_table_export(self.h, ctypes.byref(nk), ctypes.byref(nv), ctypes.byref(kb),
                                           ctypes.byref(vb), None, None, None, None, None))
        ko = np.zeros(kb.value + 1, dtype=np.uint8)
        vo = np.zeros(vb.value + 1, dtype=np.uint8)
        koff = np.zeros(nk.value + 1, dtype=np.uint64)
        voff = np.zeros(nv.value + 1, dtype=np.uint64)
        vkey = np.zeros(max(nv.value, 1), dtype=np.uint32)
        self._chk(self._L.a5x_table_export(self.h, None, None, None, None, ko.ctypes.data, koff.ctypes.data,
                                           vo.ctypes.data, voff.ctypes.data, vkey.ctypes.data))
        kbytes, vbytes = ko.tobytes(), vo.tobytes()
        keys = [kbytes[koff[i]:koff[i + 1]] for i in range(nk.value)]
        out: SubMap = {k: [] for k in keys}
        for j in range(nv.value):
            out[keys[vkey[j]]].append(vbytes[voff[j]:voff[j + 1]])
        return out

    # ---- expansion (host buffers) -----------------------------------------
    def keyspace(self, words: np.ndarray, offs: np.ndarray, mode: int = MODE_DEFAULT, mn: int = 0,
                 mx: int = 15) -> Tuple[np.ndarray, np.ndarray]:
        n = len(offs) - 1
        cnt = np.zeros(max(n, 1), dtype=np.uint64)
        byt = np.zeros(max(n, 1), dtype=np.uint64)
        self._chk(self._L.a5x_keyspace(self.h, words.ctypes.data, offs.ctypes.data, n, mode, mn, mx,
                                       cnt.ctypes.data, byt.ctypes.data))
        return cnt[:n], byt[:n]

    def expand(self, words: np.ndarray, offs: np.ndarray, mode: int = MODE_DEFAULT, mn: int = 0, mx: int = 15,
               sink=None, cand_begin: int = 0, cand_end: Optional[int] = None) -> Tuple[bytes, dict]:
        """Expand a packed batch; returns the output bytes (words in order) unless a sink is given.
        cand_begin / cand_end: only the batch's candidates [cand_begin, cand_end) (a5x_expand_range)."""
        chunks: List[bytes] = []

        def _cb(_u, p, n):
            data = ctypes.string_at(p, n)
            if sink is not None:
                return 1 if sink(data) else 0
            chunks.append(data)
            return 0

        st = Stats()
        cb = _lib.SINK(_cb)
        ce = (1 << 64) - 1 if cand_end is None else cand_end
        self._chk(self._L.a5x_expand_range(self.h, words.ctypes.data, offs.ctypes.data, len(offs) - 1, mode, mn, mx,
                                           cand_begin, ce, cb, None, ctypes.byref(st)))
        return b"".join(chunks), st.as_dict()

    def expand_words(self, words: Sequence[bytes], mode: int = MODE_DEFAULT, mn: int = 0, mx: int = 15) -> List[List[bytes]]:
        """Per-word candidate lists (newline framing removed)."""
        data, offs = pack_words(words)
        cnt, byt = self.keyspace(data, offs, mode, mn, mx)
        out, _ = self.expand(data, offs, mode, mn, mx)
        res, pos = [], 0
        for i in range(len(words)):
            seg = out[pos:pos + int(byt[i])]
            pos += int(byt[i])
            res.append(_split_lines(seg, int(cnt[i])))
        return res

    # ---- device-resident ----------------------------------------------------
    def expand_device(self, d_words: int, d_offs: int, n_words: int, d_out: int, out_cap: int,
                      mode: int = MODE_DEFAULT, mn: int = 0, mx: int = 15, cand_begin: int = 0,
                      cand_end: int = (1 << 64) - 1, d_cand_off: int = 0, d_byte_off: int = 0,
                      stream: int = 0) -> dict:
        st = Stats()
        self._chk(self._L.a5x_expand_device(self.h, d_words, d_offs, n_words, mode, mn, mx, cand_begin, cand_end,
                                            d_out or None, out_cap, d_cand_off or None, d_byte_off or None,
                                            ctypes.byref(st), stream or None))
        return st.as_dict()

    # ---- fused digest + lookup ----------------------------------
    def set_targets(self, algo: int, digests) -> None:
        """Device target set from digests of ``digest_size(algo)`` bytes each (bytes of length
        size*n or an (n, size) uint8 array)."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(digests), dtype=np.uint8) if isinstance(digests, (bytes, bytearray))
                                   else np.asarray(digests, dtype=np.uint8)).reshape(-1)
        size = self._L.a5x_digest_size(algo)
        if size <= 0:  # (a5x_set_targets names the bad algorithm)
            size = 16
        if buf.size % size:
            raise ValueError(f"digests must be {size} bytes each")
        self._chk(self._L.a5x_set_targets(self.h, algo, buf.ctypes.data if buf.size else None, buf.size // size))
        self._algo_size = size

    def hit_digest(self, hit) -> bytes:
        """The full digest of a hit ``(word, cand, digest)`` against the current target set
        (``a5x_hit_digest``): for SHA-1 and the SHA-2 family the target that the hit's 16 digest bytes begin."""
        h = _lib.Hit()
        h.word, h.cand = int(hit[0]), int(hit[1])
        ctypes.memmove(h.digest, bytes(hit[2])[:16], 16)
        out = (ctypes.c_uint8 * 64)()
        n = ctypes.c_size_t()
        self._chk(self._L.a5x_hit_digest(self.h, ctypes.byref(h), out, 64, ctypes.byref(n)))
        return bytes(out[: n.value])

    def _hits(self, arr, n) -> List[Tuple[int, int, bytes]]:
        hits = [(int(h.word), int(h.cand), bytes(h.digest)) for h in arr[:n]]
        if getattr(self, "_algo_size", 16) > 16:  # the full-width digest (a5x_hit_digest)
            hits = [(w, c, self.hit_digest((w, c, d))) for w, c, d in hits]
        return hits

    def expand_digest(self, words: np.ndarray, offs: np.ndarray, mode: int = MODE_DEFAULT, mn: int = 0,
                      mx: int = 15, hit_cap: int = 1 << 16) -> Tuple[List[Tuple[int, int, bytes]], dict]:
        """Expand + hash + probe on the device; returns ([(word, cand_in_word, digest)], stats);
        digest at the algorithm's full width."""
        arr = (_lib.Hit * max(1, hit_cap))()
        nh = ctypes.c_uint64()
        st = Stats()
        self._chk(self._L.a5x_expand_digest(self.h, words.ctypes.data, offs.ctypes.data, len(offs) - 1, mode, mn, mx,
                                            arr, hit_cap, ctypes.byref(nh), ctypes.byref(st)))
        return self._hits(arr, min(nh.value, hit_cap)), st.as_dict()

    def expand_digest_device(self, d_words: int, d_offs: int, n_words: int, mode: int = MODE_DEFAULT, mn: int = 0,
                             mx: int = 15, scratch_bytes: int = 0, hit_cap: int = 1 << 16,
                             stream: int = 0, cand_begin: int = 0,
                             cand_end: Optional[int] = None) -> Tuple[List[Tuple[int, int, bytes]], dict]:
        """Fused expansion + digest + target lookup of the batch's candidates (all of them,
        or the global candidates [cand_begin, cand_end): a5x_expand_digest_range_device)."""
        # (one hit buffer per context, grown on demand: a fresh 1M-entry ctypes array costs
        # milliseconds of host zeroing per call)
        buf = getattr(self, "_hit_buf", None)
        if buf is None or len(buf) < max(1, hit_cap):
            buf = self._hit_buf = (_lib.Hit * max(1, hit_cap))()
        arr = buf
        nh = ctypes.c_uint64()
        st = Stats()
        if cand_begin == 0 and cand_end is None:
            self._chk(self._L.a5x_expand_digest_device(self.h, d_words, d_offs, n_words, mode, mn, mx, scratch_bytes,
                                                       arr, hit_cap, ctypes.byref(nh), ctypes.byref(st),
                                                       stream or None))
        else:
            self._chk(self._L.a5x_expand_digest_range_device(
                self.h, d_words, d_offs, n_words, mode, mn, mx, cand_begin, (1 << 64) - 1 if cand_end is None else cand_end,
                scratch_bytes, arr, hit_cap, ctypes.byref(nh), ctypes.byref(st), stream or None))
        return self._hits(arr, min(nh.value, hit_cap)), st.as_dict()

    # ---- rules in the digest + lookup stage (a5x_rules.hip) ------------------------
    def set_rules(self, text_or_lines) -> Tuple[int, int]:
        """Replace the rule set from rule-file text (bytes / str) or a sequence of rule lines;
        returns (accepted, skipped).  While >= 1 rule is loaded every expand_digest* call
        hashes each candidate once per rule; ``last_hit_rules()`` names each hit's rule."""
        if isinstance(text_or_lines, str):
            text = text_or_lines.encode()
        elif isinstance(text_or_lines, (bytes, bytearray)):
            text = bytes(text_or_lines)
        else:
            text = b"".join((l.encode() if isinstance(l, str) else bytes(l)) + b"\n" for l in text_or_lines)
        n, sk = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(self._L.a5x_set_rules(self.h, text, len(text), ctypes.byref(n), ctypes.byref(sk)))
        return n.value, sk.value

    def load_rules_file(self, path: str) -> Tuple[int, int]:
        n, sk = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(self._L.a5x_load_rules_file(self.h, os.fsencode(path), ctypes.byref(n), ctypes.byref(sk)))
        return n.value, sk.value

    def clear_rules(self) -> None:
        self._chk(self._L.a5x_set_rules(self.h, None, 0, None, None))

    def rule_count(self) -> int:
        return self._L.a5x_rule_count(self.h)

    def last_hit_rules(self) -> List[int]:
        """Rule index of each hit the latest expand_digest* call returned, in hit order."""
        n = ctypes.c_uint64()
        self._chk(self._L.a5x_hit_rules(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.uint32)
        self._chk(self._L.a5x_hit_rules(self.h, out.ctypes.data, out.size, ctypes.byref(n)))
        return [int(x) for x in out[: n.value]]

    def rules_last(self) -> Tuple[int, int]:
        """(hashes computed, candidates rejected as longer than 128 bytes) of the latest ruled call."""
        h, r = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._L.a5x_rules_last(self.h, ctypes.byref(h), ctypes.byref(r)))
        return h.value, r.value

    def digest_lines_rules_device(self, algo: int, d_lines: int, nbytes: int, d_digests: int, cap: int,
                                  stream: int = 0) -> int:
        """Digest of every (line, rule) of a device "cand\\n" stream under the loaded rules, at
        index line * R + rule (cap counts digests; a line over 128 bytes gives R zero digests);
        returns the line count."""
        n = ctypes.c_uint64()
        self._chk(self._L.a5x_digest_lines_rules_device(self.h, algo, d_lines, nbytes, d_digests or None, cap,
                                                        ctypes.byref(n), stream or None))
        return n.value

    # ---- salted target lists (a5x_salt.hip) ----------------------------------------
    def set_salted_targets(self, algo: int, order: int, digests, salts: Sequence[bytes]) -> None:
        """Salted target set: digest i (``digest_size(algo)`` bytes each, bytes or an (n, size)
        uint8 array) registered with ``salts[i]`` (at most 64 bytes).  order ``ORDER_PASS_SALT``:
        hash(candidate + salt); ``ORDER_SALT_PASS``: hash(salt + candidate).  While the set is
        salted every expand_digest* call hashes each candidate once per distinct salt;
        ``last_hit_salts()`` names each hit's salt."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(digests), dtype=np.uint8) if isinstance(digests, (bytes, bytearray))
                                   else np.asarray(digests, dtype=np.uint8)).reshape(-1)
        size = self._L.a5x_digest_size(algo)
        if size <= 0:  # (a5x_set_salted_targets names the bad algorithm)
            size = 16
        salts = [bytes(s) for s in salts]
        if buf.size % size or buf.size // size != len(salts):
            raise ValueError(f"digests must be {size} bytes each, one salt per digest")
        sb = np.frombuffer(b"".join(salts) + b"\0", dtype=np.uint8)
        so = np.zeros(len(salts) + 1, dtype=np.uint64)
        if salts:
            so[1:] = np.cumsum([len(s) for s in salts])
        self._chk(self._L.a5x_set_salted_targets(self.h, algo, order, buf.ctypes.data if buf.size else None, len(salts),
                                                 sb.ctypes.data, so.ctypes.data))
        self._algo_size = size

    def load_salted_hashes(self, algo: int, order: int, text: bytes, hex_salt: bool = False) -> Tuple[int, int, int]:
        """Salted target set from the text of a ``hexdigest:salt`` file; returns (targets, distinct
        salts, lines skipped)."""
        text = text.encode() if isinstance(text, str) else bytes(text)
        nt, ns, sk = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._L.a5x_load_salted_hashes(self.h, algo, order, text, len(text), 1 if hex_salt else 0,
                                                 ctypes.byref(nt), ctypes.byref(ns), ctypes.byref(sk)))
        self._algo_size = max(16, self._L.a5x_digest_size(algo))
        return nt.value, ns.value, sk.value

    # ---- iterated target lists (a5x_pbkdf2.hip) ------------------------------------
    def set_iterated_targets(self, algo: int, digests16, salts: Sequence[bytes], iters: Sequence[int]) -> None:
        """Iterated target set (``ALGO_PBKDF2_HMAC_*``): target i is the first 16 bytes of the PBKDF2 key
        under ``salts[i]`` (at most 64 bytes) and ``iters[i]`` >= 1 iterations.  Distinct (salt, iterations)
        pairs are indexed by first appearance: ``salt_count()``, ``salt()``, ``salt_iterations()`` and
        ``last_hit_salts()`` speak of that index."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(digests16), dtype=np.uint8) if isinstance(digests16, (bytes, bytearray))
                                   else np.asarray(digests16, dtype=np.uint8)).reshape(-1)
        salts = [bytes(s) for s in salts]
        if buf.size % 16 or buf.size // 16 != len(salts) or len(iters) != len(salts):
            raise ValueError("digests must be 16 bytes each, one salt and one iteration count per digest")
        sb = np.frombuffer(b"".join(salts) + b"\0", dtype=np.uint8)
        so = np.zeros(len(salts) + 1, dtype=np.uint64)
        if salts:
            so[1:] = np.cumsum([len(s) for s in salts])
        it = np.ascontiguousarray(list(iters) + [0], dtype=np.uint32)
        self._chk(self._L.a5x_set_iterated_targets(self.h, algo, buf.ctypes.data if buf.size else None, len(salts),
                                                   sb.ctypes.data, so.ctypes.data, it.ctypes.data))
        self._algo_size = 16

    def load_pbkdf2_hashes(self, algo: int, text: bytes) -> Tuple[int, int, int]:
        """Iterated target set from hashcat's ``name:iterations:base64(salt):base64(dk)`` lines; returns
        (targets, distinct (salt, iterations) pairs, lines skipped)."""
        text = text.encode() if isinstance(text, str) else bytes(text)
        nt, ns, sk = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._L.a5x_load_pbkdf2_hashes(self.h, algo, text, len(text), ctypes.byref(nt), ctypes.byref(ns),
                                                 ctypes.byref(sk)))
        self._algo_size = 16
        return nt.value, ns.value, sk.value

    def salt_iterations(self, index: int) -> int:
        """Iteration count of index ``index`` of an iterated set (beside ``salt()``)."""
        n = ctypes.c_uint32()
        self._chk(self._L.a5x_salt_iterations(self.h, index, ctypes.byref(n)))
        return n.value

    def iter_budget(self, pair_slots: int = 0, pair_iterations: int = 0) -> int:
        """Test hook (``a5x_debug_iter_budget``): pair slots per pass and pair-iterations per loop launch of
        the iterated route from now on (0: the default); returns the loop launches of the latest call."""
        n = ctypes.c_uint64()
        self._chk(self._L.a5x_debug_iter_budget(self.h, pair_slots, pair_iterations, ctypes.byref(n)))
        return n.value

    def format_hits_iterated(self, words: np.ndarray, offs: np.ndarray, hits, salts, mode: int = MODE_DEFAULT,
                             mn: int = 0, mx: int = 15) -> Tuple[bytes, int]:
        """``original-line:plain\\n`` for hits against an iterated set (a5x_format_hits_iterated): every hit's
        whole key is derived again on the host and compared with all the list gave; returns (text, hits
        dropped because only their first 16 bytes matched)."""
        arr = (_lib.Hit * max(1, len(hits)))()
        for k, (w, c, d) in enumerate(hits):
            arr[k].word, arr[k].cand = int(w), int(c)
            ctypes.memmove(arr[k].digest, bytes(d)[:16], 16)
        sa = np.ascontiguousarray(salts, dtype=np.uint32)
        if sa.size != len(hits):
            raise ValueError("one salt index per hit")
        chunks: List[bytes] = []

        def _cb(_u, p, n):
            chunks.append(ctypes.string_at(p, n))
            return 0

        cb = _lib.SINK(_cb)
        dropped = ctypes.c_uint64()
        self._chk(self._L.a5x_format_hits_iterated(self.h, words.ctypes.data, offs.ctypes.data, len(offs) - 1, mode, mn,
                                                   mx, arr, len(hits), sa.ctypes.data if sa.size else None,
                                                   ctypes.byref(dropped), cb, None))
        return b"".join(chunks), dropped.value

    def salt_count(self) -> int:
        """Distinct salts of the current target set (0: not salted)."""
        return self._L.a5x_salt_count(self.h)

    def salt(self, index: int) -> bytes:
        out = (ctypes.c_uint8 * 64)()
        n = ctypes.c_size_t()
        self._chk(self._L.a5x_salt_get(self.h, index, out, 64, ctypes.byref(n)))
        return bytes(out[: n.value])

    def last_hit_salts(self) -> List[int]:
        """Salt index of each hit the latest expand_digest* call returned, in hit order."""
        n = ctypes.c_uint64()
        self._chk(self._L.a5x_hit_salts(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.uint32)
        self._chk(self._L.a5x_hit_salts(self.h, out.ctypes.data, out.size, ctypes.byref(n)))
        return [int(x) for x in out[: n.value]]

    def salts_last(self) -> Tuple[int, int]:
        """((candidate, salt) pairs hashed, pairs skipped as longer than 128 bytes) of the latest salted call."""
        h, s = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._L.a5x_salts_last(self.h, ctypes.byref(h), ctypes.byref(s)))
        return h.value, s.value

    def digest_lines_salted_device(self, algo: int, order: int, d_lines: int, nbytes: int, d_digests: int, cap: int,
                                   stream: int = 0) -> int:
        """Digest of every (line, salt) of a device "cand\\n" stream under the salts of the current
        set, at index line * S + salt (cap counts digests; a pair over 128 bytes gives a zero
        digest); returns the line count."""
        n = ctypes.c_uint64()
        self._chk(self._L.a5x_digest_lines_salted_device(self.h, algo, order, d_lines, nbytes, d_digests or None, cap,
                                                         ctypes.byref(n), stream or None))
        return n.value

    def format_hits_salted(self, words: np.ndarray, offs: np.ndarray, hits, salts, mode: int = MODE_DEFAULT,
                           mn: int = 0, mx: int = 15, hex_salt: bool = False) -> bytes:
        """hashcat "hexdigest:salt:plain\\n" lines for hits of this batch against a salted set
        (a5x_format_hits_salted); salts: each hit's salt index (``last_hit_salts()``)."""
        arr = (_lib.Hit * max(1, len(hits)))()
        for k, (w, c, d) in enumerate(hits):
            arr[k].word, arr[k].cand = int(w), int(c)
            ctypes.memmove(arr[k].digest, bytes(d)[:16], 16)
        sa = np.ascontiguousarray(salts, dtype=np.uint32)
        if sa.size != len(hits):
            raise ValueError("one salt index per hit")
        chunks: List[bytes] = []

        def _cb(_u, p, n):
            chunks.append(ctypes.string_at(p, n))
            return 0

        cb = _lib.SINK(_cb)
        self._chk(self._L.a5x_format_hits_salted(self.h, words.ctypes.data, offs.ctypes.data, len(offs) - 1, mode, mn,
                                                 mx, arr, len(hits), sa.ctypes.data if sa.size else None,
                                                 1 if hex_salt else 0, cb, None))
        return b"".join(chunks)

    def format_hits(self, words: np.ndarray, offs: np.ndarray, hits, mode: int = MODE_DEFAULT, mn: int = 0,
                    mx: int = 15, rules=None) -> bytes:
        """hashcat "hexdigest:plain\\n" lines for hits [(word, cand, digest)] of this batch
        (a5x_format_hits; plains in $HEX[] form when hashcat's outfile would hexify them).
        digest: the full digest or its first 16 bytes (the library prints the full width).
        rules: each hit's rule index (``last_hit_rules()``): the plain printed is the ruled one."""
        arr = (_lib.Hit * max(1, len(hits)))()
        for k, (w, c, d) in enumerate(hits):
            arr[k].word, arr[k].cand = int(w), int(c)
            ctypes.memmove(arr[k].digest, bytes(d)[:16], 16)
        chunks: List[bytes] = []

        def _cb(_u, p, n):
            chunks.append(ctypes.string_at(p, n))
            return 0

        cb = _lib.SINK(_cb)
        if rules is not None:
            ra = np.ascontiguousarray(rules, dtype=np.uint32)
            if ra.size != len(hits):
                raise ValueError("one rule index per hit")
            self._chk(self._L.a5x_format_hits_rules(self.h, words.ctypes.data, offs.ctypes.data, len(offs) - 1, mode,
                                                    mn, mx, arr, len(hits), ra.ctypes.data if ra.size else None, cb,
                                                    None))
            return b"".join(chunks)
        self._chk(self._L.a5x_format_hits(self.h, words.ctypes.data, offs.ctypes.data, len(offs) - 1, mode, mn, mx,
                                          arr, len(hits), cb, None))
        return b"".join(chunks)

    def digest_lines_device(self, algo: int, d_lines: int, nbytes: int, d_digests: int, cap: int,
                            stream: int = 0) -> int:
        """Digest of every line of a device "cand\n" stream, ``digest_size(algo)`` bytes per line
        in line order (cap counts lines); returns the line count."""
        n = ctypes.c_uint64()
        self._chk(self._L.a5x_digest_lines_device(self.h, algo, d_lines, nbytes, d_digests or None, cap,
                                                  ctypes.byref(n), stream or None))
        return n.value

    def keyspace_device(self, d_words: int, d_offs: int, n_words: int, mode: int = MODE_DEFAULT, mn: int = 0,
                        mx: int = 15, d_cand_off: int = 0, d_byte_off: int = 0, stream: int = 0) -> Tuple[int, int]:
        tc, tb = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._L.a5x_keyspace_device(self.h, d_words, d_offs, n_words, mode, mn, mx, d_cand_off or None,
                                              d_byte_off or None, ctypes.byref(tc), ctypes.byref(tb),
                                              stream or None))
        return tc.value, tb.value

    def keyspace_refit(self) -> int:
        """Words of the last keyspace pass that ``k_keyspace_thread`` walked with the fused
        position-synchronous walk because its unit log did not hold them
        (``a5x_debug_keyspace_refit``; a test hook)."""
        n = ctypes.c_uint64()
        self._chk(self._L.a5x_debug_keyspace_refit(self.h, ctypes.byref(n)))
        return n.value

    def cut_once(self, word: bytes) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(out, rec_new, rec_ref) of ``a5x_debug_cut_once`` for one word of <= 127 bytes, on the
        host (``Context(-1)`` will do): the count pass of ``k_keyspace_thread`` that keeps its
        cuts and the record built from them, against the planners it replaces (a test hook;
        the fields of ``out`` are listed in ``include/a5x.h``)."""
        word = bytes(word)
        wb = np.frombuffer(word + b"\0", dtype=np.uint8)
        out = np.zeros(_lib.CUT_ONCE_OUT, dtype=np.uint32)
        rn = np.zeros(_lib.CUT_ONCE_REC, dtype=np.uint64)
        rr = np.zeros(_lib.CUT_ONCE_REC, dtype=np.uint64)
        self._chk(self._L.a5x_debug_cut_once(self.h, wb.ctypes.data, len(word), out.ctypes.data, rn.ctypes.data,
                                             rr.ctypes.data))
        return out, rn, rr

    def keyspace_cplx_lean(self) -> Tuple[int, int]:
        """(lean, generic): the words of the last keyspace pass that ``k_keyspace_cplx`` took by
        its lean path and by its generic unit walk (``a5x_debug_keyspace_cplx_lean``; a test hook)."""
        n = (ctypes.c_uint64 * 2)()
        self._chk(self._L.a5x_debug_keyspace_cplx_lean(self.h, n))
        return n[0], n[1]

    def keyspace_small_stage(self) -> int:
        """The small word stage of ``k_keyspace_thread`` for the loaded table in bytes, 0 when
        the table leaves no room for one (``a5x_debug_keyspace_small_stage``; a test hook)."""
        n = ctypes.c_uint32()
        self._chk(self._L.a5x_debug_keyspace_small_stage(self.h, ctypes.byref(n)))
        return n.value

    def keyspace_stage(self) -> int:
        """The word stage in bytes that the last keyspace pass used
        (``a5x_debug_keyspace_stage``; a test hook)."""
        n = ctypes.c_uint32()
        self._chk(self._L.a5x_debug_keyspace_stage(self.h, ctypes.byref(n)))
        return n.value

    def keyspace_large_stage(self, on: bool = True) -> None:
        """Stop (or resume) offering the small word stage on this context
        (``a5x_debug_keyspace_large_stage``; tests and A/B runs)."""
        self._chk(self._L.a5x_debug_keyspace_large_stage(self.h, 1 if on else 0))

    def word_flags(self, n: int) -> np.ndarray:
        """The per-word class flags (``A5X_WF_*``) the last keyspace pass left on the device, for
        its first ``n`` words; after a refused batch the refused words carry their ``ERR`` bits
        (``a5x_debug_word_flags``; a test hook)."""
        out = np.zeros(max(1, n), dtype=np.uint32)
        self._chk(self._L.a5x_debug_word_flags(self.h, out.ctypes.data, n))
        return out[:n]

    def locate_device(self, d_words: int, d_offs: int, n_words: int, cands, mode: int = MODE_DEFAULT, mn: int = 0,
                      mx: int = 15, stream: int = 0) -> np.ndarray:
        """Output byte offsets of global candidate indices (``a5x_locate_device``)."""
        q = np.ascontiguousarray(cands, dtype=np.uint64)
        out = np.zeros(max(1, q.size), dtype=np.uint64)
        self._chk(self._L.a5x_locate_device(self.h, d_words, d_offs, n_words, mode, mn, mx,
                                            q.ctypes.data if q.size else None, q.size, out.ctypes.data,
                                            stream or None))
        return out[: q.size]

    def split_device(self, d_words: int, d_offs: int, n_words: int, byte_targets, mode: int = MODE_DEFAULT,
                     mn: int = 0, mx: int = 15, stream: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(global candidate, word, candidate in word) of the first candidate starting at or
        after each byte target (``a5x_split_device``: intra-word split points)."""
        t = np.ascontiguousarray(byte_targets, dtype=np.uint64)
        g, w, c = (np.zeros(max(1, t.size), dtype=np.uint64) for _ in range(3))
        self._chk(self._L.a5x_split_device(self.h, d_words, d_offs, n_words, mode, mn, mx,
                                           t.ctypes.data if t.size else None, t.size, g.ctypes.data, w.ctypes.data,
                                           c.ctypes.data, stream or None))
        return g[: t.size], w[: t.size], c[: t.size]

    def digest_device(self, d_out: int, d_byte_off: int, out_base: int, n_words: int, d_digest: int,
                      stream: int = 0) -> None:
        self._chk(self._L.a5x_digest_device(self.h, d_out, d_byte_off, out_base, n_words, d_digest,
                                            stream or None))


def _split_lines(seg: bytes, count: int) -> List[bytes]:
    if not seg:
        return []
    parts = seg.split(b"\n")
    assert parts[-1] == b""
    parts = parts[:-1]
    return parts


def format_plain(plain: bytes) -> bytes:
    """The plain as a hashcat outfile line writes it (``a5x_format_plain``)."""
    L = _lib.load()
    n = ctypes.c_size_t()
    check(L.a5x_format_plain(plain, len(plain), None, 0, ctypes.byref(n)))
    out = ctypes.create_string_buffer(max(1, n.value))
    check(L.a5x_format_plain(plain, len(plain), out, n.value, ctypes.byref(n)))
    return out.raw[:n.value]


def apply_rule(rule: bytes, word: bytes) -> bytes:
    """One rule line applied to word on the host by the interpreter the rules kernel runs
    (``a5x_debug_apply_rule``); ValueError for a line ``set_rules`` would skip."""
    rule = rule.encode() if isinstance(rule, str) else bytes(rule)
    word = bytes(word)
    L = _lib.load()
    out = (ctypes.c_uint8 * 136)()
    n = ctypes.c_size_t()
    rc = L.a5x_debug_apply_rule(rule, len(rule), word, len(word), out, 136, ctypes.byref(n))
    if rc == -1:
        raise ValueError(f"unsupported or malformed rule {rule!r} (or a word over 128 bytes)")
    check(rc)
    return bytes(out[: n.value])


def debug_digest_salted(algo: int, order: int, salt: bytes, msg: bytes) -> bytes:
    """hash(msg + salt) (order 0) or hash(salt + msg) (order 1) on the host by the message
    assembly and digest cores the salt kernel runs (``a5x_debug_digest_salted``); A5xError
    (A5X_E_UNSUPPORTED) for a pair the kernel skips: more than 128 message bytes.  For an HMAC
    algorithm (48..55) ``msg`` is the candidate: the key with order 0, the message with order 1."""
    salt, msg = bytes(salt), bytes(msg)
    out = (ctypes.c_uint8 * 64)()
    check(_lib.load().a5x_debug_digest_salted(algo, order, salt, len(salt), msg, len(msg), out, 64))
    return bytes(out[: digest_size(algo)])


def debug_pbkdf2(algo: int, password: bytes, salt: bytes, iters: int, dklen: int) -> bytes:
    """``dklen`` bytes of the PBKDF2 key of an ``ALGO_PBKDF2_HMAC_*`` on the host, by the code the iterated
    kernels run (``a5x_debug_pbkdf2``); A5xError (A5X_E_UNSUPPORTED) for a password over 128 bytes."""
    password, salt = bytes(password), bytes(salt)
    out = (ctypes.c_uint8 * max(1, dklen))()
    check(_lib.load().a5x_debug_pbkdf2(algo, password, len(password), salt, len(salt), iters, out, dklen))
    return bytes(out[:dklen])


def partition(prefix: np.ndarray, parts: int) -> np.ndarray:
    """Balanced split points over a prefix array (``a5x_partition``)."""
    L = _lib.load()
    prefix = np.ascontiguousarray(prefix, dtype=np.uint64)
    split = np.zeros(parts + 1, dtype=np.uint64)
    check(L.a5x_partition(prefix.ctypes.data, len(prefix) - 1, parts, split.ctypes.data))
    return split


# ---------------------------------------------------------------------------
# function-level mirror of main.go
# ---------------------------------------------------------------------------
_default_ctx: Optional[Context] = None


def _ctx() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("A5X_DEVICE", "0")))
    return _default_ctx


def read_substitution_table(path: str) -> SubMap:
    """``readSubstitutionTable`` (``main.go:108-144``) via the library's Go-exact parser
    (a private host-only context: the shared default context's table is left alone)."""
    with Context(-1) as c:
        c.load_tables([path])
        return c.table()


def decode_hex_notation(value: bytes) -> bytes:
    """``decodeHexNotation`` (``main.go:147-162``); raises ``ValueError`` like the Go error.
    Parsed in a private host-only context (no GPU, the default context untouched)."""
    if len(value) < 7 or not value.startswith(b"$HEX[") or not value.endswith(b"]"):
        return value
    with Context(-1) as c:
        c.parse_table(b"k=" + value + b"\n")
        t = c.table()
    if b"k" not in t:
        raise ValueError(f"invalid hex string {value[5:-1]!r}")
    return t[b"k"][0]


def _engine(word: bytes, sub_map: SubMap, mn: int, mx: int, mode: int) -> List[bytes]:
    c = _ctx()
    c.set_table(sub_map)
    return c.expand_words([word], mode, mn, mx)[0]


def process_word(word: bytes, sub_map: SubMap, min_substitute: int, max_substitute: int) -> List[bytes]:
    """``processWord`` (``main.go:168``): the candidates the reference sends on ``out``."""
    return _engine(word, sub_map, min_substitute, max_substitute, MODE_DEFAULT)


def process_word_reverse(word: bytes, sub_map: SubMap, min_substitute: int, max_substitute: int) -> List[bytes]:
    """``processWordReverse`` (``main.go:208``)."""
    return _engine(word, sub_map, min_substitute, max_substitute, MODE_REVERSE)


def process_word_substitute_all(word: bytes, sub_map: SubMap, min_substitute: int, max_substitute: int) -> List[bytes]:
    """``processWordSubstituteAll`` (``main.go:308``)."""
    return _engine(word, sub_map, min_substitute, max_substitute, MODE_SUBALL)


def process_word_substitute_all_reverse(word: bytes, sub_map: SubMap, min_substitute: int,
                                        max_substitute: int) -> List[bytes]:
    """``processWordSubstituteAllReverse`` (``main.go:369``)."""
    return _engine(word, sub_map, min_substitute, max_substitute, MODE_SUBALL_REVERSE)


MAX_SCAN_TOKEN = 64 * 1024  # bufio.MaxScanTokenSize


def iter_word_batches(f: BinaryIO, batch_words: int = 1 << 22,
                      chunk: int = 64 << 20) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
    """The dictionary stream of ``main.go:52-56,72-74`` in bounded memory: ScanLines over
    ``chunk``-byte reads (LF split, one trailing CR dropped, a final unterminated line
    kept, and the first line with no newline in 64 KiB silently ends the input: the
    reference never checks ``scanner.Err()``).  Yields packed batches of at most
    ``batch_words`` words (``split_words`` layout)."""
    pend_w: List[np.ndarray] = []
    pend_o: List[np.ndarray] = []
    npend = 0

    def flush_pending():
        nonlocal pend_w, pend_o, npend
        lens = np.concatenate([np.diff(o.astype(np.int64)) for o in pend_o])
        body = np.concatenate([w[: int(o[-1])] for w, o in zip(pend_w, pend_o)])
        offs = np.zeros(len(lens) + 1, dtype=np.uint64)
        np.cumsum(lens, out=offs[1:])
        data = np.zeros(len(body) + 16, dtype=np.uint8)
        data[: len(body)] = body
        pend_w, pend_o, npend = [], [], 0
        return data, offs

    def take(words, offs):
        # split (words, offs) into the pending batch, yielding every full batch
        nonlocal npend
        n = len(offs) - 1
        i = 0
        while i < n:
            k = min(n - i, batch_words - npend)
            sub_o = (offs[i:i + k + 1] - offs[i]).astype(np.uint64)
            pend_w.append(words[int(offs[i]):int(offs[i + k])])
            pend_o.append(sub_o)
            npend += k
            i += k
            if npend == batch_words:
                yield flush_pending()

    rest = b""
    while True:
        block = f.read(chunk)
        eof = not block
        buf = rest + block
        if eof:
            part, rest = buf, b""
        else:
            cut = buf.rfind(b"\n") + 1
            part, rest = buf[:cut], buf[cut:]
        if part:
            words, offs = split_words(part)
            yield from take(words, offs)
            complete = part.count(b"\n") + (0 if part.endswith(b"\n") else 1)
            if len(offs) - 1 < complete:  # ErrTooLong inside this part: the input ends here
                break
        if eof:
            break
        if len(rest) >= MAX_SCAN_TOKEN:  # no newline in 64 KiB: ErrTooLong
            break
    if npend:
        yield flush_pending()


def generate(dict_file: str, table_files: Sequence[str], table_min: int = 0, table_max: int = 15,
             substitute_all: bool = False, reverse_sub: bool = False, out: Optional[BinaryIO] = None,
             device: int = 0, batch_words: int = 1 << 22, chunk: int = 64 << 20) -> int:
    """The whole ``main()`` (``main.go:28-100``): dict -> candidates on ``out``; returns
    candidates.  The dictionary is streamed (``iter_word_batches``): memory is bounded by
    one chunk and one batch, whatever the file size."""
    out = out if out is not None else sys.stdout.buffer
    mode = mode_of(substitute_all, reverse_sub)
    with Context(device) as c:
        c.load_tables(table_files)
        total = 0
        with open(dict_file, "rb") as f:
            for sub_words, sub_off in iter_word_batches(f, batch_words, chunk):
                _, st = c.expand(sub_words, sub_off, mode, table_min, table_max, sink=lambda d: out.write(d) and 0)
                total += st["candidates"]
        out.flush()
        return total


class DeviceBuffer:
    """A raw HBM allocation owned by a :class:`Context` (``a5x_dev_alloc``)."""

    def __init__(self, ctx: Context, nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        ctx._chk(ctx._L.a5x_dev_alloc(ctx.h, ctypes.byref(p), max(self.nbytes, 16)))
        self.ptr = p.value

    @classmethod
    def from_array(cls, ctx: Context, arr: np.ndarray) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        b = cls(ctx, arr.nbytes)
        if arr.nbytes:
            ctx._chk(ctx._L.a5x_memcpy_h2d(ctx.h, b.ptr, arr.ctypes.data, arr.nbytes))
        return b

    def to_array(self, dtype=np.uint8, count: Optional[int] = None, offset: int = 0) -> np.ndarray:
        itemsize = np.dtype(dtype).itemsize
        n = (self.nbytes - offset) // itemsize if count is None else int(count)
        out = np.empty(n, dtype=dtype)
        if n:
            self.ctx._chk(self.ctx._L.a5x_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr + offset, n * itemsize))
        return out

    def free(self) -> None:
        if self.ptr:
            self.ctx._L.a5x_dev_free(self.ctx.h, self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            if getattr(self.ctx, "h", None):
                self.free()
        except Exception:
            pass
