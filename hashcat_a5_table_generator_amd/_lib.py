"""ctypes binding of liba5x.so (include/a5x.h).

The product path has no CPU fallback: if the in-tree HIP library is missing or a
GPU is absent, calls raise :class:`A5xError` instead of computing anything on
the host.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("A5X_LIB_PATH") or os.path.join(_PKG, "_build", "liba5x.so")

A5X_OK = 0
ERRORS = {
    -1: "A5X_E_ARG", -2: "A5X_E_HIP", -3: "A5X_E_NOMEM", -4: "A5X_E_IO", -5: "A5X_E_TOOLONG",
    -6: "A5X_E_BOUNDS", -7: "A5X_E_OVERFLOW", -8: "A5X_E_CAPACITY", -9: "A5X_E_UNSUPPORTED",
    -10: "A5X_E_NOTABLE", -11: "A5X_E_SINK",
}
E_CAPACITY = -8
CUT_ONCE_OUT, CUT_ONCE_REC = 29, 1297  # A5X_CUT_ONCE_OUT / A5X_CUT_ONCE_REC (a5x_debug_cut_once)

# the exported symbols of include/a5x.h (checked by tests/test_abi.py)
EXPORTS = (
    "a5x_abi_version", "a5x_create", "a5x_create_error", "a5x_destroy", "a5x_last_error", "a5x_device_info",
    "a5x_load_table_file", "a5x_parse_table", "a5x_set_table", "a5x_clear_table", "a5x_table_export",
    "a5x_split_words", "a5x_keyspace", "a5x_expand", "a5x_expand_range", "a5x_expand_device", "a5x_keyspace_device",
    "a5x_digest_device", "a5x_partition", "a5x_dev_alloc", "a5x_dev_free", "a5x_memcpy_h2d",
    "a5x_memcpy_d2h", "a5x_synchronize", "a5x_debug_stamps", "a5x_debug_plan_word", "a5x_debug_plan_sizes",
    "a5x_debug_piece_build", "a5x_debug_cut_once", "a5x_debug_cplx_build", "a5x_debug_keyspace_cplx_lean",
    "a5x_debug_keyspace_refit", "a5x_debug_keyspace_small_stage", "a5x_debug_keyspace_stage",
    "a5x_debug_keyspace_large_stage", "a5x_debug_word_flags",
    "a5x_set_targets", "a5x_expand_digest", "a5x_expand_digest_device", "a5x_expand_digest_range_device",
    "a5x_digest_lines_device", "a5x_digest_size", "a5x_hit_digest", "a5x_debug_digest",
    "a5x_format_plain", "a5x_format_hits", "a5x_locate_device", "a5x_split_device",
    "a5x_stream_reserve",
    "a5x_set_rules", "a5x_load_rules_file", "a5x_rule_count", "a5x_hit_rules", "a5x_rules_last",
    "a5x_format_hits_rules", "a5x_digest_lines_rules_device", "a5x_debug_apply_rule",
    "a5x_set_salted_targets", "a5x_load_salted_hashes", "a5x_salt_count", "a5x_salt_get", "a5x_hit_salts",
    "a5x_salts_last", "a5x_format_hits_salted", "a5x_digest_lines_salted_device", "a5x_debug_digest_salted",
    "a5x_algo_salt_order",
    "a5x_set_iterated_targets", "a5x_load_pbkdf2_hashes", "a5x_salt_iterations", "a5x_format_hits_iterated",
    "a5x_debug_pbkdf2", "a5x_debug_iter_budget",
    "a5x_debug_target_set",
)


class A5xError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        self.code = code
        super().__init__(f"{ERRORS.get(code, code)}: {msg}" if msg else str(ERRORS.get(code, code)))


class Stats(ctypes.Structure):
    _fields_ = [
        ("candidates", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("words", ctypes.c_uint64),
        ("words_pass_b", ctypes.c_uint64), ("ms_keyspace", ctypes.c_double), ("ms_expand", ctypes.c_double),
        ("ms_total", ctypes.c_double), ("expand_launches", ctypes.c_uint32), ("words_slow", ctypes.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class Hit(ctypes.Structure):
    """a5x_hit: word index, candidate index inside the word, digest (its first 16 bytes)."""
    _fields_ = [("word", ctypes.c_uint64), ("cand", ctypes.c_uint64), ("digest", ctypes.c_uint8 * 16)]


SINK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t)

_lib: Optional[ctypes.CDLL] = None


def load(path: Optional[str] = None) -> ctypes.CDLL:
    """Load liba5x.so (building it first if hipcc is available and it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        try:
            from . import build as _b
            _b.build()
        except Exception as e:  # pragma: no cover - depends on toolchain
            raise A5xError(-2, f"liba5x.so missing at {path} and build failed: {e}") from e
    L = ctypes.CDLL(path)
    vp, u64, u32, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_size_t
    i = ctypes.c_int
    L.a5x_abi_version.restype = i
    L.a5x_create.argtypes = [i, ctypes.POINTER(vp)]
    L.a5x_create_error.argtypes = []
    L.a5x_create_error.restype = ctypes.c_char_p
    L.a5x_destroy.argtypes = [vp]
    L.a5x_destroy.restype = None
    L.a5x_last_error.argtypes = [vp]
    L.a5x_last_error.restype = ctypes.c_char_p
    L.a5x_device_info.argtypes = [vp, ctypes.c_char_p, sz, ctypes.POINTER(i)]
    L.a5x_load_table_file.argtypes = [vp, ctypes.c_char_p]
    L.a5x_parse_table.argtypes = [vp, ctypes.c_char_p, sz]
    L.a5x_set_table.argtypes = [vp, vp, vp, u32, vp, vp, vp, u32]
    L.a5x_clear_table.argtypes = [vp]
    L.a5x_table_export.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u64),
                                   ctypes.POINTER(u64), vp, vp, vp, vp, vp]
    L.a5x_split_words.argtypes = [vp, sz, vp, vp, u64, ctypes.POINTER(u64)]
    L.a5x_keyspace.argtypes = [vp, vp, vp, u64, i, i, i, vp, vp]
    L.a5x_expand.argtypes = [vp, vp, vp, u64, i, i, i, SINK, vp, ctypes.POINTER(Stats)]
    L.a5x_expand_range.argtypes = [vp, vp, vp, u64, i, i, i, u64, u64, SINK, vp, ctypes.POINTER(Stats)]
    L.a5x_expand_device.argtypes = [vp, vp, vp, u64, i, i, i, u64, u64, vp, u64, vp, vp, ctypes.POINTER(Stats), vp]
    L.a5x_keyspace_device.argtypes = [vp, vp, vp, u64, i, i, i, vp, vp, ctypes.POINTER(u64),
                                      ctypes.POINTER(u64), vp]
    L.a5x_digest_device.argtypes = [vp, vp, vp, u64, u64, vp, vp]
    L.a5x_partition.argtypes = [vp, u64, u32, vp]
    L.a5x_dev_alloc.argtypes = [vp, ctypes.POINTER(vp), sz]
    L.a5x_dev_free.argtypes = [vp, vp]
    L.a5x_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    L.a5x_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    L.a5x_synchronize.argtypes = [vp]
    L.a5x_debug_stamps.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), i]
    L.a5x_debug_plan_word.argtypes = [vp, vp, sz, i, i, vp, sz, vp]
    if hasattr(L, "a5x_debug_plan_sizes"):  # (not in a variant build of an older commit, A5X_LIB_PATH)
        L.a5x_debug_plan_sizes.argtypes = [vp, vp, sz, vp]
    if hasattr(L, "a5x_debug_piece_build"):
        L.a5x_debug_piece_build.argtypes = [vp, vp, sz, vp]
    if hasattr(L, "a5x_debug_cut_once"):
        L.a5x_debug_cut_once.argtypes = [vp, vp, sz, vp, vp, vp]
    if hasattr(L, "a5x_debug_cplx_build"):
        L.a5x_debug_cplx_build.argtypes = [vp, vp, sz, i, i, vp]
        L.a5x_debug_keyspace_cplx_lean.argtypes = [vp, ctypes.POINTER(u64)]
    if hasattr(L, "a5x_debug_keyspace_refit"):
        L.a5x_debug_keyspace_refit.argtypes = [vp, ctypes.POINTER(u64)]
    if hasattr(L, "a5x_debug_keyspace_stage"):
        L.a5x_debug_keyspace_small_stage.argtypes = [vp, ctypes.POINTER(u32)]
        L.a5x_debug_keyspace_stage.argtypes = [vp, ctypes.POINTER(u32)]
        L.a5x_debug_keyspace_large_stage.argtypes = [vp, i]
    if hasattr(L, "a5x_debug_word_flags"):
        L.a5x_debug_word_flags.argtypes = [vp, vp, u64]
    L.a5x_set_targets.argtypes = [vp, i, vp, u64]
    L.a5x_expand_digest.argtypes = [vp, vp, vp, u64, i, i, i, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(Stats)]
    L.a5x_expand_digest_device.argtypes = [vp, vp, vp, u64, i, i, i, u64, vp, u64, ctypes.POINTER(u64),
                                           ctypes.POINTER(Stats), vp]
    L.a5x_expand_digest_range_device.argtypes = [vp, vp, vp, u64, i, i, i, u64, u64, u64, vp, u64, ctypes.POINTER(u64),
                                                 ctypes.POINTER(Stats), vp]
    L.a5x_digest_lines_device.argtypes = [vp, i, vp, u64, vp, u64, ctypes.POINTER(u64), vp]
    L.a5x_digest_size.argtypes = [i]
    if hasattr(L, "a5x_algo_salt_order"):
        L.a5x_algo_salt_order.argtypes = [i]
    L.a5x_hit_digest.argtypes = [vp, ctypes.POINTER(Hit), vp, sz, ctypes.POINTER(sz)]
    L.a5x_debug_digest.argtypes = [i, ctypes.c_char_p, sz, vp, sz]
    L.a5x_format_plain.argtypes = [ctypes.c_char_p, sz, vp, sz, ctypes.POINTER(sz)]
    L.a5x_format_hits.argtypes = [vp, vp, vp, u64, i, i, i, vp, u64, SINK, vp]
    L.a5x_locate_device.argtypes = [vp, vp, vp, u64, i, i, i, vp, u64, vp, vp]
    L.a5x_stream_reserve.argtypes = [vp, u64, u64]
    L.a5x_split_device.argtypes = [vp, vp, vp, u64, i, i, i, vp, u32, vp, vp, vp, vp]
    L.a5x_set_rules.argtypes = [vp, ctypes.c_char_p, sz, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.a5x_load_rules_file.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.a5x_rule_count.argtypes = [vp]
    L.a5x_hit_rules.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
    L.a5x_rules_last.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.a5x_format_hits_rules.argtypes = [vp, vp, vp, u64, i, i, i, vp, u64, vp, SINK, vp]
    L.a5x_digest_lines_rules_device.argtypes = [vp, i, vp, u64, vp, u64, ctypes.POINTER(u64), vp]
    L.a5x_debug_apply_rule.argtypes = [ctypes.c_char_p, sz, ctypes.c_char_p, sz, vp, sz, ctypes.POINTER(sz)]
    L.a5x_set_salted_targets.argtypes = [vp, i, i, vp, u64, vp, vp]
    L.a5x_load_salted_hashes.argtypes = [vp, i, i, ctypes.c_char_p, sz, i, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                         ctypes.POINTER(u64)]
    L.a5x_salt_count.argtypes = [vp]
    L.a5x_salt_get.argtypes = [vp, u32, vp, sz, ctypes.POINTER(sz)]
    L.a5x_hit_salts.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
    L.a5x_salts_last.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.a5x_format_hits_salted.argtypes = [vp, vp, vp, u64, i, i, i, vp, u64, vp, i, SINK, vp]
    L.a5x_digest_lines_salted_device.argtypes = [vp, i, i, vp, u64, vp, u64, ctypes.POINTER(u64), vp]
    L.a5x_debug_digest_salted.argtypes = [i, i, ctypes.c_char_p, sz, ctypes.c_char_p, sz, vp, sz]
    L.a5x_set_iterated_targets.argtypes = [vp, i, vp, u64, vp, vp, vp]
    L.a5x_load_pbkdf2_hashes.argtypes = [vp, i, ctypes.c_char_p, sz, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                         ctypes.POINTER(u64)]
    L.a5x_salt_iterations.argtypes = [vp, u32, ctypes.POINTER(u32)]
    L.a5x_format_hits_iterated.argtypes = [vp, vp, vp, u64, i, i, i, vp, u64, vp, ctypes.POINTER(u64), SINK, vp]
    L.a5x_debug_pbkdf2.argtypes = [i, ctypes.c_char_p, sz, ctypes.c_char_p, sz, u32, vp, sz]
    L.a5x_debug_iter_budget.argtypes = [vp, u64, u64, ctypes.POINTER(u64)]
    L.a5x_debug_target_set.argtypes = [u32, vp, u64, vp, vp, sz, vp, sz, vp, sz, vp, sz]
    _lib = L
    return L


def check(rc: int, ctx=None) -> None:
    if rc != A5X_OK:
        msg = ""
        if ctx:
            m = load().a5x_last_error(ctx)
            msg = m.decode(errors="replace") if m else ""
        raise A5xError(rc, msg)


def debug_target_set(width: int, digests: bytes) -> dict:
    """The target set ``a5x_set_targets`` builds from ``digests`` (n * width bytes), as the
    host lays it out before the upload (``a5x_debug_target_set``; a test hook, no context, no
    device): ``bm_log2``, ``size`` (table slots), ``has_zero``, ``shared`` and the numpy
    arrays ``table`` (size x 4 words), ``tails`` (size x (width / 4 - 4)), ``ztails`` (one row
    per zero-prefix target) and ``bitmap`` (64-bit words)."""
    import numpy as np
    L = load()
    digests = bytes(digests)
    if width <= 0 or len(digests) % width:
        raise A5xError(-1, f"{len(digests)} bytes are no whole number of {width}-byte digests")
    n = len(digests) // width
    src = np.frombuffer(digests + bytes(16), dtype=np.uint8)
    info = np.zeros(8, dtype=np.uint64)
    check(L.a5x_debug_target_set(width, src.ctypes.data, n, info.ctypes.data, None, 0, None, 0, None, 0, None, 0))
    tw = width // 4 - 4
    tab, tails, zt, bm = (np.zeros(max(1, int(k)), dtype=np.uint32) for k in info[4:8])
    check(L.a5x_debug_target_set(width, src.ctypes.data, n, info.ctypes.data, tab.ctypes.data, len(tab),
                                 tails.ctypes.data, len(tails), zt.ctypes.data, len(zt), bm.ctypes.data, len(bm)))
    size = int(info[1])
    return {"bm_log2": int(info[0]), "size": size, "has_zero": int(info[2]), "shared": int(info[3]),
            "table": tab[: int(info[4])].reshape(size, 4), "tails": tails[: int(info[5])].reshape(size, tw) if tw else tails[:0].reshape(size, 0),
            "ztails": zt[: int(info[6])].reshape(-1, tw) if tw else zt[:0].reshape(0, 0),
            "bitmap": bm[: int(info[7])].view(np.uint64)}
