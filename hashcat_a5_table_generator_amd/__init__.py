"""a5x -- MI355X-native backend for hashcat -a 5 table-attack candidate expansion.

Drop-in for the expansion hot path of ``A113L/hashcat_a5_table_generator``
(``main.go:164-440``): the Go CLI, the ``.table`` format and the ``cand\\n`` output
stay as they are; the per-word engines run as gfx950 HIP kernels behind the C ABI
of ``include/a5x.h`` (``_build/liba5x.so``).
"""
from ._lib import A5xError, LIB_PATH
from .engine import (ALGO_MD5_MD5_MD5SALT, ALGO_MD5_MD5_SALT, ALGO_MD5_MD5SALT_MD5, ALGO_MD5_SALT_MD5, ALGO_SHA1_MD5_SALT,
                     ALGO_SHA1_SALT_SHA1, ALGO_SHA1_SHA1_SALT, salt_order,
                     ALGO_HMAC_MD5_KEY_PASS, ALGO_HMAC_MD5_KEY_SALT, ALGO_HMAC_SHA1_KEY_PASS, ALGO_HMAC_SHA1_KEY_SALT,
                     ALGO_HMAC_SHA256_KEY_PASS, ALGO_HMAC_SHA256_KEY_SALT, ALGO_HMAC_SHA512_KEY_PASS, ALGO_HMAC_SHA512_KEY_SALT,
                     ALGO_PBKDF2_HMAC_MD5, ALGO_PBKDF2_HMAC_SHA1, ALGO_PBKDF2_HMAC_SHA256, ALGO_PBKDF2_HMAC_SHA512, debug_pbkdf2,
                     ALGO_MD5, ALGO_MD5_MD5, ALGO_MD5_MD5_MD5, ALGO_MD5_MD5UP, ALGO_MD5_SHA1, ALGO_NTLM, ALGO_SHA1, ALGO_SHA1_MD5,
                     ALGO_SHA1_SHA1, ALGO_SHA224, ALGO_SHA256, ALGO_SHA256_MD5, ALGO_SHA384, ALGO_SHA512, DeviceBuffer, MODE_DEFAULT, MODE_REVERSE, MODE_SUBALL, MODE_SUBALL_REVERSE, ORDER_PASS_SALT, ORDER_SALT_PASS, Context, apply_rule, debug_digest_salted, decode_hex_notation,
                     digest_size, format_plain, generate, mode_of, pack_words, partition, process_word, process_word_reverse,
                     process_word_substitute_all, process_word_substitute_all_reverse, read_substitution_table,
                     split_words)

__all__ = [
    "ALGO_MD5_MD5_SALT", "ALGO_MD5_SALT_MD5", "ALGO_MD5_MD5_MD5SALT", "ALGO_MD5_MD5SALT_MD5", "ALGO_SHA1_SHA1_SALT",
    "ALGO_SHA1_SALT_SHA1", "ALGO_SHA1_MD5_SALT", "salt_order",
    "ALGO_HMAC_MD5_KEY_PASS", "ALGO_HMAC_MD5_KEY_SALT", "ALGO_HMAC_SHA1_KEY_PASS", "ALGO_HMAC_SHA1_KEY_SALT",
    "ALGO_HMAC_SHA256_KEY_PASS", "ALGO_HMAC_SHA256_KEY_SALT", "ALGO_HMAC_SHA512_KEY_PASS", "ALGO_HMAC_SHA512_KEY_SALT",
    "ALGO_PBKDF2_HMAC_MD5", "ALGO_PBKDF2_HMAC_SHA1", "ALGO_PBKDF2_HMAC_SHA256", "ALGO_PBKDF2_HMAC_SHA512", "debug_pbkdf2",
    "ALGO_MD5_MD5", "ALGO_MD5_MD5_MD5", "ALGO_MD5_MD5UP", "ALGO_MD5_SHA1", "ALGO_SHA1_SHA1", "ALGO_SHA1_MD5", "ALGO_SHA256_MD5",
    "A5xError", "LIB_PATH", "ALGO_MD5", "ALGO_NTLM", "ALGO_SHA1", "ALGO_SHA224", "ALGO_SHA256", "ALGO_SHA384", "ALGO_SHA512", "Context", "DeviceBuffer", "MODE_DEFAULT", "MODE_REVERSE", "MODE_SUBALL", "MODE_SUBALL_REVERSE",
    "ORDER_PASS_SALT", "ORDER_SALT_PASS", "apply_rule", "debug_digest_salted", "decode_hex_notation", "digest_size", "format_plain", "generate", "mode_of", "pack_words", "partition", "process_word",
    "process_word_reverse", "process_word_substitute_all", "process_word_substitute_all_reverse",
    "read_substitution_table", "split_words",
]
