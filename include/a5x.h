/*
 * a5x.h -- C ABI of liba5x.so, the MI355X (gfx950) backend for hashcat -a 5
 * table-attack candidate expansion.
 *
 * Drop-in boundary: the reference calls one of four
 * engines per word from a goroutine,
 *     func processWord(word string, subMap map[string][]string,
 *                      minSubstitute, maxSubstitute int, out chan<- string)
 *     /root/reference/main.go:168   (also :208 -r, :308 -s, :369 -s -r;
 *                                     dispatcher main.go:77-93)
 * and sends every candidate on a channel that one writer drains as s+"\n"
 * (main.go:58-68).  liba5x replaces that per-word call with a batch call:
 * contiguous word bytes + offsets in, "cand\n" bytes out, grouped per word.
 *
 * Conventions: every function returns 0 (A5X_OK) or a negative A5X_E_* code and
 * records a message readable with a5x_last_error().  Inputs are caller-owned and
 * copied/staged; output spans handed to a sink are library-owned and valid only
 * during the callback.  One in-flight call per context (thread-compatible).
 * Go pointers must not be retained across calls (cgo rules): the library never
 * keeps a caller pointer after returning.
 *
 * mode: A5X_MODE_DEFAULT (processWord, main.go:168), A5X_MODE_REVERSE (-r,
 * main.go:208), A5X_MODE_SUBALL (-s, main.go:308), A5X_MODE_SUBALL_REVERSE
 * (-s -r, main.go:369) -- the switch of main.go:80-92.  min/max are passed raw
 * (--table-min/--table-max, main.go:21-22); the library applies processWord's
 * min==0 -> 1 bump itself (main.go:169-171).
 */
#ifndef A5X_H
#define A5X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A5X_API __attribute__((visibility("default")))

#define A5X_ABI_VERSION 1

enum {
  A5X_OK = 0,
  A5X_E_ARG = -1,         /* bad argument */
  A5X_E_HIP = -2,         /* HIP runtime error (no device, launch failure, ...) */
  A5X_E_NOMEM = -3,       /* host or device allocation failed */
  A5X_E_IO = -4,          /* table / dictionary file could not be read (main.go:43-45, 53-55) */
  A5X_E_TOOLONG = -5,     /* bufio.ErrTooLong on a table line (main.go:143 -> log.Fatal) */
  A5X_E_BOUNDS = -6,      /* -r slice-bounds panic of the reference (main.go:255) */
  A5X_E_OVERFLOW = -7,    /* a keyspace does not fit 64 bits */
  A5X_E_CAPACITY = -8,    /* caller's output buffer too small (device API) */
  A5X_E_UNSUPPORTED = -9, /* mode/word beyond this build's device limits */
  A5X_E_NOTABLE = -10,    /* no substitution table loaded */
  A5X_E_SINK = -11        /* the sink callback returned non-zero */
};

enum {
  A5X_MODE_DEFAULT = 0,
  A5X_MODE_REVERSE = 1,
  A5X_MODE_SUBALL = 2,
  A5X_MODE_SUBALL_REVERSE = 3
};

/* digest algorithms of the fused digest + lookup stage.  Values 4, 8,
 * 9..15 and 23..31 are unassigned and invalid (A5X_E_ARG everywhere); additions never renumber.
 * 16..22 are nested: a digest of the hex text of another digest, hex = lower-case ASCII
 * hex of the inner digest in its standard byte order, HEX = upper-case.  32..38 are salted
 * nested: the outer digest over that hex text and a salt ("." is concatenation); they exist
 * only as salted sets (a5x_set_salted_targets), each with its own placement of the salt
 * (a5x_algo_salt_order).  39..47 are unassigned and invalid.  48..55 are HMAC (RFC 2104) with the
 * candidate as the key and the salt as the message (key = pass) or the reverse (key = salt); they
 * too exist only as salted sets, with order 0 for key = pass and 1 for key = salt.  56..71 are
 * unassigned and invalid.  72..75 are PBKDF2 (RFC 8018) over HMAC with the candidate as the
 * password: iterated sets (a5x_set_iterated_targets), matched on the first 16 bytes of T1. */
enum {
  A5X_ALGO_MD5 = 0,   /* RFC 1321 over the candidate bytes (== Go crypto/md5); hashcat -m 0 */
  A5X_ALGO_NTLM = 1,  /* MD4 (RFC 1320) over UTF-16LE of the candidate ([]rune + utf16.Encode); -m 1000 */
  A5X_ALGO_SHA1 = 2,  /* SHA-1 (FIPS 180-4) over the candidate bytes; hashcat -m 100 */
  A5X_ALGO_SHA256 = 3, /* SHA-256 (FIPS 180-4) over the candidate bytes; hashcat -m 1400 */
  A5X_ALGO_SHA224 = 5, /* SHA-224 (FIPS 180-4) over the candidate bytes; hashcat -m 1300 */
  A5X_ALGO_SHA384 = 6, /* SHA-384 (FIPS 180-4) over the candidate bytes; hashcat -m 10800 */
  A5X_ALGO_SHA512 = 7, /* SHA-512 (FIPS 180-4) over the candidate bytes; hashcat -m 1700 */
  A5X_ALGO_MD5_MD5 = 16,     /* md5(hex(md5(p))); hashcat -m 2600 */
  A5X_ALGO_MD5_MD5_MD5 = 17, /* md5(hex(md5(hex(md5(p))))); hashcat -m 3500 */
  A5X_ALGO_MD5_MD5UP = 18,   /* md5(HEX(md5(p))); hashcat -m 4300 */
  A5X_ALGO_MD5_SHA1 = 19,    /* md5(hex(sha1(p))); hashcat -m 4400 */
  A5X_ALGO_SHA1_SHA1 = 20,   /* sha1(hex(sha1(p))); hashcat -m 4500 */
  A5X_ALGO_SHA1_MD5 = 21,    /* sha1(hex(md5(p))); hashcat -m 4700 */
  A5X_ALGO_SHA256_MD5 = 22,  /* sha256(hex(md5(p))); hashcat -m 20800 */
  A5X_ALGO_MD5_MD5_SALT = 32,    /* md5(hex(md5(p)) . salt); hashcat -m 2611 / 2711 */
  A5X_ALGO_MD5_SALT_MD5 = 33,    /* md5(salt . hex(md5(p))); -m 3710 */
  A5X_ALGO_MD5_MD5_MD5SALT = 34, /* md5(hex(md5(p)) . hex(md5(salt))); -m 3910 */
  A5X_ALGO_MD5_MD5SALT_MD5 = 35, /* md5(hex(md5(salt)) . hex(md5(p))); -m 2811 */
  A5X_ALGO_SHA1_SHA1_SALT = 36,  /* sha1(hex(sha1(p)) . salt); -m 4510 */
  A5X_ALGO_SHA1_SALT_SHA1 = 37,  /* sha1(salt . hex(sha1(p))); -m 4520 */
  A5X_ALGO_SHA1_MD5_SALT = 38,   /* sha1(hex(md5(p)) . salt); -m 4710 */
  A5X_ALGO_HMAC_MD5_KEY_PASS = 48,    /* HMAC-MD5(K = pass, salt); hashcat -m 50 */
  A5X_ALGO_HMAC_MD5_KEY_SALT = 49,    /* HMAC-MD5(K = salt, pass); -m 60 */
  A5X_ALGO_HMAC_SHA1_KEY_PASS = 50,   /* HMAC-SHA1(K = pass, salt); -m 150 */
  A5X_ALGO_HMAC_SHA1_KEY_SALT = 51,   /* HMAC-SHA1(K = salt, pass); -m 160 */
  A5X_ALGO_HMAC_SHA256_KEY_PASS = 52, /* HMAC-SHA256(K = pass, salt); -m 1450 */
  A5X_ALGO_HMAC_SHA256_KEY_SALT = 53, /* HMAC-SHA256(K = salt, pass); -m 1460 */
  A5X_ALGO_HMAC_SHA512_KEY_PASS = 54, /* HMAC-SHA512(K = pass, salt); -m 1750 */
  A5X_ALGO_HMAC_SHA512_KEY_SALT = 55, /* HMAC-SHA512(K = salt, pass); -m 1760 */
  A5X_ALGO_PBKDF2_HMAC_MD5 = 72,      /* PBKDF2-HMAC-MD5(pass, salt, c); hashcat -m 11900 */
  A5X_ALGO_PBKDF2_HMAC_SHA1 = 73,     /* PBKDF2-HMAC-SHA1; -m 12000 */
  A5X_ALGO_PBKDF2_HMAC_SHA256 = 74,   /* PBKDF2-HMAC-SHA256; -m 10900 */
  A5X_ALGO_PBKDF2_HMAC_SHA512 = 75    /* PBKDF2-HMAC-SHA512; -m 12100 */
};
/* Digest bytes of an algorithm: 16, 16, 20, 32 for 0..3, 28, 48, 64 for 5..7, 16, 16, 16,
 * 16, 20, 20, 32 for 16..22, 16, 16, 16, 16, 20, 20, 20 for 32..38 (the outer digest) and 16,
 * 16, 20, 20, 32, 32, 64, 64 for 48..55; 16 for 72..75 (the compared bytes of the derived key);
 * A5X_E_ARG for anything else (4, 8, 9..15, 23..31, 39..47, 56..71 and 76 on included).  Pure
 * host function (no HIP call). */
A5X_API int a5x_digest_size(int algo);
/* Where a salted nested algorithm (32..38) puts its salt: 0 text . salt (32, 34, 36, 38), 1
 * salt . text (33, 35, 37); an HMAC algorithm (48..55): 0 key = pass (48, 50, 52, 54), 1 key =
 * salt (49, 51, 53, 55) -- the `order` its salted entry points must be given; 0 for the PBKDF2
 * algorithms 72..75.  A5X_E_ARG for every other value.  Pure host function. */
A5X_API int a5x_algo_salt_order(int algo);

/* One target hit: word index in the batch, candidate index inside that word (in the
 * library's per-word candidate order, the one a5x_expand emits), digest bytes.  For an
 * algorithm wider than 16 bytes (SHA-1, SHA-224 / 256 / 384 / 512) digest holds the first 16 bytes of the
 * candidate's digest; the whole digest matched a target, and a5x_hit_digest returns it. */
typedef struct a5x_hit {
  uint64_t word;
  uint64_t cand;
  uint8_t digest[16];
} a5x_hit;

typedef struct a5x_ctx a5x_ctx;

/* Sink for expanded bytes: a run of complete "cand\n" lines.  Return 0 to go on. */
typedef int (*a5x_sink_fn)(void* user, const uint8_t* data, size_t len);

typedef struct a5x_stats {
  uint64_t candidates;  /* candidates produced by the call */
  uint64_t bytes;       /* bytes produced (sum of len(cand)+1) */
  uint64_t words;       /* words in the batch */
  uint64_t words_pass_b;/* words expanded by the large-LDS pass */
  double ms_keyspace;   /* device time: keyspace + scans + plan (HIP events) */
  double ms_expand;     /* device time: expansion kernels only (HIP events) */
  double ms_total;      /* device time of the whole call */
  uint32_t expand_launches;
  uint32_t words_slow;   /* words expanded by the per-word (non-FAST) pass */
} a5x_stats;

/* ---- context ------------------------------------------------------------ */
A5X_API int a5x_abi_version(void);
/* device = -1: host-only context (table parsing/export, no GPU; device calls fail). */
A5X_API int a5x_create(int device, a5x_ctx** out);
A5X_API void a5x_destroy(a5x_ctx* ctx);
A5X_API const char* a5x_last_error(const a5x_ctx* ctx);
/* Why the calling thread's last a5x_create failed ("" after a success): the failing HIP
   call with hipGetErrorString, or the argument problem (no context exists to carry it). */
A5X_API const char* a5x_create_error(void);
/* device name / gfx arch of the context's GPU */
A5X_API int a5x_device_info(a5x_ctx* ctx, char* name, size_t name_cap, int* cu_count);

/* ---- substitution tables (main.go:40-50, 102-162) ------------------------ */
/* readSubstitutionTable(path) + merge into the context's map in call order. */
A5X_API int a5x_load_table_file(a5x_ctx* ctx, const char* path);
/* Same for in-memory file contents. */
A5X_API int a5x_parse_table(a5x_ctx* ctx, const uint8_t* data, size_t len);
/* Replace the map with an already-merged one:
 * key i = keys_bytes[key_off[i] .. key_off[i+1]); value j = vals_bytes[val_off[j]
 * .. val_off[j+1]) belongs to key val_key[j]; values keep their array order per key. */
A5X_API int a5x_set_table(a5x_ctx* ctx, const uint8_t* keys_bytes, const uint64_t* key_off, uint32_t n_keys,
                          const uint8_t* vals_bytes, const uint64_t* val_off, const uint32_t* val_key,
                          uint32_t n_vals);
A5X_API int a5x_clear_table(a5x_ctx* ctx);
/* Export the merged map: sizes first (any out pointer may be NULL). */
A5X_API int a5x_table_export(const a5x_ctx* ctx, uint32_t* n_keys, uint32_t* n_vals, uint64_t* key_bytes,
                             uint64_t* val_bytes, uint8_t* keys_out, uint64_t* key_off_out, uint8_t* vals_out,
                             uint64_t* val_off_out, uint32_t* val_key_out);

/* ---- dictionary splitting (bufio.Scanner + ScanLines, main.go:72-74) ------- */
/* Splits data into words exactly as the reference's dict scanner: "\n" split,
 * one trailing "\r" dropped, a line >= 64 KiB silently ends the input.  words_out
 * receives the concatenated word bytes (<= len bytes), off_out n+1 offsets.
 * With words_out == NULL only *n_words is computed. */
A5X_API int a5x_split_words(const uint8_t* data, size_t len, uint8_t* words_out, uint64_t* off_out,
                            uint64_t off_cap, uint64_t* n_words);

/* ---- host-buffer API -------------------------------------------------------- */
/* Per-word candidate count and output bytes (len+1 per candidate). */
A5X_API int a5x_keyspace(a5x_ctx* ctx, const uint8_t* words, const uint64_t* word_off, uint64_t n_words, int mode,
                         int min, int max, uint64_t* out_count, uint64_t* out_bytes);
/* Expand and stream "cand\n" lines to sink, words in order; a word's candidates are
 * contiguous.  Replaces the goroutine-per-word dispatch + channel of main.go:70-98. */
A5X_API int a5x_expand(a5x_ctx* ctx, const uint8_t* words, const uint64_t* word_off, uint64_t n_words, int mode,
                       int min, int max, a5x_sink_fn sink, void* user, a5x_stats* stats);
/* a5x_expand of the batch's global candidates [cand_begin, cand_end) only (cand_end =
 * UINT64_MAX: to the end): a resume cursor over the stream (CLI --skip / --limit, the
 * role of hashcat's own -s / -l on the pipe the reference feeds, README.MD:69).  A
 * word's candidate order does not depend on the batch it is in, so (batch offset +
 * index) names one candidate of the dictionary's stream.  stats->candidates / bytes
 * count the window. */
A5X_API int a5x_expand_range(a5x_ctx* ctx, const uint8_t* words, const uint64_t* word_off, uint64_t n_words,
                             int mode, int min, int max, uint64_t cand_begin, uint64_t cand_end, a5x_sink_fn sink,
                             void* user, a5x_stats* stats);

/* Make a5x_expand's buffers ahead of the first call (pinned double buffer, HBM range
 * buffers, copy stream, the keyspace state of a batch of `words` words / `word_bytes`
 * bytes, the table upload), so a pipeline's first batch does not pay for them; a host may
 * call it on a second thread while it reads its first batch.  Optional. */
A5X_API int a5x_stream_reserve(a5x_ctx* ctx, uint64_t words, uint64_t word_bytes);

/* ---- device-resident API (words already in HBM; used by bench and multi-GPU) -- */
/* Expands global candidates [cand_begin, cand_end) of the batch (cand_end =
 * UINT64_MAX: to the end) into d_out (d_out[0] = first byte of cand_begin).
 * d_word_byte_off (n_words+1, optional) receives each word's byte offset in the
 * batch's full output; d_word_cand_off likewise for candidate offsets.
 * stream: a hipStream_t (NULL = the context's stream).  Synchronises once to
 * read the totals; returns A5X_E_CAPACITY (with stats->bytes = need) if the
 * range does not fit out_cap. */
A5X_API int a5x_expand_device(a5x_ctx* ctx, const uint8_t* d_words, const uint64_t* d_word_off, uint64_t n_words,
                              int mode, int min, int max, uint64_t cand_begin, uint64_t cand_end, uint8_t* d_out,
                              uint64_t out_cap, uint64_t* d_word_cand_off, uint64_t* d_word_byte_off,
                              a5x_stats* stats, void* stream);
/* Keyspace of device-resident words: totals only (and per-word offsets if given). */
A5X_API int a5x_keyspace_device(a5x_ctx* ctx, const uint8_t* d_words, const uint64_t* d_word_off, uint64_t n_words,
                                int mode, int min, int max, uint64_t* d_word_cand_off, uint64_t* d_word_byte_off,
                                uint64_t* total_cands, uint64_t* total_bytes, void* stream);
/* Order-independent per-word digest of an expanded batch (verification):
 * d_digest[4*w..] = {count, bytes, sum h, sum h^2}, h = fmix64(fnv1a64(cand)). */
A5X_API int a5x_digest_device(a5x_ctx* ctx, const uint8_t* d_out, const uint64_t* d_word_byte_off, uint64_t out_base,
                              uint64_t n_words, uint64_t* d_digest, void* stream);

/* ---- fused digest + lookup (no reference counterpart: hashcat
 * hashes the candidates main.go:66 prints, README.MD:69) ----------------------- */
/* Replace the device-resident target set: n digests of algorithm algo, each
 * a5x_digest_size(algo) bytes in the digest's standard byte order (duplicates allowed).
 * Built on the host (prefilter bitmap + open-addressing table keyed on the first 16
 * bytes, the remaining 4 to 48 bytes in a parallel array) and uploaded once.  For the wide
 * algorithms (SHA-1 and the SHA-2 family) the context keeps a host copy of the digests for a5x_hit_digest.
 * A nested algorithm (16..22) takes its outer digests: 16, 20 or 32 bytes, wide when over 16.  A nested set
 * is hashed by the two-pass route in every mode, with or without rules; it has no salted form. */
A5X_API int a5x_set_targets(a5x_ctx* ctx, int algo, const uint8_t* digests, uint64_t n);
/* The full digest of a hit against the context's current target set, *out_len =
 * a5x_digest_size of the set's algorithm (at most 64): the hit's own 16 bytes for MD5 /
 * NTLM, else the target whose first 16 bytes equal hit->digest (A5X_E_ARG when there is none;
 * should several targets share those 16 bytes, the one that the hit (word, cand) of the
 * context's latest a5x_expand_digest* call matched).  out == NULL: size only;
 * A5X_E_CAPACITY when cap is too small.  Host only. */
A5X_API int a5x_hit_digest(a5x_ctx* ctx, const a5x_hit* hit, uint8_t* out, size_t cap, size_t* out_len);
/* Expand the batch (device-resident words) in ranges that fit a device scratch of
 * scratch_bytes (0 = library default), hash every candidate on the device and probe the
 * target set.  Hits go to hits (host memory, hit_cap entries, any order); *n_hits gets
 * the total (which may exceed hit_cap: A5X_E_CAPACITY after filling hit_cap).
 * stats->candidates/bytes cover the whole batch; ms_expand is expansion time,
 * ms_total - ms_keyspace - ms_expand the digest time. */
A5X_API int a5x_expand_digest_device(a5x_ctx* ctx, const uint8_t* d_words, const uint64_t* d_word_off,
                                     uint64_t n_words, int mode, int min, int max, uint64_t scratch_bytes,
                                     a5x_hit* hits, uint64_t hit_cap, uint64_t* n_hits, a5x_stats* stats,
                                     void* stream);
/* The same for the batch's global candidates [cand_begin, cand_end) only (clipped to the
 * batch): a shard whose ends cut words (a5x_split_device gives the cut
 * points), as a5x_expand_device's range.  Hits name (word, candidate in word) of the
 * batch; stats->candidates counts the range. */
A5X_API int a5x_expand_digest_range_device(a5x_ctx* ctx, const uint8_t* d_words, const uint64_t* d_word_off,
                                           uint64_t n_words, int mode, int min, int max, uint64_t cand_begin,
                                           uint64_t cand_end, uint64_t scratch_bytes, a5x_hit* hits,
                                           uint64_t hit_cap, uint64_t* n_hits, a5x_stats* stats, void* stream);
/* Host-buffer version (stages the words into HBM first). */
A5X_API int a5x_expand_digest(a5x_ctx* ctx, const uint8_t* words, const uint64_t* word_off, uint64_t n_words,
                              int mode, int min, int max, a5x_hit* hits, uint64_t hit_cap, uint64_t* n_hits,
                              a5x_stats* stats);
/* Digest of every line of a device "cand\n" stream (d_lines 16-B aligned, nbytes
 * ending in '\n') into d_digests (a5x_digest_size(algo) bytes per line, in line order,
 * in the digest's standard byte order; 16-B aligned for MD5 / NTLM, 4-B aligned for the
 * wide algorithms: 20 / 28 / 32 / 48 / 64 bytes per line); digests_cap counts lines; *n_lines = lines.
 * Verification hook for the digest kernels (tests compare with hashlib / RFC MD4). */
A5X_API int a5x_digest_lines_device(a5x_ctx* ctx, int algo, const uint8_t* d_lines, uint64_t nbytes,
                                    uint8_t* d_digests, uint64_t digests_cap, uint64_t* n_lines, void* stream);

/* ---- hashcat-style hit output: "hash:plain" lines --------------- */
/* The plain as hashcat's outfile writes it: unchanged, or $HEX[lowercase hex] when it
 * is not valid UTF-8, contains a control byte (< 0x20, 0x7f) or has the $HEX[...] form
 * itself (README.MD:171-176 uses the same notation for input).  *out_len = the size;
 * out == NULL: size only; A5X_E_CAPACITY when cap is too small.  Pure host function. */
A5X_API int a5x_format_plain(const uint8_t* plain, size_t len, uint8_t* out, size_t cap, size_t* out_len);
/* One "hexdigest:plain\n" line per hit, in hit order, through sink (hashcat -m 0 /
 * -m 1000 / -m 100 / -m 1400 / -m 1300 / -m 10800 / -m 1700 potfile form, README.MD:74-106;
 * the full-width digest, 40 / 64 / 56 / 96 / 128 hex digits for SHA-1 / SHA-256 / SHA-224 /
 * SHA-384 / SHA-512, obtained as in a5x_hit_digest; a nested algorithm's outer digest, the
 * potfile form of -m 2600 / 3500 / 4300 / 4400 / 4500 / 4700 / 20800): the plains are
 * regenerated on the device from the hit's (word, cand) with the same batch (host
 * buffers), mode and limits the hits were found with. */
A5X_API int a5x_format_hits(a5x_ctx* ctx, const uint8_t* words, const uint64_t* word_off, uint64_t n_words,
                            int mode, int min, int max, const a5x_hit* hits, uint64_t n_hits, a5x_sink_fn sink,
                            void* user);

/* ---- hashcat rules in the digest + lookup stage (no reference counterpart: the
 * reference's pipeline hands its candidates to "hashcat ... -r best66.rule", README.MD:69,
 * :163) ------------------------------------------------------------------------- */
/* While a context holds >= 1 rule, every a5x_expand_digest* call hashes each candidate
 * once per rule (the rule applied first) and a hit names (word, cand) and a rule; with no
 * rules nothing changes.  The rule language is the hashcat subset of DESIGN.md "Rules":
 * words of at most A5X_RULE_LMAX = 128 bytes at any point, at most 31 functions a rule. */
/* Replace the context's rule set from rule-file text (NULL / 0: clear).  *n_rules =
 * accepted, *n_skipped = lines skipped as unsupported or malformed.  Works on a
 * host-only context (parse only). */
A5X_API int a5x_set_rules(a5x_ctx* ctx, const uint8_t* text, size_t len, uint32_t* n_rules, uint32_t* n_skipped);
A5X_API int a5x_load_rules_file(a5x_ctx* ctx, const char* path, uint32_t* n_rules, uint32_t* n_skipped);
A5X_API int a5x_rule_count(const a5x_ctx* ctx);
/* Latest a5x_expand_digest* call: the rule index of each hit copied to the caller, in hit
 * order (rule_out == NULL: *n only); a5x_rules_last: hashes computed, and candidates
 * rejected (hashed under no rule) as longer than A5X_RULE_LMAX.  a5x_digest_lines_rules_device
 * sets the two counts too. */
A5X_API int a5x_hit_rules(a5x_ctx* ctx, uint32_t* rule_out, uint64_t cap, uint64_t* n);
A5X_API int a5x_rules_last(a5x_ctx* ctx, uint64_t* hashed, uint64_t* rejected);
/* a5x_format_hits with the ruled plain, "hexdigest:rule(candidate)\n": the candidate is
 * regenerated as there, then hit_rule[i] (n_hits entries, of the context's current rule
 * set) is applied to it on the host with the interpreter the kernel runs. */
A5X_API int a5x_format_hits_rules(a5x_ctx* ctx, const uint8_t* words, const uint64_t* word_off, uint64_t n_words,
                                  int mode, int min, int max, const a5x_hit* hits, uint64_t n_hits,
                                  const uint32_t* hit_rule, a5x_sink_fn sink, void* user);
/* a5x_digest_lines_device under the context's R rules: the digest of (line i, rule r) at
 * index i * R + r; a rejected line's R digests are all zero.  digests_cap counts digests
 * (lines x R); d_digests 4-B aligned.  Verification hook. */
A5X_API int a5x_digest_lines_rules_device(a5x_ctx* ctx, int algo, const uint8_t* d_lines, uint64_t nbytes,
                                          uint8_t* d_digests, uint64_t digests_cap, uint64_t* n_lines, void* stream);
/* Pure host: parse one rule line and apply it to word (len <= A5X_RULE_LMAX) with the
 * a5x_rules.h interpreter.  A5X_E_ARG for a line a5x_set_rules would skip or ignore. */
A5X_API int a5x_debug_apply_rule(const uint8_t* rule, size_t rule_len, const uint8_t* word, size_t len,
                                 uint8_t* out, size_t cap, size_t* out_len);

/* ---- salted target lists: hash(pass.salt) and hash(salt.pass) (no reference counterpart:
 * hashcat -m 10 / 20 (MD5), 110 / 120 (SHA-1), 1310 / 1320 (SHA-224), 1410 / 1420 (SHA-256),
 * 10810 / 10820 (SHA-384), 1710 / 1720 (SHA-512)) ------------------------------------ */
/* Replace the target set with a salted one: n digests of algo as in a5x_set_targets, target i
 * registered with the salt salt_bytes[salt_off[i] .. salt_off[i+1]) (n + 1 offsets; at most 64
 * bytes, 0 allowed: the unsalted digest; the nested algorithms 16..22 have no salted form
 * here: A5X_E_ARG, from every salted entry point).  order 0: the message is candidate + salt
 * (pass.salt), order 1: salt + candidate (salt.pass).  The salted nested algorithms 32..38 take
 * the hex text of the candidate's inner digest in the candidate's place; order must be the
 * algorithm's own (a5x_algo_salt_order), else A5X_E_ARG; a candidate over 128 bytes is skipped
 * under every salt, and no pair is skipped for its salt; for 34 / 35 the library hashes the
 * salt itself, everything public (indices, a5x_salt_get, the output) is the caller's salt.
 * The HMAC algorithms 48..55 (RFC 2104; hashcat -m 50 / 150 / 1450 / 1750 and 60 / 160 / 1460 /
 * 1760) follow the same rules: order 0 is HMAC(key = candidate, message = salt), order 1
 * HMAC(key = salt, message = candidate), and order must be the algorithm's own; a candidate over
 * 128 bytes is skipped under every salt, no pair is skipped for its salt, and a candidate of
 * 65..128 bytes used as the key of a 64-byte-block hash is replaced by its digest, as RFC 2104
 * says.  Salts are deduplicated; a salt's index
 * is its first appearance in the caller's order.  While the set is salted every
 * a5x_expand_digest* call hashes each candidate once per distinct salt, and a digest computed
 * under one salt matches only targets registered with that salt.  A (candidate, salt) pair
 * whose message would exceed 128 bytes is skipped (not hashed) and counted.  A5X_E_ARG: NTLM
 * (no salted mode) or an invalid algo, an order other than 0 / 1, a salt over 64 bytes;
 * A5X_E_UNSUPPORTED: the context holds rules (rules and salts together are not supported;
 * a5x_set_rules on a salted set answers the same).  On a host-only context the arguments are
 * checked and the salts kept (a5x_salt_count / a5x_salt_get), nothing is uploaded.
 * a5x_set_targets makes the set unsalted again. */
A5X_API int a5x_set_salted_targets(a5x_ctx* ctx, int algo, int order, const uint8_t* digests, uint64_t n,
                                   const uint8_t* salt_bytes, const uint64_t* salt_off);
/* The same from the text of a "hexdigest:salt" file, one target per line ('\n', one trailing
 * '\r' dropped, empty lines ignored): the salt is everything after the first ':' taken
 * literally (it may contain ':'), or with hex_salt its hex decoding.  Lines with a bad digest,
 * a bad hex salt, a salt over 64 bytes or no ':' are skipped and counted in *n_skipped. */
A5X_API int a5x_load_salted_hashes(a5x_ctx* ctx, int algo, int order, const uint8_t* text, size_t len, int hex_salt,
                                   uint64_t* n_targets, uint64_t* n_salts, uint64_t* n_skipped);
/* Distinct salts of the context's salted set (0: the set is not salted), and salt `index`
 * (*out_len = its size; out == NULL: size only; A5X_E_CAPACITY when cap is too small). */
A5X_API int a5x_salt_count(const a5x_ctx* ctx);
A5X_API int a5x_salt_get(a5x_ctx* ctx, uint32_t index, uint8_t* out, size_t cap, size_t* out_len);
/* Latest a5x_expand_digest* call on a salted set: the salt index of each hit copied to the
 * caller, in hit order (salt_out == NULL: *n only); a5x_salts_last: (candidate, salt) pairs
 * hashed, and pairs skipped as longer than 128 bytes.  a5x_digest_lines_salted_device sets
 * the two counts too. */
A5X_API int a5x_hit_salts(a5x_ctx* ctx, uint32_t* salt_out, uint64_t cap, uint64_t* n);
A5X_API int a5x_salts_last(a5x_ctx* ctx, uint64_t* hashed, uint64_t* skipped);
/* a5x_format_hits for a salted set, "hexdigest:salt:plain\n" (hashcat's potfile form): the
 * salt hit_salt[i] (n_hits entries, of the context's current set) raw, or in lowercase hex
 * with hex_salt; the plain as a5x_format_plain writes it. */
A5X_API int a5x_format_hits_salted(a5x_ctx* ctx, const uint8_t* words, const uint64_t* word_off, uint64_t n_words,
                                   int mode, int min, int max, const a5x_hit* hits, uint64_t n_hits,
                                   const uint32_t* hit_salt, int hex_salt, a5x_sink_fn sink, void* user);
/* a5x_digest_lines_device under the S salts of the context's salted set, with algo and order
 * given here: the digest of (line i, salt s) at index i * S + s; a skipped pair's digest is
 * all zero.  digests_cap counts digests (lines x S); d_digests 4-B aligned.  Verification hook.
 * The salt records of a salted nested set (32..38) and of an HMAC set (48..55) are built for
 * its algorithm: algo must be the set's, any other algo on such a set is A5X_E_ARG, and so is
 * one of these algorithms on another kind of set.  The same holds for an iterated set (72..75,
 * order 0): 16 bytes per pair, the index being the (salt, iterations) pair's. */
A5X_API int a5x_digest_lines_salted_device(a5x_ctx* ctx, int algo, int order, const uint8_t* d_lines, uint64_t nbytes,
                                           uint8_t* d_digests, uint64_t digests_cap, uint64_t* n_lines, void* stream);
/* Pure host: the digest of msg + salt (order 0) or salt + msg (order 1), the message placed
 * by the a5x_salt.h code the kernel runs and hashed by the a5x_sha.h cores (MD5: an RFC 1321
 * host compression over the same padded message words).  A5X_E_UNSUPPORTED for a pair the
 * kernel would skip (len + slen > 128).  32..38: the host path of a5x_salt_nest.h (record
 * preparation included); A5X_E_UNSUPPORTED for a candidate over 128 bytes.  48..55: the host
 * path of a5x_hmac.h (record preparation, key states, inner and outer hash), salt = the salt,
 * msg = the candidate; A5X_E_UNSUPPORTED for a candidate over 128 bytes, A5X_E_ARG for a salt
 * over 64 bytes or the wrong order. */
A5X_API int a5x_debug_digest_salted(int algo, int order, const uint8_t* salt, size_t slen, const uint8_t* msg,
                                    size_t len, uint8_t* out, size_t cap);

/* ---- iterated target lists: PBKDF2-HMAC-MD5 / -SHA1 / -SHA256 / -SHA512 (no reference
 * counterpart: hashcat -m 11900 / 12000 / 10900 / 12100) ---------------------------------- */
/* Replace the target set with an iterated one: algo 72..75, n targets of 16 bytes each (the
 * first 16 bytes of the derived key's block T1 -- what hashcat compares), target i registered
 * with the salt salt_bytes[salt_off[i] .. salt_off[i+1]) (at most 64 bytes) and iters[i] >= 1
 * iterations.  Distinct (salt, iterations) pairs are deduplicated and indexed by first
 * appearance; that index is what a5x_salt_count / a5x_salt_get / a5x_salt_iterations /
 * a5x_hit_salts speak of.  The set is a salted one of order 0: every a5x_expand_digest* call
 * derives a key per (candidate, index) pair, a candidate over 128 bytes is skipped under every
 * index and counted (a5x_salts_last), a candidate of 65..128 bytes as the key of a 64-byte-block
 * hash is replaced by its digest.  A5X_E_ARG: an iteration count of 0, a salt over 64 bytes, an
 * algo other than 72..75; A5X_E_UNSUPPORTED: the context holds rules (a5x_set_rules on such a
 * set answers the same).  A host-only context checks the arguments and keeps them.
 * a5x_set_targets, a5x_set_salted_targets and a5x_debug_digest_salted answer A5X_E_ARG for
 * 72..75. */
A5X_API int a5x_set_iterated_targets(a5x_ctx* ctx, int algo, const uint8_t* digests16, uint64_t n,
                                     const uint8_t* salt_bytes, const uint64_t* salt_off, const uint32_t* iters);
/* The same from hashcat's lines "name:iterations:base64(salt):base64(dk)", name = md5 / sha1 /
 * sha256 / sha512 as algo says, standard base64 with padding ('\n', one trailing '\r' dropped,
 * empty lines ignored).  A line is skipped and counted in *n_skipped for a wrong name, bad
 * base64, iterations 0 or not a number, a salt over 64 bytes or a key under 16 bytes.  The
 * original line and the whole key are kept per target for a5x_format_hits_iterated. */
A5X_API int a5x_load_pbkdf2_hashes(a5x_ctx* ctx, int algo, const uint8_t* text, size_t len, uint64_t* n_targets,
                                   uint64_t* n_salts, uint64_t* n_skipped);
/* The iteration count of index `index` of the context's iterated set (beside a5x_salt_get). */
A5X_API int a5x_salt_iterations(a5x_ctx* ctx, uint32_t index, uint32_t* iters);
/* a5x_format_hits for an iterated set, "original-line:plain\n" (a set given by
 * a5x_set_iterated_targets has no lines: "name:iterations:base64(salt):base64(16 bytes)" is
 * written in their place).  Before a hit is printed the whole derived key is computed again on
 * the host, by the code the kernels run, and compared with every byte the list gave: a hit that
 * matched 16 bytes but not the rest is dropped and counted in *n_dropped (NULL: not wanted). */
A5X_API int a5x_format_hits_iterated(a5x_ctx* ctx, const uint8_t* words, const uint64_t* word_off, uint64_t n_words,
                                     int mode, int min, int max, const a5x_hit* hits, uint64_t n_hits,
                                     const uint32_t* hit_salt, uint64_t* n_dropped, a5x_sink_fn sink, void* user);
/* Pure host: dklen bytes of the PBKDF2 key of algo 72..75, all blocks T1..Tn, by the host path
 * of a5x_pbkdf2.h.  A5X_E_UNSUPPORTED for a candidate over 128 bytes; A5X_E_ARG for iters 0, a
 * salt over 64 bytes or another algo. */
A5X_API int a5x_debug_pbkdf2(int algo, const uint8_t* pass, size_t len, const uint8_t* salt, size_t slen,
                             uint32_t iters, uint8_t* out, size_t dklen);
/* Test hook of the iterated route's slicing: at most pair_slots pair slots per pass and
 * pair_iterations pair-iterations per loop launch from now on (0: the default is kept or
 * restored); *loop_launches (NULL: not wanted) = the loop launches of the context's latest
 * a5x_expand_digest* or a5x_digest_lines_salted_device call on an iterated set. */
A5X_API int a5x_debug_iter_budget(a5x_ctx* ctx, uint64_t pair_slots, uint64_t pair_iterations,
                                  uint64_t* loop_launches);

/* Output byte offset, in the batch's full "cand\n" stream, of each global candidate index
 * cands[i] (cands[i] = the batch's total candidates gives its total bytes; larger: clamped).
 * Device-resident words; the keyspace runs once per call.  Candidate numbering is the one
 * a5x_expand_device's [cand_begin, cand_end) uses. */
A5X_API int a5x_locate_device(a5x_ctx* ctx, const uint8_t* d_words, const uint64_t* d_word_off, uint64_t n_words,
                              int mode, int min, int max, const uint64_t* cands, uint64_t n, uint64_t* byte_off_out,
                              void* stream);
/* Candidate-granular split points for byte targets (a word larger than
 * a rank's share is cut inside, where the reference serialises it on one goroutine,
 * main.go:77-93): for each byte_targets[i] (<= the batch's total bytes), cand_out[i] =
 * the first global candidate whose first output byte is >= the target (the total
 * candidates when none), word_out[i] = the word holding it (n_words when none) and
 * cand_in_word_out[i] = its index inside that word.  Exact (binary search over
 * a5x_locate_device's offsets); the keyspace runs once per call. */
A5X_API int a5x_split_device(a5x_ctx* ctx, const uint8_t* d_words, const uint64_t* d_word_off, uint64_t n_words,
                             int mode, int min, int max, const uint64_t* byte_targets, uint32_t n_targets,
                             uint64_t* cand_out, uint64_t* word_out, uint64_t* cand_in_word_out, void* stream);

/* ---- multi-GPU partition --------------------------------------- */
/* Balanced split of [0, total) for `parts` ranks from an inclusive/exclusive
 * prefix (n+1 entries, e.g. per-word byte offsets): split[r] = first word of
 * rank r, split[parts] = n.  Pure host function. */
A5X_API int a5x_partition(const uint64_t* prefix, uint64_t n, uint32_t parts, uint64_t* split);

/* Diagnostic builds only (compiled with -DA5X_STAMPS): per-phase cycle sums of
 * the fast expansion kernel.  A5X_E_UNSUPPORTED in shipped builds. */
A5X_API int a5x_debug_stamps(unsigned long long* out16, int reset);

/* Test hook (CPU test suite): run the device keyspace classification and the FAST
 * piece plan of ONE word on the host (the same a5x_plan.h code the kernels run)
 * and, for FAST words, replay passes 1-2 of k_expand_fast into out.  info[0..3] =
 * {count, bytes, flags | big pieces << 32 | big entries << 40, bytes written};
 * out = NULL: classification and plan only.  Never called by a5x_expand*: it checks the
 * plan, it is not a compute path. */
A5X_API int a5x_debug_plan_word(a5x_ctx* ctx, const uint8_t* word, size_t len, int min_sub, int max_sub,
                                uint8_t* out, size_t cap, uint64_t* info);

/* Test hook (CPU test suite): the piece-plan sizes of ONE word (<= 64 bytes) from the
 * count-mode planner of the keyspace count pass and from the build-mode planner, which
 * must agree.  out[40]: rows of 8 = {ok, np, ng, ne, maxl, minl, nbig, bent} (past ok = 0:
 * unspecified): row 0 count mode / row 1 build mode with groups of <= 16 entries, rows 2 / 3
 * the same with groups of <= 8; out[32] = the record built from the cached units of one
 * walk (k_keyspace_cplx) against the two-walk record: 1 equal, 0 different, 2 the word does
 * not fit the unit cache, 3 not a FAST word (no record); out[33..39] = 0. */
A5X_API int a5x_debug_plan_sizes(a5x_ctx* ctx, const uint8_t* word, size_t len, uint32_t* out);

/* Test hook (CPU test suite): the record of ONE word (<= 127 bytes) of lone matches as the
 * build pass of k_keyspace_thread writes it (decisions per unit, a group's entries once per
 * piece) against the build-mode planner with groups of <= 8 entries.  out[9]: out[0] = 0 the
 * two records are equal (header, piece descriptors, entries), 1 different, 2 not applicable
 * (overlapping matches, a key index >= 1024, or a unit that an 8-entry group does not take
 * and both planners refuse), 3 not a FAST word and not comparable (more than 8 group
 * pieces; every other word is compared, FAST or not); out[1..8] = units, pieces, group
 * pieces, entries, most units in one group, groups that hold the tail, literal pieces, 1
 * when the word is FAST. */
A5X_API int a5x_debug_piece_build(a5x_ctx* ctx, const uint8_t* word, size_t len, uint32_t* out);

/* Test hook (CPU test suite): ONE word (<= 127 bytes) of lone matches by the cut-once path
 * of k_keyspace_thread -- the count pass that keeps one descriptor per group, then the record
 * built from those descriptors alone, no unit looked at again -- against the count-pass
 * planner it replaces and the build-mode planner with groups of <= 8 entries.
 * out[A5X_CUT_ONCE_OUT]: out[0..8] as a5x_debug_piece_build (0 = records and count-pass fields
 * equal, 1 different, 2 not applicable, 3 not FAST and more than 8 group pieces; "FAST" by the
 * reference planners alone); out[9] = u64 of the record, 0 when none was compared;
 * out[10..18] = ok, np, ng, ne, maxl, minl, nbig, big entries, refused units of the new count
 * pass; out[19..27] = the same of the planner it replaces; out[28] = group pieces of the
 * build-mode planner.  rec_new / rec_ref (A5X_CUT_ONCE_REC u64 each, or null): the record of
 * the new path and of the build-mode planner, zero past their ends. */
#define A5X_CUT_ONCE_OUT 29
#define A5X_CUT_ONCE_REC 1297
A5X_API int a5x_debug_cut_once(a5x_ctx* ctx, const uint8_t* word, size_t len, uint32_t* out, uint64_t* rec_new,
                               uint64_t* rec_ref);

/* Test hook (GPU test suite): how many words of the context's last keyspace pass (any
 * a5x_keyspace* / a5x_expand* call, every mode) k_keyspace_thread could not hold in its
 * per-word unit log (more than 16 lone matches, a match at byte >= 64, a key index
 * >= 1024) and walked with the fused position-synchronous walk, twice, instead of by unit
 * index.  Synchronises the device.  Never called by a compute path. */
A5X_API int a5x_debug_keyspace_refit(a5x_ctx* ctx, uint64_t* out);

/* Test hook (CPU test suite): ONE complex word (<= 127 bytes) by the two paths of
 * k_keyspace_cplx, the lean one (matches by the compact key records, units by index, a
 * record built per piece, clusters included) and the generic unit walk, on the host over
 * the same code.  out[12]: out[0] = 1 the two agree in flags, count, bytes and every u64 of
 * the record (or the word is not the lean path's), 0 they differ; out[1] = why the word is
 * left to the generic path, 0 when the lean path takes it: 1 a key longer than 4 bytes,
 * 2 more than 16 units, 4 a unit at byte >= 64, 8 a key index >= 1024, 16 a cluster of
 * more than 8 matches, more than 16 choices or a choice longer than 7 bytes, 32 more than
 * 2 clusters, 64 a word longer than the kernel's 36-byte word slot (a sum of these; the
 * cluster test runs only when nothing else is set); out[2] = flags, out[3] = a record was
 * built, out[4..5] = count, out[6..7] = bytes, and of a built record out[8] = units, out[9] =
 * clusters | 256 when one group holds two of them, out[10] = group pieces, out[11] = most
 * units in one group. */
A5X_API int a5x_debug_cplx_build(a5x_ctx* ctx, const uint8_t* word, size_t len, int min_sub, int max_sub,
                                 uint32_t* out);

/* Test hook (GPU test suite): out[2] = the words of the context's last keyspace pass that
 * k_keyspace_cplx took by its lean path and by its generic path.  Synchronises the device.
 * Never called by a compute path. */
A5X_API int a5x_debug_keyspace_cplx_lean(a5x_ctx* ctx, uint64_t* out);

/* Test hooks: the word stage of k_keyspace_thread, the LDS bytes that hold a tile's words.
 * The byte walk has two: the large one (8192 B, four workgroups per CU) and a small one sized
 * to the loaded table so that the workgroup takes <= 32,000 B of LDS (25 allocation granules
 * of 1280 B; five workgroups per CU), used by a batch when every one of its 256-word tiles
 * fits it; the choice changes no result.
 * _small_stage: the small stage for the loaded table in bytes, 0 when the table leaves less
 * than 2048 B (not offered; works on a host-only context).  _stage: the stage of the
 * context's last keyspace pass (the large one for a UTF-8 batch walked by lead bytes; 0
 * before any pass or after an empty batch); synchronises the device.  _large_stage(on):
 * on != 0 stops offering the small stage on this context (tests, A/B runs).  Never called by a
 * compute path. */
A5X_API int a5x_debug_keyspace_small_stage(a5x_ctx* ctx, uint32_t* out);
A5X_API int a5x_debug_keyspace_stage(a5x_ctx* ctx, uint32_t* out);
A5X_API int a5x_debug_keyspace_large_stage(a5x_ctx* ctx, int on);

/* Test hook (GPU test suite): the per-word class flags (A5X_WF_* of csrc/a5x_format.h) that the
 * context's last keyspace pass left on the device, out[0, n), n at most the words of that pass
 * (A5X_E_ARG beyond, and before any pass).  A pass that refused the batch (A5X_E_UNSUPPORTED,
 * A5X_E_OVERFLOW) leaves its flags too: the refused words carry A5X_WF_ERR_BIG (with the reason
 * in bits 16..23 and the count columns in 24..31) or A5X_WF_ERR_OVF, the others of the batch
 * whatever the passes that ran before the refusal decided.  After a -r / -s / -s -r pass the
 * flags are those engines': A5X_WF_FAST (with A5X_WF_VIRT / A5X_WF_VFIX and the FAST fields) for
 * a word on the FAST path, A5X_WF_GLOB for a word of mode pass G, A5X_WF_ERR_BIG / A5X_WF_ERR_OVF
 * for one refused by the count pass (a candidate too long is found by the length pass and leaves
 * no bit), 0 otherwise; the class bits RADIX / BIN / GENERAL / BIG / DEFER mean nothing
 * there.  Synchronises the device.  Never called by a compute path. */
A5X_API int a5x_debug_word_flags(a5x_ctx* ctx, uint32_t* out, uint64_t n);

/* Test hook (CPU test suite): the digest of msg[0, len) computed on the host by the
 * __host__ __device__ core the digest kernels run (a5x_sha.h: SHA-1 and the SHA-2 family;
 * a5x_nest.h: the nested algorithms 16..22), a5x_digest_size(algo) bytes into out.
 * A5X_E_ARG for MD5 and NTLM (their cores are device code), for every unassigned value and
 * for the salted nested algorithms 32..38 (salted only: a5x_debug_digest_salted).
 * Never called by a compute path. */
A5X_API int a5x_debug_digest(int algo, const uint8_t* msg, size_t len, uint8_t* out, size_t cap);

/* Test hook (CPU test suite), pure host, no context: the target set a5x_set_targets builds
 * and uploads (the same build_target_set) from n digests of `width` bytes (16, 20, 28, 32, 48
 * or 64), copied out as 32-bit words.  info[8] = {bm_log2, table slots, has_zero, shared
 * (two targets share their first 16 bytes), words of table (4 per slot), words of tails
 * (width / 4 - 4 per slot), words of ztails (the tails of the zero-prefix targets), words of
 * bitmap}.  All four buffers NULL: the size query, info only.  Otherwise table and bitmap,
 * and tails / ztails where their size is not 0, must be given (A5X_E_ARG) with capacities in
 * words of at least info[4..7] (A5X_E_CAPACITY; info is filled either way).  Honours
 * A5X_TARGET_BM_LOG2.  Never called by a compute path. */
A5X_API int a5x_debug_target_set(uint32_t width, const uint8_t* digests, uint64_t n, uint64_t* info, uint32_t* table,
                                 size_t table_cap, uint32_t* tails, size_t tails_cap, uint32_t* ztails,
                                 size_t ztails_cap, uint32_t* bitmap, size_t bitmap_cap);

/* ---- device memory helpers (so hosts without torch can drive the API) ---------- */
A5X_API int a5x_dev_alloc(a5x_ctx* ctx, void** p, size_t bytes);
A5X_API int a5x_dev_free(a5x_ctx* ctx, void* p);
A5X_API int a5x_memcpy_h2d(a5x_ctx* ctx, void* dst, const void* src, size_t bytes);
A5X_API int a5x_memcpy_d2h(a5x_ctx* ctx, void* dst, const void* src, size_t bytes);
A5X_API int a5x_synchronize(a5x_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* A5X_H */
