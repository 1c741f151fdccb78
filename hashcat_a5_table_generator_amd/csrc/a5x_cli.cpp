// a5x_cli.cpp -- `a5x_generator`: C++ replica of the reference CLI (main.go:17-100)
// on top of liba5x.  Same flags (main.go:18-26, kong conventions), same
// "cand\n" stdout format (main.go:66).  Used by tests and benchmarks because the
// Go toolchain is absent here; the Go CLI itself binds liba5x through the cgo
// stub shown in INTEGRATION.md.
//
//   a5x_generator <dict-file> -t <table> [-t <table> ...] [-m N] [-x N]
//                 [--threads N] [-s] [-r] [--device N]
//                 [--hashes <file> [--algo md5|ntlm|sha1|sha224|sha256|sha384|sha512|md5-md5|md5-md5-md5|
//                                          md5-md5up|md5-sha1|sha1-sha1|sha1-md5|sha256-md5|
//                                          md5-md5.salt|md5-salt.md5|md5-md5.md5salt|md5-md5salt.md5|
//                                          sha1-sha1.salt|sha1-salt.sha1|sha1-md5.salt|
//                                          hmac-{md5,sha1,sha256,sha512}-key-{pass,salt}|
//                                          pbkdf2-hmac-{md5,sha1,sha256,sha512}] [--rules <file>]
//                                  [--salted=pass.salt|salt.pass [--hex-salt]]]
//                 [--skip N] [--limit N] [--keyspace]
//
// --hashes (a5x extension): instead of printing the candidates for a
// hashcat pipe (README.MD:69), hash them on the GPU (MD5 / NTLM / SHA-1 / SHA-2 + lookup) against
// the hex digests of <file> and print what hashcat would report, "hash:plain" (plains
// that hashcat would hexify as $HEX[...]), each target once, at its first candidate in
// stream order (README.MD:74-106, :168).
//
// --salted (with --hashes): <file> holds "hash:salt" lines and the digest is over candidate +
// salt (pass.salt; hashcat -m 10 / 110 / 1310 / 1410 / 10810 / 1710) or salt + candidate
// (salt.pass; -m 20 / 120 / 1320 / 1420 / 10820 / 1720); --algo given as one of those mode
// numbers implies it.  Every (hash, salt) target is reported once, at its first candidate in
// stream order, as "hash:salt:plain" (--hex-salt: the salts are hex in the file and in the
// output).  Without --salted a ":suffix" after a hash is ignored, as before.
//
// The salted nested algorithms (md5-md5.salt = hashcat -m 2611 / 2711, md5-salt.md5 = 3710,
// md5-md5.md5salt = 3910, md5-md5salt.md5 = 2811, sha1-sha1.salt = 4510, sha1-salt.sha1 = 4520,
// sha1-md5.salt = 4710) are salted lists by themselves, each with its own order: --salted need
// not be given, and must agree if it is.  The salt printed is the file's own (2811 / 3910 hash
// its MD5 text; the library does that).
//
// So are the HMAC algorithms, hmac-HASH-key-pass (the candidate is the key, the salt the message:
// hashcat -m 50 / 150 / 1450 / 1750 for md5 / sha1 / sha256 / sha512, order pass.salt) and
// hmac-HASH-key-salt (the salt is the key: -m 60 / 160 / 1460 / 1760, order salt.pass).
//
// The PBKDF2 algorithms pbkdf2-hmac-md5 / -sha1 / -sha256 / -sha512 (hashcat -m 11900 / 12000 /
// 10900 / 12100) are iterated lists: <file> holds hashcat's "name:iterations:base64(salt):
// base64(key)" lines, the output is "original-line:plain".  A target matches on the first 16
// bytes of its key on the GPU; before a hit is printed the whole key is derived again on the host,
// and a hit that fails there is dropped and counted on stderr.  --salted, --hex-salt and --rules
// do not apply to them.
//
// --skip / --limit / --keyspace (a5x extension, SURVEY §5 checkpoint / resume): the
// stream's candidate order does not depend on batching (a word's candidates are
// numbered alike in any batch), so a candidate index is a resume cursor: --skip N
// --limit M prints candidates [N, N + M) of the full stream, as hashcat's -s / -l would
// on the pipe; --keyspace prints the number of candidates the run would print.  Whole
// batches before the window cost only their keyspace pass.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "a5x.h"
#include "a5x_gosem.h"

static void usage(FILE* f) {
  fprintf(f,
          "Usage: a5_generator --table-files=TABLE-FILES,... <dict-file> [flags]\n\n"
          "Generates word variations based on a substitution table. v0.2\n\n"
          "Arguments:\n  <dict-file>    Path to dictionary file\n\n"
          "Flags:\n"
          "  -h, --help                        Show context-sensitive help.\n"
          "  -t, --table-files=TABLE-FILES,... Path to substitution table (multiple possible, sequential)\n"
          "  -m, --table-min=0                 Minimum substitutions\n"
          "  -x, --table-max=15                Maximum substitutions\n"
          "      --threads=-1                  Number of threads (accepted; the GPU needs none)\n"
          "  -s, --substitute-all              Substitution Cipher, see Transliteration Attack\n"
          "  -r, --reverse-sub                 Reverse substitution direction\n"
          "      --device=0                    GPU ordinal (a5x extension)\n"
          "      --hashes=FILE                 Crack: print hash:plain for the digests in FILE (a5x extension)\n"
          "      --rules=FILE                  With --hashes: apply every hashcat rule of FILE to each candidate\n"
          "                                    before hashing (hashcat -r; long form only: -r is --reverse-sub)\n"
          "      --algo=md5                    Digest of --hashes: md5 (hashcat -m 0), ntlm (-m 1000),\n"
          "                                    sha1 (-m 100), sha224 (-m 1300), sha256 (-m 1400),\n"
          "                                    sha384 (-m 10800) or sha512 (-m 1700); a name or the -m number;\n"
          "                                    nested, a digest of the hex text of another: md5-md5 (-m 2600),\n"
          "                                    md5-md5-md5 (-m 3500), md5-md5up (-m 4300, upper-case hex),\n"
          "                                    md5-sha1 (-m 4400), sha1-sha1 (-m 4500), sha1-md5 (-m 4700),\n"
          "                                    sha256-md5 (-m 20800); outer-inner, not with --salted;\n"
          "                                    salted nested (FILE holds hash:salt lines, the order is the\n"
          "                                    algorithm's own): md5-md5.salt (-m 2611 / 2711),\n"
          "                                    md5-salt.md5 (-m 3710), md5-md5.md5salt (-m 3910),\n"
          "                                    md5-md5salt.md5 (-m 2811), sha1-sha1.salt (-m 4510),\n"
          "                                    sha1-salt.sha1 (-m 4520), sha1-md5.salt (-m 4710);\n"
          "                                    HMAC (FILE holds hash:salt lines), the candidate as the key:\n"
          "                                    hmac-md5-key-pass (-m 50), hmac-sha1-key-pass (-m 150),\n"
          "                                    hmac-sha256-key-pass (-m 1450), hmac-sha512-key-pass (-m 1750),\n"
          "                                    or the salt as the key: hmac-md5-key-salt (-m 60),\n"
          "                                    hmac-sha1-key-salt (-m 160), hmac-sha256-key-salt (-m 1460),\n"
          "                                    hmac-sha512-key-salt (-m 1760);\n"
          "                                    PBKDF2 (FILE holds name:iterations:base64(salt):base64(key)\n"
          "                                    lines, the output is line:plain): pbkdf2-hmac-md5 (-m 11900),\n"
          "                                    pbkdf2-hmac-sha1 (-m 12000), pbkdf2-hmac-sha256 (-m 10900),\n"
          "                                    pbkdf2-hmac-sha512 (-m 12100); not with --salted, --hex-salt, --rules\n"
          "      --salted=ORDER                With --hashes: FILE holds hash:salt lines; ORDER is pass.salt\n"
          "                                    (hashcat -m 10 / 110 / 1310 / 1410 / 10810 / 1710) or salt.pass\n"
          "                                    (-m 20 / 120 / 1320 / 1420 / 10820 / 1720); --algo also takes\n"
          "                                    those mode numbers, which imply the order\n"
          "      --hex-salt                    With --salted: the salts of FILE are hex-encoded\n"
          "      --skip=0                      Resume: start at candidate N of the stream (a5x extension)\n"
          "      --limit=N                     Print at most N candidates (a5x extension)\n"
          "      --keyspace                    Print the number of candidates and exit (a5x extension)\n");
}

// ---------------------------------------------------------------------------
// Dictionary stream (main.go:52-56, 72-74): bufio.Scanner + ScanLines over the file in
// bounded chunks -- LF split, one trailing CR dropped, a final unterminated line kept,
// and the first line with no '\n' in 64 KiB (bufio.ErrTooLong) silently ends the input,
// as the reference never checks scanner.Err().  At most one chunk of file bytes plus one
// batch per pipeline slot is resident, whatever the dictionary size.
// ---------------------------------------------------------------------------
struct DictStream {
  FILE* f = nullptr;
  std::vector<uint8_t> buf;
  size_t pos = 0, end = 0;
  bool eof = false, stop = false;
  explicit DictStream(FILE* fp, size_t chunk = (size_t)64 << 20) : f(fp), buf(chunk + a5x::gosem::kMaxScanToken) {}
  // keep >= 64 KiB (or the rest of the file) past pos, so a line is cut exactly where
  // the whole-file scanner would cut it
  void fill() {
    if (eof || end - pos >= a5x::gosem::kMaxScanToken) return;
    memmove(buf.data(), buf.data() + pos, end - pos);
    end -= pos;
    pos = 0;
    while (!eof && end < buf.size()) {
      const size_t r = fread(buf.data() + end, 1, buf.size() - end, f);
      if (r == 0) eof = true;
      end += r;
    }
  }
  // the next batch: up to max_words words / about max_bytes bytes (+16 B pad)
  bool next(std::vector<uint8_t>& words, std::vector<uint64_t>& off, uint64_t max_words, size_t max_bytes) {
    words.clear();
    off.assign(1, 0);
    while (!stop && off.size() - 1 < max_words && words.size() < max_bytes) {
      fill();
      const uint8_t* line;
      size_t len;
      const int r = a5x::gosem::scan_line(buf.data(), end, &pos, &line, &len);
      if (r <= 0) { stop = true; break; }  // EOF, or ErrTooLong (silently the end, main.go:73)
      words.insert(words.end(), line, line + len);
      off.push_back(words.size());
    }
    words.resize(words.size() + 16, 0);
    return off.size() > 1;
  }
};

// ---------------------------------------------------------------------------
// Batch pipeline: two liba5x contexts on the device, each driven by its own thread,
// take alternate batches; batch k + 1's upload, keyspace and first range run while
// batch k's output is still streaming to stdout.  Output stays in batch order: a
// batch's sink waits for its turn (the reference's order across words is arbitrary,
// main.go:77, but a deterministic stream is easier to check).
// ---------------------------------------------------------------------------
struct Turn {
  std::mutex mu;
  std::condition_variable cv;
  uint64_t turn = 0;
  void wait(uint64_t k) {
    std::unique_lock<std::mutex> l(mu);
    cv.wait(l, [&] { return turn == k; });
  }
  void done(uint64_t k) {
    std::lock_guard<std::mutex> l(mu);
    turn = k + 1;
    cv.notify_all();
  }
};

// host timeline (A5X_CLI_TIMELINE=1): milliseconds since main() per event, to stderr
static const auto g_t0 = std::chrono::steady_clock::now();
static bool g_tl = false;
static double ms_now() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_t0).count();
}
#define TL(...)                                \
  do {                                         \
    if (g_tl) {                                \
      fprintf(stderr, "[tl %9.2f] ", ms_now()); \
      fprintf(stderr, __VA_ARGS__);            \
      fputc('\n', stderr);                     \
    }                                          \
  } while (0)

struct SinkCtx {
  Turn* t;
  uint64_t k;
  bool waited;
  const std::atomic<int>* failed;  // a failed earlier batch: write nothing more
  uint64_t bytes;
};

static int sink_ordered(void* user, const uint8_t* data, size_t len) {
  SinkCtx* s = (SinkCtx*)user;
  if (!s->waited) {
    TL("batch %llu: first range ready, waiting for its turn", (unsigned long long)s->k);
    s->t->wait(s->k);
    TL("batch %llu: streaming", (unsigned long long)s->k);
    s->waited = true;
  }
  if (s->failed->load()) return 1;
  s->bytes += len;
  return fwrite(data, 1, len, stdout) == len ? 0 : 1;
}

static int sink_stdout(void* user, const uint8_t* data, size_t len) {
  (void)user;
  return fwrite(data, 1, len, stdout) == len ? 0 : 1;
}

static int hexv(int c) {
  return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
}

// target digests: one hex digest per line (2 * a5x_digest_size(algo) hex digits: 32 to
// 128; anything after them, e.g. a
// ":plain" of a potfile line, is ignored); other lines are counted and skipped.  Whole
// lines of any length (getline): a long potfile plain is one line, never a continuation
// piece read as a target.
static int load_targets(a5x_ctx* ctx, const char* path, int algo) {
  FILE* f = fopen(path, "rb");
  if (!f) return A5X_E_IO;
  std::vector<uint8_t> dig;
  char* line = nullptr;
  size_t cap = 0;
  ssize_t n;
  uint64_t bad = 0;
  const int dsz = a5x_digest_size(algo);
  if (dsz <= 0 || dsz > 64) { fclose(f); return a5x_set_targets(ctx, algo, nullptr, 0); }  // (reports the bad algorithm)
  const size_t nhex = 2 * (size_t)dsz;
  while ((n = getline(&line, &cap, f)) >= 0) {
    size_t k = 0;
    uint8_t d[64];
    for (; k < nhex && k < (size_t)n; k++) {
      const int v = hexv((unsigned char)line[k]);
      if (v < 0) break;
      if (k & 1) d[k / 2] |= (uint8_t)v; else d[k / 2] = (uint8_t)(v << 4);
    }
    const char t = (size_t)n > nhex ? line[nhex] : 0;
    if (k == nhex && (t == 0 || t == '\n' || t == '\r' || t == ':')) dig.insert(dig.end(), d, d + dsz);
    else if (n > 0 && line[0] != '\n' && line[0] != '\r') bad++;
  }
  free(line);
  fclose(f);
  if (bad) fprintf(stderr, "a5_generator: %llu line(s) of %s are not %zu-hex-digit hashes (skipped)\n",
                   (unsigned long long)bad, path, nhex);
  return a5x_set_targets(ctx, algo, dig.empty() ? nullptr : dig.data(), dig.size() / (size_t)dsz);
}

// --salted: the whole "hash:salt" file through a5x_load_salted_hashes
static int load_salted_targets(a5x_ctx* ctx, const char* path, int algo, int order, bool hex_salt) {
  FILE* f = fopen(path, "rb");
  if (!f) return A5X_E_IO;
  std::vector<uint8_t> text;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.insert(text.end(), buf, buf + n);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) return A5X_E_IO;
  uint64_t nt = 0, ns = 0, nsk = 0;
  const int rc = a5x_load_salted_hashes(ctx, algo, order, text.data(), text.size(), hex_salt ? 1 : 0, &nt, &ns, &nsk);
  if (rc == 0)
    fprintf(stderr, "a5_generator: salted: %llu target(s), %llu distinct salt(s), %llu line(s) skipped (not hash:salt)\n",
            (unsigned long long)nt, (unsigned long long)ns, (unsigned long long)nsk);
  return rc;
}

// a PBKDF2 --algo: the whole "name:iterations:base64(salt):base64(key)" file through a5x_load_pbkdf2_hashes
static int load_pbkdf2_targets(a5x_ctx* ctx, const char* path, int algo) {
  FILE* f = fopen(path, "rb");
  if (!f) return A5X_E_IO;
  std::vector<uint8_t> text;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.insert(text.end(), buf, buf + n);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) return A5X_E_IO;
  uint64_t nt = 0, ns = 0, nsk = 0;
  const int rc = a5x_load_pbkdf2_hashes(ctx, algo, text.data(), text.size(), &nt, &ns, &nsk);
  if (rc == 0)
    fprintf(stderr, "a5_generator: iterated: %llu target(s), %llu distinct (salt, iterations) pair(s), %llu line(s) skipped "
                    "(not name:iterations:base64:base64 of this algorithm)\n",
            (unsigned long long)nt, (unsigned long long)ns, (unsigned long long)nsk);
  return rc;
}

static int sink_string(void* user, const uint8_t* p, size_t n) {
  ((std::string*)user)->append((const char*)p, n);
  return 0;
}

static bool parse_u64(const char* s, uint64_t* out) {
  char* e;
  errno = 0;
  // digits only: strtoull would skip leading blanks and negate a '-' (" -3" -> 2^64 - 3)
  if (*s < '0' || *s > '9') return false;
  const unsigned long long v = strtoull(s, &e, 10);
  if (*e || errno) return false;
  *out = v;
  return true;
}

static bool parse_int(const char* s, int* out) {
  char* e;
  long v = strtol(s, &e, 10);
  if (!*s || *e) return false;
  *out = (int)v;
  return true;
}

// --skip / --limit / --keyspace: one context, batches in order; each batch's keyspace
// gives its candidate total T, so the window [skip, skip + limit) maps to a candidate
// range of the batches it meets (a5x_expand_range), and the batches past it are not read.
static int run_cursor(const std::string& dict, const std::vector<std::string>& tables, int device, int mode, int tmin,
                      int tmax, uint64_t B, size_t BB, size_t chunk, uint64_t skip, uint64_t limit, bool keyspace_only) {
  a5x_ctx* ctx = nullptr;
  int rc = a5x_create(device, &ctx);
  if (rc) { fprintf(stderr, "a5_generator: no usable GPU (a5x_create=%d)\n", rc); return 1; }
  for (auto& t : tables)
    if ((rc = a5x_load_table_file(ctx, t.c_str()))) {
      fprintf(stderr, "%s\n", a5x_last_error(ctx));  // log.Fatal (main.go:43-45)
      a5x_destroy(ctx);
      return 1;
    }
  FILE* f = fopen(dict.c_str(), "rb");
  if (!f) { perror(dict.c_str()); a5x_destroy(ctx); return 1; }
  const uint64_t end = limit > ~0ull - skip ? ~0ull : skip + limit;  // (saturating)
  DictStream ds(f, chunk);
  std::vector<uint8_t> words;
  std::vector<uint64_t> off, cnt;
  uint64_t G = 0;  // stream candidates before this batch
  bool ovf = false;
  while (rc == 0 && (keyspace_only || G < end) && ds.next(words, off, B, BB)) {
    const uint64_t nb = off.size() - 1;
    cnt.assign(nb, 0);
    if ((rc = a5x_keyspace(ctx, words.data(), off.data(), nb, mode, tmin, tmax, cnt.data(), nullptr))) break;
    uint64_t T = 0;
    for (uint64_t x : cnt) {
      ovf |= T + x < T;
      T += x;
    }
    if (!keyspace_only) {
      const uint64_t lo = skip > G ? std::min(T, skip - G) : 0, hi = end - G < T ? end - G : T;
      if (lo < hi)
        rc = a5x_expand_range(ctx, words.data(), off.data(), nb, mode, tmin, tmax, lo, hi, sink_stdout, nullptr,
                              nullptr);
    }
    ovf |= G + T < G;
    G += T;
  }
  fclose(f);
  if (rc == 0 && keyspace_only) {
    if (ovf) { fprintf(stderr, "a5_generator: the keyspace exceeds 2^64 - 1 candidates\n"); rc = A5X_E_OVERFLOW; }
    else printf("%llu\n", (unsigned long long)G);
  }
  if (fflush(stdout) != 0 || ferror(stdout)) {
    if (!rc) fprintf(stderr, "a5_generator: writing stdout: %s\n", strerror(errno));
    rc = rc ? rc : 1;
  } else if (rc && rc != A5X_E_OVERFLOW) {
    fprintf(stderr, "a5_generator: %s\n", a5x_last_error(ctx));
  }
  a5x_destroy(ctx);
  return rc ? 2 : 0;
}

int main(int argc, char** argv) {
  std::vector<std::string> tables;
  std::string dict;
  int tmin = 0, tmax = 15, threads = -1, device = 0, algo = A5X_ALGO_MD5;
  std::string hashes, rules, salted;
  int mode_order = -1;  // the order a hashcat mode number given as --algo implies
  bool hex_salt = false;
  bool suball = false, rev = false, keyspace_only = false, cursor = false;
  uint64_t skip = 0, limit = ~0ull;
  auto need = [&](int& i, const char* flag) -> const char* {
    if (i + 1 >= argc) {
      fprintf(stderr, "a5_generator: error: %s: expected value\n", flag);
      usage(stderr);
      exit(80);
    }
    return argv[++i];
  };
  auto add_tables = [&](const char* v) {  // kong []string flags split on ','
    std::string s(v);
    size_t p = 0;
    while (true) {
      size_t q = s.find(',', p);
      tables.push_back(s.substr(p, q == std::string::npos ? std::string::npos : q - p));
      if (q == std::string::npos) break;
      p = q + 1;
    }
  };
  for (int i = 1; i < argc; i++) {
    const char* a = argv[i];
    std::string s(a);
    auto val_of = [&](const char* flag) -> const char* {
      size_t eq = s.find('=');
      if (eq != std::string::npos) return a + eq + 1;
      return need(i, flag);
    };
    int v;
    if (s == "-h" || s == "--help") { usage(stdout); return 0; }
    else if (s == "-t" || s.rfind("--table-files", 0) == 0) add_tables(val_of("--table-files"));
    else if (s == "-m" || s.rfind("--table-min", 0) == 0) {
      if (!parse_int(val_of("--table-min"), &v)) { fprintf(stderr, "a5_generator: error: --table-min: bad int\n"); return 80; }
      tmin = v;
    } else if (s == "-x" || s.rfind("--table-max", 0) == 0) {
      if (!parse_int(val_of("--table-max"), &v)) { fprintf(stderr, "a5_generator: error: --table-max: bad int\n"); return 80; }
      tmax = v;
    } else if (s.rfind("--threads", 0) == 0) {
      if (!parse_int(val_of("--threads"), &v)) { fprintf(stderr, "a5_generator: error: --threads: bad int\n"); return 80; }
      threads = v;
    } else if (s.rfind("--device", 0) == 0) {
      if (!parse_int(val_of("--device"), &v)) { fprintf(stderr, "a5_generator: error: --device: bad int\n"); return 80; }
      device = v;
    } else if (s.rfind("--hashes", 0) == 0) {
      hashes = val_of("--hashes");
    } else if (s.rfind("--rules", 0) == 0) {
      rules = val_of("--rules");
    } else if (s.rfind("--algo", 0) == 0) {
      std::string v = val_of("--algo");
      if (v == "md5" || v == "0") algo = A5X_ALGO_MD5;
      else if (v == "ntlm" || v == "1000") algo = A5X_ALGO_NTLM;
      else if (v == "sha1" || v == "100") algo = A5X_ALGO_SHA1;
      else if (v == "sha256" || v == "1400") algo = A5X_ALGO_SHA256;
      else if (v == "sha224" || v == "1300") algo = A5X_ALGO_SHA224;
      else if (v == "sha384" || v == "10800") algo = A5X_ALGO_SHA384;
      else if (v == "sha512" || v == "1700") algo = A5X_ALGO_SHA512;
      else if (v == "10" || v == "20") { algo = A5X_ALGO_MD5; mode_order = v == "20"; }
      else if (v == "110" || v == "120") { algo = A5X_ALGO_SHA1; mode_order = v == "120"; }
      else if (v == "1310" || v == "1320") { algo = A5X_ALGO_SHA224; mode_order = v == "1320"; }
      else if (v == "1410" || v == "1420") { algo = A5X_ALGO_SHA256; mode_order = v == "1420"; }
      else if (v == "1710" || v == "1720") { algo = A5X_ALGO_SHA512; mode_order = v == "1720"; }
      else if (v == "10810" || v == "10820") { algo = A5X_ALGO_SHA384; mode_order = v == "10820"; }
      else if (v == "md5-md5" || v == "2600") algo = A5X_ALGO_MD5_MD5;
      else if (v == "md5-md5-md5" || v == "3500") algo = A5X_ALGO_MD5_MD5_MD5;
      else if (v == "md5-md5up" || v == "4300") algo = A5X_ALGO_MD5_MD5UP;
      else if (v == "md5-sha1" || v == "4400") algo = A5X_ALGO_MD5_SHA1;
      else if (v == "sha1-sha1" || v == "4500") algo = A5X_ALGO_SHA1_SHA1;
      else if (v == "sha1-md5" || v == "4700") algo = A5X_ALGO_SHA1_MD5;
      else if (v == "sha256-md5" || v == "20800") algo = A5X_ALGO_SHA256_MD5;
      else if (v == "md5-md5.salt" || v == "2611" || v == "2711") algo = A5X_ALGO_MD5_MD5_SALT;
      else if (v == "md5-salt.md5" || v == "3710") algo = A5X_ALGO_MD5_SALT_MD5;
      else if (v == "md5-md5.md5salt" || v == "3910") algo = A5X_ALGO_MD5_MD5_MD5SALT;
      else if (v == "md5-md5salt.md5" || v == "2811") algo = A5X_ALGO_MD5_MD5SALT_MD5;
      else if (v == "sha1-sha1.salt" || v == "4510") algo = A5X_ALGO_SHA1_SHA1_SALT;
      else if (v == "sha1-salt.sha1" || v == "4520") algo = A5X_ALGO_SHA1_SALT_SHA1;
      else if (v == "sha1-md5.salt" || v == "4710") algo = A5X_ALGO_SHA1_MD5_SALT;
      else if (v == "hmac-md5-key-pass" || v == "50") algo = A5X_ALGO_HMAC_MD5_KEY_PASS;
      else if (v == "hmac-md5-key-salt" || v == "60") algo = A5X_ALGO_HMAC_MD5_KEY_SALT;
      else if (v == "hmac-sha1-key-pass" || v == "150") algo = A5X_ALGO_HMAC_SHA1_KEY_PASS;
      else if (v == "hmac-sha1-key-salt" || v == "160") algo = A5X_ALGO_HMAC_SHA1_KEY_SALT;
      else if (v == "hmac-sha256-key-pass" || v == "1450") algo = A5X_ALGO_HMAC_SHA256_KEY_PASS;
      else if (v == "hmac-sha256-key-salt" || v == "1460") algo = A5X_ALGO_HMAC_SHA256_KEY_SALT;
      else if (v == "hmac-sha512-key-pass" || v == "1750") algo = A5X_ALGO_HMAC_SHA512_KEY_PASS;
      else if (v == "hmac-sha512-key-salt" || v == "1760") algo = A5X_ALGO_HMAC_SHA512_KEY_SALT;
      else if (v == "pbkdf2-hmac-md5" || v == "11900") algo = A5X_ALGO_PBKDF2_HMAC_MD5;
      else if (v == "pbkdf2-hmac-sha1" || v == "12000") algo = A5X_ALGO_PBKDF2_HMAC_SHA1;
      else if (v == "pbkdf2-hmac-sha256" || v == "10900") algo = A5X_ALGO_PBKDF2_HMAC_SHA256;
      else if (v == "pbkdf2-hmac-sha512" || v == "12100") algo = A5X_ALGO_PBKDF2_HMAC_SHA512;
      else {
        fprintf(stderr, "a5_generator: error: --algo: md5, ntlm, sha1, sha224, sha256, sha384 or sha512, or nested:\n"
                        "md5-md5, md5-md5-md5, md5-md5up, md5-sha1, sha1-sha1, sha1-md5 or sha256-md5, or salted nested:\n"
                        "md5-md5.salt, md5-salt.md5, md5-md5.md5salt, md5-md5salt.md5, sha1-sha1.salt, sha1-salt.sha1\n"
                        "or sha1-md5.salt, or HMAC: hmac-md5-key-pass, hmac-md5-key-salt, hmac-sha1-key-pass, hmac-sha1-key-salt,\n"
                        "hmac-sha256-key-pass, hmac-sha256-key-salt, hmac-sha512-key-pass or hmac-sha512-key-salt, or PBKDF2:\n"
                        "pbkdf2-hmac-md5, pbkdf2-hmac-sha1, pbkdf2-hmac-sha256 or pbkdf2-hmac-sha512\n");
        return 80;
      }
      // (a salted nested or HMAC algorithm implies a salted list in its own order, as a salted mode number does)
      // (so does a PBKDF2 algorithm: order 0, its hits carry the index of their (salt, iterations) pair)
      if (a5x_algo_salt_order(algo) >= 0) mode_order = a5x_algo_salt_order(algo);
    } else if (s.rfind("--salted", 0) == 0) {
      salted = val_of("--salted");
      if (salted != "pass.salt" && salted != "salt.pass") {
        fprintf(stderr, "a5_generator: error: --salted: pass.salt or salt.pass\n");
        return 80;
      }
    } else if (s == "--hex-salt") {
      hex_salt = true;
    } else if (s.rfind("--skip", 0) == 0) {
      if (!parse_u64(val_of("--skip"), &skip)) { fprintf(stderr, "a5_generator: error: --skip: bad count\n"); return 80; }
      cursor = true;
    } else if (s.rfind("--limit", 0) == 0) {
      if (!parse_u64(val_of("--limit"), &limit)) { fprintf(stderr, "a5_generator: error: --limit: bad count\n"); return 80; }
      cursor = true;
    } else if (s == "--keyspace") keyspace_only = true;
    else if (s == "--substitute-all") suball = true;
    else if (s == "--reverse-sub") rev = true;
    else if (s.size() > 1 && s[0] == '-' && s[1] != '-') {
      bool ok = true;  // combined boolean shorts, e.g. -sr
      for (size_t k = 1; k < s.size(); k++) {
        if (s[k] == 's') suball = true;
        else if (s[k] == 'r') rev = true;
        else ok = false;
      }
      if (!ok) { fprintf(stderr, "a5_generator: error: unknown flag %s\n", a); usage(stderr); return 80; }
    } else if (dict.empty()) dict = s;
    else { fprintf(stderr, "a5_generator: error: unexpected argument %s\n", a); usage(stderr); return 80; }
  }
  (void)threads;
  if (tables.empty()) { fprintf(stderr, "a5_generator: error: missing flags: --table-files=TABLE-FILES,...\n"); usage(stderr); return 80; }
  if (dict.empty()) { fprintf(stderr, "a5_generator: error: expected \"<dict-file>\"\n"); usage(stderr); return 80; }

  g_tl = getenv("A5X_CLI_TIMELINE") != nullptr;
  TL("main");
  const int mode = (suball ? A5X_MODE_SUBALL : A5X_MODE_DEFAULT) + (rev ? 1 : 0);
  uint64_t B = 1u << 22;           // words per batch
  size_t BB = (size_t)64 << 20;    // word bytes per batch
  size_t chunk = (size_t)64 << 20; // dictionary bytes read at a time
  // (test hooks: small batches / chunks exercise the pipeline and the chunk edges)
  if (const char* e = getenv("A5X_CLI_BATCH")) B = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
  if (const char* e = getenv("A5X_CLI_CHUNK")) chunk = std::max<size_t>(1, strtoull(e, nullptr, 10));
  static char obuf[1 << 22];
  setvbuf(stdout, obuf, _IOFBF, sizeof obuf);
  if (!rules.empty() && hashes.empty()) {
    fprintf(stderr, "a5_generator: error: --rules applies to the digest + lookup stage: it needs --hashes\n");
    return 80;
  }
  const bool iterated = algo >= A5X_ALGO_PBKDF2_HMAC_MD5 && algo <= A5X_ALGO_PBKDF2_HMAC_SHA512;
  if (iterated && (!salted.empty() || hex_salt)) {
    fprintf(stderr, "a5_generator: error: --salted / --hex-salt with a PBKDF2 --algo: its list holds\n"
                    "name:iterations:base64(salt):base64(key) lines, the salt is part of each line and always base64\n");
    return 80;
  }
  if (iterated && !rules.empty()) {
    fprintf(stderr, "a5_generator: error: --rules with a PBKDF2 --algo: rules and iterated lists together are not supported\n");
    return 80;
  }
  int order = -1;  // >= 0: the --hashes list is salted
  if (!salted.empty()) order = salted == "salt.pass";
  if (mode_order >= 0) {
    if (order >= 0 && order != mode_order) {
      fprintf(stderr, "a5_generator: error: --salted=%s contradicts the hashcat mode given as --algo\n", salted.c_str());
      return 80;
    }
    order = mode_order;
  }
  if ((order >= 0 || hex_salt) && hashes.empty()) {
    fprintf(stderr, "a5_generator: error: --salted / --hex-salt / a salted hashcat mode apply to --hashes\n");
    return 80;
  }
  if (hex_salt && order < 0) {
    fprintf(stderr, "a5_generator: error: --hex-salt needs --salted\n");
    return 80;
  }
  if (order >= 0 && !rules.empty()) {
    fprintf(stderr, "a5_generator: error: --salted with --rules: rules and salts together are not supported\n");
    return 80;
  }
  if (order >= 0 && algo == A5X_ALGO_NTLM) {
    fprintf(stderr, "a5_generator: error: --salted with --algo ntlm: NTLM has no salted mode\n");
    return 80;
  }
  if (order >= 0 && algo >= A5X_ALGO_MD5_MD5 && algo <= A5X_ALGO_SHA256_MD5) {
    fprintf(stderr, "a5_generator: error: --salted with a nested --algo: the nested digests have no salted mode here\n"
                    "(the salted nested forms are algorithms of their own: --algo 2611, 3710, 3910, 2811, 4510, 4520, 4710)\n");
    return 80;
  }
  if (!hashes.empty() && (cursor || keyspace_only)) {
    fprintf(stderr, "a5_generator: error: --skip / --limit / --keyspace select the candidate stream, not --hashes\n");
    return 80;
  }
  if (hashes.empty() && (cursor || keyspace_only)) return run_cursor(dict, tables, device, mode, tmin, tmax, B, BB, chunk,
                                                                     skip, limit, keyspace_only);
  if (hashes.empty()) {
    // The stdout pipeline.  The GPU contexts are created (and their stream buffers made)
    // on a second thread while this one reads the first batch, which is small so output
    // starts early; two contexts on two threads then take alternate batches and write
    // them in batch order.
    a5x_ctx* cx[2] = {nullptr, nullptr};
    int irc[2] = {0, 0};
    std::string ierr[2];
    auto make_ctx = [&](int i) {
      irc[i] = a5x_create(device, &cx[i]);
      if (irc[i]) {
        char m[96];
        snprintf(m, sizeof m, "a5_generator: no usable GPU (a5x_create=%d)", irc[i]);
        ierr[i] = m;
        return;
      }
      for (size_t t = 0; irc[i] == 0 && t < tables.size(); t++) {
        irc[i] = a5x_load_table_file(cx[i], tables[t].c_str());
        if (irc[i]) ierr[i] = a5x_last_error(cx[i]);  // log.Fatal (main.go:43-45)
      }
      if (irc[i] == 0) (void)a5x_stream_reserve(cx[i], B, BB);  // (optional warm-up)
      TL("context %d ready", i + 1);
    };
    std::thread init0(make_ctx, 0), init1(make_ctx, 1);
    // the first two batches (the first one small, so output starts early) are read while
    // the runtime and the contexts come up
    FILE* f = fopen(dict.c_str(), "rb");
    DictStream ds(f, chunk);
    std::vector<uint8_t> pw[2];
    std::vector<uint64_t> po[2];
    int npre = 0;
    if (f && ds.next(pw[0], po[0], std::max<uint64_t>(1, B / 16), BB / 16)) npre = 1;
    if (npre == 1 && ds.next(pw[1], po[1], B, BB)) npre = 2;
    TL("first batches read (%d)", npre);
    init0.join();
    init1.join();
    for (int i = 0; i < 2; i++)
      if (irc[i]) {  // the tables are read before the dictionary is opened (main.go:40-56)
        fprintf(stderr, "%s\n", ierr[i].c_str());
        if (f) fclose(f);
        return 1;
      }
    if (!f) { perror(dict.c_str()); return 1; }
    int rc = 0;
    Turn turn;
    std::mutex qmu;
    std::condition_variable qcv;
    std::deque<std::pair<uint64_t, std::pair<std::vector<uint8_t>, std::vector<uint64_t>>>> q[2];
    bool done_reading = false;
    std::atomic<int> failed{0};  // first error code (later batches are skipped)
    std::string emsg;
    auto worker = [&](int w) {
      for (;;) {
        std::pair<uint64_t, std::pair<std::vector<uint8_t>, std::vector<uint64_t>>> job;
        {
          std::unique_lock<std::mutex> l(qmu);
          qcv.wait(l, [&] { return !q[w].empty() || done_reading; });
          if (q[w].empty()) return;
          job = std::move(q[w].front());
          q[w].pop_front();
          qcv.notify_all();
        }
        const uint64_t k = job.first;
        auto& words = job.second.first;
        auto& off = job.second.second;
        SinkCtx sc{&turn, k, false, &failed, 0};
        TL("batch %llu: ctx %d starts (%zu words)", (unsigned long long)k, w, off.size() - 1);
        int r = failed.load() ? 0 : a5x_expand(cx[w], words.data(), off.data(), off.size() - 1, mode, tmin,
                                               tmax, sink_ordered, &sc, nullptr);
        if (!sc.waited) turn.wait(k);  // (a batch with no output still takes its turn)
        if (r == A5X_E_SINK && failed.load()) r = 0;  // stopped by an earlier batch's failure
        TL("batch %llu: done, %llu bytes", (unsigned long long)k, (unsigned long long)sc.bytes);
        int zero = 0;
        if (r && failed.compare_exchange_strong(zero, r)) emsg = a5x_last_error(cx[w]);
        turn.done(k);
      }
    };
    std::thread th0(worker, 0), th1(worker, 1);
    for (uint64_t k = 0;; k++) {
      std::vector<uint8_t> words;
      std::vector<uint64_t> off;
      if (k < 2) {
        if ((int)k >= npre) break;
        words.swap(pw[k]);
        off.swap(po[k]);
      } else {
        words.reserve(BB + 16 + (1 << 16));
        off.reserve(std::min<uint64_t>(B, 1u << 24) + 1);
        if (!ds.next(words, off, B, BB)) break;
        TL("batch %llu read (%zu words)", (unsigned long long)k, off.size() - 1);
      }
      std::unique_lock<std::mutex> l(qmu);
      qcv.wait(l, [&] { return q[k & 1].empty() || failed.load(); });  // one batch ahead per context
      if (failed.load()) break;
      q[k & 1].emplace_back(k, std::make_pair(std::move(words), std::move(off)));
      qcv.notify_all();
    }
    {
      std::lock_guard<std::mutex> l(qmu);
      done_reading = true;
      qcv.notify_all();
    }
    th0.join();
    th1.join();
    rc = failed.load();
    fclose(f);
    if (fflush(stdout) != 0 || ferror(stdout)) {  // (ENOSPC / EPIPE on the last buffer: not a success)
      if (!rc) emsg = std::string("writing stdout: ") + strerror(errno);
      rc = 1;
    }
    TL("all batches written");
    if (rc) fprintf(stderr, "a5_generator: %s\n", emsg.c_str());
    fflush(stderr);
    // (every device call has completed; the process's GPU state goes with it -- tearing
    // the two contexts down first only costs time)
    _exit(rc ? 2 : 0);
  }
  a5x_ctx* ctx = nullptr;
  int rc = a5x_create(device, &ctx);
  TL("context 1 created");
  if (rc) { fprintf(stderr, "a5_generator: no usable GPU (a5x_create=%d)\n", rc); return 1; }
  for (auto& t : tables) {
    rc = a5x_load_table_file(ctx, t.c_str());
    if (rc) { fprintf(stderr, "%s\n", a5x_last_error(ctx)); a5x_destroy(ctx); return 1; }  // log.Fatal
  }
  FILE* f = fopen(dict.c_str(), "rb");
  if (!f) { perror(dict.c_str()); a5x_destroy(ctx); return 1; }
  if ((rc = iterated ? load_pbkdf2_targets(ctx, hashes.c_str(), algo)
            : order >= 0 ? load_salted_targets(ctx, hashes.c_str(), algo, order, hex_salt) : load_targets(ctx, hashes.c_str(), algo))) {
    fprintf(stderr, "a5_generator: %s\n", rc == A5X_E_IO ? "cannot read --hashes file" : a5x_last_error(ctx));
    a5x_destroy(ctx);
    fclose(f);
    return 1;
  }
  uint64_t rejected = 0;
  if (!rules.empty()) {
    uint32_t nr = 0, nsk = 0;
    if ((rc = a5x_load_rules_file(ctx, rules.c_str(), &nr, &nsk))) {
      fprintf(stderr, "a5_generator: %s\n", rc == A5X_E_IO ? "cannot read --rules file" : a5x_last_error(ctx));
      a5x_destroy(ctx);
      fclose(f);
      return 1;
    }
    fprintf(stderr, "a5_generator: rules: %u accepted, %u line(s) skipped (unsupported or malformed)\n", nr, nsk);
    if (!nr) {
      fprintf(stderr, "a5_generator: error: no usable rule in %s\n", rules.c_str());
      a5x_destroy(ctx);
      fclose(f);
      return 1;
    }
  }
  const bool ruled = !rules.empty();
  const bool with_salts = order >= 0;
  uint64_t skipped_pairs = 0, dropped_hits = 0;
  DictStream ds(f, chunk);
  std::vector<uint8_t> words;
  std::vector<uint64_t> sub;
  std::vector<a5x_hit> hits(1 << 16);
  std::unordered_set<std::string> cracked;  // each target reported once (hashcat potfile)
  while (rc == 0 && ds.next(words, sub, B, BB)) {
    const uint64_t nb = sub.size() - 1;
    const uint8_t* wb = words.data();
    uint64_t nh = 0;
    rc = a5x_expand_digest(ctx, wb, sub.data(), nb, mode, tmin, tmax, hits.data(), hits.size(), &nh, nullptr);
    if (rc == A5X_E_CAPACITY && nh > hits.size()) {
      hits.resize(nh);
      rc = a5x_expand_digest(ctx, wb, sub.data(), nb, mode, tmin, tmax, hits.data(), hits.size(), &nh, nullptr);
    }
    if (rc) break;
    std::vector<uint32_t> hrule(nh, 0u);  // ruled: each hit's rule, carried through the sort
    if (ruled) {
      uint64_t nr = 0, rej = 0;
      if ((rc = a5x_hit_rules(ctx, hrule.data(), hrule.size(), &nr)) || (rc = a5x_rules_last(ctx, nullptr, &rej))) break;
      rejected += rej;
    }
    if (with_salts) {  // (hrule carries each hit's salt index: a list is ruled or salted, never both)
      uint64_t ns = 0, skp = 0;
      if ((rc = a5x_hit_salts(ctx, hrule.data(), hrule.size(), &ns)) || (rc = a5x_salts_last(ctx, nullptr, &skp))) break;
      skipped_pairs += skp;
    }
    // stream order (then rule order), then the first candidate of each digest
    std::vector<uint64_t> ord(nh);
    for (uint64_t h = 0; h < nh; h++) ord[h] = h;
    std::sort(ord.begin(), ord.end(), [&](uint64_t x, uint64_t y) {
      if (hits[x].word != hits[y].word) return hits[x].word < hits[y].word;
      if (hits[x].cand != hits[y].cand) return hits[x].cand < hits[y].cand;
      return hrule[x] < hrule[y];
    });
    std::vector<a5x_hit> first;
    std::vector<uint32_t> first_rule;
    for (uint64_t k = 0; k < nh && rc == 0; k++) {  // keyed on the full digest (20 to 64 bytes for the wide algorithms)
      const uint64_t h = ord[k];
      uint8_t full[64];
      size_t fl = 0;
      if ((rc = a5x_hit_digest(ctx, &hits[h], full, sizeof full, &fl))) break;
      std::string key((const char*)full, fl);
      if (with_salts) key.append((const char*)&hrule[h], 4);  // a target is a (hash, salt) pair
      // (an iterated list: a hit on 16 bytes may still be dropped, so every hit goes to the check
      // below and the lines that come out of it are deduplicated)
      if (iterated || cracked.insert(key).second) {
        first.push_back(hits[h]);
        first_rule.push_back(hrule[h]);
      }
    }
    if (rc) break;
    if (iterated) {
      std::string text;
      uint64_t drop = 0;
      rc = a5x_format_hits_iterated(ctx, wb, sub.data(), nb, mode, tmin, tmax, first.data(), first.size(), first_rule.data(),
                                    &drop, sink_string, &text);
      dropped_hits += drop;
      for (size_t p0 = 0; rc == 0 && p0 < text.size();) {
        const size_t e = text.find('\n', p0);
        size_t k = p0;  // the target: the list's line, which has three ':' (base64 has none)
        for (int colons = 0; k < e && colons < 4; k++) colons += text[k] == ':';
        if (cracked.insert(text.substr(p0, k - p0)).second) fwrite(text.data() + p0, 1, e + 1 - p0, stdout);
        p0 = e + 1;
      }
    } else if (with_salts)
      rc = a5x_format_hits_salted(ctx, wb, sub.data(), nb, mode, tmin, tmax, first.data(), first.size(),
                                  first_rule.data(), hex_salt ? 1 : 0, sink_stdout, nullptr);
    else if (ruled)
      rc = a5x_format_hits_rules(ctx, wb, sub.data(), nb, mode, tmin, tmax, first.data(), first.size(),
                                 first_rule.data(), sink_stdout, nullptr);
    else
      rc = a5x_format_hits(ctx, wb, sub.data(), nb, mode, tmin, tmax, first.data(), first.size(), sink_stdout,
                           nullptr);
  }
  if (ruled)
    fprintf(stderr, "a5_generator: rules: %llu candidate(s) longer than 128 bytes rejected\n",
            (unsigned long long)rejected);
  if (with_salts)
    fprintf(stderr, "a5_generator: salted: %llu (candidate, salt) pair(s) longer than 128 bytes skipped\n",
            (unsigned long long)skipped_pairs);
  if (iterated)
    fprintf(stderr, "a5_generator: iterated: %llu hit(s) on the first 16 bytes dropped (the rest of the key differs)\n",
            (unsigned long long)dropped_hits);
  fclose(f);
  fflush(stdout);
  if (rc) fprintf(stderr, "a5_generator: %s\n", a5x_last_error(ctx));
  a5x_destroy(ctx);
  return rc ? 2 : 0;
}
