"""Salted route of the digest + lookup stage against the rules route doing the same number and
length of messages, and against the two-pass route without salts, one GPU.

Workload C5 as bench.py --workload c5 builds it (greek-hebrew x the synthetic Greek words of
synth.py), default mode, 1M random targets of the algorithm's width,
a5x_expand_digest_device.  Per algorithm, in one process and one context, five legs:

  (a) nosalt     the two-pass route, no rules, no salts (A5X_NO_FUSED_DIGEST=1): k_digest_stream
  (b) append64   64 rules that append 8 bytes ($x eight times): k_rules_stream
      prepend64  64 rules that prepend 8 bytes (^x eight times)
  (c) pass.salt  a salted set of 64 distinct 8-byte salts, hash(candidate + salt): k_salt_stream
      salt.pass  the same salts, hash(salt + candidate)

reported as hashes/s of the digest pass (ms_total - ms_keyspace - ms_expand, HIP events):
candidates for (a), candidates x 64 for (b) and (c).  (c) / (b) compares the salt loop with the
rule interpreter on messages of equal count and length (pass.salt with append64, salt.pass
with prepend64); (c) / (a) is the cost of a salted hash beside an unsalted one.  Every leg
carries the min and max over its steps: the run's own spread is the margin of a comparison.

    python tools/bench_digest_salted.py [--words N] [--wide-words N] [--steps K] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = {"md5": 0, "sha1": 2, "sha256": 3, "sha224": 5, "sha384": 6, "sha512": 7}
WIDE = ("sha384", "sha512")  # a quarter of the hash rate: fewer words
CH = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789!?"
assert len(set(CH)) == 64
TAILS = [(c * 3 + CH[(i * 7 + 1) % 64] * 2 + CH[(i * 11 + 3) % 64] * 3) for i, c in enumerate(CH)]  # 64 distinct 8-byte strings
assert len(set(TAILS)) == 64 and all(len(t) == 8 for t in TAILS)
APPEND = ["".join("$" + ch for ch in t) for t in TAILS]
PREPEND = ["".join("^" + ch for ch in reversed(t)) for t in TAILS]  # (^ builds the prefix back to front)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=1_000_000)
    ap.add_argument("--wide-words", type=int, default=250_000, help="words for sha384 / sha512")
    ap.add_argument("--targets", type=int, default=1_000_000)
    ap.add_argument("--algos", default="md5,sha1,sha256,sha512")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scratch-gb", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ["A5X_NO_FUSED_DIGEST"] = "1"  # leg (a): MD5 on the two-pass route too
    from bench import kernel_src_sha
    from hashcat_a5_table_generator_amd import Context, DeviceBuffer, digest_size, synth

    scratch = int(args.scratch_gb * (1 << 30))
    salts = [t.encode() for t in TAILS]
    legs = ["nosalt", "append64", "prepend64", "pass.salt", "salt.pass"]
    res = {"tool": "tools/bench_digest_salted.py", "kernel_src_sha": kernel_src_sha(),
           "workload": f"c5: greek-hebrew x synthetic Greek words ({args.words}; {args.wide_words} for sha384 / sha512), default "
                       f"mode, two-pass route (A5X_NO_FUSED_DIGEST=1), {args.targets} random targets, scratch {args.scratch_gb} GiB",
           "legs": {"nosalt": "no rules, no salts: k_digest_stream", "append64": "64 rules of $x * 8: k_rules_stream",
                    "prepend64": "64 rules of ^x * 8: k_rules_stream",
                    "pass.salt": "64 distinct 8-byte salts, hash(cand + salt): k_salt_stream",
                    "salt.pass": "64 distinct 8-byte salts, hash(salt + cand): k_salt_stream"},
           "steps": args.steps, "warmup": args.warmup, "algos": {}}
    for name in args.algos.split(","):
        words = args.wide_words if name in WIDE else args.words
        tables, (data, offs) = synth.config_words("c5", words)
        tabs = [os.path.join(ROOT, "tests", "golden", "tables", t + ".table") for t in tables]
        n = len(offs) - 1
        ctx = Context(0)
        res["device"] = ctx.device_name
        ctx.load_tables(tabs)
        rng = np.random.default_rng(0xD16E57)
        tg = rng.integers(0, 256, size=(args.targets, digest_size(NAMES[name])), dtype=np.uint8)
        dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
        out = {"words": words}
        for leg in legs:
            ctx.clear_rules()
            if leg in ("pass.salt", "salt.pass"):
                ctx.set_salted_targets(NAMES[name], 0 if leg == "pass.salt" else 1, tg, [salts[i % 64] for i in range(args.targets)])
                assert ctx.salt_count() == 64
            else:
                ctx.set_targets(NAMES[name], tg)
                if leg != "nosalt":
                    assert ctx.set_rules(APPEND if leg == "append64" else PREPEND) == (64, 0)
            M = 1 if leg == "nosalt" else 64
            steps = []
            for k in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                hits, st = ctx.expand_digest_device(dw.ptr, do.ptr, n, 0, 0, 15, scratch_bytes=scratch, hit_cap=1 << 20)
                st["wall_ms"] = (time.perf_counter() - t0) * 1e3
                st["hits"] = len(hits)
                st["hashed"], st["left_out"] = ctx.salts_last() if leg in ("pass.salt", "salt.pass") else ctx.rules_last()
                if k >= args.warmup:
                    steps.append(st)
            dig = [x["ms_total"] - x["ms_keyspace"] - x["ms_expand"] for x in steps]
            hashes = steps[0]["candidates"] * M
            left_out = steps[0]["left_out"]  # rules: candidates over 128 bytes; salts: pairs over 128 bytes (0: like with like)
            rate = lambda ms: hashes / (ms * 1e-3)
            out[leg] = {"messages_per_candidate": M, "candidates": steps[0]["candidates"], "hashes": hashes,
                        "hits": steps[0]["hits"], "hashed": steps[0]["hashed"], "left_out": left_out, "expand_launches": steps[0]["expand_launches"],
                        "ms_expand": statistics.median(x["ms_expand"] for x in steps),
                        "ms_digest": {"median": statistics.median(dig), "min": min(dig), "max": max(dig)},
                        "wall_ms": statistics.median(x["wall_ms"] for x in steps),
                        "digest_hashes_per_s": rate(statistics.median(dig)),
                        "digest_hashes_per_s_min": rate(max(dig)), "digest_hashes_per_s_max": rate(min(dig))}
            print(f"{name:7s} {leg:9s} digest {out[leg]['ms_digest']['median']:9.2f} ms "
                  f"[{min(dig):.2f}, {max(dig):.2f}]  {out[leg]['digest_hashes_per_s']:.3e} hashes/s  hits {out[leg]['hits']}",
                  flush=True)
        r = lambda x, y: out[x]["digest_hashes_per_s"] / out[y]["digest_hashes_per_s"]
        out["pass.salt_over_append64"] = r("pass.salt", "append64")
        out["salt.pass_over_prepend64"] = r("salt.pass", "prepend64")
        out["pass.salt_over_nosalt"] = r("pass.salt", "nosalt")
        out["salt.pass_over_nosalt"] = r("salt.pass", "nosalt")
        # at or above the rules route, the run's own step-to-step spread as the margin
        out["pass.salt_at_or_above_append64"] = out["pass.salt"]["digest_hashes_per_s_max"] >= out["append64"]["digest_hashes_per_s_min"]
        out["salt.pass_at_or_above_prepend64"] = out["salt.pass"]["digest_hashes_per_s_max"] >= out["prepend64"]["digest_hashes_per_s_min"]
        print(f"{name:7s} pass.salt / append64 {out['pass.salt_over_append64']:.3f}  salt.pass / prepend64 "
              f"{out['salt.pass_over_prepend64']:.3f}  pass.salt / nosalt {out['pass.salt_over_nosalt']:.3f}", flush=True)
        res["algos"][name] = out
        ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
