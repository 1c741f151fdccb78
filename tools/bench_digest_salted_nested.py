"""Salted nested route of the digest + lookup stage (k_salt_nest_stream) against the two routes
it is built from, one GPU, one process, one context per family.

Workload C5 as bench.py --workload c5 builds it (greek-hebrew x the synthetic Greek words of
synth.py), default mode, 1M random targets of the algorithm's width, a5x_expand_digest_device
on the two-pass route.  Per family (md5: md5-md5.salt = 32 beside MD5 and md5-md5; sha1:
sha1-sha1.salt = 36 beside SHA-1 and sha1-sha1), the legs

  (a) salted64   the plain salted set, hash(candidate + salt), 64 distinct 8-byte salts: k_salt_stream
  (b) nested     the unsalted nested set, outer(hex(inner(p))): k_digest_stream's nested form
      nest64     the salted nested set under the same 64 salts: k_salt_nest_stream
      nest1      the salted nested set under one 8-byte salt
      prefix64   the family's salt . text form (33 / 37) under the 64 salts (reported, no expectation)
      md5salt64  md5 only: md5(hex(md5(salt)) . hex(md5(p))) (35) under the 64 salts (reported, no expectation)

as hashes/s of the digest pass (ms_total - ms_keyspace - ms_expand, HIP events): (candidate,
salt) pairs for the 64-salt legs, candidates for nested and nest1.  Every leg carries the min
and max over its steps: the run's own spread is the margin of the two expectations,

  nest64 at or above salted64   per pair it does one fixed-shape block behind a shared inner digest
                                where (a) places and pads a message by length;
  nest1 at or above nested      at one salt the route does what the nested pass does, with the
                                pad words read from the salt record.

    python tools/bench_digest_salted_nested.py [--words N] [--steps K] [--warmup W] [--out FILE]
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

# family -> (plain, unsalted nested, text . salt, salt . text)
FAMILIES = {"md5": (0, 16, 32, 33), "sha1": (2, 20, 36, 37)}
CH = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789!?"
assert len(set(CH)) == 64
TAILS = [(c * 3 + CH[(i * 7 + 1) % 64] * 2 + CH[(i * 11 + 3) % 64] * 3) for i, c in enumerate(CH)]  # 64 distinct 8-byte strings
assert len(set(TAILS)) == 64 and all(len(t) == 8 for t in TAILS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=1_000_000)
    ap.add_argument("--targets", type=int, default=1_000_000)
    ap.add_argument("--families", default="md5,sha1")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scratch-gb", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ["A5X_NO_FUSED_DIGEST"] = "1"  # every leg on the two-pass route
    from bench import kernel_src_sha
    from hashcat_a5_table_generator_amd import Context, DeviceBuffer, digest_size, synth

    scratch = int(args.scratch_gb * (1 << 30))
    salts = [t.encode() for t in TAILS]
    res = {"tool": "tools/bench_digest_salted_nested.py", "kernel_src_sha": kernel_src_sha(),
           "workload": f"c5: greek-hebrew x {args.words} synthetic Greek words, default mode, two-pass route "
                       f"(A5X_NO_FUSED_DIGEST=1), {args.targets} random targets, scratch {args.scratch_gb} GiB",
           "legs": {"salted64": "plain salted set, hash(cand + salt), 64 distinct 8-byte salts: k_salt_stream",
                    "nested": "unsalted nested set: k_digest_stream (nested form)",
                    "nest64": "salted nested set, outer(hex(inner(cand)) + salt), the same 64 salts: k_salt_nest_stream",
                    "nest1": "salted nested set, one 8-byte salt: k_salt_nest_stream",
                    "prefix64": "salted nested set, outer(salt + hex(inner(cand))), the same 64 salts: k_salt_nest_stream",
                    "md5salt64": "md5 only: md5(hex(md5(salt)) + hex(md5(cand))), the same 64 salts: k_salt_nest_stream"},
           "steps": args.steps, "warmup": args.warmup, "families": {}}
    tables, (data, offs) = synth.config_words("c5", args.words)
    tabs = [os.path.join(ROOT, "tests", "golden", "tables", t + ".table") for t in tables]
    n = len(offs) - 1
    for fam in args.families.split(","):
        plain, nested, suffix, prefix = FAMILIES[fam]
        ctx = Context(0)
        res["device"] = ctx.device_name
        ctx.load_tables(tabs)
        rng = np.random.default_rng(0xD16E57)
        tg = rng.integers(0, 256, size=(args.targets, digest_size(plain)), dtype=np.uint8)
        dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
        out = {"words": args.words}
        legs = [("salted64", plain, 0, 64), ("nested", nested, None, 0), ("nest64", suffix, 0, 64), ("nest1", suffix, 0, 1),
                ("prefix64", prefix, 1, 64)] + ([("md5salt64", 35, 1, 64)] if fam == "md5" else [])
        for leg, algo, order, S in legs:
            if S:
                ctx.set_salted_targets(algo, order, tg, [salts[i % S] for i in range(args.targets)])
                assert ctx.salt_count() == S
            else:
                ctx.set_targets(algo, tg)
            M = max(S, 1)
            steps = []
            for k in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                hits, st = ctx.expand_digest_device(dw.ptr, do.ptr, n, 0, 0, 15, scratch_bytes=scratch, hit_cap=1 << 20)
                st["wall_ms"] = (time.perf_counter() - t0) * 1e3
                st["hits"] = len(hits)
                st["hashed"], st["left_out"] = ctx.salts_last()
                if k >= args.warmup:
                    steps.append(st)
            dig = [x["ms_total"] - x["ms_keyspace"] - x["ms_expand"] for x in steps]
            hashes = steps[0]["candidates"] * M
            rate = lambda ms: hashes / (ms * 1e-3)
            out[leg] = {"algo": algo, "salts": S, "candidates": steps[0]["candidates"], "hashes": hashes, "hits": steps[0]["hits"],
                        "hashed": steps[0]["hashed"], "left_out": steps[0]["left_out"], "expand_launches": steps[0]["expand_launches"],
                        "ms_expand": statistics.median(x["ms_expand"] for x in steps),
                        "ms_digest": {"median": statistics.median(dig), "min": min(dig), "max": max(dig)},
                        "wall_ms": statistics.median(x["wall_ms"] for x in steps),
                        "digest_hashes_per_s": rate(statistics.median(dig)),
                        "digest_hashes_per_s_min": rate(max(dig)), "digest_hashes_per_s_max": rate(min(dig))}
            print(f"{fam:5s} {leg:9s} digest {out[leg]['ms_digest']['median']:9.2f} ms [{min(dig):.2f}, {max(dig):.2f}]  "
                  f"{out[leg]['digest_hashes_per_s']:.3e} hashes/s  hits {out[leg]['hits']}", flush=True)
        r = lambda x, y: out[x]["digest_hashes_per_s"] / out[y]["digest_hashes_per_s"]
        out["nest64_over_salted64"] = r("nest64", "salted64")
        out["nest1_over_nested"] = r("nest1", "nested")
        out["prefix64_over_nest64"] = r("prefix64", "nest64")
        if "md5salt64" in out:
            out["md5salt64_over_nest64"] = r("md5salt64", "nest64")
        # the expectations, the run's own step-to-step spread as the margin
        out["nest64_at_or_above_salted64"] = out["nest64"]["digest_hashes_per_s_max"] >= out["salted64"]["digest_hashes_per_s_min"]
        out["nest1_at_or_above_nested"] = out["nest1"]["digest_hashes_per_s_max"] >= out["nested"]["digest_hashes_per_s_min"]
        print(f"{fam:5s} nest64 / salted64 {out['nest64_over_salted64']:.3f} ({out['nest64_at_or_above_salted64']})  "
              f"nest1 / nested {out['nest1_over_nested']:.3f} ({out['nest1_at_or_above_nested']})  "
              f"prefix64 / nest64 {out['prefix64_over_nest64']:.3f}", flush=True)
        res["families"][fam] = out
        ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
