"""HMAC route of the digest + lookup stage (k_hmac_stream) against the plain salted route of the
same hash, one GPU, one process, one context per hash.

Workload C5 as bench.py --workload c5 builds it (greek-hebrew x the synthetic Greek words of
synth.py), default mode, 1M random targets of the hash's width, a5x_expand_digest_device on the
two-pass route.  Per hash (md5, sha1, sha256, sha512), the legs

  salted64     the plain salted set, hash(candidate + salt), 64 distinct 8-byte salts: k_salt_stream
  hmac_pass64  HMAC(key = candidate, salt) under the same 64 salts: k_hmac_stream
  hmac_salt64  HMAC(key = salt, candidate) under the same 64 salts
  hmac_pass1   HMAC(key = candidate, salt) under one 8-byte salt (reported, no expectation: at one
  hmac_salt1   HMAC(key = salt, candidate) under one salt         salt the key states are not amortised)

as (candidate, salt) pairs/s of the digest pass (ms_total - ms_keyspace - ms_expand, HIP events).
Every leg carries the min and max over its steps: the run's own spread is the margin of the
expectation,

  hmac_pass64 and hmac_salt64 at or above half of salted64   at C5's candidate lengths a plain
      salted pair is one compression and a placed message, an HMAC pair two compressions with
      nothing to place.

    python tools/bench_digest_hmac.py [--words N] [--steps K] [--warmup W] [--out FILE]
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

# hash -> (plain, HMAC key = pass, HMAC key = salt)
HASHES = {"md5": (0, 48, 49), "sha1": (2, 50, 51), "sha256": (3, 52, 53), "sha512": (7, 54, 55)}
CH = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789!?"
assert len(set(CH)) == 64
TAILS = [(c * 3 + CH[(i * 7 + 1) % 64] * 2 + CH[(i * 11 + 3) % 64] * 3) for i, c in enumerate(CH)]  # 64 distinct 8-byte strings
assert len(set(TAILS)) == 64 and all(len(t) == 8 for t in TAILS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=1_000_000)
    ap.add_argument("--targets", type=int, default=1_000_000)
    ap.add_argument("--hashes", default="md5,sha1,sha256,sha512")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scratch-gb", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmac_bench_digest_hmac.json"))
    args = ap.parse_args()

    os.environ["A5X_NO_FUSED_DIGEST"] = "1"  # every leg on the two-pass route
    from bench import kernel_src_sha
    from hashcat_a5_table_generator_amd import Context, DeviceBuffer, digest_size, synth

    scratch = int(args.scratch_gb * (1 << 30))
    salts = [t.encode() for t in TAILS]
    res = {"tool": "tools/bench_digest_hmac.py", "kernel_src_sha": kernel_src_sha(),
           "workload": f"c5: greek-hebrew x {args.words} synthetic Greek words, default mode, two-pass route "
                       f"(A5X_NO_FUSED_DIGEST=1), {args.targets} random targets, scratch {args.scratch_gb} GiB",
           "legs": {"salted64": "plain salted set, hash(cand + salt), 64 distinct 8-byte salts: k_salt_stream",
                    "hmac_pass64": "HMAC(key = cand, salt), the same 64 salts: k_hmac_stream",
                    "hmac_salt64": "HMAC(key = salt, cand), the same 64 salts: k_hmac_stream",
                    "hmac_pass1": "HMAC(key = cand, salt), one 8-byte salt: k_hmac_stream",
                    "hmac_salt1": "HMAC(key = salt, cand), one 8-byte salt: k_hmac_stream"},
           "steps": args.steps, "warmup": args.warmup, "hashes": {}}
    tables, (data, offs) = synth.config_words("c5", args.words)
    tabs = [os.path.join(ROOT, "tests", "golden", "tables", t + ".table") for t in tables]
    n = len(offs) - 1
    for name in args.hashes.split(","):
        plain, kpass, ksalt = HASHES[name]
        ctx = Context(0)
        res["device"] = ctx.device_name
        ctx.load_tables(tabs)
        rng = np.random.default_rng(0xD16E57)
        tg = rng.integers(0, 256, size=(args.targets, digest_size(plain)), dtype=np.uint8)
        dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
        out = {"words": args.words}
        legs = [("salted64", plain, 0, 64), ("hmac_pass64", kpass, 0, 64), ("hmac_salt64", ksalt, 1, 64),
                ("hmac_pass1", kpass, 0, 1), ("hmac_salt1", ksalt, 1, 1)]
        for leg, algo, order, S in legs:
            ctx.set_salted_targets(algo, order, tg, [salts[i % S] for i in range(args.targets)])
            assert ctx.salt_count() == S
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
            pairs = steps[0]["candidates"] * S
            rate = lambda ms: pairs / (ms * 1e-3)
            out[leg] = {"algo": algo, "salts": S, "candidates": steps[0]["candidates"], "pairs": pairs, "hits": steps[0]["hits"],
                        "hashed": steps[0]["hashed"], "left_out": steps[0]["left_out"], "expand_launches": steps[0]["expand_launches"],
                        "ms_expand": statistics.median(x["ms_expand"] for x in steps),
                        "ms_digest": {"median": statistics.median(dig), "min": min(dig), "max": max(dig)},
                        "wall_ms": statistics.median(x["wall_ms"] for x in steps),
                        "digest_pairs_per_s": rate(statistics.median(dig)),
                        "digest_pairs_per_s_min": rate(max(dig)), "digest_pairs_per_s_max": rate(min(dig))}
            print(f"{name:6s} {leg:11s} digest {out[leg]['ms_digest']['median']:9.2f} ms [{min(dig):.2f}, {max(dig):.2f}]  "
                  f"{out[leg]['digest_pairs_per_s']:.3e} pairs/s  hits {out[leg]['hits']}", flush=True)
        r = lambda x, y: out[x]["digest_pairs_per_s"] / out[y]["digest_pairs_per_s"]
        # the expectation, the run's own step-to-step spread as the margin
        for leg in ("hmac_pass64", "hmac_salt64"):
            out[leg + "_over_salted64"] = r(leg, "salted64")
            out[leg + "_at_or_above_half_salted64"] = (out[leg]["digest_pairs_per_s_max"] >=
                                                      0.5 * out["salted64"]["digest_pairs_per_s_min"])
        out["hmac_pass1_over_hmac_pass64"] = r("hmac_pass1", "hmac_pass64")
        out["hmac_salt1_over_hmac_salt64"] = r("hmac_salt1", "hmac_salt64")
        print(f"{name:6s} hmac_pass64 / salted64 {out['hmac_pass64_over_salted64']:.3f} ({out['hmac_pass64_at_or_above_half_salted64']})  "
              f"hmac_salt64 / salted64 {out['hmac_salt64_over_salted64']:.3f} ({out['hmac_salt64_at_or_above_half_salted64']})", flush=True)
        res["hashes"][name] = out
        ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
