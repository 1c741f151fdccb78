"""Iterated route of the digest + lookup stage (k_pbkdf2_init / _loop / _compare) against the HMAC
key = pass route and the plain digest pass of the same hash, one GPU, one process, one context per
hash, all legs in the same run.

Workload C5's stream as bench.py --workload c5 builds it (greek-hebrew x the synthetic Greek words
of synth.py), default mode, random targets, a5x_expand_digest_device on the two-pass route.  The
default is 20 000 words (about 23M candidates): at c = 1000 a million words would be 1.2e12
pair-iterations.  Per hash (md5, sha1, sha256, sha512), the legs

  plain         the unsalted set: k_digest_stream, hashes/s
  hmac_pass1    HMAC(key = candidate, salt) under one 8-byte salt: k_hmac_stream, pairs/s
  pbkdf2_c1     PBKDF2 under the same salt, c = 1: init and compare alone, no loop launch
  pbkdf2_c1000  PBKDF2 under the same salt, c = 1000: whole-route pairs/s

as rates of the digest pass (ms_total - ms_keyspace - ms_expand, HIP events).  The loop kernel's
share is the difference of the two PBKDF2 legs, over its 999 iterations a pair:

  loop pair-iterations/s = candidates * 999 / (digest ms at c = 1000 - digest ms at c = 1)

and the mean time of one loop launch is that difference over the launch count
(a5x_debug_iter_budget).  One iteration is the two compressions of an HMAC key = pass pair and
nothing else, so the yardstick is hmac_pass1's pairs/s; half the plain pass's hashes/s is given
beside it.

    python tools/bench_digest_pbkdf2.py [--words N] [--iters C] [--steps K] [--warmup W] [--out FILE]
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

# hash -> (plain, HMAC key = pass, PBKDF2)
HASHES = {"md5": (0, 48, 72), "sha1": (2, 50, 73), "sha256": (3, 52, 74), "sha512": (7, 54, 75)}
SALT = b"aaabbccc"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=20_000)
    ap.add_argument("--targets", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--hashes", default="md5,sha1,sha256,sha512")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pair-slots", type=int, default=0, help="a5x_debug_iter_budget: pair slots per pass (0: default)")
    ap.add_argument("--pair-iters", type=int, default=0, help="... pair-iterations per loop launch (0: default)")
    ap.add_argument("--scratch-gb", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbkdf2_bench_digest_pbkdf2.json"))
    args = ap.parse_args()

    os.environ["A5X_NO_FUSED_DIGEST"] = "1"  # every leg on the two-pass route
    from bench import kernel_src_sha
    from hashcat_a5_table_generator_amd import Context, DeviceBuffer, digest_size, synth

    scratch = int(args.scratch_gb * (1 << 30))
    C = args.iters
    res = {"tool": "tools/bench_digest_pbkdf2.py", "kernel_src_sha": kernel_src_sha(),
           "workload": f"c5: greek-hebrew x {args.words} synthetic Greek words, default mode, two-pass route "
                       f"(A5X_NO_FUSED_DIGEST=1), {args.targets} random targets, one 8-byte salt, scratch {args.scratch_gb} GiB",
           "legs": {"plain": "unsalted set: k_digest_stream", "hmac_pass1": "HMAC(key = cand, salt), one salt: k_hmac_stream",
                    "pbkdf2_c1": "PBKDF2, c = 1: k_pbkdf2_init + k_pbkdf2_compare",
                    f"pbkdf2_c{C}": f"PBKDF2, c = {C}: + k_pbkdf2_loop"},
           "pair_slots": args.pair_slots, "pair_iters": args.pair_iters, "steps": args.steps, "warmup": args.warmup, "hashes": {}}
    tables, (data, offs) = synth.config_words("c5", args.words)
    tabs = [os.path.join(ROOT, "tests", "golden", "tables", t + ".table") for t in tables]
    n = len(offs) - 1
    for name in args.hashes.split(","):
        plain, kpass, kpb = HASHES[name]
        ctx = Context(0)
        res["device"] = ctx.device_name
        ctx.load_tables(tabs)
        ctx.iter_budget(args.pair_slots, args.pair_iters)
        rng = np.random.default_rng(0xD16E57)
        dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
        out = {"words": args.words}

        def leg(label, setup, pairs_of):
            setup()
            steps = []
            for k in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                hits, st = ctx.expand_digest_device(dw.ptr, do.ptr, n, 0, 0, 15, scratch_bytes=scratch, hit_cap=1 << 16)
                st["wall_ms"] = (time.perf_counter() - t0) * 1e3
                st["hits"] = len(hits)
                if k >= args.warmup:
                    steps.append(st)
            dig = [x["ms_total"] - x["ms_keyspace"] - x["ms_expand"] for x in steps]
            md = statistics.median(dig)
            out[label] = {"candidates": steps[0]["candidates"], "hits": steps[0]["hits"],
                          "expand_launches": steps[0]["expand_launches"],
                          "ms_digest": {"median": md, "min": min(dig), "max": max(dig)},
                          "wall_ms": statistics.median(x["wall_ms"] for x in steps),
                          "per_s": steps[0]["candidates"] / (md * 1e-3)}
            print(f"{name:6s} {label:13s} digest {md:10.2f} ms [{min(dig):.2f}, {max(dig):.2f}]  {out[label]['per_s']:.3e} /s",
                  flush=True)
            return out[label]

        tg = lambda w: rng.integers(0, 256, size=(args.targets, w), dtype=np.uint8)
        leg("plain", lambda: ctx.set_targets(plain, tg(digest_size(plain))), None)
        leg("hmac_pass1", lambda: ctx.set_salted_targets(kpass, 0, tg(digest_size(kpass)), [SALT] * args.targets), None)
        c1 = leg("pbkdf2_c1", lambda: ctx.set_iterated_targets(kpb, tg(16), [SALT] * args.targets, [1] * args.targets), None)
        c1["loop_launches"] = ctx.iter_budget(args.pair_slots, args.pair_iters)
        cn = leg(f"pbkdf2_c{C}", lambda: ctx.set_iterated_targets(kpb, tg(16), [SALT] * args.targets, [C] * args.targets), None)
        cn["loop_launches"] = ctx.iter_budget(args.pair_slots, args.pair_iters)
        cn["hashed"], cn["left_out"] = ctx.salts_last()
        loop_ms = cn["ms_digest"]["median"] - c1["ms_digest"]["median"]
        out["loop_ms"] = loop_ms
        out["loop_ms_per_launch"] = loop_ms / max(1, cn["loop_launches"])
        out["loop_pair_iterations_per_s"] = cn["candidates"] * (C - 1) / (loop_ms * 1e-3)
        out["route_pairs_per_s"] = cn["per_s"]
        out["loop_over_hmac_pass1"] = out["loop_pair_iterations_per_s"] / out["hmac_pass1"]["per_s"]
        out["loop_over_half_plain"] = out["loop_pair_iterations_per_s"] / (0.5 * out["plain"]["per_s"])
        print(f"{name:6s} loop {out['loop_pair_iterations_per_s']:.3e} pair-iterations/s in {cn['loop_launches']} launches of "
              f"{out['loop_ms_per_launch']:.1f} ms;  / hmac_pass1 {out['loop_over_hmac_pass1']:.3f}  / (plain / 2) "
              f"{out['loop_over_half_plain']:.3f};  route {out['route_pairs_per_s']:.3e} pairs/s", flush=True)
        res["hashes"][name] = out
        ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
