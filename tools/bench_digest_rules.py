"""Rules route of the digest + lookup stage against the two-pass route without rules, one GPU.

Workload C5 as bench.py --workload c5 builds it (greek-hebrew x the synthetic Greek words
of synth.py), default mode, 1M random targets of the algorithm's width,
a5x_expand_digest_device.  Per algorithm, in one process and one context, three legs:

  (a) norules  the two-pass route without rules (A5X_NO_FUSED_DIGEST=1): k_digest_stream
  (b) colon64  64 ':' rules: k_rules_stream, the interpreter idle -- copy + hash + probe
  (c) mix64    64 rules of the common functions (l u c $X ^X sXY r d TN ])

reported as hashes/s of the digest pass (ms_total - ms_keyspace - ms_expand, HIP events):
candidates for (a), candidates x 64 for (b) and (c).  (b) / (a) is the route's cost beside
the plain stream kernel, (c) / (b) the interpreter's.

    python tools/bench_digest_rules.py [--words N] [--steps K] [--warmup W] [--out FILE]
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

NAMES = {"md5": 0, "ntlm": 1, "sha1": 2, "sha256": 3, "sha224": 5, "sha384": 6, "sha512": 7}
MIX = ["l", "u", "c", "$1", "$2", "$3", "$!", "$s", "^1", "^a", "sa@", "se3", "so0", "si1", "r", "d", "T0", "T1", "T2",
       "]", "l$1", "u$1", "c$1", "c$!", "l]", "u]", "c]", "r$1", "d]", "T0$1", "c$1$2", "c$2$0", "l$1$2$3", "sa@c",
       "se3u", "so0l", "^1$1", "^!$!", "T0T1", "T1T2", "]]", "]$s", "]$1", "c]$1", "rc", "rl", "ru", "r]", "dl",
       "du", "ss$", "ss5c", "st7", "sl1", "sb8", "sg9", "^2^1", "^a$z", "$0$0", "$9$9", "$1$!", "$7", "$8", "$9"]
assert len(MIX) == 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=2_000_000)
    ap.add_argument("--targets", type=int, default=1_000_000)
    ap.add_argument("--algos", default="md5,ntlm,sha1,sha256")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scratch-gb", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ["A5X_NO_FUSED_DIGEST"] = "1"  # leg (a): MD5 / NTLM on the two-pass route too
    from bench import kernel_src_sha
    from hashcat_a5_table_generator_amd import Context, DeviceBuffer, digest_size, synth

    tables, (data, offs) = synth.config_words("c5", args.words)
    tabs = [os.path.join(ROOT, "tests", "golden", "tables", t + ".table") for t in tables]
    n = len(offs) - 1
    scratch = int(args.scratch_gb * (1 << 30))
    legs = {"norules": None, "colon64": [":"] * 64, "mix64": MIX}
    res = {"tool": "tools/bench_digest_rules.py", "kernel_src_sha": kernel_src_sha(),
           "workload": f"c5: greek-hebrew x {args.words} synthetic Greek words, default mode, two-pass route "
                       f"(A5X_NO_FUSED_DIGEST=1), {args.targets} random targets, scratch {args.scratch_gb} GiB",
           "legs": {"norules": "no rules: k_digest_stream", "colon64": "64 x ':'", "mix64": MIX},
           "steps": args.steps, "warmup": args.warmup, "algos": {}}
    for name in args.algos.split(","):
        ctx = Context(0)
        res["device"] = ctx.device_name
        ctx.load_tables(tabs)
        rng = np.random.default_rng(0xD16E57)
        ctx.set_targets(NAMES[name], rng.integers(0, 256, size=(args.targets, digest_size(NAMES[name])), dtype=np.uint8))
        dw, do = DeviceBuffer.from_array(ctx, data), DeviceBuffer.from_array(ctx, offs)
        out = {}
        for leg, rules in legs.items():
            if rules is None:
                ctx.clear_rules()
            else:
                assert ctx.set_rules(rules) == (64, 0)
            R = 1 if rules is None else 64
            steps = []
            for k in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                hits, st = ctx.expand_digest_device(dw.ptr, do.ptr, n, 0, 0, 15, scratch_bytes=scratch, hit_cap=1 << 20)
                st["wall_ms"] = (time.perf_counter() - t0) * 1e3
                st["hits"] = len(hits)
                st["hashed"], st["rejected"] = ctx.rules_last()
                if k >= args.warmup:
                    steps.append(st)
            dig = [x["ms_total"] - x["ms_keyspace"] - x["ms_expand"] for x in steps]
            hashes = steps[0]["candidates"] * R
            if rules is not None:
                assert steps[0]["hashed"] == hashes - steps[0]["rejected"] * R
            out[leg] = {"rules": R, "candidates": steps[0]["candidates"], "hashes": hashes, "hits": steps[0]["hits"],
                        "rejected": steps[0]["rejected"], "expand_launches": steps[0]["expand_launches"],
                        "ms_expand": statistics.median(x["ms_expand"] for x in steps),
                        "ms_digest": {"median": statistics.median(dig), "min": min(dig), "max": max(dig)},
                        "wall_ms": statistics.median(x["wall_ms"] for x in steps),
                        "digest_hashes_per_s": hashes / (statistics.median(dig) * 1e-3)}
            print(f"{name:7s} {leg:8s} digest {out[leg]['ms_digest']['median']:9.2f} ms  "
                  f"{out[leg]['digest_hashes_per_s']:.3e} hashes/s  hits {out[leg]['hits']}", flush=True)
        out["colon64_over_norules"] = out["colon64"]["digest_hashes_per_s"] / out["norules"]["digest_hashes_per_s"]
        out["mix64_over_colon64"] = out["mix64"]["digest_hashes_per_s"] / out["colon64"]["digest_hashes_per_s"]
        res["algos"][name] = out
        ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
