"""Two-pass digest + lookup rate per algorithm on one GPU (the SHA family beside MD5).

Workload C5 as bench.py --workload c5 builds it (greek-hebrew x the synthetic Greek words
of synth.py), default mode, 1M random targets of the algorithm's width,
a5x_expand_digest_device.  Every algorithm runs the two-pass route (expand into the
device scratch, k_digest_stream, k_hits_resolve): the SHA algorithms always do, MD5 / NTLM
are forced onto it with A5X_NO_FUSED_DIGEST=1 -- the yardstick, same expansion kernels.
One context per algorithm, the timed steps alternate between them; per step the library's
own split (HIP events): keyspace, expansion, digest = total - keyspace - expansion.

    python tools/bench_digest_algo.py [--words N] [--steps K] [--warmup W] [--isa-mix FILE] [--out FILE]

--isa-mix: the JSON tools/isa_mix.py wrote (CPU); its per-block VALU counts (64-byte blocks;
128-byte for sha384 / sha512) are copied into the record beside the rates.  With sha256 among
--algos every other algorithm's digest-pass time is also given as a ratio of SHA-256's.
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
BLOCK_FN = {"md5": "md5_block", "ntlm": "md4_block", "sha1": "sha1_block", "sha256": "sha256_block",
            "sha224": "sha256_block", "sha384": "sha512_block", "sha512": "sha512_block"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=2_000_000)
    ap.add_argument("--targets", type=int, default=1_000_000)
    ap.add_argument("--algos", default="md5,sha1,sha256")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scratch-gb", type=float, default=8.0)
    ap.add_argument("--isa-mix", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ["A5X_NO_FUSED_DIGEST"] = "1"  # MD5 / NTLM on the two-pass route too
    from hashcat_a5_table_generator_amd import Context, DeviceBuffer, digest_size, synth

    tables, (data, offs) = synth.config_words("c5", args.words)
    tabs = [os.path.join(ROOT, "tests", "golden", "tables", t + ".table") for t in tables]
    n = len(offs) - 1
    scratch = int(args.scratch_gb * (1 << 30))
    algos = args.algos.split(",")
    runs = {}
    for name in algos:
        ctx = Context(0)
        ctx.load_tables(tabs)
        rng = np.random.default_rng(0xD16E57)
        ctx.set_targets(NAMES[name], rng.integers(0, 256, size=(args.targets, digest_size(NAMES[name])), dtype=np.uint8))
        runs[name] = {"ctx": ctx, "dw": DeviceBuffer.from_array(ctx, data), "do": DeviceBuffer.from_array(ctx, offs),
                      "steps": []}

    def step(r):
        t0 = time.perf_counter()
        hits, st = r["ctx"].expand_digest_device(r["dw"].ptr, r["do"].ptr, n, 0, 0, 15, scratch_bytes=scratch)
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3  # (the call ends in a stream synchronise)
        st["hits"] = len(hits)
        return st

    for _ in range(args.warmup):
        for name in algos:
            step(runs[name])
    for _ in range(args.steps):  # alternating, so drift hits every algorithm alike
        for name in algos:
            runs[name]["steps"].append(step(runs[name]))

    isa = json.load(open(args.isa_mix)) if args.isa_mix else {}
    res = {"tool": "tools/bench_digest_algo.py", "device": runs[algos[0]]["ctx"].device_name,
           "workload": f"c5: greek-hebrew x {args.words} synthetic Greek words, default mode, two-pass route "
                       f"(A5X_NO_FUSED_DIGEST=1), {args.targets} random targets, scratch {args.scratch_gb} GiB",
           "steps": args.steps, "warmup": args.warmup, "algos": {}}
    for name in algos:
        s = runs[name]["steps"]
        med = lambda k: statistics.median(x[k] for x in s)
        dig = [x["ms_total"] - x["ms_keyspace"] - x["ms_expand"] for x in s]
        wall = [x["wall_ms"] for x in s]
        r = {"candidates": s[0]["candidates"], "bytes": s[0]["bytes"], "expand_launches": s[0]["expand_launches"],
             "hits": s[0]["hits"],
             "candidates_per_s": s[0]["candidates"] / (statistics.median(wall) * 1e-3),
             "wall_ms": {"median": statistics.median(wall), "min": min(wall), "max": max(wall)},
             "ms_keyspace": med("ms_keyspace"),
             "ms_expand": {"median": med("ms_expand"), "min": min(x["ms_expand"] for x in s),
                           "max": max(x["ms_expand"] for x in s)},
             "ms_digest": {"median": statistics.median(dig), "min": min(dig), "max": max(dig)},
             "digest_candidates_per_s": s[0]["candidates"] / (statistics.median(dig) * 1e-3)}
        m = isa.get(BLOCK_FN[name])
        if m:
            r["isa_per_block"] = {"block_bytes": 128 if BLOCK_FN[name] == "sha512_block" else 64, "function": BLOCK_FN[name], "valu_instructions": m["valu_instructions"],
                                  "half_rate_instructions": round(m["half_rate_share"] * m["valu_instructions"]),
                                  "mean_issue_cycles": m["mean_issue_cycles"]}
        if "sha256" in runs and name != "sha256":
            y = statistics.median(x["ms_total"] - x["ms_keyspace"] - x["ms_expand"] for x in runs["sha256"]["steps"])
            r["digest_ms_over_sha256"] = statistics.median(dig) / y
        res["algos"][name] = r
        print(f"{name:7s} {r['candidates_per_s']:.3e} cand/s  wall {r['wall_ms']['median']:.2f} ms  keyspace "
              f"{r['ms_keyspace']:.2f}  expand {r['ms_expand']['median']:.2f} ({r['ms_expand']['min']:.2f}-"
              f"{r['ms_expand']['max']:.2f})  digest {r['ms_digest']['median']:.2f} ms", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    for r in runs.values():
        r["ctx"].close()


if __name__ == "__main__":
    main()
