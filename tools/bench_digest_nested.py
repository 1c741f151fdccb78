"""Two-pass digest + lookup rate of the nested algorithms beside the plain ones they nest.

Workload C5 as bench.py --workload c5 builds it (greek-hebrew x the synthetic Greek words
of synth.py), default mode, 1M random targets of the algorithm's width,
a5x_expand_digest_device, as tools/bench_digest_algo.py.  Every algorithm runs the two-pass
route (expand into the device scratch, k_digest_stream, k_hits_resolve): the nested and the
SHA algorithms always do, MD5 is forced onto it with A5X_NO_FUSED_DIGEST=1.  One context per
algorithm, the timed steps alternate between them; per step the library's own split (HIP
events): keyspace, expansion, digest = total - keyspace - expansion.

Per nested algorithm the record holds its digest-pass time and its ratio to the sum of the
plain digest passes of its stages in the same run: md5-md5 against 2 x md5, md5-md5-md5
against 3 x md5, sha256-md5 against md5 + sha256.  That sum pays stream staging and line
finding once per stage and a length-generic block per stage; the nested kernel pays staging
once, a constant-length outer block, and the hex encoding.

    python tools/bench_digest_nested.py [--words N] [--steps K] [--warmup W] [--rules FILE] [--out FILE]

--rules FILE: the ruled digest rate (hashes per second of the digest pass) of md5-md5 and
sha1-sha1 beside their no-rule rate, in contexts of their own.
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

PLAIN = {"md5": 0, "sha1": 2, "sha256": 3}
NESTED = {"md5-md5": 16, "md5-md5-md5": 17, "md5-md5up": 18, "md5-sha1": 19, "sha1-sha1": 20, "sha1-md5": 21,
          "sha256-md5": 22}
# the plain digest passes a nested algorithm is measured against, inner first
STAGES = {"md5-md5": ["md5", "md5"], "md5-md5-md5": ["md5", "md5", "md5"], "md5-md5up": ["md5", "md5"],
          "md5-sha1": ["sha1", "md5"], "sha1-sha1": ["sha1", "sha1"], "sha1-md5": ["md5", "sha1"],
          "sha256-md5": ["md5", "sha256"]}
RULED = ["md5-md5", "sha1-sha1"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=2_000_000)
    ap.add_argument("--targets", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scratch-gb", type=float, default=8.0)
    ap.add_argument("--rules", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_bench_digest_nested.json"))
    args = ap.parse_args()

    os.environ["A5X_NO_FUSED_DIGEST"] = "1"  # MD5 on the two-pass route too
    from hashcat_a5_table_generator_amd import Context, DeviceBuffer, digest_size, synth

    tables, (data, offs) = synth.config_words("c5", args.words)
    tabs = [os.path.join(ROOT, "tests", "golden", "tables", t + ".table") for t in tables]
    n = len(offs) - 1
    scratch = int(args.scratch_gb * (1 << 30))
    values = dict(PLAIN, **NESTED)
    legs = list(values)  # (name of the run, algorithm name)
    algo_of = {name: name for name in legs}
    rule_text = open(args.rules, "rb").read() if args.rules else None
    if rule_text is not None:
        for name in RULED:
            legs.append(name + "+rules")
            algo_of[name + "+rules"] = name
    runs = {}
    for leg in legs:
        a = values[algo_of[leg]]
        ctx = Context(0)
        ctx.load_tables(tabs)
        rng = np.random.default_rng(0xD16E57)
        ctx.set_targets(a, rng.integers(0, 256, size=(args.targets, digest_size(a)), dtype=np.uint8))
        nrules = 0
        if leg.endswith("+rules"):
            nrules, _ = ctx.set_rules([ln for ln in rule_text.split(b"\n")])
            assert nrules >= 1, "no rule of --rules was accepted"
        runs[leg] = {"ctx": ctx, "dw": DeviceBuffer.from_array(ctx, data), "do": DeviceBuffer.from_array(ctx, offs),
                     "steps": [], "nrules": nrules}

    def step(r):
        t0 = time.perf_counter()
        hits, st = r["ctx"].expand_digest_device(r["dw"].ptr, r["do"].ptr, n, 0, 0, 15, scratch_bytes=scratch)
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3  # (the call ends in a stream synchronise)
        st["hits"] = len(hits)
        if r["nrules"]:
            st["hashed"], st["rejected"] = r["ctx"].rules_last()
        return st

    for _ in range(args.warmup):
        for leg in legs:
            step(runs[leg])
    for _ in range(args.steps):  # alternating, so drift hits every algorithm alike
        for leg in legs:
            runs[leg]["steps"].append(step(runs[leg]))

    res = {"tool": "tools/bench_digest_nested.py", "device": runs[legs[0]]["ctx"].device_name,
           "workload": f"c5: greek-hebrew x {args.words} synthetic Greek words, default mode, two-pass route "
                       f"(A5X_NO_FUSED_DIGEST=1), {args.targets} random targets, scratch {args.scratch_gb} GiB",
           "steps": args.steps, "warmup": args.warmup, "bound": 1.10, "algos": {}}
    dig_ms = {}
    for leg in legs:
        s = runs[leg]["steps"]
        dig = [x["ms_total"] - x["ms_keyspace"] - x["ms_expand"] for x in s]
        wall = [x["wall_ms"] for x in s]
        dig_ms[leg] = statistics.median(dig)
        hashes = s[0].get("hashed", s[0]["candidates"])
        r = {"candidates": s[0]["candidates"], "bytes": s[0]["bytes"], "expand_launches": s[0]["expand_launches"],
             "hits": s[0]["hits"],
             "candidates_per_s": s[0]["candidates"] / (statistics.median(wall) * 1e-3),
             "wall_ms": {"median": statistics.median(wall), "min": min(wall), "max": max(wall)},
             "ms_keyspace": statistics.median(x["ms_keyspace"] for x in s),
             "ms_expand": statistics.median(x["ms_expand"] for x in s),
             "ms_digest": {"median": statistics.median(dig), "min": min(dig), "max": max(dig)},
             "digest_hashes_per_s": hashes / (statistics.median(dig) * 1e-3)}
        if runs[leg]["nrules"]:
            r["rules"] = runs[leg]["nrules"]
            r["hashed"], r["rejected"] = s[0]["hashed"], s[0]["rejected"]
        res["algos"][leg] = r
    worst = 0.0
    for name, stages in STAGES.items():
        r = res["algos"][name]
        r["stages"] = stages
        r["stages_ms_digest"] = sum(dig_ms[x] for x in stages)
        r["digest_ms_over_stages"] = dig_ms[name] / r["stages_ms_digest"]
        worst = max(worst, r["digest_ms_over_stages"])
    for name in RULED:
        if name + "+rules" in res["algos"]:
            r = res["algos"][name + "+rules"]
            r["hash_rate_over_norules"] = r["digest_hashes_per_s"] / res["algos"][name]["digest_hashes_per_s"]
    res["worst_ratio"] = worst
    res["within_bound"] = worst <= res["bound"]
    for leg in legs:
        r = res["algos"][leg]
        extra = f"  {r['digest_ms_over_stages']:.3f} of {'+'.join(r['stages'])}" if "stages" in r else ""
        extra += f"  {r['hash_rate_over_norules']:.3f} of the no-rule hash rate" if "hash_rate_over_norules" in r else ""
        print(f"{leg:18s} digest {r['ms_digest']['median']:8.2f} ms ({r['ms_digest']['min']:.2f}-{r['ms_digest']['max']:.2f})  "
              f"{r['digest_hashes_per_s']:.3e} hashes/s{extra}", flush=True)
    print(f"worst ratio {worst:.3f} (bound {res['bound']:.2f})", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    for r in runs.values():
        r["ctx"].close()


if __name__ == "__main__":
    main()
