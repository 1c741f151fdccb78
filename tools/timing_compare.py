"""Per-leg digest-pass comparison of two runs of one tools/bench_digest_*.py tool.

    python tools/timing_compare.py PARENT.json NEW.json [PARENT.json NEW.json ...]

Every leg of the records that carries "ms_digest" {median, min, max}: a leg is ok when the new
median exceeds the parent's by no more than the parent's own max - min over its steps.
"""
import json
import sys


def legs(d, path=()):
    if isinstance(d, dict):
        md = d.get("ms_digest")
        if isinstance(md, dict) and "median" in md:
            yield "/".join(path), md
        for k, v in d.items():
            if not isinstance(v, list):
                yield from legs(v, path + (str(k),))


def main():
    if len(sys.argv) < 3 or len(sys.argv) % 2 != 1:
        sys.exit(__doc__)
    over = 0
    for p, n in zip(sys.argv[1::2], sys.argv[2::2]):
        with open(p) as f:
            rec = json.load(f)
        with open(n) as f:
            new = dict(legs(json.load(f)))
        for k, o in legs(rec):
            m, spread = new[k], o["max"] - o["min"]
            ok = m["median"] <= o["median"] + spread
            over += not ok
            print(f"{rec.get('tool', p):28s} {k:24s} parent {o['median']:9.2f} [{o['min']:.2f}, {o['max']:.2f}]  new "
                  f"{m['median']:9.2f} [{m['min']:.2f}, {m['max']:.2f}]  delta {m['median'] - o['median']:+7.2f} ms "
                  f"({(m['median'] / o['median'] - 1) * 100:+.2f} %)  margin {spread:5.2f}  {'ok' if ok else 'OVER'}")
    print("legs over the margin:", over)
    return 1 if over else 0


if __name__ == "__main__":
    sys.exit(main())
