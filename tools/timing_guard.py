#!/usr/bin/env python3
"""tools/timing_guard.py PARENT.json CHANGE.json [--out FILE] -- the guard DESIGN 4c holds existing legs to: two result files of one
timing script (tools/sort_merge_time.py, tools/order_merge_time.py, tools/sort_time.py: {"legs": {name: {ms_median, ms_min,
ms_max}}}), one of the commit before and one of the change, built side by side and run in one session.  For every leg both files
hold, the change's median must fall inside the parent's [min - spread .. max + spread], spread = the parent's max - min.  Prints one
line per leg, writes the verdicts with --out, exits 1 if a leg is outside."""
import json
import sys


def guard(parent_legs, change_legs):
    """{leg: {parent, change, lo, hi, inside}} over the legs both runs hold"""
    out = {}
    for name, p in parent_legs.items():
        c = change_legs.get(name)
        if c is None:
            continue
        spread = p["ms_max"] - p["ms_min"]
        lo, hi = p["ms_min"] - spread, p["ms_max"] + spread
        out[name] = {"parent": [p["ms_median"], p["ms_min"], p["ms_max"]], "change": [c["ms_median"], c["ms_min"], c["ms_max"]], "lo": lo, "hi": hi,
                     "inside": bool(lo <= c["ms_median"] <= hi)}
    return out


def report(g):
    for name, v in g.items():
        p, c = v["parent"], v["change"]
        print(f"{name:40s} parent {p[0]:.3f} [{p[1]:.3f} .. {p[2]:.3f}]  change {c[0]:.3f} [{c[1]:.3f} .. {c[2]:.3f}]  guard {v['lo']:.3f} .. {v['hi']:.3f}: "
              f"{'inside' if v['inside'] else 'OUTSIDE'}", flush=True)
    return all(v["inside"] for v in g.values())


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) < 2:
        sys.exit(__doc__)
    g = guard(json.load(open(args[0]))["legs"], json.load(open(args[1]))["legs"])
    ok = report(g)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(g, f, indent=1)
    sys.exit(0 if ok else 1)
