"""The four victim calls before and after the shared walk loop: one figure per call from the probe that
timed it when it was added, several runs per build, the two builds alternating in one session.

Run each probe with KBHIP_LIB naming the build and --out DIR/<probe>.<parent|new>.<k>.json, then

    python profiles/victims_refactor_probe.py DIR [--out profiles/victims_refactor_probe.json]

Per call: each run's figure, the two medians, the parent's run-to-run spread (min .. max) and whether the
new median lies inside it.
"""
import argparse
import glob
import json
import os
import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# call -> (probe, path of the figure in the probe's JSON: a median in microseconds)
CALLS = {"kbhip_head_victims": ("head_victims_probe", ("modes", "1", "b_cap64", "median_us")),
         "kbhip_heads_victims": ("heads_victims_probe", ("modes", "1", "b_one_call_64", "median_us")),
         "kbhip_walk_victims": ("walk_victims_probe", ("b_walk", "wall_us_per_task", "median")),
         "kbhip_walk_victims_from": ("walk_from_probe", ("c_walk_from", "walk_call_us", "median"))}


def figures(d, probe, build, path, snapshots):
    out = []
    for f in sorted(glob.glob(os.path.join(d, "%s.%s.*.json" % (probe, build)))):
        v = json.load(open(f))
        snapshots.add(v["snapshot"])
        for k in path:
            v = v[k]
        out.append(float(v))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "victims_refactor_probe.json"))
    a = ap.parse_args()
    out, snapshots = {"calls": {}}, set()
    for call, (probe, path) in CALLS.items():
        p, n = figures(a.dir, probe, "parent", path, snapshots), figures(a.dir, probe, "new", path, snapshots)
        if not p or not n:
            continue
        pm, nm = statistics.median(p), statistics.median(n)
        out["calls"][call] = {"probe": probe, "figure": ".".join(path), "parent_us": p, "new_us": n,
                              "parent_median_us": pm, "new_median_us": nm, "parent_spread_us": [min(p), max(p)],
                              "ratio_to_parent": nm / pm, "within_parent_spread": min(p) <= nm <= max(p)}
    out["snapshot"] = ", ".join(sorted(snapshots))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
