"""The eviction-walk cursor against kbhip_walk_victims_from, to the end of the walk, at C5.

One task's reclaim node loop through the Python binding, two ways, on twin
sessions of one snapshot, alternating task by task so that both see the same
drift of the machine:
  (c) kbhip_walk_victims_from + kbhip_apply_ops, window by window until
      ASSIGNED or EXHAUSTED: §4.21's to-the-end run, every window ranked again;
  (k) kbhip_walk_begin once, then kbhip_walk_next + kbhip_apply_ops from the
      position each call returns.
Both apply what they decide, so the twins move through the same states; the op
logs are compared task by task.  The tasks are the first --full of
walk_from_probe.py's sample (pending tasks in pod order), the ones §4.21 ran
to the end.  Per task: ABI calls, kernel launches and wall time of either
protocol, and for (k) the ranking's share.

    python profiles/walk_cursor_probe.py [--tasks 120] [--full 8] [--out profiles/walk_cursor_probe.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "kube-batch-1_amd"), os.path.join(ROOT, "profiles")]
import kbgen  # noqa: E402
import kbhip  # noqa: E402
from walk_victims_probe import _pct  # noqa: E402

DONE = (kbhip.WALK_ASSIGNED, kbhip.WALK_EXHAUSTED)


def _apply(s, op, pod, node, ops):
    """-> the launches of the kbhip_apply_ops call"""
    ops += [(int(o), int(p), int(n)) for o, p, n in zip(op, pod, node)]
    return s.apply_ops(op, pod, node)


def windows(s, task, max_calls=1 << 20):
    """(c) -> (ops, ABI calls, launches, entries decided, acted-on nodes, stop)"""
    ops, calls, launches, decided, acted, after = [], 0, 0, 0, 0, None
    while True:
        op, pod, node, info = s.walk_victims_from(task, False, 1, 64, after, 4096)
        calls += 1
        launches += info["launches"]
        decided += info["visited"]
        acted += info["acted"]
        if len(op):
            launches += _apply(s, op, pod, node, ops)
            calls += 1
        stuck = info["stop"] == kbhip.WALK_CAPACITY and info["visited"] <= 1 and info["acted"] == 0
        if info["stop"] in DONE or stuck or calls >= max_calls:
            return ops, calls, launches, decided, acted, info["stop"]
        after = (info["resume_node"], info["resume_score"])


def cursor(s, task, max_calls=1 << 20):
    """(k) -> (ops, ABI calls, launches, entries decided, acted-on nodes, stop, kbhip_walk_begin's wall us, T,
    entries the scans decided, of them behind the call's `first`)"""
    t0 = time.perf_counter()
    total, binfo = s.walk_begin(task, False, 1)
    begin_us = (time.perf_counter() - t0) * 1e6
    ops, calls, launches, decided, acted, pos, scanned, vain = [], 1, binfo["launches"], 0, 0, 0, 0, 0
    while True:
        op, pod, node, info = s.walk_next(pos, 64, 4096)
        calls += 1
        launches += info["launches"]
        decided += info["decided"]
        acted += info["acted"]
        scanned += info["scanned"]
        vain += info["scanned"] - ((info["first"] - pos + 1) if info["first"] >= 0 else total - pos)
        if len(op):
            launches += _apply(s, op, pod, node, ops)
            calls += 1
        stuck = info["stop"] == kbhip.WALK_CAPACITY and info["next"] == pos and not len(op)
        if info["stop"] in DONE or stuck or calls >= max_calls:
            return ops, calls, launches, decided, acted, info["stop"], begin_us, total, scanned, vain
        pos = info["next"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=120)
    ap.add_argument("--full", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_cursor_probe.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "c5.kbs")
        kbgen.gen_c5(path)
        with kbhip.EncodedSnapshot(path) as enc:
            cls, job = enc.table("pod_class"), enc.table("pod_job")
            pend = np.nonzero((cls >= 0) & (job >= 0))[0]
        tasks = [int(t) for t in pend[:: max(1, len(pend) // a.tasks)][:a.tasks]][:a.full]
        keys = ("us", "calls", "launches", "decided", "acted", "stop")
        rec = {w: {k: [] for k in keys} for w in "ck"}
        begin_us, totals, same, scanned, vain = [], [], 0, [], []
        with kbhip.Session(path) as sc, kbhip.Session(path) as sk:
            nodes = sc.stats()["nodes"]
            sc.walk_victims_from(tasks[0], False, 1, 1)  # the tables built and the kernels loaded outside the timed part
            sc.walk_victims_from(tasks[0], False, 1, 1, (0, 0))
            sk.walk_begin(tasks[0], False, 1)
            sk.walk_next(0, 1)
            sk.walk_end()
            for k, t in enumerate(tasks):
                got = {}
                for which in ("ck", "kc")[k % 2]:
                    t0 = time.perf_counter()
                    got[which] = windows(sc, t) if which == "c" else cursor(sk, t)
                    rec[which]["us"].append((time.perf_counter() - t0) * 1e6)
                    for name, v in zip(keys[1:], got[which][1:6]):
                        rec[which][name].append(int(v))
                same += got["c"][0] == got["k"][0]
                begin_us.append(got["k"][6])
                totals.append(int(got["k"][7]))
                scanned.append(int(got["k"][8]))
                vain.append(int(got["k"][9]))
        out = {"snapshot": "gen_c5", "nodes": int(nodes), "tasks": len(tasks), "logs_equal": same,
               "walk_entries_per_task": _pct(totals), "per_task": []}
        for w, name in (("c", "c_walk_from"), ("k", "k_cursor")):
            out[name] = {"calls_per_task": _pct(rec[w]["calls"]), "launches_per_task": _pct(rec[w]["launches"]),
                         "entries_decided_per_task": _pct(rec[w]["decided"]),
                         "acted_nodes_per_task": _pct(rec[w]["acted"]), "wall_us_per_task": _pct(rec[w]["us"]),
                         "stops": sorted(set(rec[w]["stop"]))}
        out["k_cursor"]["begin_us"] = _pct(begin_us)
        out["k_cursor"]["scanned_per_task"] = _pct(scanned)
        out["k_cursor"]["scanned_behind_first_per_task"] = _pct(vain)
        for i, t in enumerate(tasks):
            out["per_task"].append({"task": t, "walk_entries": totals[i],
                                    "c": {k: rec["c"][k][i] for k in keys}, "k": {k: rec["k"][k][i] for k in keys},
                                    "k_begin_us": begin_us[i], "k_scanned": scanned[i],
                                    "k_scanned_behind_first": vain[i]})
        cu, ku = np.array(rec["c"]["us"]), np.array(rec["k"]["us"])
        out["k_over_c"] = {"wall_median_of_ratios": float(np.median(ku / cu)), "wall_sum": float(ku.sum() / cu.sum()),
                           "calls_sum": float(sum(rec["k"]["calls"]) / max(sum(rec["c"]["calls"]), 1)),
                           "launches_sum": float(sum(rec["k"]["launches"]) / max(sum(rec["c"]["launches"]), 1))}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
