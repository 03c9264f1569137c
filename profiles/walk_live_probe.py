"""The live cursor against the fixed cursor and the window protocol, at C3 with required pod affinity
(DESIGN §4.23).

One task's reclaim node loop through the Python binding, three ways, on twin
sessions of one snapshot (kbgen.gen_c3 with pod_affinity), for a handful of
pending tasks whose class reads pod-affinity targets (kbhip_walk_begin's
out_info[3]), each to ASSIGNED / EXHAUSTED:
  (l) kbhip_walk_begin_live, then kbhip_walk_next + kbhip_apply_ops: one call
      pair per acting node;
  (k) kbhip_walk_begin(by_score 0), then kbhip_walk_next + kbhip_apply_ops:
      the node set fixed at begin;
  (c) kbhip_walk_victims_from + kbhip_apply_ops, window by window.
Every protocol applies what it decides on its own session.  The reference log
of a task is taken on a fourth twin from existing calls only: the fixed cursor
ranked again after every acting node (kbhip_walk_begin, kbhip_walk_next with
cap 1 from the first entry behind the node last acted on), so that every
predicate is tested on the tables as they stand when the loop reaches the node
— reclaim.go:115-117.  Per task: ABI calls, kernel launches, wall time, and
whether the op log equals the reference's.  The sessions drift apart where the
logs differ; a task is run on all of them before the next one.

    python profiles/walk_live_probe.py [--tasks 6] [--nodes 20000] [--pending 50000] [--out profiles/walk_live_probe.json]
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
from walk_cursor_probe import _apply, windows  # noqa: E402

DONE = (kbhip.WALK_ASSIGNED, kbhip.WALK_EXHAUSTED)


def cursor(s, task, live, max_calls=1 << 16):
    """(l) / (k) -> (ops, ABI calls, launches, stop, T)"""
    total, binfo = s.walk_begin_live(task, 1) if live else s.walk_begin(task, False, 1)
    ops, calls, launches, pos = [], 1, binfo["launches"], 0
    while True:
        op, pod, node, info = s.walk_next(pos, 64, 4096)
        calls += 1
        launches += info["launches"]
        if len(op):
            launches += _apply(s, op, pod, node, ops)
            calls += 1
        stuck = info["stop"] == kbhip.WALK_CAPACITY and info["next"] == pos and not len(op)
        if info["stop"] in DONE or stuck or calls >= max_calls:
            return ops, calls, launches, info["stop"], total
        pos = info["next"]


def reranked(s, task, max_calls=1 << 16):
    """The reference: the fixed cursor ranked again behind every acting node.  -> (ops, ABI calls, stop)"""
    ops, calls, last = [], 0, -1
    while True:
        total, _ = s.walk_begin(task, False, 1)
        nodes = s.walk_order()[1]
        pos = int(np.searchsorted(nodes, last, side="right"))  # (by_score 0: the order is the node index)
        op, pod, node, info = s.walk_next(pos, 1, 4096)
        calls += 3
        if len(op):
            _apply(s, op, pod, node, ops)
            calls += 1
            last = info["last_node"]
        if info["stop"] in DONE or not len(op) and info["next"] in (pos, total) or calls >= max_calls:
            return ops, calls, info["stop"]
        if not len(op):
            last = int(nodes[info["next"] - 1])


def snapshot(n_nodes, n_pending, pod_affinity):
    """gen_c3 holds pending pods only: nothing to reclaim.  Here every second gang runs, its pods dealt
    round-robin over the nodes (the victims, MinAvailable 1), and the first two pods of every gang with a required
    pod-affinity term run too (the term's targets, in their nodes' zones); the rest stays pending."""
    c = kbgen.gen_c3(n_nodes=n_nodes, n_pending=n_pending, pod_affinity=pod_affinity)
    names = [n.name for n in c.nodes]
    index, count, k = {}, {}, 0
    for p in c.pods:
        j = index.setdefault(p.group, len(index))
        count[p.group] = nth = count.get(p.group, -1) + 1
        if j % 2 == 0 or ((p.affinity or {}).get("pod") or {}).get("required") and nth < 2:
            p.phase, p.node = "Running", names[k % len(names)]
            k += 1
    for j in c.jobs:  # gang lets a running gang's tasks go (gang.go:107-129 refuses a gang at its MinAvailable)
        if index.get(j.name, 1) % 2 == 0:
            j.min_member = 1
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=6)
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--pending", type=int, default=50000)
    ap.add_argument("--pod-affinity", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_live_probe.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = snapshot(a.nodes, a.pending, a.pod_affinity).write(os.path.join(d, "c3.kbs"))
        with kbhip.EncodedSnapshot(path) as enc:
            cls, job = enc.table("pod_class"), enc.table("pod_job")
            pend = [int(t) for t in np.nonzero((cls >= 0) & (job >= 0))[0]]
        out = {"snapshot": "gen_c3, every second gang and two pods of each pod-affinity gang running", "pod_affinity": a.pod_affinity, "pending": a.pending, "per_task": []}
        with kbhip.Session(path) as sl, kbhip.Session(path) as sk, kbhip.Session(path) as sc, kbhip.Session(path) as sr:
            out["nodes"] = int(sl.stats()["nodes"])
            tasks, seen = [], set()
            for t in pend:  # one task per class that reads affinity targets, until there are enough
                if int(cls[t]) in seen:
                    continue
                seen.add(int(cls[t]))
                total, info = sl.walk_begin(t, False, 1)
                if info["affinity_targets"] and total > 0:
                    tasks.append(t)
                if len(tasks) >= a.tasks or len(seen) > 4000:
                    break
            sl.walk_end()
            for s in (sl, sk, sc, sr):  # the tables built and the kernels loaded outside the timed part
                s.walk_victims_from(pend[0], False, 1, 1)
                s.walk_begin_live(pend[0], 1)
                s.walk_next(0, 1)
                s.walk_end()
            for t in tasks:
                rec = {"task": t}
                ref = reranked(sr, t)
                for name, s, run in (("l_live", sl, lambda s: cursor(s, t, True)), ("k_fixed", sk, lambda s: cursor(s, t, False)),
                                     ("c_windows", sc, lambda s: windows(s, t))):
                    t0 = time.perf_counter()
                    got = run(s)
                    us = (time.perf_counter() - t0) * 1e6
                    stop = got[3] if name != "c_windows" else got[5]
                    rec[name] = {"us": us, "calls": int(got[1]), "launches": int(got[2]), "stop": int(stop),
                                 "ops": len(got[0]), "log_equals_reference": got[0] == ref[0]}
                    if name != "c_windows":
                        rec[name]["walk_entries"] = int(got[4])
                rec["reference"] = {"calls": ref[1], "ops": len(ref[0]), "stop": int(ref[2])}
                out["per_task"].append(rec)
        out["tasks"] = len(out["per_task"])
        for name in ("l_live", "k_fixed", "c_windows"):
            rows = [r[name] for r in out["per_task"]]
            out[name] = {k: float(np.median([r[k] for r in rows])) if rows else None for k in ("us", "calls", "launches")}
            out[name]["logs_equal_reference"] = sum(r["log_equals_reference"] for r in rows)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
