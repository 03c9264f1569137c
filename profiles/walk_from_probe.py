"""kbhip_walk_victims_from against kbhip_walk_victims and the per-node recipe, at C5.

One task's reclaim node loop through the Python binding, three ways, on three
sessions of the same snapshot, alternating task by task so that all see the
same drift of the machine:
  (a) the per-node recipe of §4.18: kbhip_head_victims, act on the first valid
      node after the last one acted on, kbhip_apply_ops, ask again;
  (b) kbhip_walk_victims, then one kbhip_apply_ops with its batch: the
      baseline;
  (c) kbhip_walk_victims_from, then kbhip_apply_ops.
So that the three sessions move through the same states and the op logs can
be compared, all three decide the same entries: the task's first window, the
64-entry head as ranked at its first call — as far as (a) and (b) can go.
(a) reads only rows of that head's nodes when it asks again, (b) and (c) stop
at HEAD_END and go on only after a CAPACITY stop.
All apply what they decide; the op logs are compared task by task.  The tasks
are the sample of walk_victims_probe.py (pending tasks in pod order).
After the comparison a fourth, fresh session runs (c)'s protocol to its end —
ASSIGNED or EXHAUSTED, however long the walk — for the first --full tasks,
which nothing else here can do: calls, windows and wall time per task.

    python profiles/walk_from_probe.py [--tasks 120] [--full 8] [--out profiles/walk_from_probe.json]
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
from walk_victims_probe import STRIDE, _pct  # noqa: E402


def per_node_window(s, node_of, task):
    """(a) over the first window: walk_victims_probe.per_node, reading only rows of the nodes the first head
    held (a later head starts again at the top and can hold a few entries more).  -> (ops, calls, acted)."""
    ops, calls, acted, after, window = [], 0, 0, -1, None
    while True:
        n, nodes, _, count, evict, flags, rows, info = s.head_victims(task, False, 1, 64, STRIDE)
        calls += 1
        if info["max_count"] > STRIDE:  # a truncated row: asked again with room for the longest
            n, nodes, _, count, evict, flags, rows, info = s.head_victims(task, False, 1, 64, info["max_count"])
            calls += 1
        if window is None:
            window = {int(x) for x in nodes[:min(n, 64)]}
        hit = [i for i in range(min(n, 64))
               if nodes[i] > after and int(nodes[i]) in window and flags[i] & kbhip.HEAD_VICTIMS_VALID]
        if not hit:
            return ops, calls, acted
        i = hit[0]
        batch = [(kbhip.OP_EVICT, int(v), int(node_of[v])) for v in rows[i][:int(evict[i])]]
        covers = bool(flags[i] & kbhip.HEAD_VICTIMS_COVERS)
        if covers:
            batch.append((kbhip.OP_PIPELINE, task, int(nodes[i])))
        s.apply_ops([o for o, _, _ in batch], [p for _, p, _ in batch], [x for _, _, x in batch])
        calls += 1
        acted += 1
        ops += batch
        after = int(nodes[i])
        if covers:
            return ops, calls, acted


def walked_window(s, task):
    """(b) over the first window: kbhip_walk_victims, resumed after a CAPACITY stop only (a resumed call
    after HEAD_END would rank the head again).  -> (ops, calls, acted, entries decided)."""
    ops, calls, acted, visited, after = [], 0, 0, 0, None
    while True:
        op, pod, node, info = s.walk_victims(task, False, 1, 64, after, 4096)
        calls += 1
        acted += info["acted"]
        visited += info["visited"]
        if len(op):
            s.apply_ops(op, pod, node)
            calls += 1
            ops += [(int(o), int(p), int(n)) for o, p, n in zip(op, pod, node)]
        if info["stop"] != kbhip.WALK_CAPACITY or info["acted"] == 0:
            return ops, calls, acted, visited
        after = (info["last_node"], info["last_score"])


def walked_from(s, task, first_window_only=True, max_calls=1 << 20):
    """(c): -> (ops, ABI calls, acted-on nodes, entries decided, the walk calls' wall time in us, stop)."""
    ops, calls, acted, visited, walk_us, after = [], 0, 0, 0, 0.0, None
    while True:
        t0 = time.perf_counter()
        op, pod, node, info = s.walk_victims_from(task, False, 1, 64, after, 4096)
        walk_us += (time.perf_counter() - t0) * 1e6
        calls += 1
        acted += info["acted"]
        visited += info["visited"]
        if len(op):
            s.apply_ops(op, pod, node)
            calls += 1
            ops += [(int(o), int(p), int(n)) for o, p, n in zip(op, pod, node)]
        done = info["stop"] in (kbhip.WALK_ASSIGNED, kbhip.WALK_EXHAUSTED)
        stuck = info["stop"] == kbhip.WALK_CAPACITY and info["visited"] <= 1 and info["acted"] == 0
        if done or stuck or (first_window_only and info["stop"] == kbhip.WALK_HEAD_END) or calls >= max_calls:
            return ops, calls, acted, visited, walk_us, info["stop"]
        after = (info["resume_node"], info["resume_score"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=120)
    ap.add_argument("--full", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_from_probe.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "c5.kbs")
        kbgen.gen_c5(path)
        with kbhip.EncodedSnapshot(path) as enc:
            cls, job = enc.table("pod_class"), enc.table("pod_job")
            pend = np.nonzero((cls >= 0) & (job >= 0))[0]
        tasks = [int(t) for t in pend[:: max(1, len(pend) // a.tasks)][:a.tasks]]
        rec = {k: [] for k in ("a_us", "b_us", "c_us", "a_calls", "b_calls", "c_calls", "acted", "visited",
                               "c_walk_us_per_call")}
        same = 0
        with kbhip.Session(path) as sa, kbhip.Session(path) as sb, kbhip.Session(path) as sc:
            node_of = sa.table("pod_node").copy()
            for s in (sa, sb, sc):  # the tables built and the kernels loaded outside the timed part
                s.head_victims(tasks[0], False, 1, 64, STRIDE)
                s.walk_victims(tasks[0], False, 1, 1)
                s.walk_victims_from(tasks[0], False, 1, 1)
                s.walk_victims_from(tasks[0], False, 1, 1, (0, 0))
            for k, t in enumerate(tasks):
                order = ("abc", "bca", "cab")[k % 3]
                got = {}
                for which in order:
                    t0 = time.perf_counter()
                    got[which] = (per_node_window(sa, node_of, t) if which == "a" else walked_window(sb, t) if which == "b"
                                  else walked_from(sc, t))
                    got[which + "_us"] = (time.perf_counter() - t0) * 1e6
                same += got["a"][0] == got["b"][0] == got["c"][0]
                for w in "abc":
                    rec[w + "_us"].append(got[w + "_us"])
                    rec[w + "_calls"].append(got[w][1])
                rec["acted"].append(got["c"][2]); rec["visited"].append(got["c"][3])
                n_walk = got["c"][1] - (1 if got["c"][0] else 0)
                rec["c_walk_us_per_call"].append(got["c"][4] / max(n_walk, 1))
        acted = np.array(rec["acted"])
        out = {"snapshot": "gen_c5", "tasks": len(tasks), "logs_equal": same,
               "acted_nodes_per_task": _pct(acted), "window_entries_decided_per_task": _pct(rec["visited"]),
               "a_per_node": {"calls_per_task": _pct(rec["a_calls"]), "wall_us_per_task": _pct(rec["a_us"])},
               "b_walk": {"calls_per_task": _pct(rec["b_calls"]), "wall_us_per_task": _pct(rec["b_us"])},
               "c_walk_from": {"calls_per_task": _pct(rec["c_calls"]), "wall_us_per_task": _pct(rec["c_us"]),
                               "walk_call_us": _pct(rec["c_walk_us_per_call"])},
               "by_acted_nodes": {}}
        for lo, hi, name in ((0, 0, "0"), (1, 1, "1"), (2, 4, "2-4"), (5, 1 << 30, "5+")):
            pick = (acted >= lo) & (acted <= hi)
            if pick.any():
                au, bu, cu = (np.array(rec[w + "_us"])[pick] for w in "abc")
                out["by_acted_nodes"][name] = {"tasks": int(pick.sum()), "a_wall_us": _pct(au), "b_wall_us": _pct(bu),
                                               "c_wall_us": _pct(cu),
                                               "c_over_b_median": float(np.median(cu) / np.median(bu)),
                                               "c_over_a_median": float(np.median(cu) / np.median(au))}
        # the protocol to its end on a fresh session: walks of any length
        full = {k: [] for k in ("calls", "windows", "us", "visited", "acted", "stop")}
        with kbhip.Session(path) as sd:
            sd.walk_victims_from(tasks[0], False, 1, 1)
            sd.walk_victims_from(tasks[0], False, 1, 1, (0, 0))
            for t in tasks[:a.full]:
                t0 = time.perf_counter()
                ops, calls, n_act, visited, _, stop = walked_from(sd, t, first_window_only=False)
                full["us"].append((time.perf_counter() - t0) * 1e6)
                full["calls"].append(calls); full["visited"].append(visited); full["acted"].append(n_act)
                full["windows"].append(-(-visited // 64)); full["stop"].append(int(stop))
        if full["us"]:
            out["c_to_the_end"] = {"tasks": len(full["us"]), "calls_per_task": _pct(full["calls"]),
                                   "entries_decided_per_task": _pct(full["visited"]),
                                   "acted_nodes_per_task": _pct(full["acted"]), "wall_us_per_task": _pct(full["us"]),
                                   "wall_us_per_64_entries": _pct(np.array(full["us"]) / np.maximum(full["windows"], 1)),
                                   "stops": sorted(set(full["stop"]))}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
