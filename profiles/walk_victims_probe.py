"""kbhip_walk_victims against the per-node recipe it replaces, at C5.

One task's reclaim node loop through the Python binding, two ways, on two
sessions of the same snapshot, alternating task by task so that both see the
same drift of the machine:
  (a) the per-node recipe: kbhip_head_victims, act on the first valid node
      after the last one acted on, kbhip_apply_ops, ask again — one round trip
      per acted-on node and one last call that finds nothing more;
  (b) kbhip_walk_victims, then one kbhip_apply_ops with its batch (another
      pair after a CAPACITY or HEAD_END stop).
Both apply what they decide, so both sessions move through the same states;
the op logs of the two are compared task by task.  The tasks are a sample of
the pending tasks in pod order (not reclaim's queue order: the probe measures
the calls, not the action).  Recorded per task: ABI calls, host wall time, and
for (b) the wall time per decided head entry; medians and 10th - 90th
percentiles go to walk_victims_probe.json.

    python profiles/walk_victims_probe.py [--tasks 200] [--out profiles/walk_victims_probe.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "kube-batch-1_amd")]
import kbgen  # noqa: E402
import kbhip  # noqa: E402

STRIDE = 64


def _pct(v):
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}


def per_node(s, node_of, task):
    """(a): -> (ops, ABI calls, acted-on nodes)."""
    ops, calls, acted, after = [], 0, 0, -1
    while True:
        n, nodes, _, count, evict, flags, rows, info = s.head_victims(task, False, 1, 64, STRIDE)
        calls += 1
        if info["max_count"] > STRIDE:  # a truncated row: asked again with room for the longest
            n, nodes, _, count, evict, flags, rows, info = s.head_victims(task, False, 1, 64, info["max_count"])
            calls += 1
        hit = [i for i in range(min(n, 64)) if nodes[i] > after and flags[i] & kbhip.HEAD_VICTIMS_VALID]
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


def walked(s, task):
    """(b): -> (ops, ABI calls, acted-on nodes, head entries decided, the walk calls' wall time in us)."""
    ops, calls, acted, visited, walk_us, after = [], 0, 0, 0, 0.0, None
    while True:
        t0 = time.perf_counter()
        op, pod, node, info = s.walk_victims(task, False, 1, 64, after, 4096)
        walk_us += (time.perf_counter() - t0) * 1e6
        calls += 1
        acted += info["acted"]
        visited += info["visited"]
        if len(op):
            s.apply_ops(op, pod, node)
            calls += 1
            ops += [(int(o), int(p), int(n)) for o, p, n in zip(op, pod, node)]
        if info["stop"] in (kbhip.WALK_ASSIGNED, kbhip.WALK_EXHAUSTED) or info["acted"] == 0:
            return ops, calls, acted, visited, walk_us
        after = (info["last_node"], info["last_score"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_victims_probe.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "c5.kbs")
        kbgen.gen_c5(path)
        with kbhip.EncodedSnapshot(path) as enc:
            cls, job = enc.table("pod_class"), enc.table("pod_job")
            pend = np.nonzero((cls >= 0) & (job >= 0))[0]
        tasks = [int(t) for t in pend[:: max(1, len(pend) // a.tasks)][:a.tasks]]
        rec = {k: [] for k in ("a_calls", "b_calls", "a_us", "b_us", "acted", "visited", "b_walk_us_per_entry")}
        same = 0
        with kbhip.Session(path) as sa, kbhip.Session(path) as sb:
            node_of = sa.table("pod_node").copy()
            for s in (sa, sb):  # the tables built and the kernels loaded outside the timed part
                s.head_victims(tasks[0], False, 1, 64, STRIDE)
                s.walk_victims(tasks[0], False, 1, 1)
            for k, t in enumerate(tasks):
                order = ("a", "b") if k % 2 == 0 else ("b", "a")
                got = {}
                for which in order:
                    t0 = time.perf_counter()
                    got[which] = per_node(sa, node_of, t) if which == "a" else walked(sb, t)
                    got[which + "_us"] = (time.perf_counter() - t0) * 1e6
                same += got["a"][0] == got["b"][0]
                rec["a_calls"].append(got["a"][1]); rec["b_calls"].append(got["b"][1])
                rec["a_us"].append(got["a_us"]); rec["b_us"].append(got["b_us"])
                rec["acted"].append(got["b"][2]); rec["visited"].append(got["b"][3])
                if got["b"][3]:
                    rec["b_walk_us_per_entry"].append(got["b"][4] / got["b"][3])
        acted = np.array(rec["acted"])
        out = {"snapshot": "gen_c5", "tasks": len(tasks), "logs_equal": same,
               "acted_nodes_per_task": _pct(acted), "head_entries_decided_per_task": _pct(rec["visited"]),
               "a_per_node": {"calls_per_task": _pct(rec["a_calls"]), "wall_us_per_task": _pct(rec["a_us"])},
               "b_walk": {"calls_per_task": _pct(rec["b_calls"]), "wall_us_per_task": _pct(rec["b_us"]),
                          "walk_call_us_per_decided_entry": _pct(rec["b_walk_us_per_entry"] or [0])},
               "by_acted_nodes": {}}
        for lo, hi, name in ((0, 0, "0"), (1, 1, "1"), (2, 4, "2-4"), (5, 1 << 30, "5+")):
            pick = (acted >= lo) & (acted <= hi)
            if pick.any():
                out["by_acted_nodes"][name] = {"tasks": int(pick.sum()),
                                               "a_wall_us": _pct(np.array(rec["a_us"])[pick]),
                                               "b_wall_us": _pct(np.array(rec["b_us"])[pick])}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
