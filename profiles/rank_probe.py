"""Wall time of one ranked node walk request on a C4-shaped session.

After kbhip_allocate on a gen_c4 snapshot (100k nodes by default), for a
handful of still-pending tasks, three ways for a host to get preempt's walk
(preempt.go:270-287) are timed per request, binding overhead included:

  sweep_sort  kbhip_sweep_scores (all N keys copied back) + a host sort of the
              non-zero keys, descending (numpy here) — all a host could do
              before kbhip_rank_nodes existed;
  rank_head   kbhip_rank_nodes, first 0, cap 64 (the top-64 kernel);
  rank_full   kbhip_rank_nodes, every entry (the full device sort).

Each request is repeated --reps times after --warmup unrecorded ones; the
median, minimum and 90th percentile in microseconds go to the JSON, per task
and pooled.  by_index repeats rank_head / rank_full for reclaim's order.

    python profiles/rank_probe.py [--nodes N] [--pending P] [--tasks K] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-batch-1_amd"))

import kbgen  # noqa: E402
import kbhip  # noqa: E402


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    a = np.asarray(us)
    return {"median_us": float(np.median(a)), "min_us": float(a.min()), "p90_us": float(np.percentile(a, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--pending", type=int, default=200_000)
    ap.add_argument("--tasks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_probe.json"))
    a = ap.parse_args()

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "c4.kbs")
        meta = kbgen.gen_c4(path, n_nodes=a.nodes, n_pending=a.pending)
        with kbhip.EncodedSnapshot(path) as enc:
            pend = np.nonzero(enc.table("pod_class") >= 0)[0]
        with kbhip.Session(path) as s:
            placed = len(s.allocate()[0])
            status = s.table("pod_status")
            todo = [int(q) for q in pend if status[q] == 1]
            state = "after allocate"
            if not todo:  # everything was placed: nothing left to rank in this session
                raise SystemExit("no task is still pending after allocate: raise --pending")
            step = max(len(todo) // a.tasks, 1)
            todo = todo[::step][: a.tasks]
            N = a.nodes
            rows = []
            for pod in todo:
                total, keys = s.sweep_scores(pod, N)

                def sweep_sort():
                    _, k = s.sweep_scores(pod, N)
                    k = k[k != 0]
                    k[::-1].sort()  # ascending sort of the reversed view = descending in place
                    return k

                ref = sweep_sort()
                t_h, n_h, _ = s.rank_nodes(pod, True, 0, 64)
                t_f, n_f, _ = s.rank_nodes(pod, True, 0, max(total, 65))
                exp = (0x7FFFFFFF - ((ref >> np.uint64(1)) & np.uint64(0x7FFFFFFF)).astype(np.int64)).astype(np.int32)
                assert t_h == t_f == total and np.array_equal(n_f, exp) and np.array_equal(n_h, exp[:64])
                rows.append({
                    "task": pod, "passing_nodes": int(total),
                    "sweep_sort": _time(sweep_sort, a.reps, a.warmup),
                    "rank_head": _time(lambda: s.rank_nodes(pod, True, 0, 64), a.reps, a.warmup),
                    "rank_full": _time(lambda: s.rank_nodes(pod, True, 0, max(total, 65)), a.reps, a.warmup),
                    "by_index_head": _time(lambda: s.rank_nodes(pod, False, 0, 64), a.reps, a.warmup),
                    "by_index_full": _time(lambda: s.rank_nodes(pod, False, 0, max(total, 65)), a.reps, a.warmup),
                })
            st = s.stats()
    pooled = {k: float(np.median([r[k]["median_us"] for r in rows]))
              for k in ("sweep_sort", "rank_head", "rank_full", "by_index_head", "by_index_full")}
    out = {"config": {"nodes": a.nodes, "pending": a.pending, "placed_by_allocate": placed, "state": state,
                      "reps": a.reps, "warmup": a.warmup, "snapshot": meta},
           "median_of_task_medians_us": pooled, "tasks": rows,
           "rank_heads": int(st["rank_heads"]), "rank_fulls": int(st["rank_fulls"])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(pooled))


if __name__ == "__main__":
    main()
