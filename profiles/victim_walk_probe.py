"""kbhip_rank_victim_nodes at C5's size (50k nodes, ~1.45M running pods, 2k
pending): what the pruned walk removes and what it costs, each time against
the unchanged call in the same run.

Tasks: the first pending tasks the engine's own reclaim pipelines on a session
of its own (the tasks reclaim takes first); every measurement below runs on
fresh sessions that never ran an action.  Per mode (1 other queues, by_score
0 as reclaim walks; 2 / 3 same queue / same job, by_score 1 as preempt walks):
  - per task the length of kbhip_rank_nodes' walk and of the pruned one;
  - the wall time of a head call (first 0, cap 64) of each, alternating, the
    median over --reps rounds;
and once per run:
  - the first kbhip_rank_victim_nodes call of a session (it builds and uploads
    the candidate table) and a full-path call of each function;
  - the engine's reclaim records replayed through kbhip_apply_ops in batches
    of 1024 on a session whose table is live and on one that never ranked.
Writes one JSON object (default profiles/victim_walk_probe.json) and prints it.

Usage: python profiles/victim_walk_probe.py [--nodes N] [--pending T] [--tasks K] [--reps R] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-batch-1_amd"))
import numpy as np  # noqa: E402

import kbgen  # noqa: E402
import kbhip  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def replay(s, op, pod, node, batch):
    """Wall seconds of the records through apply_ops in batches (the last read waits for the device)."""
    n_nodes = s.stats()["nodes"]
    launches = calls = 0
    t0 = time.perf_counter()
    for i in range(0, len(op), batch):
        launches += s.apply_ops(op[i:i + batch], pod[i:i + batch], node[i:i + batch])
        calls += 1
    s.read_nodes(n_nodes)
    return {"ops": int(len(op)), "calls": calls, "launches": int(launches), "wall_s": time.perf_counter() - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pending", type=int, default=2000)
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cache", default=os.environ.get("KBHIP_BENCH_CACHE", "/tmp/kbhip_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "victim_walk_probe.json"))
    args = ap.parse_args()
    os.makedirs(args.cache, exist_ok=True)
    p = os.path.join(args.cache, f"c5_{args.nodes}_{args.pending}_0.kbs")
    if not os.path.exists(p):
        print("generating the C5 snapshot", file=sys.stderr, flush=True)
        kbgen.gen_c5(p + ".tmp", seed=kbgen.BASE_SEED + 5, n_nodes=args.nodes, n_pending=args.pending)
        os.replace(p + ".tmp", p)
    with open(p, "rb") as f:
        buf = f.read()
    with kbhip.Session(buf) as own:
        n_nodes = own.stats()["nodes"]
        own.read_nodes(n_nodes)
        reclaim_s, (rpod, rnode, rkind) = timed(own.reclaim)
        st = own.stats()
    tasks = []
    for q, k in zip(rpod.tolist(), rkind.tolist()):
        if k == kbhip.PIPELINED and q not in tasks:
            tasks.append(q)
        if len(tasks) == args.tasks:
            break
    out = {"config": "C5: kbhip_rank_victim_nodes against kbhip_rank_nodes", "nodes": int(n_nodes),
           "tasks": tasks, "reps": args.reps, "engine_reclaim_s": reclaim_s,
           "engine_reclaim_walk_s": st["evict_walk_s"], "engine_reclaim_visits": st["evict_visits"],
           "engine_reclaim_cands": st["evict_cands"], "modes": {}}
    with kbhip.Session(buf) as s:
        s.read_nodes(n_nodes)
        t = tasks[0]
        s.rank_nodes(t, False, 0, 64)  # the head path's buffers and code objects
        first_s, first = timed(lambda: s.rank_victim_nodes(t, False, 1, 0, 64))
        assert first[4]["rebuilt"] == 1
        second_s, second = timed(lambda: s.rank_victim_nodes(t, False, 1, 0, 64))
        assert second[4]["rebuilt"] == 0
        out["first_call_with_table_build_s"] = first_s
        out["same_call_again_s"] = second_s
        s.rank_nodes(t, False, 0, 65)
        s.rank_victim_nodes(t, False, 1, 0, 65)
        out["full_path_rank_nodes_s"] = statistics.median(timed(lambda: s.rank_nodes(t, False, 0, 65))[0]
                                                           for _ in range(args.reps))
        out["full_path_rank_victim_nodes_s"] = statistics.median(
            timed(lambda: s.rank_victim_nodes(t, False, 1, 0, 65))[0] for _ in range(args.reps))
        for mode, by_score in ((1, False), (2, True), (3, True)):
            rows = []
            for t in tasks:
                full = s.rank_nodes(t, by_score, 0, 0)[0]
                pruned = s.rank_victim_nodes(t, by_score, mode, 0, 0)[0]
                a, b = [], []
                for _ in range(args.reps):
                    a.append(timed(lambda: s.rank_nodes(t, by_score, 0, 64))[0])
                    b.append(timed(lambda: s.rank_victim_nodes(t, by_score, mode, 0, 64))[0])
                rows.append({"task": t, "walk": int(full), "pruned_walk": int(pruned),
                             "head_rank_nodes_us": statistics.median(a) * 1e6,
                             "head_rank_victim_nodes_us": statistics.median(b) * 1e6})
            out["modes"][str(mode)] = {
                "by_score": int(by_score), "per_task": rows,
                "walk_sum": sum(r["walk"] for r in rows), "pruned_walk_sum": sum(r["pruned_walk"] for r in rows)}
    op = np.where(rkind == kbhip.EVICTED, kbhip.OP_EVICT, kbhip.OP_PIPELINE).astype(np.uint8)
    pod, node = np.ascontiguousarray(rpod, np.int32), np.ascontiguousarray(rnode, np.int32)
    out["apply_ops_batches_of_1024"] = {}
    for name, rank_first in (("never_ranked", False), ("table_live", True), ("never_ranked_again", False),
                             ("table_live_again", True)):
        with kbhip.Session(buf) as s:
            s.read_nodes(n_nodes)
            if rank_first:
                assert s.rank_victim_nodes(tasks[0], False, 1, 0, 64)[4]["rebuilt"] == 1
            r = replay(s, op, pod, node, 1024)
            if rank_first:  # the table followed the whole replay: the next ranking does not rebuild it
                r["rebuilt_after"] = None
                for q in np.nonzero(s.table("pod_status") == 1)[0][:64].tolist():  # a task still Pending
                    try:
                        r["rebuilt_after"] = s.rank_victim_nodes(q, False, 1, 0, 64)[4]["rebuilt"]
                        break
                    except kbhip.KbhipError:  # (a Pending pod without a task class)
                        continue
            r["us_per_op"] = r["wall_s"] * 1e6 / max(r["ops"], 1)
            out["apply_ops_batches_of_1024"][name] = r
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
