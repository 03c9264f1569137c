"""kbhip_apply_ops at C5's size (50k nodes, ~1.45M running pods, 2k pending):
the records of the engine's own reclaim on one session — every eviction and
pipeline it decided, in order — replayed through kbhip_apply_ops on fresh
sessions: as one batch, in batches of 1024, and one operation per call (the
launch shape of one node-operation launch per decision).  Per replay: the host
wall time of the calls, their number, the sum of the launches they report, and
whether the node rows afterwards equal those of the session that ran reclaim.
Writes one JSON object (default profiles/apply_ops_probe.json) and prints it.

Usage: python profiles/apply_ops_probe.py [--nodes N] [--pending T] [--single-cap K] [--out PATH]
(--single-cap K > 0: the one-per-call replay stops after K operations; its rows are then not compared)
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-batch-1_amd"))
import numpy as np  # noqa: E402

import kbgen  # noqa: E402
import kbhip  # noqa: E402


def replay(buf, op, pod, node, batch, limit):
    """(wall seconds of the calls, calls, launches) and the node rows afterwards."""
    fn = kbhip.lib().kbhip_apply_ops
    n = len(op) if limit <= 0 else min(limit, len(op))
    launches = ctypes.c_int64(0)
    total = calls = 0
    with kbhip.Session(buf) as s:
        n_nodes = s.stats()["nodes"]
        s.read_nodes(n_nodes)  # the session's first device work is not part of the replay
        t0 = time.perf_counter()
        for i in range(0, n, batch):
            m = min(batch, n - i)
            rc = fn(s._h, ctypes.c_void_p(op.ctypes.data + i), ctypes.c_void_p(pod.ctypes.data + 4 * i),
                    ctypes.c_void_p(node.ctypes.data + 4 * i), m, ctypes.byref(launches))
            if rc != m:
                raise RuntimeError(f"kbhip_apply_ops: {rc}: {kbhip.lib().kbhip_last_error().decode()}")
            total += launches.value
            calls += 1
        rows = s.read_nodes(n_nodes)  # (waits for the device)
        wall = time.perf_counter() - t0
    return {"ops": n, "calls": calls, "wall_s": wall, "launches": total}, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pending", type=int, default=2000)
    ap.add_argument("--single-cap", type=int, default=0)
    ap.add_argument("--cache", default=os.environ.get("KBHIP_BENCH_CACHE", "/tmp/kbhip_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "apply_ops_probe.json"))
    args = ap.parse_args()
    os.makedirs(args.cache, exist_ok=True)
    p = os.path.join(args.cache, f"c5_{args.nodes}_{args.pending}_0.kbs")
    if not os.path.exists(p):
        print("generating the C5 snapshot", file=sys.stderr, flush=True)
        kbgen.gen_c5(p + ".tmp", seed=kbgen.BASE_SEED + 5, n_nodes=args.nodes, n_pending=args.pending)
        os.replace(p + ".tmp", p)
    with open(p, "rb") as f:
        buf = f.read()
    with kbhip.Session(buf) as s:
        n_nodes = s.stats()["nodes"]
        s.read_nodes(n_nodes)
        t0 = time.perf_counter()
        rpod, rnode, rkind = s.reclaim()
        reclaim_s = time.perf_counter() - t0
        st = s.stats()
        want = s.read_nodes(n_nodes)
    op = np.where(rkind == kbhip.EVICTED, kbhip.OP_EVICT, kbhip.OP_PIPELINE).astype(np.uint8)
    pod = np.ascontiguousarray(rpod, np.int32)
    node = np.ascontiguousarray(rnode, np.int32)
    out = {"config": "C5 reclaim records through kbhip_apply_ops", "nodes": int(n_nodes), "records": int(len(op)),
           "evictions": int((rkind == kbhip.EVICTED).sum()), "pipelines": int((rkind == kbhip.PIPELINED).sum()),
           "distinct_nodes": int(np.unique(node).size),
           "engine_reclaim_s": reclaim_s, "engine_reclaim_walk_s": st["evict_walk_s"],
           "engine_reclaim_rank_s": st["evict_rank_s"], "replays": {}}
    for name, batch, limit in (("one_batch", max(len(op), 1), 0), ("batches_of_1024", 1024, 0),
                               ("one_per_call", 1, args.single_cap)):
        r, rows = replay(buf, op, pod, node, batch, limit)
        r["rows_equal_reclaim"] = bool(np.array_equal(rows, want)) if r["ops"] == len(op) else None
        r["us_per_op"] = r["wall_s"] * 1e6 / max(r["ops"], 1)
        out["replays"][name] = r
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
