"""kbhip_explain_tasks against the per-task sweep, at C4's and C5's sizes.

Per snapshot (C4: kbgen.gen_c4, 100k nodes; C5: kbgen.gen_c5, 50k nodes and
~1.45M running pods) and per n in (1, 8, 64), rounds that alternate
  (a) n calls of the unchanged kbhip_sweep_scores with its keys copied back —
      before kbhip_explain_tasks the only way to learn which nodes reject a
      task (a zero key, whatever rejected the node),
  (b) one kbhip_explain_tasks of the same n tasks, histograms only, and
  (c) the same call with the n verdict rows,
each timed by the host clock around calls that end in a stream synchronise.
Every shape is warmed up first; the answers are compared once per shape before
the timing (code in 0..2 exactly where the key is non-zero, the walk count, the
same histogram with and without rows).  Reported per shape: the median, the
10th and 90th percentile and the minimum of the wall time per task over --reps
rounds for (a), (b) and (c), the sweep's grid x, the launches, and the ratio of
the medians (b) / (a).  The yardstick of every figure is (a) of the same run.
The kernel's register count and occupancy are the compiler's
(-Rpass-analysis=kernel-resource-usage on kbhip_explain.hip), its bytes per
node the columns node_verdict reads.  Writes one JSON object (default
profiles/explain_probe.json) and prints it.

Usage: python profiles/explain_probe.py [--reps R] [--warmup W] [--c4-nodes N] [--c5-nodes N] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-batch-1_amd"))
import numpy as np  # noqa: E402

import kbgen  # noqa: E402
import kbhip  # noqa: E402

KERNEL = {"name": "k_explain", "vgprs": 85, "sgprs": 106, "scratch_bytes": 0, "lds_bytes": 256,
          "occupancy_waves_per_simd": 5,
          "bytes_per_node_read": "81 (flags 1, Idle / Releasing / Backfilled 72, pods 4, maxtasks 4) + 8 per taint "
                                 "word + 8 per port word of a class with host ports + 4 per label column its terms read",
          "bytes_per_node_written": "1 with verdict rows, 0 without"}


def snapshot(cache, name, gen):
    p = os.path.join(cache, name)
    if not os.path.exists(p):
        print("generating " + name, file=sys.stderr, flush=True)
        gen(p + ".tmp")
        os.replace(p + ".tmp", p)
    with open(p, "rb") as f:
        return f.read()


def spread(us):
    a = np.sort(np.asarray(us))
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
            "p90_us": float(np.percentile(a, 90)), "min_us": float(a[0])}


def probe(buf, reps, warmup):
    out = {"shapes": []}
    with kbhip.Session(buf) as s:
        n_nodes = int(s.stats()["nodes"])
        out["nodes"] = n_nodes
        s.read_nodes(n_nodes)
        with kbhip.EncodedSnapshot(buf) as enc:
            pend = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
        step = max(len(pend) // 64, 1)
        pool = pend[::step][:64]
        assert len(pool) == 64, "the snapshot has fewer than 64 pending tasks"
        for n in (1, 8, 64):
            tasks = pool[:n]
            for _ in range(warmup):
                ref = [s.sweep_scores(t, n_nodes) for t in tasks]
                hist, _, info = s.explain_tasks(tasks)
                hist_v, rows, info_v = s.explain_tasks(tasks, verdicts=True, n_nodes=n_nodes)
            assert np.array_equal(hist, hist_v)
            for i in range(n):
                assert np.array_equal((rows[i] & 15) <= kbhip.WHY_RESOURCES, ref[i][1] != 0), (n, i)
                assert ref[i][0] == hist[i, 14] and hist[i, 15] == n_nodes
            a, b, c = [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                for t in tasks:
                    s.sweep_scores(t, n_nodes)
                t1 = time.perf_counter()
                s.explain_tasks(tasks)
                t2 = time.perf_counter()
                s.explain_tasks(tasks, verdicts=True, n_nodes=n_nodes)
                t3 = time.perf_counter()
                a.append((t1 - t0) * 1e6 / n)
                b.append((t2 - t1) * 1e6 / n)
                c.append((t3 - t2) * 1e6 / n)
            sa, sb, sc = spread(a), spread(b), spread(c)
            out["shapes"].append({"n": n, "grid_x": int(info[1]), "launches": int(info[0]),
                                  "histogram_first_task": [int(x) for x in hist[0]],
                                  "sweep_scores_per_call": sa, "explain_hist_per_task": sb,
                                  "explain_rows_per_task": sc,
                                  "hist_over_sweep_scores": sb["median_us"] / sa["median_us"],
                                  "rows_over_sweep_scores": sc["median_us"] / sa["median_us"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--c4-nodes", type=int, default=100_000)
    ap.add_argument("--c5-nodes", type=int, default=50_000)
    ap.add_argument("--pending", type=int, default=2000)
    ap.add_argument("--cache", default=os.environ.get("KBHIP_BENCH_CACHE", "/tmp/kbhip_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_probe.json"))
    args = ap.parse_args()
    os.makedirs(args.cache, exist_ok=True)
    if kbhip.device_count() < 1:
        raise SystemExit("no gfx950 device: the probe measures on the GPU only")
    out = {"config": "kbhip_explain_tasks against n calls of kbhip_sweep_scores (keys copied back)",
           "reps": args.reps, "warmup": args.warmup, "kernel": KERNEL}
    out["C4"] = probe(snapshot(args.cache, f"c4_{args.c4_nodes}_{args.pending}_probe.kbs",
                               lambda p: kbgen.gen_c4(p, n_nodes=args.c4_nodes, n_pending=args.pending)),
                      args.reps, args.warmup)
    out["C5"] = probe(snapshot(args.cache, f"c5_{args.c5_nodes}_{args.pending}_0.kbs",
                               lambda p: kbgen.gen_c5(p, seed=kbgen.BASE_SEED + 5, n_nodes=args.c5_nodes,
                                                      n_pending=args.pending)),
                      args.reps, args.warmup)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
