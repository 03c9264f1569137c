"""kbhip_rank_heads against the per-task head calls, at C4's and C5's sizes.

Per snapshot (C4: kbgen.gen_c4, 100k nodes; C5: kbgen.gen_c5, 50k nodes and
~1.45M running pods), per victims in (0, 3) and per n in (1, 8, 64), rounds
that alternate
  (a) n head calls (first 0, cap 64, by_score 1) of the unchanged
      kbhip_rank_nodes (victims 0) / kbhip_rank_victim_nodes (victims 3), and
  (b) one kbhip_rank_heads of the same n tasks,
each timed by the host clock around calls that end in a stream synchronise.
Every shape is warmed up first (code objects, buffers, the candidate table);
the answers of (a) and (b) are compared once per shape before the timing.
Reported per shape: the median, the 10th and 90th percentile and the minimum
of the wall time per task over --reps rounds, for (a) and for (b), the sweep's
grid x and the launches of (b).  The yardstick of every figure is (a) of the
same run.  Writes one JSON object (default profiles/rank_heads_probe.json) and
prints it.

Usage: python profiles/rank_heads_probe.py [--reps R] [--warmup W] [--c4-nodes N] [--c5-nodes N] [--out PATH]
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


def snapshot(cache, name, gen):
    p = os.path.join(cache, name)
    if not os.path.exists(p):
        print("generating " + name, file=sys.stderr, flush=True)
        gen(p + ".tmp")
        os.replace(p + ".tmp", p)
    with open(p, "rb") as f:
        return f.read()


def singles(s, tasks, victims):
    if victims == 0:
        return [s.rank_nodes(t, True, 0, 64) for t in tasks]
    return [s.rank_victim_nodes(t, True, victims, 0, 64)[:4] for t in tasks]


def same(one, heads, i):
    k = min(int(one[0]), 64)
    ok = int(heads[0][i]) == int(one[0]) and np.array_equal(heads[1][i, :k], one[1]) and \
        np.array_equal(heads[2][i, :k], one[2]) and (heads[1][i, k:] == -1).all()
    if len(one) > 3:
        ok = ok and np.array_equal(heads[3][i, :k], one[3])
    return bool(ok)


def spread(us):
    a = np.sort(np.asarray(us))
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
            "p90_us": float(np.percentile(a, 90)), "min_us": float(a[0])}


def probe(buf, reps, warmup):
    out = {"shapes": []}
    with kbhip.Session(buf) as s:
        n_nodes = s.stats()["nodes"]
        out["nodes"] = int(n_nodes)
        s.read_nodes(n_nodes)
        with kbhip.EncodedSnapshot(buf) as enc:
            pend = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
        step = max(len(pend) // 64, 1)
        pool = pend[::step][:64]
        assert len(pool) == 64, "the snapshot has fewer than 64 pending tasks"
        for victims in (0, 3):
            for n in (1, 8, 64):
                tasks = pool[:n]
                for _ in range(warmup):
                    ref = singles(s, tasks, victims)
                    heads = s.rank_heads(tasks, True, victims, 64)
                assert all(same(ref[i], heads, i) for i in range(n)), (victims, n)
                a, b = [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    singles(s, tasks, victims)
                    t1 = time.perf_counter()
                    s.rank_heads(tasks, True, victims, 64)
                    t2 = time.perf_counter()
                    a.append((t1 - t0) * 1e6 / n)
                    b.append((t2 - t1) * 1e6 / n)
                out["shapes"].append({"victims": victims, "n": n, "grid_x": int(heads[4][2]),
                                      "launches": int(heads[4][1]), "walk_total_first_task": int(heads[0][0]),
                                      "single_calls_per_task": spread(a), "rank_heads_per_task": spread(b)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--c4-nodes", type=int, default=100_000)
    ap.add_argument("--c5-nodes", type=int, default=50_000)
    ap.add_argument("--pending", type=int, default=2000)
    ap.add_argument("--cache", default=os.environ.get("KBHIP_BENCH_CACHE", "/tmp/kbhip_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_heads_probe.json"))
    args = ap.parse_args()
    os.makedirs(args.cache, exist_ok=True)
    if kbhip.device_count() < 1:
        raise SystemExit("no gfx950 device: the probe measures on the GPU only")
    out = {"config": "kbhip_rank_heads against n head calls of kbhip_rank_nodes / kbhip_rank_victim_nodes",
           "reps": args.reps, "warmup": args.warmup, "by_score": 1, "cap": 64}
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
