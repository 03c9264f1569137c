"""kbhip_head_victims against the plain head call it extends, at C5.

One run, alternating repetitions, host wall clock around calls that end in a
stream synchronise (the methodology of §4.15): for 8 pending tasks and the
three victim modes
  (a) kbhip_rank_victim_nodes(task, by_score, mode, 0, 64): the yardstick
  (b) kbhip_head_victims with cap 64 and with cap 8
  (c) the first call's build and upload (time of the call that rebuilt)
  (d) a call after 1024 operations went through kbhip_apply_ops (the patch)
and kbhip_stats.evict_visits of a kbhip_reclaim on a second session, the bound
on the host work the call replaces.  Medians go to head_victims_probe.json.

    python profiles/head_victims_probe.py [--reps 100] [--out profiles/head_victims_probe.json]
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


def _timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e6, r


def _med(v):
    return {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)),
            "p90_us": float(np.percentile(v, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_victims_probe.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "c5.kbs")
        kbgen.gen_c5(path)
        with kbhip.EncodedSnapshot(path) as enc:
            pend = np.nonzero(enc.table("pod_class") >= 0)[0]
        tasks = [int(t) for t in pend[:: max(1, len(pend) // 8)][:8]]
        out = {"snapshot": "gen_c5", "tasks": tasks, "reps": a.reps, "modes": {}}
        with kbhip.Session(path) as s:
            us, first = _timed(lambda: s.head_victims(tasks[0], False, 1, 64, 16))
            built = s.table_raw("victim_state", np.int64)
            out["first_call"] = {"us": us, "info": first[7], "state_bytes": int(built[0]),
                                 "build_and_upload_us": int(built[1]), "candidate_tasks": int(built[2]),
                                 "largest_node": int(built[3])}
            for mode in (1, 2, 3):
                ta, tb64, tb8, heads = [], [], [], []
                for r in range(-5, a.reps):  # five warm-up rounds
                    for t in tasks:
                        try:
                            x, ra = _timed(lambda: s.rank_victim_nodes(t, mode != 1, mode, 0, 64))
                            y, rb = _timed(lambda: s.head_victims(t, mode != 1, mode, 64, 16))
                            z, _ = _timed(lambda: s.head_victims(t, mode != 1, mode, 8, 16))
                        except kbhip.KbhipError:
                            continue  # (a task without a job)
                        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1][:len(ra[1])])
                        if r >= 0:
                            ta.append(x); tb64.append(y); tb8.append(z); heads.append(min(ra[0], 64))
                if ta:
                    d64 = float(np.median(tb64) - np.median(ta))
                    out["modes"][mode] = {"a_head": _med(ta), "b_cap64": _med(tb64), "b_cap8": _med(tb8),
                                          "b_minus_a_us": d64, "head_nodes_mean": float(np.mean(heads)),
                                          "b_minus_a_per_head_node_us": d64 / max(float(np.mean(heads)), 1.0)}
            # (d): 1024 evictions, then one call that patches
            st, job, node = s.table("pod_status"), s.table("pod_job"), s.table("pod_node")
            run = [int(p) for p in np.nonzero((st == 64) & (job >= 0) & (node >= 0))[0][:1024]]
            s.apply_ops([kbhip.OP_EVICT] * len(run), run)
            us, got = _timed(lambda: s.head_victims(tasks[0], False, 1, 64, 16))
            out["after_1024_ops"] = {"us": us, "info": got[7]}
        with kbhip.Session(path) as s:
            us, _ = _timed(s.reclaim)
            stt = s.stats()
            out["reclaim"] = {"us": us, "evict_visits": int(stt["evict_visits"]), "evict_cands": int(stt["evict_cands"]),
                              "evict_walk_s": float(stt["evict_walk_s"])}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
