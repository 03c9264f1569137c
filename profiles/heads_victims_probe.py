"""kbhip_heads_victims against the per-task call it batches, at C5.

One run, alternating repetitions, host wall clock around calls that end in a
stream synchronise (the methodology of §4.16): for 64 pending tasks sampled in
pod order and the three victim modes
  (a)  64 kbhip_head_victims calls (cap 64, stride 16), this build, through
       raw ctypes calls into preallocated buffers on a session of its own
  (a0) the same 64 calls, made the same way, on a baseline library
       (--baseline-lib: the parent commit's build) in the same process
  (b)  one kbhip_heads_victims call of the 64 tasks through the Python
       binding (its allocations included); also of the first 16 and 8 of
       them, and of the 64 with cap 8
  (h)  one kbhip_rank_heads call of the 64 tasks in the same victims mode: (b)
       minus (h) is what the victims launch, the larger copy back and the
       unpacking add to the batched heads
The rows of (a) and (b) are compared for every task before anything is timed.
Medians with 10th / 90th percentiles go to heads_victims_probe.json.

    python profiles/heads_victims_probe.py [--reps 50] [--baseline-lib PATH] [--out profiles/heads_victims_probe.json]
"""
import argparse
import ctypes
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

CAP, STRIDE = 64, 16


def _med(v):
    return {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)),
            "p90_us": float(np.percentile(v, 90))}


class Baseline:
    """kbhip_head_victims of another build of the library, on its own session."""

    def __init__(self, lib_path, snapshot):
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        self.L = ctypes.CDLL(lib_path)
        self.L.kbhip_session_open_file.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(vp)]
        self.L.kbhip_session_close.argtypes = [vp]
        self.L.kbhip_head_victims.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        self.L.kbhip_head_victims.restype = ctypes.c_int64
        self.h = vp()
        assert self.L.kbhip_session_open_file(snapshot.encode(), 0, ctypes.byref(self.h)) == 0
        self.node, self.score = np.zeros(CAP, np.int32), np.zeros(CAP, np.int32)
        self.count, self.evict = np.zeros(CAP, np.int32), np.zeros(CAP, np.int32)
        self.flags, self.victim = np.zeros(CAP, np.uint8), np.zeros(CAP * STRIDE, np.int32)
        self.info = np.zeros(5, np.int64)
        self.ptr = [x.ctypes.data for x in (self.node, self.score, self.count, self.evict, self.flags, self.victim,
                                            self.info)]

    def head_victims(self, task, by_score, mode):
        n = int(self.L.kbhip_head_victims(self.h, task, int(by_score), mode, CAP, STRIDE, *self.ptr))
        assert n >= 0
        return n

    def close(self):
        self.L.kbhip_session_close(self.h)


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads_victims_probe.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "c5.kbs")
        kbgen.gen_c5(path)
        with kbhip.EncodedSnapshot(path) as enc:
            pend = np.nonzero((enc.table("pod_class") >= 0) & (enc.table("pod_job") >= 0))[0]
        tasks = [int(t) for t in pend[:: max(1, len(pend) // 64)][:64]]
        out = {"snapshot": "gen_c5", "tasks": len(tasks), "reps": a.reps, "cap": CAP, "stride": STRIDE,
               "baseline": bool(a.baseline_lib), "modes": {}}
        base = Baseline(a.baseline_lib, path) if a.baseline_lib else None
        own = Baseline(kbhip.LIB_PATH, path)
        with kbhip.Session(path) as s:
            s.head_victims(tasks[0], False, 1, CAP, STRIDE)  # the tables built
            built = s.table_raw("victim_state", np.int64)
            out["largest_node"] = int(built[3])
            equal = True
            for mode in (1, 2, 3):
                by_score = mode != 1
                # the rows of (a) and (b), compared for every task
                got = s.heads_victims(tasks, by_score, mode, CAP, STRIDE)
                acting = 0
                for i, t in enumerate(tasks):
                    one = s.head_victims(t, by_score, mode, CAP, STRIDE)
                    equal &= int(got[0][i]) == one[0] and all(np.array_equal(x[i], y) for x, y in zip(got[1:7], one[1:7]))
                    for other in (own, base):
                        if other:
                            equal &= other.head_victims(t, by_score, mode) == one[0] and \
                                np.array_equal(other.count, one[3]) and \
                                np.array_equal(other.victim.reshape(CAP, STRIDE), one[6])
                    acting += int(got[7][i] >= 0)
                ta, t0, tb, tb16, tb8, tc8, th = [], [], [], [], [], [], []
                for r in range(-3, a.reps):  # three warm-up rounds
                    x = _wall(lambda: [own.head_victims(t, by_score, mode) for t in tasks])
                    x0 = _wall(lambda: [base.head_victims(t, by_score, mode) for t in tasks]) if base else 0.0
                    y = _wall(lambda: s.heads_victims(tasks, by_score, mode, CAP, STRIDE))
                    y16 = _wall(lambda: s.heads_victims(tasks[:16], by_score, mode, CAP, STRIDE))
                    y8 = _wall(lambda: s.heads_victims(tasks[:8], by_score, mode, CAP, STRIDE))
                    z8 = _wall(lambda: s.heads_victims(tasks, by_score, mode, 8, STRIDE))
                    h = _wall(lambda: s.rank_heads(tasks, by_score, mode, CAP))
                    if r >= 0:
                        ta.append(x); t0.append(x0); tb.append(y); tb16.append(y16); tb8.append(y8); tc8.append(z8)
                        th.append(h)
                n = len(tasks)
                m = {"a_64_calls": _med(ta), "b_one_call_64": _med(tb), "b_one_call_16": _med(tb16),
                     "b_one_call_8": _med(tb8), "b_one_call_64_cap8": _med(tc8), "h_rank_heads_64": _med(th),
                     "a_over_b": float(np.median(ta) / np.median(tb)),
                     "a_per_task_us": float(np.median(ta) / n), "b_per_task_us": float(np.median(tb) / n),
                     "b16_per_task_us": float(np.median(tb16) / 16), "b8_per_task_us": float(np.median(tb8) / 8),
                     "b_minus_h_us": float(np.median(tb) - np.median(th)),
                     "info": got[8], "tasks_with_a_valid_node": acting}
                if base:
                    m["a0_64_calls_baseline"] = _med(t0)
                    m["a_over_a0"] = float(np.median(ta) / np.median(t0))
                out["modes"][mode] = m
            out["rows_equal"] = bool(equal)
        own.close()
        if base:
            base.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
