"""kbhip — Python binding of libkbhip.so (the MI355X placement engine).

This is the host-side mirror of the reference's plugin boundary for callers
that are not Go (tests, bench): it loads the in-tree ``_build/libkbhip.so`` and
exposes the C ABI of include/kbhip.h.  There is no fallback: if the library or
a gfx950 device is missing, calls raise ``KbhipError``.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Optional, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KBHIP_LIB") or os.path.join(HERE, "_build", "libkbhip.so")  # KBHIP_LIB: tuning builds

ALLOCATED, PIPELINED, EVICTED = 1, 2, 3
EV_DELETE, EV_SUCCEEDED, EV_FAILED = 1, 2, 3  # kbhip_session_carry_events
STOP_ALL, STOP_UNASSIGNED, STOP_READY = 0, 1, 2
OP_EVICT, OP_PIPELINE, OP_UNPIPELINE, OP_UNEVICT = 1, 2, 3, 4  # kbhip_apply_ops
VICTIMS_OTHER_QUEUES, VICTIMS_QUEUE_OTHER_JOBS, VICTIMS_SAME_JOB = 1, 2, 3  # kbhip_rank_victim_nodes
RANK_HEADS_MAX = 64  # KBHIP_RANK_HEADS_MAX: tasks per kbhip_rank_heads
HEADS_VICTIMS_MAX = 64  # KBHIP_HEADS_VICTIMS_MAX: tasks per kbhip_heads_victims
HEAD_VICTIMS_VALID, HEAD_VICTIMS_COVERS = 1, 2  # kbhip_head_victims: out_flags bits
WALK_ASSIGNED, WALK_EXHAUSTED, WALK_HEAD_END, WALK_CAPACITY = 1, 2, 3, 4  # kbhip_walk_victims: stop reasons
_WALK_INFO = ("stop", "total", "visited", "acted", "last_node", "last_score", "launches")
_WALK_FROM_INFO = ("stop", "remaining", "visited", "acted", "resume_node", "resume_score", "launches")
_WALK_NEXT_INFO = ("stop", "total", "decided", "acted", "next", "first", "launches")


def _walk_info(info, names=_WALK_INFO, tail=()):
    """out_info of either walk: seven named words, the packed word 7, then the words named by `tail`."""
    d = dict(zip(names, map(int, info[:7])))
    d.update(rebuilt=int(info[7]) & 1, state_rebuilt=(int(info[7]) >> 1) & 1, patched=int(info[7]) >> 8)
    d.update(zip(tail, map(int, info[8:])))
    return d


def _walk_from_info(info):
    return _walk_info(info, _WALK_FROM_INFO, ("last_node", "first_valid"))


def _walk_next_info(info):
    return _walk_info(info, _WALK_NEXT_INFO, ("last_node", "scanned"))


def _walk_arrays(cap_ops, info_words=8):
    """(op, pod, node, info) for a walk call of up to cap_ops ops"""
    room = max(int(cap_ops), 1)
    return (np.zeros(room, np.uint8), np.full(room, -1, np.int32), np.full(room, -1, np.int32),
            np.zeros(info_words, np.int64))


# kbhip_explain_tasks: the verdict codes (low four bits of a verdict byte), the short bits of codes 0..2
(WHY_FITS_IDLE, WHY_FITS_RELEASING, WHY_RESOURCES, WHY_POD_COUNT, WHY_NODE_SELECTOR, WHY_HOST_PORTS,
 WHY_UNSCHEDULABLE, WHY_TAINTS, WHY_POD_AFFINITY, WHY_SCORE_ERROR) = range(10)
WHY_SHORT_CPU, WHY_SHORT_MEM, WHY_SHORT_GPU = 0x10, 0x20, 0x40
EXPLAIN_MAX, EXPLAIN_BINS = 64, 16

# int kbhip_* entry points declared by include/kbhip.h
EXPORTS = ("kbhip_device_count", "kbhip_session_open", "kbhip_session_open_file", "kbhip_place_job",
           "kbhip_allocate", "kbhip_read_nodes", "kbhip_get_stats", "kbhip_set_option",
           "kbhip_session_close", "kbhip_last_error", "kbhip_debug_encode", "kbhip_debug_table",
           "kbhip_backfill", "kbhip_session_open_shard", "kbhip_shard_info", "kbhip_rccl_unique_id",
           "kbhip_shard_connect_rccl", "kbhip_shard_connect_host", "kbhip_debug_replay",
           "kbhip_gang_unschedulable", "kbhip_reclaim", "kbhip_preempt", "kbhip_session_carry",
           "kbhip_first_fit", "kbhip_sweep_scores", "kbhip_shard_connect_host_gather",
           "kbhip_session_carry_events", "kbhip_shard_connect_mailbox", "kbhip_shard_mailbox_fits", "kbhip_place_job_submit",
           "kbhip_place_job_wait", "kbhip_place_job_cancel", "kbhip_time_sweeps", "kbhip_time_rank_multi",
           "kbhip_session_carry_snapshot", "kbhip_walk_visits", "kbhip_fit_deltas", "kbhip_rank_nodes",
           "kbhip_apply_ops", "kbhip_rank_victim_nodes", "kbhip_rank_heads", "kbhip_explain_tasks",
           "kbhip_debug_explain", "kbhip_head_victims", "kbhip_debug_victims", "kbhip_walk_victims",
           "kbhip_debug_walk_victims", "kbhip_heads_victims", "kbhip_walk_victims_from",
           "kbhip_walk_begin", "kbhip_walk_next", "kbhip_walk_order", "kbhip_walk_end",
           "kbhip_walk_begin_live")

RED_MAX_U64, RED_MIN_I64, RED_MAX_I64, RED_SUM_I64 = 0, 1, 2, 3
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32,
                                ctypes.c_int32)
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)


class KbhipError(RuntimeError):
    pass


class Stats(ctypes.Structure):
    _fields_ = [("open_s", ctypes.c_double), ("allocate_s", ctypes.c_double), ("device_s", ctypes.c_double),
                ("pops", ctypes.c_int64), ("tasks", ctypes.c_int64), ("placed", ctypes.c_int64),
                ("sweeps", ctypes.c_int64), ("batched_pops", ctypes.c_int64), ("nodes", ctypes.c_int64),
                ("timed_launches", ctypes.c_int64), ("host_launch_s", ctypes.c_double),
                ("host_wait_s", ctypes.c_double), ("spec_hits", ctypes.c_int64), ("spec_missed", ctypes.c_int64),
                ("alloc_device_s", ctypes.c_double), ("unassigned_pops", ctypes.c_int64),
                ("collectives", ctypes.c_int64), ("rank_requests", ctypes.c_int64),
                ("rank_batch_sum", ctypes.c_int64), ("pop_requests", ctypes.c_int64),
                ("pop_batch_sum", ctypes.c_int64), ("comm_reused", ctypes.c_int64),
                ("async_launched", ctypes.c_int64), ("async_retracted", ctypes.c_int64),
                ("async_cancelled", ctypes.c_int64), ("sweep_requests", ctypes.c_int64),
                ("sweep_batch_sum", ctypes.c_int64), ("score_sweep_s", ctypes.c_double),
                ("score_sweeps", ctypes.c_int64), ("pertask_sweeps", ctypes.c_int64),
                ("seq_launches", ctypes.c_int64), ("seq_cut", ctypes.c_int64), ("seq_none", ctypes.c_int64),
                ("evict_rank_s", ctypes.c_double), ("evict_walk_s", ctypes.c_double),
                ("evict_visits", ctypes.c_int64), ("evict_cands", ctypes.c_int64), ("fit_syncs", ctypes.c_int64),
                ("alloc_setup_s", ctypes.c_double), ("evict_setup_s", ctypes.c_double),
                ("engine_pops", ctypes.c_int64), ("engine_launches", ctypes.c_int64),
                ("engine_workers", ctypes.c_int64), ("engine_owners", ctypes.c_int64),
                ("engine_not_resident", ctypes.c_int64), ("rank_heads", ctypes.c_int64),
                ("rank_fulls", ctypes.c_int64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib: Optional[ctypes.CDLL] = None


def build() -> str:
    """Compile libkbhip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KbhipError(f"{LIB_PATH} is missing: run kbhip.build() (no CPU fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        L.kbhip_last_error.restype = ctypes.c_char_p
        L.kbhip_device_count.restype = ctypes.c_int
        L.kbhip_session_open.argtypes = [vp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(vp)]
        L.kbhip_session_open_file.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(vp)]
        L.kbhip_place_job.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
        L.kbhip_place_job_submit.argtypes = [vp, vp, i32, i32, i32, i32]
        L.kbhip_place_job_submit.restype = i64
        L.kbhip_place_job_wait.argtypes = [vp, i64, vp, vp, vp, vp]
        L.kbhip_place_job_cancel.argtypes = [vp, i64]
        L.kbhip_allocate.argtypes = [vp, vp, vp, vp, i64]
        L.kbhip_backfill.argtypes = [vp, vp, vp, vp, i64]
        L.kbhip_first_fit.argtypes = [vp, vp, i32, vp]
        L.kbhip_sweep_scores.argtypes = [vp, i32, vp]
        L.kbhip_time_sweeps.argtypes = [vp, vp, i32, vp]
        L.kbhip_time_rank_multi.argtypes = [vp, i32, vp, i32, i32, i32, vp]
        L.kbhip_reclaim.argtypes = [vp, vp, vp, vp, i64]
        L.kbhip_session_carry.argtypes = [vp, vp]
        L.kbhip_session_carry_events.argtypes = [vp, vp, vp, i64, vp]
        L.kbhip_session_carry_snapshot.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, vp]
        L.kbhip_preempt.argtypes = [vp, vp, vp, vp, i64]
        L.kbhip_session_open_shard.argtypes = [vp, ctypes.c_size_t, ctypes.c_int, i32, i32, ctypes.POINTER(vp)]
        L.kbhip_shard_info.argtypes = [vp, vp]
        L.kbhip_rccl_unique_id.argtypes = [vp, i64]
        L.kbhip_shard_connect_rccl.argtypes = [vp, vp, i64]
        L.kbhip_shard_connect_host.argtypes = [vp, ALLREDUCE_FN, vp]
        L.kbhip_shard_connect_host_gather.argtypes = [vp, ALLGATHER_FN, vp]
        L.kbhip_shard_connect_mailbox.argtypes = [vp, ALLGATHER_FN, vp]
        L.kbhip_shard_mailbox_fits.argtypes = [ctypes.c_int32, ctypes.c_int32]
        L.kbhip_shard_mailbox_fits.restype = ctypes.c_int
        L.kbhip_read_nodes.argtypes = [vp, vp, i64]
        L.kbhip_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
        L.kbhip_set_option.argtypes = [vp, ctypes.c_char_p, i64]
        L.kbhip_session_close.argtypes = [vp]
        L.kbhip_debug_encode.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.kbhip_debug_table.argtypes = [vp, ctypes.c_char_p, vp, i64]
        L.kbhip_debug_table.restype = i64
        L.kbhip_gang_unschedulable.argtypes = [vp, ctypes.c_char_p, i64]
        L.kbhip_gang_unschedulable.restype = i64
        L.kbhip_debug_replay.argtypes = [vp, i32, vp, vp, vp, vp, vp]
        L.kbhip_walk_visits.argtypes = [vp, vp, vp, i64]
        L.kbhip_walk_visits.restype = i64
        L.kbhip_fit_deltas.argtypes = [vp, i32, vp, vp, i64]
        L.kbhip_fit_deltas.restype = i64
        L.kbhip_rank_nodes.argtypes = [vp, i32, i32, i64, vp, vp, i64]
        L.kbhip_rank_nodes.restype = i64
        L.kbhip_apply_ops.argtypes = [vp, vp, vp, vp, i64, vp]
        L.kbhip_apply_ops.restype = i64
        L.kbhip_rank_victim_nodes.argtypes = [vp, i32, i32, i32, i64, vp, vp, vp, i64, vp]
        L.kbhip_rank_victim_nodes.restype = i64
        L.kbhip_rank_heads.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
        L.kbhip_rank_heads.restype = i64
        L.kbhip_explain_tasks.argtypes = [vp, vp, i32, vp, vp, vp]
        L.kbhip_explain_tasks.restype = i64
        L.kbhip_debug_explain.argtypes = [vp, i32, vp, vp]
        L.kbhip_head_victims.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.kbhip_head_victims.restype = i64
        L.kbhip_debug_victims.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp]
        L.kbhip_heads_victims.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.kbhip_heads_victims.restype = i64
        L.kbhip_walk_victims.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp]
        L.kbhip_walk_victims.restype = i64
        L.kbhip_debug_walk_victims.argtypes = [vp, i32, i32, vp, i32, i64, vp, vp, vp, vp]
        L.kbhip_debug_walk_victims.restype = i64
        L.kbhip_walk_victims_from.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp]
        L.kbhip_walk_victims_from.restype = i64
        L.kbhip_walk_begin.argtypes = [vp, i32, i32, i32, vp]
        L.kbhip_walk_begin.restype = i64
        L.kbhip_walk_begin_live.argtypes = [vp, i32, i32, vp]
        L.kbhip_walk_begin_live.restype = i64
        L.kbhip_walk_next.argtypes = [vp, i64, i32, vp, vp, vp, i64, vp]
        L.kbhip_walk_next.restype = i64
        L.kbhip_walk_order.argtypes = [vp, i64, vp, vp, i64]
        L.kbhip_walk_order.restype = i64
        L.kbhip_walk_end.argtypes = [vp]
        _lib = L
    return _lib


def _check(rc: int) -> int:
    if rc < 0:
        raise KbhipError(f"kbhip error {rc}: {lib().kbhip_last_error().decode()}")
    return rc


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def device_count() -> int:
    return _check(lib().kbhip_device_count())


class Session:
    """One scheduling session on one GPU (framework.Session equivalent)."""

    def __init__(self, snapshot, device: int = 0):
        self._h = ctypes.c_void_p()
        if isinstance(snapshot, (bytes, bytearray, memoryview)):
            buf = bytes(snapshot)
            _check(lib().kbhip_session_open(ctypes.c_char_p(buf), len(buf), device, ctypes.byref(self._h)))
        else:
            _check(lib().kbhip_session_open_file(str(snapshot).encode(), device, ctypes.byref(self._h)))

    def close(self) -> None:
        if self._h:
            _check(lib().kbhip_session_close(self._h))
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key: str, value: int) -> None:
        _check(lib().kbhip_set_option(self._h, key.encode(), int(value)))

    def allocate(self, cap: int = 1 << 21) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Run allocateAction.Execute; returns (pod, node, kind) in decision order."""
        pod = np.zeros(cap, np.int32)
        node = np.zeros(cap, np.int32)
        kind = np.zeros(cap, np.uint8)
        n = _check(lib().kbhip_allocate(self._h, _p(pod), _p(node), _p(kind), cap))
        if n > cap:
            raise KbhipError("placement log larger than cap")
        return pod[:n].copy(), node[:n].copy(), kind[:n].copy()

    def _action(self, fn, cap: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        pod = np.zeros(cap, np.int32)
        node = np.zeros(cap, np.int32)
        kind = np.zeros(cap, np.uint8)
        n = _check(fn(self._h, _p(pod), _p(node), _p(kind), cap))
        if n > cap:
            raise KbhipError("placement log larger than cap")
        return pod[:n].copy(), node[:n].copy(), kind[:n].copy()

    def backfill(self, cap: int = 1 << 21) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Run backfillAction.Execute on the current session state."""
        return self._action(lib().kbhip_backfill, cap)

    def first_fit(self, task_ids) -> np.ndarray:
        """kbhip_first_fit: backfill.go:51-65 for the given pending tasks, in
        order (lowest-index node passing the predicates, Session.Allocate);
        returns the node per task (-1: none)."""
        ids = np.ascontiguousarray(task_ids, dtype=np.int32)
        out = np.full(max(ids.size, 1), -1, np.int32)
        _check(lib().kbhip_first_fit(self._h, _p(ids), ids.size, _p(out)))
        return out[: ids.size].copy()

    def sweep_scores(self, task_id: int, n_nodes: int, keys: bool = True) -> Tuple[int, np.ndarray]:
        """kbhip_sweep_scores: preempt.go:270-287's predicate + score sweep of
        one task: (passing nodes, per-node packed keys; 0 = node fails).
        keys=False: the count only (no copy of the keys)."""
        if not keys:
            return _check(lib().kbhip_sweep_scores(self._h, int(task_id), None)), np.zeros(0, np.uint64)
        out = np.zeros(max(n_nodes, 1), np.uint64)
        n = _check(lib().kbhip_sweep_scores(self._h, int(task_id), _p(out)))
        return n, out[:n_nodes].copy()

    def rank_nodes(self, task_id: int, by_score: bool = True, first: int = 0,
                   cap: Optional[int] = None) -> Tuple[int, np.ndarray, np.ndarray]:
        """kbhip_rank_nodes: the ranked node walk of one pending task:
        (total, nodes, scores) with entries [first, first + cap) of the walk.
        by_score=True: preempt.go:270-287's util.SelectBestNode order of the
        nodes passing PredicateFn with a NodeOrderFn score; False: reclaim's
        walk, the passing nodes in ascending index (scores 0).  first + cap <=
        64 is served by the top-64 kernel, anything else by the full device
        sort.  cap=None: a size query, then every entry from `first`."""
        bs = int(by_score)
        if cap is None:
            n = int(lib().kbhip_rank_nodes(self._h, int(task_id), bs, int(first), None, None, 0))
            _check(n if n < 0 else 0)
            cap = max(n - int(first), 0)
            if cap == 0:
                return n, np.zeros(0, np.int32), np.zeros(0, np.int32)
        node = np.full(max(int(cap), 1), -1, np.int32)
        score = np.zeros(max(int(cap), 1), np.int32)
        n = int(lib().kbhip_rank_nodes(self._h, int(task_id), bs, int(first), _p(node), _p(score), int(cap)))
        _check(n if n < 0 else 0)
        k = max(min(n, int(first) + int(cap)) - int(first), 0)
        return n, node[:k].copy(), score[:k].copy()

    def rank_victim_nodes(self, task_id: int, by_score: bool = True, victims: int = VICTIMS_OTHER_QUEUES,
                          first: int = 0, cap: Optional[int] = None):
        """kbhip_rank_victim_nodes: rank_nodes' walk without the nodes that can
        yield no victim set for the task (no candidate of the `victims` kind, or
        candidates together strictly short of its InitResreq in all three
        resources): (total, nodes, scores, cands, info).  cands: the candidate
        count per returned node; info: {"head", "rebuilt", "launches"} of the
        call that read the entries.  cap=None: a size query, then every entry
        from `first`."""
        bs, vi = int(by_score), int(victims)
        info = np.zeros(3, np.int64)
        fn = lib().kbhip_rank_victim_nodes
        rebuilt = 0
        if cap is None:
            n = int(fn(self._h, int(task_id), bs, vi, int(first), None, None, None, 0, _p(info)))
            _check(n if n < 0 else 0)
            rebuilt = int(info[1])
            cap = max(n - int(first), 0)
            if cap == 0:
                z = np.zeros(0, np.int32)
                return n, z, z.copy(), z.copy(), {"head": int(info[0]), "rebuilt": rebuilt, "launches": int(info[2])}
        node = np.full(max(int(cap), 1), -1, np.int32)
        score = np.zeros(max(int(cap), 1), np.int32)
        cands = np.zeros(max(int(cap), 1), np.int32)
        n = int(fn(self._h, int(task_id), bs, vi, int(first), _p(node), _p(score), _p(cands), int(cap), _p(info)))
        _check(n if n < 0 else 0)
        k = max(min(n, int(first) + int(cap)) - int(first), 0)
        return (n, node[:k].copy(), score[:k].copy(), cands[:k].copy(),
                {"head": int(info[0]), "rebuilt": int(info[1]) | rebuilt, "launches": int(info[2])})

    def rank_heads(self, task_ids, by_score: bool = True, victims: int = 0, cap: int = 64):
        """kbhip_rank_heads: the walk heads of up to RANK_HEADS_MAX pending
        tasks of the session as it stands, from one sweep launch, one merge
        launch and one copy: (totals[n], nodes[n, cap], scores[n, cap],
        cands[n, cap], info).  Row i is what rank_nodes(task_ids[i], by_score,
        0, cap) answers (victims=0) or rank_victim_nodes(task_ids[i], by_score,
        victims, 0, cap) (victims 1..3), padded beyond the total with node -1,
        score 0, cands 0.  info (3 int64): table rebuilt, kernel launches, the
        sweep grid's x size."""
        ids = np.ascontiguousarray(task_ids, dtype=np.int32).reshape(-1)
        n, cap = int(ids.size), int(cap)
        rows = max(n, 1) * max(cap, 1)
        total = np.zeros(max(n, 1), np.int64)
        node = np.full(rows, -1, np.int32)
        score = np.zeros(rows, np.int32)
        cands = np.zeros(rows, np.int32)
        info = np.zeros(3, np.int64)
        r = int(lib().kbhip_rank_heads(self._h, _p(ids), n, int(by_score), int(victims), cap, _p(total), _p(node),
                                       _p(score), _p(cands), _p(info)))
        _check(r if r < 0 else 0)
        shape = (n, max(cap, 0))
        return (total[:n].copy(), node[: n * cap].reshape(shape), score[: n * cap].reshape(shape),
                cands[: n * cap].reshape(shape), info)

    @staticmethod
    def _head_arrays(rows: int, stride: int):
        """(node, score, count, evict, flags, victim) of head_victims / heads_victims for `rows` head entries"""
        return (np.full(rows, -1, np.int32), np.zeros(rows, np.int32), np.zeros(rows, np.int32),
                np.zeros(rows, np.int32), np.zeros(rows, np.uint8), np.full(rows * max(stride, 1), -1, np.int32))

    def _walk(self, fn, info_words, decode, task_id, by_score, victims, cap, after, cap_ops):  # either walk call
        op, pod, node, info = _walk_arrays(cap_ops, info_words)
        a_node, a_score = (-1, 0) if after is None else (int(after[0]), int(after[1]))
        n = int(fn(self._h, int(task_id), int(by_score), int(victims), int(cap), a_node, a_score, _p(op), _p(pod),
                   _p(node), int(cap_ops), _p(info)))
        _check(n if n < 0 else 0)
        return op[:n].copy(), pod[:n].copy(), node[:n].copy(), decode(info)

    def head_victims(self, task_id: int, by_score: bool = True, victims: int = VICTIMS_OTHER_QUEUES,
                     cap: int = 64, stride: int = 16):
        """kbhip_head_victims: the head of rank_victim_nodes' walk and, per head
        node, what Reclaimable / Preemptable, validateVictims and the eviction
        loop decide on it: (total, nodes[cap], scores[cap], counts[cap],
        evicts[cap], flags[cap], victim_rows[cap, stride], info).  Rows beyond
        min(cap, total) are -1 / 0.  A victim row holds the first min(count,
        stride) victims' pod indices, then -1.
        info: {"rebuilt", "state_rebuilt", "patched", "launches", "max_count"}."""
        cap, stride = int(cap), int(stride)
        node, score, count, evict, flags, victim = self._head_arrays(max(cap, 1), stride)
        info = np.zeros(5, np.int64)
        n = int(lib().kbhip_head_victims(self._h, int(task_id), int(by_score), int(victims), cap, stride, _p(node),
                                         _p(score), _p(count), _p(evict), _p(flags), _p(victim), _p(info)))
        _check(n if n < 0 else 0)
        return (n, node[:cap], score[:cap], count[:cap], evict[:cap], flags[:cap],
                victim[: cap * stride].reshape(cap, stride),
                dict(zip(("rebuilt", "state_rebuilt", "patched", "launches", "max_count"), map(int, info))))

    def heads_victims(self, task_ids, by_score: bool = True, victims: int = VICTIMS_OTHER_QUEUES,
                      cap: int = 64, stride: int = 16):
        """kbhip_heads_victims: head_victims for up to HEADS_VICTIMS_MAX pending
        tasks of the session as it stands in one call: (totals[n], nodes[n,
        cap], scores[n, cap], counts[n, cap], evicts[n, cap], flags[n, cap],
        victim_rows[n, cap, stride], first[n], info).  Row i is what
        head_victims(task_ids[i], by_score, victims, cap, stride) answers, no
        eviction carried between tasks; first[i] is the index of task i's first
        head entry with HEAD_VICTIMS_VALID, or -1.
        info: {"rebuilt", "state_rebuilt", "patched", "launches", "max_count",
        "victim_launches"}."""
        ids = np.ascontiguousarray(task_ids, dtype=np.int32).reshape(-1)
        n, cap, stride = int(ids.size), int(cap), int(stride)
        total = np.zeros(max(n, 1), np.int64)
        node, score, count, evict, flags, victim = self._head_arrays(max(n, 1) * max(cap, 1), stride)
        first = np.full(max(n, 1), -1, np.int32)
        info = np.zeros(6, np.int64)
        r = int(lib().kbhip_heads_victims(self._h, _p(ids), n, int(by_score), int(victims), cap, stride, _p(total),
                                          _p(node), _p(score), _p(count), _p(evict), _p(flags), _p(victim),
                                          _p(first), _p(info)))
        _check(r if r < 0 else 0)
        k = n * cap
        shape = (n, cap)
        return (total[:n].copy(), node[:k].reshape(shape), score[:k].reshape(shape), count[:k].reshape(shape),
                evict[:k].reshape(shape), flags[:k].reshape(shape), victim[: k * stride].reshape(n, cap, stride),
                first[:n].copy(),
                dict(zip(("rebuilt", "state_rebuilt", "patched", "launches", "max_count", "victim_launches"),
                         map(int, info))))

    def walk_victims(self, task_id: int, by_score: bool = True, victims: int = VICTIMS_OTHER_QUEUES,
                     cap: int = 64, after=None, cap_ops: int = 4096):
        """kbhip_walk_victims: the task's whole eviction walk over the head of
        its pruned walk, the evictions of each node carried to the next:
        (ops[n], pods[n], nodes[n], info), ready for apply_ops.  after: None,
        or (node, score) of the last acted-on node of the call to resume.
        info: {"stop" (a WALK_* reason), "total", "visited", "acted",
        "last_node", "last_score", "launches", "rebuilt", "state_rebuilt",
        "patched"}."""
        return self._walk(lib().kbhip_walk_victims, 8, _walk_info, task_id, by_score, victims, cap, after, cap_ops)

    def walk_victims_from(self, task_id: int, by_score: bool = True, victims: int = VICTIMS_OTHER_QUEUES,
                          cap: int = 64, after=None, cap_ops: int = 4096):
        """kbhip_walk_victims_from: one window (up to 64 entries) of the
        task's eviction walk behind a resume point: (ops[n], pods[n], nodes[n],
        info), ready for apply_ops.  after: None (from the top), or
        (resume_node, resume_score) of the call to go on from — after a
        WALK_HEAD_END or WALK_CAPACITY stop, with the ops applied in between.
        info: {"stop" (a WALK_* reason), "remaining" (walk entries behind the
        resume point at the call), "visited", "acted", "resume_node",
        "resume_score", "launches", "rebuilt", "state_rebuilt", "patched",
        "last_node", "first_valid"}."""
        return self._walk(lib().kbhip_walk_victims_from, 10, _walk_from_info, task_id, by_score, victims, cap, after,
                          cap_ops)

    def walk_begin(self, task_id: int, by_score: bool = True, victims: int = VICTIMS_OTHER_QUEUES):
        """kbhip_walk_begin: the task's pruned walk ranked once and kept on
        the device as the session's eviction-walk cursor: (total, info).
        info: {"launches", "rebuilt", "bytes", "affinity_targets"}."""
        info = np.zeros(4, np.int64)
        n = int(lib().kbhip_walk_begin(self._h, int(task_id), int(by_score), int(victims), _p(info)))
        _check(n if n < 0 else 0)
        return n, dict(zip(("launches", "rebuilt", "bytes", "affinity_targets"), map(int, info)))

    def walk_begin_live(self, task_id: int, victims: int = VICTIMS_OTHER_QUEUES):
        """kbhip_walk_begin_live: the cursor for reclaim's order (by_score 0),
        exact for every task class: (total, info) as walk_begin.  For a class
        whose predicates read pod-affinity targets the cursor is live
        (info["affinity_targets"] == 2): the kept order leaves that predicate
        out, walk_next tests it per call and returns behind the first node it
        acts on.  Any other class: walk_begin(task_id, False, victims)."""
        info = np.zeros(4, np.int64)
        n = int(lib().kbhip_walk_begin_live(self._h, int(task_id), int(victims), _p(info)))
        _check(n if n < 0 else 0)
        return n, dict(zip(("launches", "rebuilt", "bytes", "affinity_targets"), map(int, info)))

    def walk_next(self, pos: int = 0, cap: int = 64, cap_ops: int = 4096):
        """kbhip_walk_next: the cursor's walk from position `pos` of the kept
        order — the entries that cannot act passed over side by side, the
        serial walk over up to `cap` entries from the first that can: (ops[n],
        pods[n], nodes[n], info), ready for apply_ops; go on from info["next"].
        info: {"stop" (a WALK_* reason), "total", "decided", "acted", "next",
        "first" (-1: none), "launches", "rebuilt", "state_rebuilt", "patched",
        "last_node", "scanned"}."""
        op, pod, node, info = _walk_arrays(cap_ops, 10)
        n = int(lib().kbhip_walk_next(self._h, int(pos), int(cap), _p(op), _p(pod), _p(node), int(cap_ops), _p(info)))
        _check(n if n < 0 else 0)
        return op[:n].copy(), pod[:n].copy(), node[:n].copy(), _walk_next_info(info)

    def walk_order(self, first: int = 0, cap: Optional[int] = None):
        """kbhip_walk_order: entries [first, first + cap) of the cursor's kept
        order: (total, nodes, scores).  cap=None: every entry from `first`."""
        fn = lib().kbhip_walk_order
        if cap is None:
            n = int(fn(self._h, int(first), None, None, 0))
            _check(n if n < 0 else 0)
            cap = max(n - int(first), 0)
        node = np.full(max(int(cap), 1), -1, np.int32)
        score = np.zeros(max(int(cap), 1), np.int32)
        n = int(fn(self._h, int(first), _p(node), _p(score), int(cap)))
        _check(n if n < 0 else 0)
        k = max(min(n, int(first) + int(cap)) - int(first), 0)
        return n, node[:k].copy(), score[:k].copy()

    def walk_end(self) -> bool:
        """kbhip_walk_end: drops the cursor; whether one was open."""
        return bool(_check(lib().kbhip_walk_end(self._h)))

    def explain_tasks(self, task_ids, verdicts: bool = False, n_nodes: Optional[int] = None):
        """kbhip_explain_tasks: why each node is, or is not, in the allocate
        walk of up to EXPLAIN_MAX pending tasks of the session as it stands:
        (hist[n, EXPLAIN_BINS], verdict[n, n_nodes] or None, info).  A verdict
        byte is a WHY_* code, or-ed with the WHY_SHORT_* bits for the codes
        0..2; hist[i, c] counts the nodes with code c, [11..13] the walk nodes
        with the cpu / memory / GPU short bit, [14] the walk, [15] the nodes.
        info (3 int64): kernel launches, the sweep grid's x size, whether
        verdict rows were written.  verdicts=True needs the node count, which
        one histogram-only call answers when n_nodes is not given."""
        ids = np.ascontiguousarray(task_ids, dtype=np.int32).reshape(-1)
        n = int(ids.size)
        hist = np.zeros((max(n, 1), EXPLAIN_BINS), np.int64)
        info = np.zeros(3, np.int64)
        fn = lib().kbhip_explain_tasks
        verdict = None
        if verdicts and n:
            if n_nodes is None:
                r = int(fn(self._h, _p(ids), 1, None, _p(hist), None))
                _check(r if r < 0 else 0)
                n_nodes = int(hist[0, 15])
            verdict = np.zeros((n, max(int(n_nodes), 1)), np.uint8)
        r = int(fn(self._h, _p(ids), n, None if verdict is None else _p(verdict), _p(hist), _p(info)))
        _check(r if r < 0 else 0)
        if verdict is not None:
            verdict = verdict.reshape(-1)[: n * int(n_nodes)].reshape(n, int(n_nodes))
        return hist[:n].copy(), verdict, info

    def apply_ops(self, ops, pods, nodes=None) -> int:
        """kbhip_apply_ops: the evictions and pipelines a host-driven reclaim /
        preempt loop decided (OP_EVICT / OP_PIPELINE / OP_UNPIPELINE /
        OP_UNEVICT per pod, in order; nodes: the node of each OP_PIPELINE,
        ignored otherwise) applied to the host model and the device as the
        engine's own actions apply theirs.  Returns the device kernel launches
        the call issued."""
        o = np.ascontiguousarray(ops, dtype=np.uint8)
        p = np.ascontiguousarray(pods, dtype=np.int32)
        nd = np.zeros(p.size, np.int32) if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
        if not (o.ndim == p.ndim == nd.ndim == 1 and o.size == p.size == nd.size):
            raise ValueError("ops, pods and nodes differ in length")
        launches = np.zeros(1, np.int64)
        n = int(lib().kbhip_apply_ops(self._h, _p(o) if o.size else None, _p(p) if p.size else None,
                                      _p(nd) if nd.size else None, int(o.size), _p(launches)))
        _check(n if n < 0 else 0)
        return int(launches[0])

    def time_sweeps(self, task_ids) -> float:
        """kbhip_time_sweeps: device time per launch (us) of the standalone sweep,
        one launch per task, back to back."""
        ids = np.ascontiguousarray(task_ids, dtype=np.int32)
        out = np.zeros(1, np.float64)
        _check(lib().kbhip_time_sweeps(self._h, _p(ids), ids.size, _p(out)))
        return float(out[0])

    def carry(self) -> int:
        """kbhip_session_carry: become the next session (binds / evictions applied); bytes uploaded."""
        out = np.zeros(1, np.int64)
        _check(lib().kbhip_session_carry(self._h, _p(out)))
        return int(out[0])

    def carry_events(self, pods, events) -> int:
        """kbhip_session_carry_events: carry, then the cache's events on existing pods
        (EV_DELETE / EV_SUCCEEDED / EV_FAILED per pod index); bytes uploaded."""
        p = np.ascontiguousarray(pods, np.int32)
        e = np.ascontiguousarray(events, np.uint8)
        if p.shape != e.shape:
            raise ValueError("pods and events differ in length")
        out = np.zeros(1, np.int64)
        _check(lib().kbhip_session_carry_events(self._h, _p(p), _p(e), int(p.size), _p(out)))
        return int(out[0])

    def carry_snapshot(self, snapshot, old_pod, old_node) -> int:
        """kbhip_session_carry_snapshot: become the session of the cache's next
        snapshot (KBS1 bytes or a path); old_pod / old_node map its pods / nodes
        to this session's indices (-1: new).  Bytes uploaded (-1: re-opened)."""
        if not isinstance(snapshot, (bytes, bytearray, memoryview)):
            with open(snapshot, "rb") as f:
                snapshot = f.read()
        buf = bytes(snapshot)
        op = np.ascontiguousarray(old_pod, np.int32)
        on = np.ascontiguousarray(old_node, np.int32)
        out = np.zeros(1, np.int64)
        _check(lib().kbhip_session_carry_snapshot(self._h, ctypes.c_char_p(buf), len(buf), _p(op) if op.size else None,
                                                  _p(on) if on.size else None, _p(out)))
        return int(out[0])

    def reclaim(self, cap: int = 1 << 21) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Run reclaimAction.Execute: (pod, node, EVICTED | PIPELINED) records in decision order."""
        return self._action(lib().kbhip_reclaim, cap)

    def preempt(self, cap: int = 1 << 21) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Run preemptAction.Execute: records of the committed statements, in operation order."""
        return self._action(lib().kbhip_preempt, cap)

    def run_actions(self, actions: str = "allocate") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The conf's actions in order (scheduler.go:93-97): allocate, backfill, reclaim, preempt."""
        logs = []
        for a in (x.strip() for x in actions.split(",")):
            if a == "allocate":
                logs.append(self.allocate())
            elif a == "backfill":
                logs.append(self.backfill())
            elif a == "reclaim":
                logs.append(self.reclaim())
            elif a == "preempt":
                logs.append(self.preempt())
            else:
                raise KbhipError(f"action {a!r} is not implemented by this engine")
        if not logs:
            z = np.zeros(0, np.int32)
            return z, z.copy(), np.zeros(0, np.uint8)
        return tuple(np.concatenate([lg[k] for lg in logs]) for k in range(3))

    def place_job(self, task_ids, gang_mode: int, min_available: int, ready_count: int):
        ids = np.ascontiguousarray(task_ids, dtype=np.int32)
        n = ids.size
        node = np.full(max(n, 1), -1, np.int32)
        kind = np.zeros(max(n, 1), np.uint8)
        done = np.zeros(1, np.int32)
        stop = np.zeros(1, np.int32)
        _check(lib().kbhip_place_job(self._h, _p(ids), n, gang_mode, min_available, ready_count, _p(node),
                                     _p(kind), _p(done), _p(stop)))
        d = int(done[0])
        return node[:d].copy(), kind[:d].copy(), int(stop[0])

    def place_job_submit(self, task_ids, gang_mode: int, min_available: int, ready_count: int) -> int:
        """kbhip_place_job_submit: queue a job pop (run on the state the earlier submitted pops leave); a ticket."""
        ids = np.ascontiguousarray(task_ids, dtype=np.int32)
        t = int(lib().kbhip_place_job_submit(self._h, _p(ids), ids.size, gang_mode, min_available, ready_count))
        _check(t if t < 0 else 0)
        self._tix = getattr(self, "_tix", {})
        self._tix[t] = max(ids.size, 1)
        return t

    def place_job_wait(self, ticket: int):
        """kbhip_place_job_wait: results of the oldest outstanding ticket, as place_job."""
        # the result arrays hold every task of the ticket; its size leaves the
        # table only once the wait succeeded (a refused wait can be retried)
        tix = getattr(self, "_tix", {})
        # a ticket this binding does not hold is refused by the library (EINVAL): arrays as large as any held one
        n = tix.get(ticket, max(list(tix.values()) + [1]))
        node = np.full(n, -1, np.int32)
        kind = np.zeros(n, np.uint8)
        done = np.zeros(1, np.int32)
        stop = np.zeros(1, np.int32)
        _check(lib().kbhip_place_job_wait(self._h, int(ticket), _p(node), _p(kind), _p(done), _p(stop)))
        tix.pop(ticket, None)
        d = int(done[0])
        return node[:d].copy(), kind[:d].copy(), int(stop[0])

    def place_job_cancel(self, ticket: int) -> int:
        """kbhip_place_job_cancel: withdraw `ticket` and every later one; the number withdrawn."""
        k = _check(lib().kbhip_place_job_cancel(self._h, int(ticket)))
        for t in [t for t in getattr(self, "_tix", {}) if t >= ticket]:
            del self._tix[t]
        return k

    def read_nodes(self, n_nodes: int) -> np.ndarray:
        out = np.zeros((n_nodes, 12), np.int64)
        _check(lib().kbhip_read_nodes(self._h, _p(out), n_nodes))
        return out

    def walk_visits(self) -> Tuple[np.ndarray, np.ndarray]:
        """kbhip_walk_visits: (node, count) of the nodes allocate walks visited
        since the previous call (GetAccessibleResource calls: each added the
        node's Backfilled to its Idle), ascending node index; clears them."""
        n = int(lib().kbhip_walk_visits(self._h, None, None, 0))
        _check(n if n < 0 else 0)
        node = np.zeros(max(n, 1), np.int32)
        cnt = np.zeros(max(n, 1), np.uint32)
        if n:
            m = int(lib().kbhip_walk_visits(self._h, _p(node), _p(cnt), n))
            _check(m if m < 0 else 0)
            if m != n:
                raise KbhipError("kbhip_walk_visits: the count changed between the size query and the read")
        return node[:n].copy(), cnt[:n].copy()

    def fit_deltas(self, task_id: int) -> Tuple[np.ndarray, np.ndarray]:
        """kbhip_fit_deltas: job.NodesFitDelta of the task on which the most
        recent pop stopped unassigned: (node [k], delta [k, 3] = cpu, memory,
        GPU), ascending node index."""
        n = int(lib().kbhip_fit_deltas(self._h, int(task_id), None, None, 0))
        _check(n if n < 0 else 0)
        node = np.zeros(max(n, 1), np.int32)
        delta = np.zeros((max(n, 1), 3), np.int64)
        if n:
            m = int(lib().kbhip_fit_deltas(self._h, int(task_id), _p(node), _p(delta), n))
            _check(m if m < 0 else 0)
        return node[:n].copy(), delta[:n].copy()

    def debug_keys(self) -> Tuple[np.ndarray, np.ndarray]:
        """Test support (after set_option("debug_keys", 1) and a run): the pod of
        every per-task sweep and its row: per-node keys, per-node raw inter-pod
        counts (npad each), then ipa lo, ipa hi, fallback node, max key."""
        L = lib()
        n = int(L.kbhip_debug_table(self._h, b"dbg_keys", None, 0))
        _check(n if n < 0 else 0)
        keys = np.zeros(max(n // 8, 1), np.uint64)
        if n:
            _check(int(L.kbhip_debug_table(self._h, b"dbg_keys", _p(keys), keys.nbytes)))
        m = int(L.kbhip_debug_table(self._h, b"dbg_pods", None, 0))
        pods = np.zeros(max(m // 4, 1), np.int32)
        if m:
            _check(int(L.kbhip_debug_table(self._h, b"dbg_pods", _p(pods), pods.nbytes)))
        pods = pods[: m // 4]
        return pods, keys[: n // 8].reshape(len(pods), -1) if len(pods) else keys[:0]

    def table(self, name: str) -> np.ndarray:
        """Test support: a device table read back (kbhip_debug_table)."""
        n = lib().kbhip_debug_table(self._h, name.encode(), None, 0)
        _check(int(n) if n < 0 else 0)
        out = np.zeros(max(int(n) // 4, 1), np.int32)
        _check(int(lib().kbhip_debug_table(self._h, name.encode(), _p(out), out.nbytes)) if n > 0 else 0)
        return out[: int(n) // 4]

    def table_raw(self, name: str, dtype) -> np.ndarray:
        """A table of another element type (job_drf_alloc, queue_allocated, queue_deserved: float64;
        victim_state: int64)."""
        n = int(lib().kbhip_debug_table(self._h, name.encode(), None, 0))
        _check(n if n < 0 else 0)
        out = np.zeros(max(n // np.dtype(dtype).itemsize, 1), dtype)
        if n:
            _check(int(lib().kbhip_debug_table(self._h, name.encode(), _p(out), out.nbytes)))
        return out[: n // np.dtype(dtype).itemsize]

    def gang_unschedulable(self) -> dict:
        """The gang plugin's OnSessionClose messages: {job uid: message} for
        every job not Ready (kbhip_gang_unschedulable)."""
        L = lib()
        n = int(L.kbhip_gang_unschedulable(self._h, None, 0))
        _check(n if n < 0 else 0)
        buf = ctypes.create_string_buffer(n + 1)
        _check(int(L.kbhip_gang_unschedulable(self._h, buf, n + 1)))
        out = {}
        for line in buf.value.decode().splitlines():
            if line:
                uid, msg = line.split("\t", 1)
                out[uid] = msg
        return out

    def stats(self) -> dict:
        st = Stats()
        _check(lib().kbhip_get_stats(self._h, ctypes.byref(st)))
        return st.as_dict()


class EncodedSnapshot:
    """Test support: the engine's compiled host tables for a snapshot, built
    without a device (kbhip_debug_encode).  It cannot place anything."""

    def __init__(self, snapshot):
        if not isinstance(snapshot, (bytes, bytearray, memoryview)):
            with open(snapshot, "rb") as f:
                snapshot = f.read()
        buf = bytes(snapshot)
        self._h = ctypes.c_void_p()
        _check(lib().kbhip_debug_encode(ctypes.c_char_p(buf), len(buf), ctypes.byref(self._h)))

    def table(self, name: str) -> np.ndarray:
        n = lib().kbhip_debug_table(self._h, name.encode(), None, 0)
        _check(int(n) if n < 0 else 0)
        out = np.zeros(max(int(n) // 4, 1), np.int32)
        _check(int(lib().kbhip_debug_table(self._h, name.encode(), _p(out), out.nbytes)) if n > 0 else 0)
        return out[: int(n) // 4]

    def table_raw(self, name: str, dtype) -> np.ndarray:
        """A table of another element type (node_idle / node_backfilled: int64, node_visits: uint32)."""
        n = int(lib().kbhip_debug_table(self._h, name.encode(), None, 0))
        _check(n if n < 0 else 0)
        out = np.zeros(max(n // np.dtype(dtype).itemsize, 1), dtype)
        if n:
            _check(int(lib().kbhip_debug_table(self._h, name.encode(), _p(out), out.nbytes)))
        return out[: n // np.dtype(dtype).itemsize]

    def explain(self, task_id: int) -> Tuple[np.ndarray, np.ndarray]:
        """kbhip_debug_explain: (verdict[n_nodes], hist[EXPLAIN_BINS]) of one
        task, by the kernel's own per-node function on the host tables."""
        n_nodes = int(self.table("dims")[0])
        verdict = np.zeros(max(n_nodes, 1), np.uint8)
        hist = np.zeros(EXPLAIN_BINS, np.int64)
        _check(lib().kbhip_debug_explain(self._h, int(task_id), _p(verdict), _p(hist)))
        return verdict[:n_nodes].copy(), hist

    def victims(self, task_id: int, victims: int, node: int, stride: int = 256):
        """kbhip_debug_victims: (count, evict, flags, victims[min(count, stride)])
        of one node, by the kernel's own per-node functions on the host tables."""
        count, evict = np.zeros(1, np.int32), np.zeros(1, np.int32)
        flags = np.zeros(1, np.uint8)
        row = np.full(max(int(stride), 1), -1, np.int32)
        _check(lib().kbhip_debug_victims(self._h, int(task_id), int(victims), int(node), int(stride), _p(count),
                                         _p(evict), _p(flags), _p(row)))
        return int(count[0]), int(evict[0]), int(flags[0]), row[: min(int(count[0]), int(stride))].copy()

    def walk_victims(self, task_id: int, victims: int, nodes, cap_ops: int = 4096):
        """kbhip_debug_walk_victims: kbhip_walk_victims' node loop over `nodes`
        in the given order, by the kernel's own functions on the host tables:
        (ops[n], pods[n], nodes[n], info) as Session.walk_victims."""
        nd = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        op, pod, node, info = _walk_arrays(cap_ops)
        n = int(lib().kbhip_debug_walk_victims(self._h, int(task_id), int(victims), _p(nd) if nd.size else None,
                                               int(nd.size), int(cap_ops), _p(op), _p(pod), _p(node), _p(info)))
        _check(n if n < 0 else 0)
        return op[:n].copy(), pod[:n].copy(), node[:n].copy(), _walk_info(info)

    def set_option(self, key: str, value: int) -> None:
        _check(lib().kbhip_set_option(self._h, key.encode(), int(value)))

    def replay(self, pods, modes, nodes, kinds) -> np.ndarray:
        """Per-step, per-node selection keys along a given decision sequence
        (kbhip_debug_replay); kinds: KBHIP_ALLOCATED / KBHIP_PIPELINED."""
        pods = np.ascontiguousarray(pods, np.int32)
        modes = np.ascontiguousarray(modes, np.int32)
        nodes = np.ascontiguousarray(nodes, np.int32)
        kinds = np.ascontiguousarray(kinds, np.uint8)
        n_nodes = int(self.table("dims")[0])
        out = np.zeros((len(pods), max(n_nodes, 1)), np.uint64)
        _check(lib().kbhip_debug_replay(self._h, len(pods), _p(pods), _p(modes), _p(nodes), _p(kinds), _p(out)))
        return out[:, :n_nodes]

    def close(self) -> None:
        if self._h:
            _check(lib().kbhip_session_close(self._h))
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def time_rank_multi(sessions, task_ids, reps: int = 16, evict: int = 0, mapped: int = 0) -> float:
    """kbhip_time_rank_multi: device microseconds of one multi-session preempt
    ranking launch chain over the given sessions (session i for its pending
    task task_ids[i])."""
    hs = (ctypes.c_void_p * len(sessions))(*[s._h for s in sessions])
    ids = np.ascontiguousarray(task_ids, dtype=np.int32)
    if ids.size != len(sessions):
        raise ValueError("one task id per session")
    out = np.zeros(1, np.float64)
    _check(lib().kbhip_time_rank_multi(hs, len(sessions), _p(ids), reps, evict, mapped, _p(out)))
    return float(out[0])


def shard_range(n_nodes: int, rank: int, world: int) -> Tuple[int, int]:
    """Node range [lo, hi) of a shard (the library's partition)."""
    return n_nodes * rank // world, n_nodes * (rank + 1) // world


def torch_gather(group=None, device=None):
    """An all-gather callback for kbhip_shard_connect_host_gather over
    torch.distributed (gloo on CPU tensors; device = a cuda device for the
    nccl (RCCL) backend): recv <- every rank's `send` bytes in rank order."""
    import torch
    import torch.distributed as dist

    def fn(send: np.ndarray, recv: np.ndarray) -> None:
        world = dist.get_world_size(group)
        out = [torch.empty(send.size, dtype=torch.uint8, device=device) for _ in range(world)]
        dist.all_gather(out, torch.from_numpy(send.copy()).to(device) if device is not None
                        else torch.from_numpy(send.copy()), group=group)
        recv[:] = torch.cat(out).cpu().numpy()
    return fn


def torch_exchange(group=None, device=None):
    """An exchange callback for kbhip_shard_connect_host doing the all-reduce
    with torch.distributed (gloo on CPU tensors; device = a cuda device for the
    nccl backend).  u64 keys are mapped to i64 by flipping the top bit, which
    preserves their order."""
    import torch
    import torch.distributed as dist

    def fn(vals: np.ndarray, op: int) -> None:
        v = vals.view(np.int64).copy()
        if op == RED_MAX_U64:
            v ^= np.int64(-0x8000000000000000)
        t = torch.from_numpy(v)
        if device is not None:
            t = t.to(device)
        rop = {RED_MIN_I64: dist.ReduceOp.MIN, RED_SUM_I64: dist.ReduceOp.SUM}.get(op, dist.ReduceOp.MAX)
        dist.all_reduce(t, op=rop, group=group)
        out = t.cpu().numpy()
        if op == RED_MAX_U64:
            out = out ^ np.int64(-0x8000000000000000)
        vals.view(np.int64)[:] = out
    return fn


class ShardedSession(Session):
    """A node-array shard of a session (include/kbhip.h): this
    rank's device holds nodes [lo, hi); every rank runs the same host loop and
    gets the same placements.  Connect with RCCL (connect_rccl, one GPU per
    rank) or with a Python exchange (connect_host, e.g. torch_exchange())."""

    def __init__(self, snapshot, device: int, rank: int, world: int):
        if not isinstance(snapshot, (bytes, bytearray, memoryview)):
            with open(snapshot, "rb") as f:
                snapshot = f.read()
        buf = bytes(snapshot)
        self._h = ctypes.c_void_p()
        self._cb = None
        _check(lib().kbhip_session_open_shard(ctypes.c_char_p(buf), len(buf), device, rank, world,
                                              ctypes.byref(self._h)))

    def info(self) -> Tuple[int, int, int, int]:
        out = np.zeros(4, np.int32)
        _check(lib().kbhip_shard_info(self._h, _p(out)))
        return tuple(int(x) for x in out)

    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = ctypes.create_string_buffer(512)
        n = _check(lib().kbhip_rccl_unique_id(buf, 512))
        return buf.raw[:n]

    def connect_rccl(self, unique_id: bytes) -> int:
        """1 when a pooled communicator of an earlier session was reused, 0 after a new init."""
        b = ctypes.create_string_buffer(unique_id, len(unique_id))
        _check(lib().kbhip_shard_connect_rccl(self._h, b, len(unique_id)))
        return int(self.stats()["comm_reused"])

    def connect_host(self, fn, gather=None) -> None:
        """fn(vals: np.ndarray[uint64], op) reduces vals in place across ranks
        (per-task pops); gather(send: np.ndarray[uint8], recv) fills recv with
        every rank's send bytes in rank order (batched pops; without it every
        pop takes the per-task path)."""
        def cb(_ctx, vals, n, op):
            try:
                fn(np.ctypeslib.as_array(vals, shape=(n,)), op)
                return 0
            except Exception:  # reported to the library as a failed exchange
                return 1
        self._cb = ALLREDUCE_FN(cb)  # keep the trampoline alive
        _check(lib().kbhip_shard_connect_host(self._h, self._cb, None))
        if gather is not None:
            world = self.info()[1]

            def gcb(_ctx, send, recv, nbytes):
                try:
                    s_arr = np.ctypeslib.as_array(ctypes.cast(send, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
                    r_arr = np.ctypeslib.as_array(ctypes.cast(recv, ctypes.POINTER(ctypes.c_uint8)),
                                                  shape=(nbytes * world,))
                    gather(s_arr, r_arr)
                    return 0
                except Exception:
                    return 1
            self._gcb = ALLGATHER_FN(gcb)
            _check(lib().kbhip_shard_connect_host_gather(self._h, self._gcb, None))

    def connect_mailbox(self, gather) -> None:
        """Peer mailboxes for the batched pops (kbhip_shard_connect_mailbox):
        gather(send, recv) all-gathers the ranks' IPC handles once."""
        world = self.info()[1]

        def mcb(_ctx, send, recv, nbytes):
            try:
                s_arr = np.ctypeslib.as_array(ctypes.cast(send, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
                r_arr = np.ctypeslib.as_array(ctypes.cast(recv, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes * world,))
                gather(s_arr.copy(), r_arr)
                return 0
            except Exception:
                return 1
        cb = ALLGATHER_FN(mcb)
        _check(lib().kbhip_shard_connect_mailbox(self._h, cb, None))
