"""kbhip_walk_visits / kbhip_fit_deltas without a GPU: the exports, the
null-session answers, and the visit counters of the host restatement.

kbhip_debug_replay restates the device's commit arithmetic on an encode-only
session, the GetAccessibleResource mutation included (Idle += Backfilled on
every node a tracked walk visits, node_info.go:209-211) — and with it the
per-node visit counter the device keeps beside that mutation.  Along the
oracle's decision sequence the replay's tables must satisfy, per node,

    Idle_now == Idle_at_open + visits x Backfilled - sum of Allocated Resreq

and Idle_now must be the faithful restatement's Idle.  The device path is
tests/test_gpu_walk.py.
"""
import ctypes

import numpy as np
import pytest

from walkmodel import PIPELINED_ST

FEATURES = ("labels", "taints", "ports", "init", "running", "releasing", "backfill", "selector", "nodeaffinity",
            "unsched")


def test_walk_symbols_exported(engine_lib):
    import kbhip
    for name in ("kbhip_walk_visits", "kbhip_fit_deltas"):
        assert name in kbhip.EXPORTS
        assert hasattr(engine_lib, name)


def test_walk_null_session(engine_lib):
    node = np.zeros(4, np.int32)
    cnt = np.zeros(4, np.uint32)
    delta = np.zeros((4, 3), np.int64)
    vp = ctypes.c_void_p
    assert engine_lib.kbhip_walk_visits(None, None, None, 0) == -1  # KBHIP_EINVAL
    assert engine_lib.kbhip_walk_visits(None, node.ctypes.data_as(vp), cnt.ctypes.data_as(vp), 4) == -1
    assert engine_lib.kbhip_fit_deltas(None, 0, None, None, 0) == -1
    assert engine_lib.kbhip_fit_deltas(None, 0, node.ctypes.data_as(vp), delta.ctypes.data_as(vp), 4) == -1
    assert b"null session" in engine_lib.kbhip_last_error()


def test_walk_encode_only_refused(engine_lib, kbgen_mod, tmp_path):
    """An encode-only session has no device state to read out."""
    import kbhip
    p = kbgen_mod.gen_random(7, n_nodes=4, n_jobs=2, max_tasks=2, features=FEATURES).write(str(tmp_path / "e.kbs"))
    with kbhip.EncodedSnapshot(p) as enc:
        assert engine_lib.kbhip_walk_visits(enc._h, None, None, 0) == -1
        assert engine_lib.kbhip_fit_deltas(enc._h, 0, None, None, 0) == -1


def _replay_invariant(path, n_pods, oracle_mod):
    import kbhip
    with kbhip.EncodedSnapshot(path) as enc:
        n_nodes = int(enc.table("dims")[0])
        idle0 = enc.table_raw("node_idle", np.int64).reshape(n_nodes, 3).copy()
        bf0 = enc.table_raw("node_backfilled", np.int64).reshape(n_nodes, 3).copy()
        assert not enc.table_raw("node_visits", np.uint32).any()  # zero at open
        tr = oracle_mod.fast_trace_affinity(path, n_nodes, cap_tasks=8192, actions="allocate")
        kinds = np.where(tr["status"] == PIPELINED_ST, 2, 1).astype(np.uint8)
        enc.replay(tr["pod"], tr["mode"], tr["node"], kinds)
        idle = enc.table_raw("node_idle", np.int64).reshape(n_nodes, 3)
        bf = enc.table_raw("node_backfilled", np.int64).reshape(n_nodes, 3)
        visits = enc.table_raw("node_visits", np.uint32).astype(np.int64)
    assert np.array_equal(bf, bf0)  # no pending task of these clusters is backfill-annotated
    req = oracle_mod.ref_task_requests(path, n_pods).astype(np.int64)
    committed = np.zeros((n_nodes, 3), np.int64)
    for pod, node, st in zip(tr["pod"], tr["node"], tr["status"]):
        if node >= 0 and st != PIPELINED_ST:  # Allocated (or Binding once the job was dispatched): Idle -= Resreq
            committed[node] += req[pod, 0:3]
    assert np.array_equal(idle, idle0 + visits[:, None] * bf0 - committed)
    _, ons = oracle_mod.ref_allocate(path, with_nodes=True)
    assert np.array_equal(idle.astype(np.float64), ons[:n_nodes, 0:3])
    return int((visits[(bf0 != 0).any(axis=1)] > 0).sum())


@pytest.mark.parametrize("seed", range(16))
def test_replay_visit_invariant(engine_lib, oracle_mod, kbgen_mod, tmp_path, seed):
    c = kbgen_mod.gen_random(7300 + seed, n_nodes=3 + seed % 13, n_jobs=5 + seed % 9, max_tasks=2 + seed % 12,
                             features=FEATURES)
    p = c.write(str(tmp_path / "r.kbs"))
    _replay_invariant(p, len(c.pods), oracle_mod)


def test_replay_visits_reach_backfilled_nodes(engine_lib, oracle_mod, kbgen_mod, tmp_path):
    """The invariant above says nothing where no Backfilled node is visited:
    most of these seeds must visit one."""
    hit = 0
    for seed in range(16):
        c = kbgen_mod.gen_random(7300 + seed, n_nodes=3 + seed % 13, n_jobs=5 + seed % 9, max_tasks=2 + seed % 12,
                                 features=FEATURES)
        hit += _replay_invariant(c.write(str(tmp_path / f"r{seed}.kbs")), len(c.pods), oracle_mod) > 0
    assert hit >= 8
