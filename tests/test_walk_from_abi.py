"""kbhip_walk_victims_from without a device: the declaration and the binding,
every argument refusal on an encode-only session, and the conditions the device
test's inputs (tests/walkwindows.py) have to meet, checked with the
restatement alone (tests/walkvictims.py over tests/victimmodel.py): each
cluster's chain has the stated length, stops and acted-on positions, and the
chain cut at window edges — the model moved on by the ops between the cuts —
concatenates to the uncut chain."""
import ctypes
import os
import re

import numpy as np
import pytest

import victimmodel
import walkvictims
import walkwindows as ww
from walkvictims import ASSIGNED, CAPACITY, EXHAUSTED, HEAD_END, EVICT, PIPELINE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
vp = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(vp)


def test_declared_exported_and_bound(engine_lib):
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    assert re.search(r"\bint64_t\s+kbhip_walk_victims_from\s*\(", src)
    assert "kbhip_walk_victims_from" in kbhip.EXPORTS and hasattr(engine_lib, "kbhip_walk_victims_from")
    assert callable(getattr(kbhip.Session, "walk_victims_from", None))
    assert (ASSIGNED, EXHAUSTED, HEAD_END, CAPACITY) == (kbhip.WALK_ASSIGNED, kbhip.WALK_EXHAUSTED,
                                                         kbhip.WALK_HEAD_END, kbhip.WALK_CAPACITY)
    info = kbhip._walk_from_info(np.array([3, 130, 64, 2, 17, -5, 6, 1 | 2 | (9 << 8), 12, 4], np.int64))
    assert info == dict(stop=3, remaining=130, visited=64, acted=2, resume_node=17, resume_score=-5, launches=6,
                        rebuilt=1, state_rebuilt=1, patched=9, last_node=12, first_valid=4)
    go = open(os.path.join(ROOT, "go", "kbhip", "kbhip.go")).read()
    assert "C.kbhip_walk_victims_from(" in go and "func (e *Engine) WalkVictimsFrom(" in go


def test_argument_validation(engine_lib, kbgen_mod, tmp_path):
    """Every refusal, on an encode-only session (no device needed): KBHIP_EINVAL, and no output written."""
    import kbhip
    L = engine_lib
    o = [np.full(8, 77, np.uint8), np.full(8, 77, np.int32), np.full(8, 77, np.int32), np.full(10, 77, np.int64)]
    ptr = [_p(a) for a in o]
    wf = L.kbhip_walk_victims_from
    assert wf(None, 0, 1, 1, 4, -1, 0, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
    assert b"null session" in L.kbhip_last_error()
    enc = kbhip.EncodedSnapshot(ww.build(ww.blocked(4)).write(str(tmp_path / "v.kbs")))
    try:
        t = int(np.nonzero(enc.table("pod_class") >= 0)[0][0])
        assert wf(enc._h, t, 1, 1, 4, -1, 0, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
        assert b"encode-only" in L.kbhip_last_error()
        for cap, cap_ops, word in ((0, 8, b"cap is"), (65, 8, b"cap is"), (-1, 8, b"cap is"), (4, 0, b"cap_ops"),
                                   (4, -1, b"cap_ops")):
            assert wf(enc._h, t, 1, 1, cap, -1, 0, ptr[0], ptr[1], ptr[2], cap_ops, ptr[3]) == EINVAL
            assert b"kbhip_walk_victims_from" in L.kbhip_last_error() and word in L.kbhip_last_error()
        for k in range(3):  # a null required output (out_info is optional)
            q = list(ptr)
            q[k] = None
            assert wf(enc._h, t, 1, 1, 4, -1, 0, q[0], q[1], q[2], 8, q[3]) == EINVAL
            assert b"null out_op" in L.kbhip_last_error()
        for by_score in (2, -1):
            assert wf(enc._h, t, by_score, 1, 4, -1, 0, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
            assert b"by_score" in L.kbhip_last_error()
        for mode in (0, 4, -1):
            assert wf(enc._h, t, 1, mode, 4, -1, 0, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
            assert b"KBHIP_VICTIMS" in L.kbhip_last_error()
        for after in (-2, 4, 1 << 30):  # (a device session refuses these by name; here the session itself is)
            assert wf(enc._h, t, 1, 1, 4, after, 0, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
        assert wf(enc._h, t, 1, 1, 4, -1, 0, ptr[0], ptr[1], ptr[2], 8, None) == EINVAL
        assert all((a == 77).all() for a in o)  # a refused call writes nothing
    finally:
        enc.close()


# ---- the inputs of the device test ------------------------------------------------------------------
def _model(name, mode):
    c = ww.CLUSTERS[name][0](mode)
    m = victimmodel.VictimModel(c)
    return c, m, ww.task_of(m)


def _cat(calls):
    return [op for ops, _ in calls for op in ops]


@pytest.mark.parametrize("name", sorted(ww.CLUSTERS))
def test_every_node_is_in_the_pruned_walk(name):
    """Each node has candidates of the mode and the task asks for no GPU: kbhip_rank_victim_nodes' test keeps
    every node, so the walk in index order is 0 .. n - 1 (and the by-score walk a permutation of it)."""
    for mode in ww.CLUSTERS[name][1]:
        c, m, task = _model(name, mode)
        assert m.ireq[task][2] == 0
        assert all(m.candidates(task, mode, n) for n in range(m.n_nodes))
        for by_score in (False, True):
            assert sorted(ww.walk_of(name, by_score)) == list(range(m.n_nodes))


@pytest.mark.parametrize("name", sorted(ww.LENGTHS))
def test_walk_lengths(name):
    for mode in ww.CLUSTERS[name][1]:
        c, m, task = _model(name, mode)
        walk = ww.walk_of(name, False)
        ops, info = walkvictims.chain(m, task, mode, walk)
        assert (ops, info["stop"], info["visited"], info["acted"]) == ([], EXHAUSTED, len(walk), 0)
        calls = ww.expected_calls(m, task, mode, walk)
        assert [(i["stop"], i["remaining"], i["visited"]) for _, i in calls] == ww.LENGTHS[name]
        assert all(i["first_valid"] == -1 and i["last_node"] == -1 and not o for o, i in calls)
        assert sum(i["visited"] for _, i in calls) == len(walk)
        assert [i["resume_node"] for _, i in calls] == [min(64 * (k + 1), len(walk)) - 1 for k in range(len(calls))]


@pytest.mark.parametrize("pos", [0, 63, 64, 65, 129])
@pytest.mark.parametrize("kind", ["covers", "valid"])
def test_first_valid_positions(kind, pos):
    name = "%s_at%d" % (kind, pos)
    for mode in ww.CLUSTERS[name][1]:
        c, m, task = _model(name, mode)
        walk = ww.walk_of(name, False)
        ops, info = walkvictims.chain(m, task, mode, walk)
        assert info["acted"] == 1 and info["last_node"] == pos
        exp = [(EVICT, pos, pos)] + ([(PIPELINE, task, pos)] if kind == "covers" else [])
        assert ops == exp and info["stop"] == (ASSIGNED if kind == "covers" else EXHAUSTED)
        assert info["visited"] == (pos + 1 if kind == "covers" else 130)
        calls = ww.expected_calls(m, task, mode, walk)
        assert _cat(calls) == ops
        w = pos // 64  # the window the node is in: its first, its last slot, or just over the edge
        assert [i["first_valid"] for _, i in calls[:w + 1]] == [-1] * w + [pos % 64]
        assert len(calls) == (w + 1 if kind == "covers" else 3)


@pytest.mark.parametrize("name,acted,stateless", [("gang_carried", ww.GANG_ACTED, ww.GANG_STATELESS),
                                                  ("drf_carried", ww.DRF_ACTED, ww.DRF_STATELESS),
                                                  ("proportion_carried", ww.PROP_ACTED, ww.PROP_STATELESS)])
def test_carried_state_crosses_a_window_edge(name, acted, stateless):
    for mode in ww.CLUSTERS[name][1]:
        c, m, task = _model(name, mode)
        walk = ww.walk_of(name, False)
        ops, info = walkvictims.chain(m, task, mode, walk)
        flat, _ = walkvictims.chain(m, task, mode, walk, carried=False)
        assert [n for o, _, n in ops if o == EVICT] == acted and info["stop"] == ASSIGNED
        assert [n for o, _, n in flat if o == EVICT] == stateless != acted
        assert ops[-1] == (PIPELINE, task, 100) and info["acted"] == 3
        # cut at the window edge: the first eviction reaches the second window through the model, as through
        # kbhip_apply_ops; within that window the second one is carried by the chain
        calls = ww.expected_calls(m, task, mode, walk)
        assert _cat(calls) == ops and [i["stop"] for _, i in calls] == [HEAD_END, ASSIGNED]
        assert [i["acted"] for _, i in calls] == [1, 2] and [i["first_valid"] for _, i in calls] == [10, 70 - 64]
        # the second window answered on the opened state (nothing applied between the cuts) acts on other
        # nodes: the eviction of the first window really crosses the edge
        late, _ = walkvictims.chain(m, task, mode, walk[64:128])
        assert [n for o, _, n in late if o == EVICT] == ww.UNAPPLIED[name] != [n for n in acted if n >= 64]
        # every cap and a cap_ops of one step give the same log
        for cap in (1, 7):
            assert _cat(ww.expected_calls(m, task, mode, walk, cap=cap)) == ops
        capped = ww.expected_calls(m, task, mode, walk, cap_ops=2, ov_max=1)
        assert _cat(capped) == ops and CAPACITY in [i["stop"] for _, i in capped]


@pytest.mark.parametrize("name,valid", [("ties", (62, 66)), ("negative", (5, 70))])
def test_scored_walks(name, valid):
    for mode in ww.CLUSTERS[name][1]:
        c, m, task = _model(name, mode)
        by_index, by_score = ww.walk_of(name, False), ww.walk_of(name, True)
        assert by_index != by_score
        ops, info = walkvictims.chain(m, task, mode, by_score)
        assert [n for _, _, n in ops] == [by_score[p] for p in valid] and info["stop"] == EXHAUSTED
        calls = ww.expected_calls(m, task, mode, by_score, scores=[0] * len(by_score))
        assert _cat(calls) == ops and [i["stop"] for _, i in calls] == [HEAD_END, EXHAUSTED]
        assert calls[0][1]["resume_node"] == by_score[63] and calls[1][1]["remaining"] == len(by_score) - 64
    if name == "ties":  # the window edge is inside the run of equal scores (same group: positions 60 .. 70)
        assert len(c.nodes) == 91 and by_score[60:71] == list(range(11))


def test_long_node():
    name = "long_node"
    for mode in ww.CLUSTERS[name][1]:
        c, m, task = _model(name, mode)
        walk = ww.walk_of(name, False)
        assert len(m.candidates(task, mode, 65)) == ww.LONG == 257
        ops, info = walkvictims.chain(m, task, mode, walk)
        assert info["stop"] == ASSIGNED and info["acted"] == 3 and info["last_node"] == 80
        assert sum(n == 65 for _, _, n in ops) == 257
        calls = ww.expected_calls(m, task, mode, walk)
        assert _cat(calls) == ops and [i["first_valid"] for _, i in calls] == [10, 1]


def test_reclaim_snapshot_leaves_the_first_window(oracle_mod, tmp_path):
    """The end-to-end snapshot: the oracle's reclaim evicts on walk position 66 and pipelines the task there;
    the host loop over chain-made windows reproduces its log in two asks."""
    c = ww.reclaim_snapshot()
    p = c.write(str(tmp_path / "r.kbs"))
    log = [tuple(r) for r in oracle_mod.ref_allocate(p, actions="reclaim").as_list()]
    m = victimmodel.VictimModel(c)
    task = ww.task_of(m)
    assert log == [(66, 66, 128), (task, 66, 8)]
    walk = list(range(m.n_nodes))

    def ask(t, after):
        pos = 0 if after is None else walk.index(after[0]) + 1
        calls = ww.expected_calls(m, t, 1, walk[pos:])
        return calls[0]

    got, asks, stops = ww.host_reclaim_walk_windows(m, ask, lambda ops: None)
    assert got == log and asks == [2] and stops == [HEAD_END, ASSIGNED]
