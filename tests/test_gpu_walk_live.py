"""kbhip_walk_begin_live on the device: the eviction-walk cursor opened for
reclaim's order so that the pod-affinity predicate is tested per call.

The yardsticks: the oracle's reclaim records for the host loop, the
restatement of the live protocol (tests/walklive.py over walkvictims.chain and
victimmodel) call by call, kbhip_walk_begin on the same session for the kept
order of a class that reads no affinity targets, and the session's own tables
for what the calls must leave alone."""
import functools

import numpy as np
import pytest

import victimmodel
import walkcursor as wc
import walklive as wl
import walkvictims
import walkwindows as ww
from walkvictims import ASSIGNED, EXHAUSTED, HEAD_END

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"
KEYS = ("stop", "total", "decided", "acted", "next", "first", "last_node")  # out_info[0 .. 5] and [8]


def _send(engine, s, ops):
    assert s.apply_ops([o for o, _, _ in ops], [p for _, p, _ in ops], [n for _, _, n in ops]) <= 2


def _order(s):
    total, nodes, scores = s.walk_order()
    assert total == len(nodes) and not scores.any()
    return [int(n) for n in nodes]


def _check_scan(info, pos, extra=0):
    """out_info[9] within its bounds and the launch count: 2, plus the two documented extras."""
    room = info["total"] - pos
    if info["first"] >= 0:
        assert info["first"] - pos + 1 <= info["scanned"] <= room, info
    else:
        assert info["scanned"] == room, info
    assert info["launches"] == 2 + bool(info["patched"]) + extra, info


def _ask(s, cap=64, cap_ops=4096):
    def ask(pos):
        got = s.walk_next(pos, cap, cap_ops)
        _check_scan(got[3], pos)
        return walkvictims.as_ops(got), got[3]
    return ask


def _same_calls(got, exp, where):
    assert len(got) == len(exp), (where, got, exp)
    for k, ((g_ops, g), (e_ops, e)) in enumerate(zip(got, exp)):
        assert g_ops == e_ops, (where, k)
        assert {x: g[x] for x in KEYS} == {x: e[x] for x in KEYS}, (where, k)


@pytest.fixture(scope="module")
def clusters(tmp_path_factory, oracle_mod):
    d = tmp_path_factory.mktemp("walk_live")

    @functools.lru_cache(maxsize=None)
    def get(name):
        c = wl.big() if name == "big" else wl.CLUSTERS[name]()
        path = c.write(str(d / (name + ".kbs")))
        m = victimmodel.VictimModel(c)
        return path, c, m, wl.AffPred(c), ww.task_of(m)

    return get


# ---- 1. the host reclaim loop: fails without kbhip_walk_begin_live -------------------------------------
@pytest.mark.parametrize("name", ["leave", "enter"])
def test_host_reclaim_loop_equals_the_oracle_and_the_restatement(engine, clusters, oracle_mod, name):
    path, c, m, aff, task = clusters(name)
    ref = [tuple(r) for r in oracle_mod.ref_allocate(path, actions="reclaim").as_list()]
    assert [n for _, n, _ in ref] == wl.EXPECTED_NODES[name]
    for cap in (1, 64):
        got, begins = [], []
        with engine.Session(path) as s:
            ask = _ask(s, cap)

            def asked(pos):
                got.append(ask(pos))
                return got[-1]

            log, asks, stops = wl.host_reclaim_walk_live(
                victimmodel.VictimModel(c), lambda t: begins.append((t,) + s.walk_begin_live(t, 1)), asked,
                lambda ops: _send(engine, s, ops))
        assert log == ref, (name, cap)
        assert [(t, i["affinity_targets"]) for t, _, i in begins] == [(task, wl.LIVE)]
        order, exp, live = wl.expected_calls(m, aff, task, 1, cap)
        assert live and begins[0][1] == len(order) == 4
        _same_calls(got, exp, (name, cap))
        assert asks == [2] and stops == [HEAD_END, ASSIGNED]


# ---- 2. the kept order ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["leave", "enter", "spill"])
def test_kept_order(engine, clusters, name):
    path, c, m, aff, task = clusters(name)
    with engine.Session(path) as s:
        fixed_total, fixed_info = s.walk_begin(task, False, 1)
        fixed = _order(s)
        assert fixed == wl.fixed_order(m, aff, task, 1) and fixed_info["affinity_targets"] == 1
        total, info = s.walk_begin_live(task, 1)  # a second begin, of the other kind, replaces the first
        live = _order(s)
        assert live == wl.live_order(m, task, 1) == sorted(live) and total == len(live) >= fixed_total
        assert set(fixed) <= set(live) and info["affinity_targets"] == wl.LIVE and not info["rebuilt"]
        assert info["launches"] == 4 and info["bytes"] >= 8 * total  # the marks and the compaction's three
        assert s.walk_order(1, 2)[1].tolist() == live[1:3]
        if name == "enter":
            assert total > fixed_total
        assert s.walk_begin(task, False, 1)[0] == fixed_total and _order(s) == fixed


# ---- 3. a class that reads no affinity targets ---------------------------------------------------------------
def test_control_cluster_is_walk_begin(engine, clusters):
    path, c, m, aff, task = clusters("control")
    for cap in (1, 64):
        runs = []
        for live_call in (False, True):
            with engine.Session(path) as s:
                s.rank_victim_nodes(task, False, 1, 0, 1 << 16)  # (the candidate table: built before either begin)
                total, info = s.walk_begin_live(task, 1) if live_call else s.walk_begin(task, False, 1)
                assert info["affinity_targets"] == 0
                runs.append((total, info, _order(s), wc.protocol(_ask(s, cap), lambda ops: _send(engine, s, ops))))
        assert runs[0][:3] == runs[1][:3]
        _same_calls(runs[1][3], runs[0][3], cap)
        order, exp, live = wl.expected_calls(m, aff, task, 1, cap)
        assert not live and runs[1][2] == order
        _same_calls(runs[1][3], exp, cap)
        assert len(exp) == (2 if cap == 1 else 1)  # cap 64: both acting nodes in one call, as on any fixed cursor


# ---- 4. one acting node per call; the spill rule with the predicate -------------------------------------------
def test_one_acting_node_per_call_and_the_spill_rule(engine, clusters):
    """spill: node 0 holds 257 candidate tasks in a zone without a target, nodes 1 and 2 (zone b) are VALID and
    within cap of it.  The scan does not decide node 0 (`first` = 0), the serial loop passes it over by the
    predicate, and the call acts on node 1 alone: HEAD_END, the next position behind node 1, although node 2
    is VALID and two entries further.  The second call assigns on node 2."""
    path, c, m, aff, task = clusters("spill")
    assert len(m.candidates(task, 1, 0)) == ww.LONG and not aff.holds(m, task, 0)
    assert all(aff.holds(m, task, n) and m.decide(task, 1, n)[2] & 1 for n in (1, 2))
    with engine.Session(path) as s:
        assert s.walk_begin_live(task, 1)[0] == 4 and _order(s) == [0, 1, 2, 3]
        a = s.walk_next(0, 64)
        _check_scan(a[3], 0)
        assert [a[3][k] for k in KEYS] == [HEAD_END, 4, 2, 1, 2, 0, 1]
        assert set(a[2].tolist()) == {1} and len(a[0]) == 1
        _send(engine, s, walkvictims.as_ops(a))
        b = s.walk_next(a[3]["next"], 64)
        assert [b[3][k] for k in KEYS] == [ASSIGNED, 4, 1, 1, 3, 2, 2] and b[3]["patched"] > 0
        exp = wl.expected_live_calls(m, aff, task, 1, [0, 1, 2, 3], 64, spill={0})
        _same_calls([(walkvictims.as_ops(a), a[3]), (walkvictims.as_ops(b), b[3])], exp, "spill")
    with engine.Session(path) as s:  # cap 1: the long node uses the call up
        s.walk_begin_live(task, 1)
        got = wc.protocol(_ask(s, 1), lambda ops: _send(engine, s, ops))
        _same_calls(got, wl.expected_live_calls(m, aff, task, 1, [0, 1, 2, 3], 1, spill={0}), "spill cap 1")
        assert got[0][0] == [] and got[0][1]["next"] == 1 and len(got) == 3


# ---- 5. the grid-stride path ---------------------------------------------------------------------------------
def test_walk_longer_than_the_scan_grid(engine, clusters):
    """2100 entries, `first` = 2090: every entry in front of it is victims-VALID (kbhip_walk_begin's scan would
    stop at 0) and fails the predicate, so the scan's blocks decide their second entry too."""
    path, c, m, aff, task = clusters("big")
    with engine.Session(path) as s:
        total, info = s.walk_begin_live(task, 1)
        assert total == wl.BIG_N and info["affinity_targets"] == wl.LIVE
        assert s.walk_begin(task, False, 1)[0] == 1  # the fixed order: the one node whose zone has a target
        assert s.walk_begin_live(task, 1)[0] == wl.BIG_N
        got = s.walk_next(0)
        _check_scan(got[3], 0)
        gap = got[3]["first"]
        assert gap == wl.BIG_FIRST > wl.BIG_GRID and gap + 1 <= got[3]["scanned"] <= wl.BIG_N
        exp = wl.expected_live_calls(m, aff, task, 1, list(range(wl.BIG_N)))
        _same_calls([(walkvictims.as_ops(got), got[3])], exp, "big")
        assert got[3]["stop"] == ASSIGNED and got[3]["decided"] == wl.BIG_FIRST + 1


# ---- 6. launch counts and read-only --------------------------------------------------------------------------
def test_launches_and_read_only(engine, clusters):
    path, c, m, aff, task = clusters("leave")
    tables = ("pod_status", "job_ready", "pod_job", "pod_queue")
    with engine.Session(path) as s:
        n_nodes = s.stats()["nodes"]
        s.walk_begin_live(task, 1)
        first = s.walk_next(0)  # (builds the victim state)
        assert first[3]["launches"] == 2 and first[3]["state_rebuilt"] and not first[3]["patched"]
        rows = s.read_nodes(n_nodes)
        tab0 = [s.table(n).copy() for n in tables]
        sweeps = s.stats()["sweeps"]
        total, info = s.walk_begin_live(task, 1)
        assert info["launches"] == 4 and not info["rebuilt"]
        for _ in range(2):  # nothing was applied: the same answer twice
            again = s.walk_next(0)
            assert walkvictims.as_ops(again) == walkvictims.as_ops(first) and again[3]["launches"] == 2
            assert [again[3][k] for k in KEYS] == [first[3][k] for k in KEYS]
        order = _order(s)
        assert s.stats()["sweeps"] == sweeps + 3
        assert all(np.array_equal(a, s.table(n)) for a, n in zip(tab0, tables))
        assert np.array_equal(s.read_nodes(n_nodes), rows)
        # the two documented extras: the patch of the victim state, and (counted by the call that flushes them)
        # the pending pod-affinity count changes — kbhip_apply_ops flushes its own, so kbhip_walk_next sees none
        _send(engine, s, walkvictims.as_ops(first))
        nxt = s.walk_next(first[3]["next"])
        assert nxt[3]["patched"] > 0 and nxt[3]["launches"] == 3 and not nxt[3]["state_rebuilt"]
        assert _order(s) == order  # the cursor survives kbhip_apply_ops


# ---- 7. lifetime and errors ------------------------------------------------------------------------------------
def test_lifetime(engine, clusters):
    path, c, m, aff, task = clusters("leave")

    def gone(s):
        for call in (lambda: s.walk_next(0), lambda: s.walk_order()):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                call()
        assert s.walk_end() is False

    with engine.Session(path) as s:
        assert s.walk_begin_live(task, 1)[0] == 4
        a = s.walk_next(0)
        _send(engine, s, walkvictims.as_ops(a))
        assert _order(s) == [0, 1, 2, 3]  # survives kbhip_apply_ops
        assert s.walk_begin(task, False, 1)[0] == 2  # a second begin of the other kind: node 1's zone lost its target
        assert _order(s) == [2, 3]
        assert s.walk_begin_live(task, 1)[0] == 3 and _order(s) == [1, 2, 3]  # (node 0's only candidate is evicted)
        assert s.walk_begin_live(task, 1)[0] == 3  # and of the same kind
        b = s.walk_next(0)
        assert (b[3]["first"], b[3]["last_node"], b[3]["stop"]) == (1, 2, ASSIGNED)
        s.first_fit([task])
        gone(s)
    with engine.Session(path) as s:
        s.walk_begin_live(task, 1)
        assert s.walk_end() is True
        gone(s)


def test_errors(engine, clusters):
    path, c, m, aff, task = clusters("leave")
    with engine.Session(path) as s:
        for victims in (0, 4, -1):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.walk_begin_live(task, victims)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_begin_live(0, 1)  # a Running pod: no task class
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_begin_live(len(m.h.pods), 1)
        with pytest.raises(engine.KbhipError, match=EINVAL):  # no cursor is open after refused begins
            s.walk_order()
        assert s.walk_begin(task, False, 1)[0] == 4
        info = np.full(4, 77, np.int64)
        L = engine.lib()
        assert L.kbhip_walk_begin_live(s._h, task, 0, info.ctypes.data) == -1
        assert L.kbhip_walk_begin_live(s._h, 0, 1, info.ctypes.data) == -1
        assert (info == 77).all() and _order(s) == [0, 1, 2, 3]  # refused calls write nothing and leave the cursor open
        assert s.walk_begin_live(task, 1)[0] == 4
        for pos, cap, cap_ops in ((-1, 4, 4), (5, 4, 4), (0, 0, 4), (0, 65, 4), (0, 4, 0)):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.walk_next(pos, cap, cap_ops)
        last = s.walk_next(4)
        assert len(last[0]) == 0 and (last[3]["stop"], last[3]["decided"], last[3]["first"], last[3]["next"]) == (
            EXHAUSTED, 0, -1, 4)
    sh = engine.ShardedSession(path, 0, 0, 2)
    try:
        with pytest.raises(engine.KbhipError, match=EUNSUP):
            sh.walk_begin_live(task, 1)
    finally:
        sh.close()
