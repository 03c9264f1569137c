"""kbhip_walk_victims_from on the device: a task's eviction walk of any length,
one window of up to 64 entries per call.

The yardstick is the restatement's chain (tests/walkvictims.py over
tests/victimmodel.py) cut into windows (walkwindows.expected_calls) along the
whole pruned walk that kbhip_rank_victim_nodes' full-sort path returns on the
session as opened, kbhip_walk_victims on a twin session where the two calls
agree by contract, and the oracle's reclaim records for the host loop."""
import functools

import numpy as np
import pytest

import victimmodel
import walkvictims
import walkwindows as ww
from test_gpu_victim_walk import CASES, EXACT, _gen, _jobs
from test_gpu_walk_victims import _packed
from walkvictims import ASSIGNED, CAPACITY, EXHAUSTED, HEAD_END

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"


def _send(engine, s, ops):
    assert (engine.OP_EVICT, engine.OP_PIPELINE) == (walkvictims.EVICT, walkvictims.PIPELINE)
    assert s.apply_ops([o for o, _, _ in ops], [p for _, p, _ in ops], [n for _, _, n in ops]) <= 2


def _full_walk(s, task, by_score, mode):
    """The whole pruned walk of the session as it stands, from the full-sort path: (nodes, scores)."""
    total, nodes, scores, _, info = s.rank_victim_nodes(task, by_score, mode, 0, 1 << 16)
    assert info["head"] == 0 and len(nodes) == total
    return [int(n) for n in nodes], [int(x) for x in scores]


def _loop(engine, s, task, by_score, mode, cap=64, cap_ops=4096):
    def ask(after):
        got = s.walk_victims_from(task, by_score, mode, cap, after, cap_ops)
        assert len(got[0]) <= cap_ops
        return walkvictims.as_ops(got), got[3]

    return ww.protocol(ask, lambda ops: _send(engine, s, ops))


def _same_calls(got, exp, where):
    assert len(got) == len(exp), where
    for k, ((g_ops, g), (e_ops, e)) in enumerate(zip(got, exp)):
        assert g_ops == e_ops, (where, k)
        assert {x: g[x] for x in ww.INFO_KEYS} == {x: e[x] for x in ww.INFO_KEYS}, (where, k)


def _run(engine, path, m, task, mode, by_score, **kw):
    """One protocol loop on a fresh session against expected_calls over the walk ranked once.  -> (calls, walk)"""
    with engine.Session(path) as s:
        if kw.get("ov_max"):
            s.set_option("walk_overlay_max", kw["ov_max"])
        nodes, scores = _full_walk(s, task, by_score, mode)
        exp = ww.expected_calls(m, task, mode, nodes, scores if by_score else None, cap=kw.get("cap", 64),
                                cap_ops=kw.get("cap_ops"), ov_max=kw.get("ov_max", 0))
        got = _loop(engine, s, task, by_score, mode, kw.get("cap", 64), kw.get("cap_ops") or 4096)
        _same_calls(got, exp, (mode, by_score, kw))
        return got, nodes


@pytest.fixture(scope="module")
def clusters(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_from")

    @functools.lru_cache(maxsize=None)
    def get(name, mode):
        c = ww.CLUSTERS[name][0](mode)
        m = victimmodel.VictimModel(c)
        return c.write(str(d / ("%s_%d.kbs" % (name, mode)))), m, ww.task_of(m)

    return get


# ---- 1. the expected walk ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ww.CLUSTERS))
def test_expected_walk(engine, clusters, name):
    for mode in ww.CLUSTERS[name][1]:
        path, m, task = clusters(name, mode)
        for by_score in (False, True):
            got, nodes = _run(engine, path, m, task, mode, by_score)
            # the walk is the one the cluster was built for
            assert nodes == ww.walk_of(name, by_score), (name, mode, by_score)
            assert got[-1][1]["stop"] in (ASSIGNED, EXHAUSTED)
            if name in ww.LENGTHS:
                assert [(i["stop"], i["remaining"], i["visited"]) for _, i in got] == ww.LENGTHS[name]
                assert not any(o for o, _ in got) and all(i["first_valid"] == -1 for _, i in got)
    if name == "negative":
        with engine.Session(clusters(name, 1)[0]) as s:
            assert max(_full_walk(s, clusters(name, 1)[2], True, 1)[1]) < 0
    if name == "ties":
        with engine.Session(clusters(name, 1)[0]) as s:
            sc = _full_walk(s, clusters(name, 1)[2], True, 1)[1]
            assert len(set(sc[60:71])) == 1 and sc[59] > sc[60] and sc[70] > sc[71]


# ---- 2. agreement with kbhip_walk_victims ------------------------------------------------------
@pytest.fixture(scope="module")
def snaps(oracle_mod, kbgen_mod, tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_from_snaps")

    @functools.lru_cache(maxsize=None)
    def get(case):
        c = _gen(kbgen_mod, case)
        p = c.write(str(d / ("c%d_%d_%d_%d.kbs" % case)))
        return p, oracle_mod.ref_allocate(p, actions="reclaim").as_list(), c

    return get


def _agree(s, twin, tasks):
    for t in tasks:
        for by_score in (True, False):
            for mode in (1, 2, 3):
                a, b = s.walk_victims_from(t, by_score, mode), twin.walk_victims(t, by_score, mode)
                where = (t, by_score, mode)
                assert walkvictims.as_ops(a) == walkvictims.as_ops(b), where
                assert [a[3][k] for k in ("stop", "visited", "acted")] == [b[3][k] for k in ("stop", "visited", "acted")], where
                assert a[3]["remaining"] == b[3]["total"] and a[3]["last_node"] == b[3]["last_node"], where
                assert a[3]["launches"] - bool(a[3]["patched"]) == b[3]["launches"] - bool(b[3]["patched"]) + 1, where


@pytest.mark.parametrize("case", CASES[:6], ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_agrees_with_walk_victims(engine, snaps, case):
    p, reclaim, c = snaps(case)
    m = victimmodel.VictimModel(c)
    with engine.Session(p) as s, engine.Session(p) as twin:
        _agree(s, twin, m.pending())
        if reclaim:
            E, P = engine.OP_EVICT, engine.OP_PIPELINE
            for x in (s, twin):
                x.apply_ops([E if k == 128 else P for _, _, k in reclaim], [q for q, _, _ in reclaim],
                            [n for _, n, _ in reclaim])
            m.records(reclaim)
            left = m.pending()
            if left:  # patched, not rebuilt
                i0 = s.walk_victims_from(left[0], False, 1)[3]
                assert i0["patched"] > 0 and not i0["rebuilt"] and not i0["state_rebuilt"]
                twin.walk_victims(left[0], False, 1)
            _agree(s, twin, left)


# ---- 3. capacity ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gang_carried", "drf_carried", "proportion_carried"])
def test_capacity_and_caps(engine, clusters, name):
    mode = ww.CLUSTERS[name][1][-1]
    path, m, task = clusters(name, mode)
    for by_score in (False, True):
        full, nodes = _run(engine, path, m, task, mode, by_score)
        log = [op for ops, _ in full for op in ops]
        assert full[-1][1]["stop"] == ASSIGNED and sum(i["acted"] for _, i in full) == 3
        steps = [sum(1 for o in log if o[2] == n and o[0] == walkvictims.EVICT) for n in dict.fromkeys(o[2] for o in log)]
        capped, _ = _run(engine, path, m, task, mode, by_score, cap_ops=max(steps) + 1, ov_max=1)
        assert [op for ops, _ in capped for op in ops] == log
        stops = [i["stop"] for _, i in capped]
        assert CAPACITY in stops
        # a node refused by CAPACITY is not behind the resume point: it is the walk entry right behind it, and
        # the next call meets it first and acts on it
        k = stops.index(CAPACITY)
        refused = nodes[nodes.index(capped[k][1]["resume_node"]) + 1]
        assert capped[k + 1][1]["first_valid"] == 0 and capped[k + 1][0][0][2] == refused
        for cap in (1, 7):
            got, _ = _run(engine, path, m, task, mode, by_score, cap=cap)
            assert [op for ops, _ in got for op in ops] == log
            assert all(i["visited"] <= cap for _, i in got)


# ---- 4. end to end ------------------------------------------------------------------------------
def _host_loop(engine, p, c):
    m = victimmodel.VictimModel(c)
    with engine.Session(p) as s:
        def ask(task, after):
            got = s.walk_victims_from(task, False, 1, 64, after)
            return walkvictims.as_ops(got), got[3]

        return ww.host_reclaim_walk_windows(m, ask, lambda ops: _send(engine, s, ops))


def test_host_reclaim_walk_equals_the_oracle(engine, snaps, oracle_mod, tmp_path):
    for case in EXACT:
        p, reclaim, c = snaps(case)
        log, asks, stops = _host_loop(engine, p, c)
        assert log == [tuple(r) for r in reclaim], case
        assert sum(k == 8 for _, _, k in log) >= 2 and asks and set(stops) <= {ASSIGNED, EXHAUSTED}, case
    c = ww.reclaim_snapshot()
    p = c.write(str(tmp_path / "r.kbs"))
    reclaim = [tuple(r) for r in oracle_mod.ref_allocate(p, actions="reclaim").as_list()]
    assert any(k == 128 and n > 64 for _, n, k in reclaim)  # an eviction beyond walk position 64
    log, asks, stops = _host_loop(engine, p, c)
    assert log == reclaim and asks == [2] and stops == [HEAD_END, ASSIGNED]


# ---- 5. launch accounting, read-only, node sizes ---------------------------------------------------
def test_launches_and_read_only(engine, snaps):
    p, _, c = snaps(CASES[2])
    m = victimmodel.VictimModel(c)
    t = m.pending()[0]
    with engine.Session(p) as s, engine.Session(p) as twin:
        n_nodes = s.stats()["nodes"]
        old0 = [twin.walk_victims(t, b, mode) for b in (True, False) for mode in (1, 2, 3)]
        tables = ("pod_status", "job_ready", "pod_job", "pod_queue")
        raw = ("job_drf_alloc", "queue_allocated", "queue_deserved")
        s.walk_victims_from(t, True, 1)  # (builds the two tables, as the twin's first call did)
        rows = s.read_nodes(n_nodes)
        before = [s.head_victims(t, b, mode, 64, 8) for b in (True, False) for mode in (1, 2, 3)]
        tab0 = [s.table(n).copy() for n in tables] + [s.table_raw(n, np.float64).copy() for n in raw]
        sweeps = s.stats()["sweeps"]
        acted, k = 0, 0
        for b in (True, False):
            for mode in (1, 2, 3):
                for after in (None, (0, 0), (n_nodes - 1, 0)):
                    got = s.walk_victims_from(t, b, mode, 64, after)
                    acted += got[3]["acted"]
                    k += 1
                    # kbhip_walk_victims' launches on the twin, and the pre-pass
                    ref = twin.walk_victims(t, b, mode)
                    assert got[3]["launches"] == ref[3]["launches"] + 1, (b, mode, after)
        assert acted and s.stats()["sweeps"] == sweeps + k
        after_ = [s.head_victims(t, b, mode, 64, 8) for b in (True, False) for mode in (1, 2, 3)]
        for x, y in zip(before, after_):
            assert x[0] == y[0] and all(np.array_equal(a, b) for a, b in zip(x[1:7], y[1:7]))
        tab1 = [s.table(n) for n in tables] + [s.table_raw(n, np.float64) for n in raw]
        assert all(np.array_equal(a, b) for a, b in zip(tab0, tab1))
        assert np.array_equal(s.read_nodes(n_nodes), rows)
        a, b = s.walk_visits(), twin.walk_visits()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # the existing call on the same session, after the new one ran: its old launch count and outputs
        old1 = [s.walk_victims(t, b, mode) for b in (True, False) for mode in (1, 2, 3)]
        for x, y in zip(old0, old1):
            assert walkvictims.as_ops(x) == walkvictims.as_ops(y)
            keys = [k for k in x[3] if k not in ("rebuilt", "state_rebuilt", "launches")]
            assert {k: x[3][k] for k in keys} == {k: y[3][k] for k in keys}
        assert [y[3]["launches"] for y in old1] == [twin.walk_victims(t, b, mode)[3]["launches"]
                                                    for b in (True, False) for mode in (1, 2, 3)]


@pytest.mark.parametrize("tiers", [None, [["conformance"], ["gang", "drf", "proportion"]]], ids=["default", "two_tiers"])
def test_node_sizes(engine, kbgen_mod, tmp_path, tiers):
    """test_gpu_walk_victims' SIZES layout (0 .. 257 tasks per node: the lane chunks, the LDS rows and the
    spill row in the pre-pass and in the walk), whole and cut into windows of 3 entries."""
    c = _packed(kbgen_mod, tiers)
    m = victimmodel.VictimModel(c)
    p = c.write(str(tmp_path / "p.kbs"))
    acted = 0
    for t in m.pending():
        for mode in (1, 2, 3):
            for by_score in (True, False):
                whole, _ = _run(engine, p, m, t, mode, by_score)
                cut, _ = _run(engine, p, m, t, mode, by_score, cap=3)
                assert [op for ops, _ in whole for op in ops] == [op for ops, _ in cut for op in ops]
                acted += sum(i["acted"] for _, i in whole)
    assert acted


# ---- 6. errors and staleness ------------------------------------------------------------------------
def test_errors(engine, kbgen_mod, tmp_path):
    c = _jobs(kbgen_mod)
    p = c.write(str(tmp_path / "e.kbs"))
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    with engine.Session(p) as s:
        n_nodes = s.stats()["nodes"]
        for kw in (dict(victims=0), dict(victims=4), dict(cap=0), dict(cap=65), dict(cap_ops=0), dict(by_score=2),
                   dict(after=(-2, 0)), dict(after=(n_nodes, 0))):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.walk_victims_from(t_one, **kw)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_victims_from(0, True, 1)  # a Running pod: no task class
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_victims_from(len(c.pods), True, 1)
        t = s.place_job_submit([t_wide], 0, 1, 0)
        with pytest.raises(engine.KbhipError, match=EINVAL):  # a ticket is outstanding
            s.walk_victims_from(t_one, True, 1)
        assert s.place_job_cancel(t) == 1
        first = s.walk_victims_from(t_one, True, 1)[3]
        assert first["remaining"] > 0
        # a resume point past every node of the walk: nothing behind it
        last = s.walk_victims_from(t_one, False, 1, 64, (n_nodes - 1, 0))
        assert len(last[0]) == 0 and last[3]["stop"] == EXHAUSTED and last[3]["remaining"] == 0
        assert (last[3]["resume_node"], last[3]["visited"], last[3]["first_valid"]) == (n_nodes - 1, 0, -1)
        # a refused call on a device session writes nothing
        outs = [np.full(4, 77, np.uint8), np.full(4, 77, np.int32), np.full(4, 77, np.int32), np.full(10, 77, np.int64)]
        ptr = [a.ctypes.data for a in outs]
        L = engine.lib()
        for args, cap_ops in (((t_one, 1, 1, 65, -1, 0), 4), ((t_one, 1, 0, 4, -1, 0), 4), ((t_one, 1, 1, 4, -1, 0), 0),
                              ((0, 1, 1, 4, -1, 0), 4), ((t_one, 2, 1, 4, -1, 0), 4), ((t_one, 1, 1, 4, n_nodes, 0), 4)):
            assert L.kbhip_walk_victims_from(s._h, *args, *ptr[:3], cap_ops, ptr[3]) == -1
        assert all((a == 77).all() for a in outs)
    sh = engine.ShardedSession(p, 0, 0, 2)
    try:
        with pytest.raises(engine.KbhipError, match=EUNSUP):
            sh.walk_victims_from(t_one, True, 1)
        outs = [np.full(4, 77, np.uint8), np.full(4, 77, np.int32), np.full(4, 77, np.int32), np.full(10, 77, np.int64)]
        ptr = [a.ctypes.data for a in outs]
        assert engine.lib().kbhip_walk_victims_from(sh._h, t_one, 1, 1, 4, -1, 0, *ptr[:3], 4, ptr[3]) == -3
        assert all((a == 77).all() for a in outs)
    finally:
        sh.close()
