"""kbhip_walk_victims on the device: one task's whole eviction walk over the
head of its pruned walk, the evictions of each node carried to the next.

The yardstick is the restatement's chain (tests/walkvictims.py over
tests/victimmodel.py) along the head kbhip_head_victims returns on the same
session, the oracle's reclaim records for the host loop, and the hand answers
of tests/walkedges.py."""
import functools

import numpy as np
import pytest

import victimmodel
import walkedges
import walkvictims
from test_gpu_victim_walk import CASES, EXACT, GI, _gen, _jobs
from walkvictims import ASSIGNED, CAPACITY, EXHAUSTED, HEAD_END

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"
KEYS = ("stop", "total", "visited", "acted", "last_node", "last_score")


def _expect(s, m, task, by_score, mode, cap, **kw):
    """The chain over the first `cap` nodes of the head kbhip_head_victims gives: (ops, info, head call's info)."""
    total, nodes, scores, _, _, _, _, hinfo = s.head_victims(task, by_score, mode, 64, 1)
    k = min(cap, total, 64)
    ops, info = walkvictims.chain(m, task, mode, nodes[:k], **kw)
    if info["stop"] == EXHAUSTED and total > k:
        info["stop"] = HEAD_END
    at = nodes[:k].tolist().index(info["last_node"]) if info["last_node"] >= 0 else -1
    info.update(total=total, last_score=int(scores[at]) if at >= 0 and by_score else 0)
    return ops, info, hinfo


def _check(s, m, task, modes=(1, 2, 3), caps=(1, 64), orders=(True, False)):
    """Every (order, mode, cap): ops and info are the chain's.  Returns the infos and the walks that acted on
    more than one node."""
    infos, multi = [], 0
    for by_score in orders:
        for mode in modes:
            for cap in caps:
                got = s.walk_victims(task, by_score, mode, cap)
                ops, info, hinfo = _expect(s, m, task, by_score, mode, cap)
                where = (task, by_score, mode, cap)
                assert walkvictims.as_ops(got) == ops, where
                assert {k: got[3][k] for k in KEYS} == {k: info[k] for k in KEYS}, where
                # the head's launches, then one (whichever call comes first after a kbhip_apply_ops patches)
                assert got[3]["launches"] - bool(got[3]["patched"]) == hinfo["launches"] - bool(hinfo["patched"]), where
                infos.append(got[3])
                multi += info["acted"] > 1
    return infos, multi


def _apply(engine, s, m, rec):
    E, P = engine.OP_EVICT, engine.OP_PIPELINE
    assert s.apply_ops([E if k == 128 else P for _, _, k in rec], [q for q, _, _ in rec], [n for _, n, _ in rec]) <= 2
    m.records(rec)


def _send(engine, s, ops):
    assert (engine.OP_EVICT, engine.OP_PIPELINE) == (walkvictims.EVICT, walkvictims.PIPELINE)
    assert s.apply_ops([o for o, _, _ in ops], [p for _, p, _ in ops], [n for _, _, n in ops]) <= 2


@pytest.fixture(scope="module")
def snaps(oracle_mod, kbgen_mod, tmp_path_factory):
    """case -> (path, the oracle's reclaim records, its preempt records, the cluster): computed once."""
    d = tmp_path_factory.mktemp("walk_victims")

    @functools.lru_cache(maxsize=None)
    def get(case):
        c = _gen(kbgen_mod, case)
        p = c.write(str(d / ("c%d_%d_%d_%d.kbs" % case)))
        return (p, oracle_mod.ref_allocate(p, actions="reclaim").as_list(),
                oracle_mod.ref_allocate(p, actions="preempt").as_list(), c)

    return get


# ---- 1. parity ---------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_parity(engine, snaps, case):
    p, reclaim, preempt, c = snaps(case)
    with engine.Session(p) as s:
        m = victimmodel.VictimModel(c)
        todo = m.pending()
        assert todo
        first = s.walk_victims(todo[0], True, 1)[3]
        assert (first["rebuilt"], first["state_rebuilt"], first["patched"]) == (1, 1, 0)
        for t in todo:
            infos, _ = _check(s, m, t)
            assert not any(i["rebuilt"] or i["state_rebuilt"] or i["patched"] for i in infos)
        if reclaim:
            _apply(engine, s, m, reclaim)
            left = m.pending()
            if left:  # patched, not rebuilt: the first call uploads the dirty records
                i0 = s.walk_victims(left[0], False, 1)[3]
                assert i0["patched"] > 0 and not i0["rebuilt"] and not i0["state_rebuilt"]
            for t in left:
                infos, _ = _check(s, m, t)
                assert not any(i["rebuilt"] or i["state_rebuilt"] or i["patched"] for i in infos)
    if preempt:
        with engine.Session(p) as s:
            m = victimmodel.VictimModel(c)
            assert s.walk_victims(m.pending()[0], True, 2)[3]["state_rebuilt"] == 1
            _apply(engine, s, m, preempt)
            for t in m.pending():
                infos, _ = _check(s, m, t, modes=(2, 3))
                assert not any(i["state_rebuilt"] for i in infos)


# ---- 2. the host loop end to end ----------------------------------------------
def test_host_reclaim_walk_equals_the_oracle(engine, snaps):
    """reclaim.go:41-196 restated on gohost's ordering (walkvictims.host_reclaim_walk), fed only by
    kbhip_walk_victims and kbhip_apply_ops: the oracle's record log on the four EXACT snapshots, with one
    ranking call per popped task (no walk of them leaves the head or meets a capacity:
    tests/test_walk_victims_abi.py checks that with the restatement alone)."""
    for case in EXACT:
        p, reclaim, _, c = snaps(case)
        m = victimmodel.VictimModel(c)
        with engine.Session(p) as s:
            def ask(task, after):
                got = s.walk_victims(task, False, 1, 64, after)
                return walkvictims.as_ops(got), got[3]

            log, asks, stops = walkvictims.host_reclaim_walk(m, ask, lambda ops: _send(engine, s, ops))
            assert log == [tuple(r) for r in reclaim], case
            assert sum(k == 8 for _, _, k in log) >= 2
            assert asks and set(asks) == {1} and set(stops) <= {ASSIGNED, EXHAUSTED}, case


# ---- 3. the carried-state edges -------------------------------------------------
@pytest.mark.parametrize("name", sorted(walkedges.BUILDERS))
def test_edges(engine, tmp_path, name):
    c, task, mode, carried, stateless = walkedges.BUILDERS[name]()
    task, (carried, stateless) = walkedges.resolve(c, task, [carried, stateless])
    m = victimmodel.VictimModel(c)
    with engine.Session(c.write(str(tmp_path / "e.kbs"))) as s:
        got = s.walk_victims(task, False, mode)  # index order: the hand answer
        assert walkvictims.as_ops(got) == carried != stateless
        assert got[3]["stop"] == EXHAUSTED
        infos, _ = _check(s, m, task, modes=(mode,), caps=(64,))  # both orders against the chain
        assert all(i["acted"] for i in infos)
        s.set_option("walk_overlay_max", 1)  # one job and one queue: what each of these walks touches
        assert walkvictims.as_ops(s.walk_victims(task, False, mode)) == carried


# ---- 4. capacity and resume -----------------------------------------------------
def _resumed(engine, s, m, task, by_score, mode, cap_ops):
    """The walk in as many calls as its CAPACITY stops ask for, each batch applied before the next call."""
    log, after, calls = [], None, 0
    while True:
        got = s.walk_victims(task, by_score, mode, 64, after, cap_ops)
        ops, info = walkvictims.as_ops(got), got[3]
        calls += 1
        assert len(ops) <= cap_ops
        log += ops
        if ops:
            _send(engine, s, ops)
        if info["stop"] != CAPACITY:
            return log, info["stop"], calls
        assert info["acted"] > 0  # (cap_ops holds the largest step: every call moves on)
        after = (info["last_node"], info["last_score"])


@pytest.mark.parametrize("case", [c for c in CASES if not c[0]][:6], ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_capacity_and_resume(engine, snaps, case):
    p, _, _, c = snaps(case)
    m = victimmodel.VictimModel(c)
    resumed = 0
    for mode, by_score in ((1, False), (2, True)):
        for task in m.pending():
            with engine.Session(p) as s:
                full = s.walk_victims(task, by_score, mode)
            ops = walkvictims.as_ops(full)
            if full[3]["acted"] < 2:
                continue
            steps = [sum(1 for o in ops if o[2] == n) for n in dict.fromkeys(o[2] for o in ops)]
            for opt, cap_ops in ((0, max(steps) + 1), (1, 4096)):
                with engine.Session(p) as s:
                    s.set_option("walk_overlay_max", opt)
                    # the capped call is the chain with the same bounds, a prefix of the uncapped answer
                    first = s.walk_victims(task, by_score, mode, 64, None, cap_ops)
                    exp, info, _ = _expect(s, m, task, by_score, mode, 64, cap_ops=cap_ops, ov_max=opt)
                    assert walkvictims.as_ops(first) == exp == ops[:len(exp)]
                    assert first[3]["stop"] == info["stop"]
                    log, stop, calls = _resumed(engine, s, m, task, by_score, mode, cap_ops)
                    assert (log, stop) == (ops, full[3]["stop"]), (task, mode, opt)
                    resumed += calls > 1
    assert resumed or case != CASES[0]  # (the first snapshot has walks of several nodes)


# ---- 5. node sizes ----------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 256, 257)  # tasks per node: the lane chunks, the LDS rows (256) and the spill row


def _packed(kbgen, tiers, sizes=SIZES):
    """test_gpu_head_victims' layout: one node per size, its tasks alternating between queue q1 (job "far",
    every fourth of job "gang3" with MinAvailable 3) and the pending tasks' own queue q0 (job "mate", every
    sixth of the pending job "pend" itself); every seventh pod critical, every fifth larger."""
    c = kbgen.Cluster(tiers=tiers)
    c.add_queue("q0", 1)
    c.add_queue("q1", 3)
    for i, _ in enumerate(sizes):
        c.add_node("n%02d" % i, 64000, 256 * GI, 16000, 400)
    for job, q, mm in (("far", "q1", 1), ("gang3", "q1", 3), ("mate", "q0", 2), ("pend", "q0", 1)):
        c.add_job("ns", job, q, min_member=mm, ts=1 if job == "pend" else 0)
    k = 0
    for i, size in enumerate(sizes):
        for j in range(size):
            if j % 2 == 0:
                job = "gang3" if j % 8 == 0 else "far"
            else:
                job = "pend" if j % 6 == 1 else "mate"
            c.add_pod("ns", "r%05d" % k, uid="a%05d" % k, group=job, node="n%02d" % i, phase="Running",
                      priority_class="system-node-critical" if k % 7 == 3 else "",
                      containers=[kbgen.res(cpu=20 + (k % 5 == 0) * 300, mem=GI // 64, gpu=10 * (k % 3 == 0))])
            k += 1
    c.add_pod("ns", "pend-small", uid="p0", group="pend", priority=5, ts=1, containers=[kbgen.res(cpu=500, mem=GI)])
    # more than the nodes before the largest hold: the walk evicts on them and carries that into the large ones
    c.add_pod("ns", "pend-wide", uid="p1", group="pend", priority=5, ts=1,
              containers=[kbgen.res(cpu=30000, mem=2 * GI, gpu=2000)])
    return c


@pytest.mark.parametrize("tiers", [None, [["priority", "gang", "drf", "predicates", "proportion", "nodeorder"]],
                                   [["conformance"], ["gang", "drf", "proportion"]]],
                         ids=["default", "one_tier", "two_tiers"])
def test_node_sizes(engine, kbgen_mod, tmp_path, tiers):
    c = _packed(kbgen_mod, tiers)
    m = victimmodel.VictimModel(c)
    tasks = m.pending()
    assert len(tasks) == 2
    with engine.Session(c.write(str(tmp_path / "p.kbs"))) as s:
        multi = sum(_check(s, m, t, caps=(64,))[1] for t in tasks)
        assert multi  # evictions carried across the LDS rows and the spill row
        # evictions in the middle of the large nodes, patched not rebuilt
        mid = [q for q in range(len(m.node)) if m.status(q) == victimmodel.RUNNING and q % 9 == 4]
        s.apply_ops([engine.OP_EVICT] * len(mid), mid)
        for q in mid:
            m.evict(q)
        infos, _ = _check(s, m, tasks[1], caps=(64,), orders=(False,))
        assert infos[0]["patched"] > 0 and not any(i["state_rebuilt"] for i in infos)


# ---- 6. head lengths ---------------------------------------------------------------
def _long(kbgen, n_nodes):
    """n_nodes equal nodes with one small Running pod of queue q1 each; the Pending task of q0 asks for far
    more than any of them: gang and conformance admit every pod, every node is valid, none covers."""
    c = kbgen.Cluster(tiers=[["gang", "conformance"]])
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    for i in range(n_nodes):
        c.add_node("n%05d" % i, 8000, 16 * GI, 0, 110)
    c.add_job("ns", "run", "q1", min_member=1)
    for i in range(n_nodes):
        c.add_pod("ns", "run-%05d" % i, uid="a%05d" % i, group="run", node="n%05d" % i, phase="Running",
                  containers=[kbgen.res(cpu=500 + (i % 5) * 100, mem=GI)])
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    c.add_pod("ns", "pend-0", uid="p00000", group="pend", priority=5, ts=1, containers=[kbgen.res(cpu=6000, mem=8 * GI)])
    return c


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65])
def test_head_lengths(engine, kbgen_mod, tmp_path, n_nodes):
    c = _long(kbgen_mod, n_nodes)
    m = victimmodel.VictimModel(c)
    task = m.pending()[0]
    with engine.Session(c.write(str(tmp_path / "u.kbs"))) as s:
        _check(s, m, task, modes=(1,), caps=(1, 63, 64))
        for by_score in (True, False):
            ops, pods, nodes, info = s.walk_victims(task, by_score, 1)
            assert info["total"] == n_nodes and info["visited"] == info["acted"] == len(ops) == min(n_nodes, 64)
            assert info["stop"] == (HEAD_END if n_nodes > 64 else EXHAUSTED)
            assert (ops == engine.OP_EVICT).all() and len(set(nodes.tolist())) == len(ops)
        if n_nodes == 65:  # the resume point is inside the new head: the last node, then EXHAUSTED
            ops, pods, nodes, info = s.walk_victims(task, False, 1)
            _send(engine, s, walkvictims.as_ops((ops, pods, nodes)))
            more = s.walk_victims(task, False, 1, 64, (info["last_node"], info["last_score"]))
            assert walkvictims.as_ops(more) == [(engine.OP_EVICT, 64, 64)]
            assert more[3]["stop"] == EXHAUSTED and more[3]["visited"] == 1 and more[3]["total"] == 1


# ---- 7. read-only --------------------------------------------------------------------
def test_read_only(engine, snaps):
    p, _, _, c = snaps(CASES[2])
    with engine.Session(p) as s, engine.Session(p) as twin:
        n_nodes = s.stats()["nodes"]
        m = victimmodel.VictimModel(c)
        t = m.pending()[0]
        rows = s.read_nodes(n_nodes)
        tables = ("pod_status", "job_ready", "pod_job", "pod_queue")
        raw = ("job_drf_alloc", "queue_allocated", "queue_deserved")
        before = [s.head_victims(t, b, mode, 64, 8) for b in (True, False) for mode in (1, 2, 3)]
        tab0 = [s.table(n).copy() for n in tables] + [s.table_raw(n, np.float64).copy() for n in raw]
        acted = 0
        for b in (True, False):
            for mode in (1, 2, 3):
                acted += s.walk_victims(t, b, mode)[3]["acted"]
        assert acted
        after = [s.head_victims(t, b, mode, 64, 8) for b in (True, False) for mode in (1, 2, 3)]
        for x, y in zip(before, after):
            assert x[0] == y[0] and all(np.array_equal(a, b) for a, b in zip(x[1:7], y[1:7]))
        tab1 = [s.table(n) for n in tables] + [s.table_raw(n, np.float64) for n in raw]
        assert all(np.array_equal(a, b) for a, b in zip(tab0, tab1))
        assert np.array_equal(s.read_nodes(n_nodes), rows)
        a, b = s.walk_visits(), twin.walk_visits()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # an allocate leaves walk counters and a FitDelta answer: neither moves under the call
        s.allocate()
        left = [q for q in m.pending() if s.table("pod_status")[q] == 1]
        size = lambda: int(engine.lib().kbhip_walk_visits(s._h, None, None, 0))  # (a full read clears the counters)
        v0 = size()
        assert left and v0 >= 0
        try:
            d0 = s.fit_deltas(left[0])
        except engine.KbhipError:
            d0 = None
        s.walk_victims(left[0], True, 1)
        assert size() == v0
        if d0 is not None:
            assert all(np.array_equal(x, y) for x, y in zip(d0, s.fit_deltas(left[0])))


# ---- 8. errors ---------------------------------------------------------------------------
def test_errors(engine, kbgen_mod, tmp_path):
    c = _jobs(kbgen_mod)
    p = c.write(str(tmp_path / "e.kbs"))
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    with engine.Session(p) as s:
        n_nodes = s.stats()["nodes"]
        for kw in (dict(victims=0), dict(victims=4), dict(cap=0), dict(cap=65), dict(cap_ops=0), dict(by_score=2),
                   dict(after=(-2, 0)), dict(after=(n_nodes, 0))):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.walk_victims(t_one, **kw)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_victims(0, True, 1)  # a Running pod: no task class
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_victims(len(c.pods), True, 1)
        t = s.place_job_submit([t_wide], 0, 1, 0)
        with pytest.raises(engine.KbhipError, match=EINVAL):  # a ticket is outstanding
            s.walk_victims(t_one, True, 1)
        assert s.place_job_cancel(t) == 1
        assert s.walk_victims(t_one, True, 1)[3]["total"] > 0
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.set_option("walk_overlay_max", 257)
        # a refused call on a device session writes nothing
        outs = [np.full(4, 77, np.uint8), np.full(4, 77, np.int32), np.full(4, 77, np.int32), np.full(8, 77, np.int64)]
        ptr = [a.ctypes.data for a in outs]
        L = engine.lib()
        for args, cap_ops in (((t_one, 1, 1, 65, -1, 0), 4), ((t_one, 1, 0, 4, -1, 0), 4), ((t_one, 1, 1, 4, -1, 0), 0),
                              ((0, 1, 1, 4, -1, 0), 4), ((t_one, 2, 1, 4, -1, 0), 4), ((t_one, 1, 1, 4, n_nodes, 0), 4)):
            assert L.kbhip_walk_victims(s._h, *args, *ptr[:3], cap_ops, ptr[3]) == -1
        assert all((a == 77).all() for a in outs)
    sh = engine.ShardedSession(p, 0, 0, 2)
    try:
        with pytest.raises(engine.KbhipError, match=EUNSUP):
            sh.walk_victims(t_one, True, 1)
    finally:
        sh.close()
