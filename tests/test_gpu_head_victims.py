"""kbhip_head_victims on the device: the head of kbhip_rank_victim_nodes' walk
with, per head node, the victims ssn.Reclaimable / ssn.Preemptable give,
validateVictims and the evicted prefix.

The yardstick is tests/victimmodel.py (the reference's plugin sources restated
over the kbgen.Cluster) following the operations the test applied, and the
oracle's reclaim / preempt records; the head itself is the one
kbhip_rank_victim_nodes returns on the same session."""
import functools

import numpy as np
import pytest

import victimedges
import victimmodel
from test_gpu_victim_walk import CASES, EXACT, GI, _gen, _jobs, _uniform

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"
TIER_ALL = [["priority", "gang", "drf", "predicates", "proportion", "nodeorder"]]


def _check(s, m, task, modes=(1, 2, 3), caps=(1, 64), stride=8, orders=(True, False)):
    """Every (order, mode, cap): the head is rank_victim_nodes', the rows are the model's.  Returns the
    infos and how many rows had victims."""
    infos, nonempty = [], 0
    for by_score in orders:
        for mode in modes:
            for cap in caps:
                total, nodes, scores, _, _ = s.rank_victim_nodes(task, by_score, mode, 0, cap)
                got = s.head_victims(task, by_score, mode, cap, stride)
                n, g_node, g_score, count, evict, flags, rows, info = got
                k = min(cap, total)
                assert n == total and np.array_equal(g_node[:k], nodes) and np.array_equal(g_score[:k], scores)
                assert (g_node[k:] == -1).all() and not g_score[k:].any() and not count[k:].any()
                assert not evict[k:].any() and not flags[k:].any() and (rows[k:] == -1).all()
                top = 0
                for i in range(k):
                    exp_v, exp_e, exp_f = m.decide(task, mode, int(nodes[i]))
                    where = (task, by_score, mode, cap, i, int(nodes[i]))
                    assert int(count[i]) == len(exp_v), where
                    assert rows[i].tolist() == (exp_v + [-1] * stride)[:stride], where
                    assert (int(evict[i]), int(flags[i])) == (exp_e, exp_f), where
                    top = max(top, len(exp_v))
                    nonempty += bool(exp_v)
                assert info["max_count"] == top
                infos.append(info)
    return infos, nonempty


def _apply(engine, s, m, rec):
    E, P = engine.OP_EVICT, engine.OP_PIPELINE
    assert s.apply_ops([E if k == 128 else P for _, _, k in rec], [q for q, _, _ in rec], [n for _, n, _ in rec]) <= 2
    m.records(rec)


@pytest.fixture(scope="module")
def snaps(oracle_mod, kbgen_mod, tmp_path_factory):
    """case -> (path, the oracle's reclaim records, its preempt records, the cluster): computed once."""
    d = tmp_path_factory.mktemp("head_victims")

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
        first = True
        for t in todo:
            infos, _ = _check(s, m, t)
            assert [i["state_rebuilt"] for i in infos] == [1 if first else 0] + [0] * (len(infos) - 1)
            assert all(i["patched"] == 0 for i in infos)
            first = False
        if reclaim:
            _apply(engine, s, m, reclaim)
            first = True
            for t in m.pending():
                infos, _ = _check(s, m, t)
                assert not any(i["state_rebuilt"] for i in infos)
                assert (infos[0]["patched"] > 0) == first and not any(i["patched"] for i in infos[1:])
                first = False
    if preempt:
        with engine.Session(p) as s:
            m = victimmodel.VictimModel(c)
            t0 = m.pending()[0]
            assert s.head_victims(t0, True, 2)[7]["state_rebuilt"] == 1
            _apply(engine, s, m, preempt)
            first = True
            for t in m.pending():
                infos, _ = _check(s, m, t, modes=(2, 3))
                assert not any(i["state_rebuilt"] for i in infos)
                assert (infos[0]["patched"] > 0) == first
                first = False


# ---- 2. boundary shapes ------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 129, 200, 256, 257)  # tasks per node: the 64-lane chunks, the LDS rows (256) and past them


def _packed(kbgen, tiers, sizes=SIZES):
    """One node per size in SIZES.  Its tasks alternate between queue q1 (job "far", and every fourth of job
    "gang3" with MinAvailable 3) and the pending tasks' own queue q0 (job "mate", every sixth of the
    pending job "pend" itself), so every mode has candidates between non-candidates and one job spans many
    candidates of a node; every seventh pod is critical, every fifth larger than the rest."""
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
    c.add_pod("ns", "pend-wide", uid="p1", group="pend", priority=5, ts=1,
              containers=[kbgen.res(cpu=2500, mem=2 * GI, gpu=200)])
    return c


@pytest.mark.parametrize("tiers", [None, TIER_ALL, [["conformance"], ["gang", "drf", "proportion"]]],
                         ids=["default", "one_tier", "two_tiers"])
def test_node_sizes(engine, kbgen_mod, tmp_path, tiers):
    c = _packed(kbgen_mod, tiers)
    p = c.write(str(tmp_path / "p.kbs"))
    m = victimmodel.VictimModel(c)
    tasks = m.pending()
    assert len(tasks) == 2
    with engine.Session(p) as s:
        seen = truncated = 0
        for t in tasks:
            for stride in (1, 7, 300):
                _, nonempty = _check(s, m, t, caps=(64,), stride=stride, orders=(False,))
                seen += nonempty
            # the truncation is visible: rows of one entry, the largest count reported (_check compared both)
            for mode in (1, 2, 3):
                n, _, _, count, _, _, rows, info = s.head_victims(t, False, mode, 64, 1)
                assert rows.shape == (64, 1) and info["max_count"] == count.max()
                truncated += int(info["max_count"] > 1)
        assert truncated
        assert seen
        # evictions in the middle of the large nodes, patched not rebuilt: the running sums move
        mid = [q for q in range(len(m.node)) if m.status(q) == victimmodel.RUNNING and q % 9 == 4]
        s.apply_ops([engine.OP_EVICT] * len(mid), mid)
        for q in mid:
            m.evict(q)
        infos, _ = _check(s, m, tasks[1], caps=(64,), stride=300, orders=(True,))
        assert infos[0]["patched"] > 0 and not any(i["state_rebuilt"] for i in infos)



# ---- 2c. the host loop end to end ---------------------------------------------
def test_host_reclaim_loop_equals_the_oracle(engine, snaps):
    """reclaim.go:41-196 restated on gohost's ordering (victimmodel.host_reclaim): nodes, victims, prefix
    and the pipeline decision come only from kbhip_head_victims, every decision goes back through
    kbhip_apply_ops, and the record log is the oracle's on the four EXACT snapshots.  A walk of more than 64
    nodes would need kbhip_rank_victim_nodes windows: it happens on none of the four (at most one allowed)."""
    fallbacks = 0
    for case in EXACT:
        p, reclaim, _, c = snaps(case)
        m = victimmodel.VictimModel(c)
        long_walks = []
        with engine.Session(p) as s:
            def ask(task):
                n, nodes, _, count, evict, flags, rows, info = s.head_victims(task, False, 1, 64, 128)
                assert info["max_count"] <= 128
                if n > 64:
                    long_walks.append(task)
                return [(int(nodes[i]), rows[i][:int(count[i])].tolist(), int(evict[i]), int(flags[i]))
                        for i in range(min(n, 64))]

            def apply(ops):
                E, P = engine.OP_EVICT, engine.OP_PIPELINE
                assert s.apply_ops([E if k == 128 else P for k, _, _ in ops], [q for _, q, _ in ops],
                                   [n for _, _, n in ops]) <= 2

            log = victimmodel.host_reclaim(m, ask, apply)
            assert log == [tuple(r) for r in reclaim], case
            assert sum(k == 8 for _, _, k in log) >= 2
        fallbacks += bool(long_walks)
    assert fallbacks <= 1 and fallbacks == 0  # (no walk of these snapshots is longer than 64 nodes)


# ---- 2b. the comparison edges --------------------------------------------------
@pytest.mark.parametrize("name", sorted(victimedges.BUILDERS))
def test_edges(engine, tmp_path, name):
    """The hand-placed clusters of tests/victimedges.py: the rows of the head equal the hand calculation
    (and the restatement everywhere), in both orders."""
    c, exp = victimedges.BUILDERS[name]()
    exp = victimedges.resolve(c, exp)
    m = victimmodel.VictimModel(c)
    with engine.Session(c.write(str(tmp_path / "e.kbs"))) as s:
        hit = set()
        for task in sorted({t for t, _, _ in exp}):
            for mode in sorted({md for t, _, md in exp if t == task}):
                _check(s, m, task, modes=(mode,), caps=(64,), stride=4)
                for by_score in (True, False):
                    n, nodes, _, count, evict, flags, rows, _ = s.head_victims(task, by_score, mode, 64, 4)
                    for i in range(min(n, 64)):
                        e = exp.get((task, int(nodes[i]), mode))
                        if e is None:
                            continue
                        assert (rows[i][:int(count[i])].tolist(), int(evict[i]), int(flags[i])) == e, (task, nodes[i])
                        hit.add((task, int(nodes[i]), mode))
        # every hand-placed node with a candidate sum that keeps it in the walk was seen on the device
        assert {k for k, e in exp.items() if e is not None and e[0]} <= hit


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65])
def test_head_lengths(engine, kbgen_mod, tmp_path, n_nodes):
    c = _uniform(kbgen_mod, n_nodes, "all")
    p = c.write(str(tmp_path / "u.kbs"))
    m = victimmodel.VictimModel(c)
    task = m.pending()[0]
    with engine.Session(p) as s:
        _, nonempty = _check(s, m, task, modes=(1,), caps=(1, 63, 64))
        assert nonempty
        assert s.head_victims(task, True, 1, 64)[0] == n_nodes


# ---- 3. staleness --------------------------------------------------------------
def _records(log):
    return [(int(p), int(n), {1: 4, 2: 8, 3: 128}[int(k)]) for p, n, k in zip(*log)]


@pytest.mark.parametrize("case", [CASES[0], CASES[9]], ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_rebuilt_after_everything_but_apply_ops(engine, snaps, case):
    p, reclaim, _, c = snaps(case)
    with engine.Session(p) as s:
        m = victimmodel.VictimModel(c)
        t = m.pending()[0]
        assert s.head_victims(t, True, 1)[7]["state_rebuilt"] == 1
        assert s.head_victims(t, True, 1)[7]["state_rebuilt"] == 0
        half = reclaim[: max(1, len(reclaim) // 2)]
        _apply(engine, s, m, half)
        for t in m.pending():
            infos, _ = _check(s, m, t)
            assert not any(i["state_rebuilt"] for i in infos)  # kbhip_apply_ops alone never forces a rebuild
        for step in ("reclaim", "allocate"):
            m.records(_records(getattr(s, step)()))
            todo = m.pending()
            for i, t in enumerate(todo):
                infos, _ = _check(s, m, t)
                assert [x["state_rebuilt"] for x in infos][:2] == [1 if i == 0 else 0, 0], step
        # preempt's discarded statements leave no record for the restatement to follow (an unevicted pod's
        # node copy stays Releasing), backfill binds BestEffort tasks: the rebuild alone is checked
        asked = 0
        for step in ("preempt", "backfill"):
            getattr(s, step)()
            st = s.table("pod_status")
            left = [t for t in m.pending() if st[t] == 1]
            if left:
                assert s.head_victims(left[0], True, 2)[7]["state_rebuilt"] == 1, step
                asked += 1
        assert asked  # (a Pending task is left to ask for after at least one of the two)


def test_rebuilt_after_place_job_first_fit_and_carries(engine, kbgen_mod, tmp_path):
    c = _jobs(kbgen_mod)
    p = c.write(str(tmp_path / "f.kbs"))
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    with engine.Session(p) as s:
        m = victimmodel.VictimModel(c)
        assert _check(s, m, t_one)[0][0]["state_rebuilt"] == 1
        nodes, kinds, _ = s.place_job([t_wide], 0, 1, 0)[:3]
        m.records([(t_wide, int(nodes[0]), 4 if int(kinds[0]) == 1 else 8)])
        assert _check(s, m, t_one)[0][0]["state_rebuilt"] == 1
        s.carry()
        m = victimmodel.VictimModel(c)  # nothing was bound or evicted: the carried session is the opened one
        assert _check(s, m, t_one)[0][0]["state_rebuilt"] == 1
        assert s.first_fit([t_wide])[0] >= 0
        assert s.head_victims(t_one, True, 1)[7]["state_rebuilt"] == 1
        s.carry()
        assert s.head_victims(t_one, True, 1)[7]["state_rebuilt"] == 1
        ticket = s.place_job_submit([t_wide], 0, 1, 0)  # the asynchronous form
        s.place_job_wait(ticket)
        assert s.head_victims(t_one, True, 1)[7]["state_rebuilt"] == 1
        s.carry_events([0], [engine.EV_SUCCEEDED])
        assert s.head_victims(t_one, True, 1)[7]["state_rebuilt"] == 1
        # the dirty bound: more pods waiting than the host allows is a rebuild
        s.set_option("victims_dirty_max", 1)
        run = [q for q in range(1, len(c.pods)) if m.status(q) == victimmodel.RUNNING][:3]
        s.apply_ops([engine.OP_EVICT] * 3, run)
        assert s.head_victims(t_one, True, 1)[7]["state_rebuilt"] == 1


# ---- 4. read-only --------------------------------------------------------------
def test_read_only(engine, snaps):
    p, reclaim, _, c = snaps(CASES[2])
    with engine.Session(p) as s, engine.Session(p) as twin:
        n_nodes = s.stats()["nodes"]
        m = victimmodel.VictimModel(c)
        t = m.pending()[0]
        rows = s.read_nodes(n_nodes)
        before = [s.rank_victim_nodes(t, b, mode, 0, 64) for b in (True, False) for mode in (1, 2, 3)]
        for b in (True, False):
            for mode in (1, 2, 3):
                s.head_victims(t, b, mode, 64, 4)
        after = [s.rank_victim_nodes(t, b, mode, 0, 64) for b in (True, False) for mode in (1, 2, 3)]
        for x, y in zip(before, after):
            assert x[0] == y[0] and all(np.array_equal(a, b) for a, b in zip(x[1:4], y[1:4]))
        assert np.array_equal(s.read_nodes(n_nodes), rows)
        a, b = s.walk_visits(), twin.walk_visits()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # with the state live and never built: the rankings and kbhip_apply_ops agree
        part = reclaim[: max(1, len(reclaim) // 2)]
        E, P = engine.OP_EVICT, engine.OP_PIPELINE
        args = ([E if k == 128 else P for _, _, k in part], [q for q, _, _ in part], [n for _, n, _ in part])
        if part:
            assert s.apply_ops(*args) == twin.apply_ops(*args)
        assert np.array_equal(s.table("pod_status"), twin.table("pod_status"))
        assert np.array_equal(s.read_nodes(n_nodes), twin.read_nodes(n_nodes))
        for mode in (1, 2, 3):
            for live, cold in ((s.rank_victim_nodes(t, True, mode, 0, 64), twin.rank_victim_nodes(t, True, mode, 0, 64)),
                               (s.rank_nodes(t, True, 0, 64), twin.rank_nodes(t, True, 0, 64))):
                assert live[0] == cold[0] and all(np.array_equal(x, y) for x, y in zip(live[1:3], cold[1:3]))
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
        s.head_victims(left[0], True, 1, 64, 4)
        assert size() == v0
        if d0 is not None:
            d1 = s.fit_deltas(left[0])
            assert all(np.array_equal(x, y) for x, y in zip(d0, d1))
        twin.allocate()
        a, b = s.walk_visits(), twin.walk_visits()
        assert len(a[0]) == v0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 5. errors -----------------------------------------------------------------
def test_errors(engine, kbgen_mod, tmp_path):
    c = _jobs(kbgen_mod)
    p = c.write(str(tmp_path / "e.kbs"))
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    with engine.Session(p) as s:
        for kw in (dict(victims=0), dict(victims=4), dict(cap=0), dict(cap=65), dict(stride=0), dict(by_score=2)):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.head_victims(t_one, **kw)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.head_victims(0, True, 1)  # a Running pod: no task class
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.head_victims(len(c.pods), True, 1)
        t = s.place_job_submit([t_wide], 0, 1, 0)
        with pytest.raises(engine.KbhipError, match=EINVAL):  # a ticket is outstanding
            s.head_victims(t_one, True, 1)
        assert s.place_job_cancel(t) == 1
        assert s.head_victims(t_one, True, 1)[0] > 0  # (a cancelled asynchronous pop left the state stale or not: either is answered)
        # a refused call on a device session writes nothing
        outs = [np.full(4, 77, np.int32) for _ in range(4)] + [np.full(4, 77, np.uint8), np.full(12, 77, np.int32),
                                                                np.full(5, 77, np.int64)]
        ptr = [a.ctypes.data for a in outs]
        L = engine.lib()
        for args in ((t_one, 1, 1, 65, 3), (t_one, 1, 0, 4, 3), (t_one, 1, 1, 4, 0), (0, 1, 1, 4, 3), (t_one, 2, 1, 4, 3)):
            assert L.kbhip_head_victims(s._h, *args, *ptr) == -1
        assert all((a == 77).all() for a in outs)
    sh = engine.ShardedSession(p, 0, 0, 2)
    try:
        with pytest.raises(engine.KbhipError, match=EUNSUP):
            sh.head_victims(t_one, True, 1)
    finally:
        sh.close()
