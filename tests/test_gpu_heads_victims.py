"""kbhip_heads_victims on the device: kbhip_head_victims' answer for up to 64 tasks from one call.

The yardsticks are kbhip_head_victims on the same session, element for element, and tests/victimmodel.py
(the reference's plugin sources restated over the kbgen.Cluster) following the operations the test applied."""
import functools
import re

import numpy as np
import pytest

import victimedges
import victimmodel
from headsvictims import check_batch, first_valid, packed
from test_gpu_victim_walk import CASES, EXACT, _gen, _jobs, _uniform

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"
TIER_ALL = [["priority", "gang", "drf", "predicates", "proportion", "nodeorder"]]


def _chunks(tasks, n=64):
    return [tasks[i:i + n] for i in range(0, len(tasks), n)]


def _apply(engine, s, m, rec):
    E, P = engine.OP_EVICT, engine.OP_PIPELINE
    assert s.apply_ops([E if k == 128 else P for _, _, k in rec], [q for q, _, _ in rec], [n for _, n, _ in rec]) <= 2
    m.records(rec)


@pytest.fixture(scope="module")
def snaps(oracle_mod, kbgen_mod, tmp_path_factory):
    """case -> (path, the oracle's reclaim records, the cluster): computed once."""
    d = tmp_path_factory.mktemp("heads_victims")

    @functools.lru_cache(maxsize=None)
    def get(case):
        c = _gen(kbgen_mod, case)
        p = c.write(str(d / ("c%d_%d_%d_%d.kbs" % case)))
        return p, oracle_mod.ref_allocate(p, actions="reclaim").as_list(), c

    return get


def _sweep(s, m, tasks):
    """Every (order, mode, cap, stride) for the tasks in chunks of at most 64.  Returns the batched calls' infos."""
    infos, memo = [], {}
    for by_score in (True, False):
        for mode in (1, 2, 3):
            for cap in (1, 64):
                for stride in (1, 8):
                    for chunk in _chunks(tasks):
                        got, _ = check_batch(s, m, chunk, by_score, mode, cap, stride, memo)
                        infos.append(got[8])
    return infos


# ---- 1. parity with the per-task call and the model ----------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_parity(engine, snaps, case):
    p, reclaim, c = snaps(case)
    with engine.Session(p) as s:
        m = victimmodel.VictimModel(c)
        todo = m.pending()
        assert todo
        infos = _sweep(s, m, todo)
        assert [i["state_rebuilt"] for i in infos] == [1] + [0] * (len(infos) - 1)
        assert all(i["patched"] == 0 and i["victim_launches"] == 1 for i in infos)
        if reclaim:
            _apply(engine, s, m, reclaim)
            infos = _sweep(s, m, m.pending())
            assert not any(i["state_rebuilt"] for i in infos)
            assert infos[0]["patched"] > 0 and not any(i["patched"] for i in infos[1:])


# ---- 2. batch sizes and request independence -----------------------------------
def _equal(a, b, i, j):
    return all(np.array_equal(x[i], y[j]) for x, y in zip(a[:8], b[:8]))


@pytest.mark.parametrize("size", [1, 2, 63, 64])
def test_batch_sizes(engine, snaps, size):
    p, _, c = snaps(CASES[0])
    m = victimmodel.VictimModel(c)
    pend = m.pending()
    # (the first task twice in a row where the batch has room, then the pending tasks over and over)
    tasks = ([pend[0]] + pend * (size // len(pend) + 1))[:size]
    with engine.Session(p) as s:
        for by_score, mode in ((True, 1), (False, 2)):
            got, _ = check_batch(s, m, tasks, by_score, mode, 64, 8)
            seen = {}
            for i, t in enumerate(tasks):
                if t in seen:
                    assert _equal(got, got, i, seen[t]), (i, t)
                seen.setdefault(t, i)
            assert size == 1 or len(seen) < size  # (a task appeared twice)
            rev = s.heads_victims(tasks[::-1], by_score, mode, 64, 8)
            for i in range(size):
                assert _equal(rev, got, i, size - 1 - i), i
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.heads_victims([pend[0]] * 65)


def test_requests_are_independent(engine, kbgen_mod, tmp_path):
    """Two requests of one batch with different answers on the same node: a kernel that read request 0's
    header or head for every request would give them the same row."""
    found = 0
    for name in sorted(victimedges.BUILDERS):
        c, _ = victimedges.BUILDERS[name]()
        m = victimmodel.VictimModel(c)
        pend = m.pending()
        pairs = [(mode, a, b, node) for mode in (1, 2, 3) for i, a in enumerate(pend) for b in pend[i + 1:]
                 for node in range(m.n_nodes)
                 if m.decide(a, mode, node) != m.decide(b, mode, node)]
        if not pairs:
            continue
        with engine.Session(c.write(str(tmp_path / (name + ".kbs")))) as s:
            for mode in sorted({q[0] for q in pairs}):
                got, _ = check_batch(s, m, pend, False, mode, 64, 4)
                nodes, counts, evicts, flags, rows = got[1], got[3], got[4], got[5], got[6]
                for _, a, b, node in (q for q in pairs if q[0] == mode):
                    ia, ib = pend.index(a), pend.index(b)
                    ja, jb = np.nonzero(nodes[ia] == node)[0], np.nonzero(nodes[ib] == node)[0]
                    if not ja.size or not jb.size:
                        continue  # (the node is not in both pruned walks)
                    ja, jb = int(ja[0]), int(jb[0])
                    ra = (int(counts[ia][ja]), int(evicts[ia][ja]), int(flags[ia][ja]), rows[ia][ja].tolist())
                    rb = (int(counts[ib][jb]), int(evicts[ib][jb]), int(flags[ib][jb]), rows[ib][jb].tolist())
                    assert ra != rb, (name, mode, a, b, node)
                    found += 1
    assert found
    # tasks of two jobs (and the modes that read the job) in one batch: each request is its per-task answer
    c = _jobs(kbgen_mod)
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    m = victimmodel.VictimModel(c)
    with engine.Session(c.write(str(tmp_path / "jobs.kbs"))) as s:
        for mode in (1, 2, 3):
            for by_score in (True, False):
                check_batch(s, m, [t_wide, t_one, t_one, t_wide], by_score, mode, 64, 4)


# ---- 3. node sizes and the spill ranges ----------------------------------------
@pytest.mark.parametrize("tiers", [None, TIER_ALL, [["conformance"], ["gang", "drf", "proportion"]]],
                         ids=["default", "one_tier", "two_tiers"])
def test_node_sizes(engine, kbgen_mod, tmp_path, tiers):
    c = packed(kbgen_mod, tiers)
    p = c.write(str(tmp_path / "p.kbs"))
    m = victimmodel.VictimModel(c)
    pend = m.pending()
    assert len(pend) == 2
    tasks = [pend[0], pend[1], pend[0], pend[1]]
    shapes = [(mode, stride) for mode in (1, 2, 3) for stride in (1, 7, 300)]
    with engine.Session(p) as s:
        memo, base, seen = {}, {}, 0
        for mode, stride in shapes:
            got, nonempty = check_batch(s, m, tasks, False, mode, 64, stride, memo)
            assert got[8]["victim_launches"] == 1
            base[(mode, stride)] = got
            seen += nonempty
        assert seen
        assert max(base[(mode, 1)][8]["max_count"] for mode in (1, 2, 3)) > 1  # (stride 1 truncated a row)
        # a bound below one request's rows: refused before any device work, nothing written
        L = engine.lib()
        ids = np.asarray(tasks, np.int32)
        outs = [np.full(4, 77, np.int64)] + [np.full(4 * 64, 77, np.int32) for _ in range(4)] + \
               [np.full(4 * 64, 77, np.uint8), np.full(4 * 64 * 7, 77, np.int32), np.full(4, 77, np.int32),
                np.full(6, 77, np.int64)]
        s.set_option("victims_spill_max", 1)
        assert L.kbhip_heads_victims(s._h, ids.ctypes.data, 4, 0, 1, 64, 7, *[a.ctypes.data for a in outs]) == -3
        one = int(re.search(rb"take (\d+) bytes", L.kbhip_last_error()).group(1))
        assert one >= 64 * 257 * 160  # (64 rows of the longest node's 257 records)
        assert all((a == 77).all() for a in outs)
        s.set_option("victims_spill_max", one - 1)
        with pytest.raises(engine.KbhipError, match=EUNSUP):
            s.heads_victims(tasks, False, 1, 64, 7)
        # room for one request's rows and not for two: a launch per request, the same rows
        s.set_option("victims_spill_max", 2 * one - 1)
        for mode, stride in shapes:
            got = s.heads_victims(tasks, False, mode, 64, stride)
            assert got[8]["victim_launches"] == 4
            assert got[8]["launches"] == base[(mode, stride)][8]["launches"] + 3
            assert all(np.array_equal(x, y) for x, y in zip(got[:8], base[(mode, stride)][:8])), (mode, stride)
        s.set_option("victims_spill_max", 2 * one)  # two requests per range
        assert s.heads_victims(tasks, False, 1, 64, 7)[8]["victim_launches"] == 2
        s.set_option("victims_spill_max", 256 << 20)
        # evictions in the middle of the large nodes, patched not rebuilt: the running sums move
        mid = [q for q in range(len(m.node)) if m.status(q) == victimmodel.RUNNING and q % 9 == 4]
        s.apply_ops([engine.OP_EVICT] * len(mid), mid)
        for q in mid:
            m.evict(q)
        first = True
        for mode in (1, 2, 3):
            got, _ = check_batch(s, m, tasks, True, mode, 64, 300)
            assert (got[8]["patched"] > 0) == first and not got[8]["state_rebuilt"]
            assert got[8]["victim_launches"] == 1
            first = False


# ---- 4. head lengths -----------------------------------------------------------
@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65])
def test_head_lengths(engine, kbgen_mod, tmp_path, n_nodes):
    c = _uniform(kbgen_mod, n_nodes, "all")
    p = c.write(str(tmp_path / "u.kbs"))
    m = victimmodel.VictimModel(c)
    task = m.pending()[0]
    with engine.Session(p) as s:
        for cap in (1, 63, 64):
            for by_score in (True, False):
                got, nonempty = check_batch(s, m, [task, task], by_score, 1, cap, 8)
                assert nonempty
                assert got[0].tolist() == [n_nodes, n_nodes]
                k = min(cap, n_nodes)
                assert (got[1][:, :k] >= 0).all() and (got[1][:, k:] == -1).all()
                assert (got[6][:, k:] == -1).all() and not got[3][:, k:].any()


# ---- 5. the host loop with a prefetching ask -----------------------------------
def test_host_reclaim_loop_with_prefetch(engine, snaps):
    """victimmodel.host_reclaim, its rows from kbhip_heads_victims: a miss asks for the task and up to 63
    further pending tasks, the answers are kept until the next kbhip_apply_ops."""
    asked = called = 0
    for case in EXACT:
        p, reclaim, c = snaps(case)
        m = victimmodel.VictimModel(c)
        with engine.Session(p) as s:
            cache, count = {}, {"ask": 0, "call": 0, "apply": 0, "hit": 0}

            def ask(task):
                count["ask"] += 1
                if task not in cache:
                    batch = [task] + [t for t in m.pending() if t != task][:63]
                    count["call"] += 1
                    totals, nodes, _, counts, evicts, flags, rows, first, info = s.heads_victims(batch, False, 1, 64, 128)
                    assert info["max_count"] <= 128 and (totals <= 64).all()
                    for i, t in enumerate(batch):
                        k = int(totals[i])
                        assert int(first[i]) == first_valid(flags[i])
                        cache[t] = (count["apply"], [(int(nodes[i][j]), rows[i][j][:int(counts[i][j])].tolist(),
                                                      int(evicts[i][j]), int(flags[i][j])) for j in range(k)])
                else:
                    count["hit"] += 1
                stamp, rows_of = cache[task]
                assert stamp == count["apply"]  # no kbhip_apply_ops came after these rows
                return rows_of

            def apply(ops):
                E, P = engine.OP_EVICT, engine.OP_PIPELINE
                assert s.apply_ops([E if k == 128 else P for k, _, _ in ops], [q for _, q, _ in ops],
                                   [n for _, _, n in ops]) <= 2
                count["apply"] += 1
                cache.clear()

            log = victimmodel.host_reclaim(m, ask, apply)
            assert log == [tuple(r) for r in reclaim], case
            assert count["call"] + count["hit"] == count["ask"] and count["call"] <= count["ask"]
            print(case, count)
            asked += count["ask"]
            called += count["call"]
    assert called < asked  # the batched calls issued are fewer than the tasks asked for


# ---- 6. read-only --------------------------------------------------------------
def test_read_only(engine, snaps):
    p, reclaim, c = snaps(CASES[2])
    with engine.Session(p) as s, engine.Session(p) as twin:
        n_nodes = s.stats()["nodes"]
        m = victimmodel.VictimModel(c)
        pend = m.pending()[:64]
        t = pend[0]
        rows = s.read_nodes(n_nodes)
        st0 = s.stats()
        before = [s.rank_victim_nodes(t, b, mode, 0, 64) for b in (True, False) for mode in (1, 2, 3)]
        calls = 0
        for b in (True, False):
            for mode in (1, 2, 3):
                s.heads_victims(pend, b, mode, 64, 4)
                calls += 1
        after = [s.rank_victim_nodes(t, b, mode, 0, 64) for b in (True, False) for mode in (1, 2, 3)]
        for x, y in zip(before, after):
            assert x[0] == y[0] and all(np.array_equal(a, b) for a, b in zip(x[1:4], y[1:4]))
        assert np.array_equal(s.read_nodes(n_nodes), rows)
        st1 = s.stats()
        assert st1["rank_heads"] - st0["rank_heads"] == calls * len(pend)
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
        s.heads_victims(left[:64], True, 1, 64, 4)
        assert size() == v0
        if d0 is not None:
            d1 = s.fit_deltas(left[0])
            assert all(np.array_equal(x, y) for x, y in zip(d0, d1))
        twin.allocate()
        a, b = s.walk_visits(), twin.walk_visits()
        assert len(a[0]) == v0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 7. errors and staleness ---------------------------------------------------
def _raw_outs(n, cap, stride):
    return [np.full(n, 77, np.int64)] + [np.full(n * cap, 77, np.int32) for _ in range(4)] + \
           [np.full(n * cap, 77, np.uint8), np.full(n * cap * stride, 77, np.int32), np.full(n, 77, np.int32),
            np.full(6, 77, np.int64)]


def test_errors(engine, kbgen_mod, tmp_path):
    c = _jobs(kbgen_mod)
    p = c.write(str(tmp_path / "e.kbs"))
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    L = engine.lib()
    with engine.Session(p) as s:
        for kw in (dict(victims=0), dict(victims=4), dict(cap=0), dict(cap=65), dict(stride=0), dict(by_score=2)):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.heads_victims([t_one, t_wide], **kw)
        outs = _raw_outs(3, 4, 3)
        ptr = [a.ctypes.data for a in outs]
        # a Running pod in the middle of a batch: the message names its index, nothing is written
        ids = np.asarray([t_one, 0, t_wide], np.int32)
        assert L.kbhip_heads_victims(s._h, ids.ctypes.data, 3, 1, 1, 4, 3, *ptr) == -1
        assert b"task_ids[1]" in L.kbhip_last_error()
        ids = np.asarray([t_one, t_wide, len(c.pods)], np.int32)
        assert L.kbhip_heads_victims(s._h, ids.ctypes.data, 3, 1, 1, 4, 3, *ptr) == -1
        assert b"task_ids[2]" in L.kbhip_last_error()
        assert all((a == 77).all() for a in outs)
        # an empty batch returns 0 and leaves the outputs alone
        assert L.kbhip_heads_victims(s._h, ids.ctypes.data, 0, 1, 1, 4, 3, *ptr) == 0
        assert all((a == 77).all() for a in outs)
        got = s.heads_victims([], True, 1, 4, 3)
        assert got[0].shape == (0,) and got[1].shape == (0, 4) and got[6].shape == (0, 4, 3)
        # an outstanding ticket
        ids = np.asarray([t_one, t_wide, t_one], np.int32)
        t = s.place_job_submit([t_wide], 0, 1, 0)
        assert L.kbhip_heads_victims(s._h, ids.ctypes.data, 3, 1, 1, 4, 3, *ptr) == -1
        assert all((a == 77).all() for a in outs)
        assert s.place_job_cancel(t) == 1
        assert s.heads_victims([t_one, t_wide], True, 1)[0].min() > 0
        # a task pipelined through kbhip_apply_ops is no longer Pending
        node = int(s.rank_nodes(t_wide, True, 0, 1)[1][0])
        s.apply_ops([engine.OP_PIPELINE], [t_wide], [node])
        assert L.kbhip_heads_victims(s._h, ids.ctypes.data, 3, 1, 1, 4, 3, *ptr) == -1
        assert b"task_ids[1]" in L.kbhip_last_error()
        assert all((a == 77).all() for a in outs)
        assert s.heads_victims([t_one, t_one], True, 1)[0].min() > 0
    sh = engine.ShardedSession(p, 0, 0, 2)
    try:
        with pytest.raises(engine.KbhipError, match=EUNSUP):
            sh.heads_victims([t_one, t_wide], True, 1)
    finally:
        sh.close()


def test_rebuilt_once_after_what_changes_pod_statuses(engine, kbgen_mod, snaps, tmp_path):
    def once(s, tasks):
        assert s.heads_victims(tasks, True, 1)[8]["state_rebuilt"] == 1
        assert s.heads_victims(tasks, True, 1)[8]["state_rebuilt"] == 0
        assert s.head_victims(tasks[0], True, 1)[7]["state_rebuilt"] == 0  # (one state serves both calls)

    p, _, c = snaps(CASES[0])
    with engine.Session(p) as s:
        m = victimmodel.VictimModel(c)
        once(s, m.pending()[:64])
        s.allocate()
        st = s.table("pod_status")
        left = [t for t in m.pending() if st[t] == 1]
        assert left
        once(s, left[:64])
    c = _jobs(kbgen_mod)
    p = c.write(str(tmp_path / "f.kbs"))
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    with engine.Session(p) as s:
        once(s, [t_one, t_wide])
        s.place_job([t_wide], 0, 1, 0)
        once(s, [t_one, t_one])
        s.carry()
        once(s, [t_one, t_one])  # (first_fit placed the other task)
        assert s.first_fit([t_wide])[0] >= 0
        once(s, [t_one, t_one])
        s.carry()
        once(s, [t_one, t_one])  # (first_fit placed the other task)
