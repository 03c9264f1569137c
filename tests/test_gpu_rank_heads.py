"""kbhip_rank_heads on the device: the walk heads of up to 64 tasks of one
session from one sweep launch, one merge launch and one copy.

Row i of a call must be what kbhip_rank_nodes (victims 0) or
kbhip_rank_victim_nodes (victims 1..3) answers for (task_ids[i], by_score,
first 0, cap) on the same session, padded beyond the total with node -1, score
0, cands 0.  The small snapshots are also held against the faithful
restatement's per-node keys (oracle.ref_sweep_scores, as
tests/test_gpu_rank_nodes.py reads them), the 70 000-node one against
kbhip_sweep_scores' keys.  References of a snapshot are computed once per test
and not changed."""
import numpy as np
import pytest

from test_gpu_parity import NO_POD_AFFINITY
from test_gpu_rank_nodes import _walks
from test_gpu_victim_walk import _jobs
from walkmodel import uniform_oversized

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"
GI = 1 << 30
PENDING = 1


def _classes(engine, path):
    """(pending task ids, class per pod, inter-pod term count per class) of a snapshot."""
    with engine.EncodedSnapshot(path) as enc:
        cls = enc.table("pod_class")
        ipa_n = enc.table("class_aff").reshape(-1, 16)[:, 11]
    return [int(i) for i in np.nonzero(cls >= 0)[0]], cls, ipa_n


def _still_pending(s, tasks):
    st = s.table("pod_status")
    return [t for t in tasks if st[t] == PENDING]


def _single(s, task, by_score, victims, cap):
    """(total, nodes, scores, cands) of the per-task call."""
    if victims == 0:
        t, n, sc = s.rank_nodes(task, by_score, 0, cap)
        return t, n, sc, np.zeros(n.size, np.int32)
    return s.rank_victim_nodes(task, by_score, victims, 0, cap)[:4]


def _row_is(got, i, ref, cap):
    """Row i of a rank_heads answer equals the per-task answer ref, padding included."""
    totals, nodes, scores, cands, _ = got
    t, n, sc, cd = ref
    k = min(t, cap)
    assert totals[i] == t, (i, totals[i], t)
    assert n.size == k
    assert np.array_equal(nodes[i, :k], n), (i, nodes[i], n)
    assert np.array_equal(scores[i, :k], sc), (i, scores[i], sc)
    assert np.array_equal(cands[i, :k], cd), (i, cands[i], cd)
    assert (nodes[i, k:] == -1).all() and not scores[i, k:].any() and not cands[i, k:].any(), i


def _same_as_singles(s, tasks, by_score, victims, cap):
    """One call first (it may build the candidate table), then the per-task calls."""
    got = s.rank_heads(tasks, by_score, victims, cap)
    assert got[1].shape == got[2].shape == got[3].shape == (len(tasks), cap)
    for i, t in enumerate(tasks):
        _row_is(got, i, _single(s, t, by_score, victims, cap), cap)
    return got


def _with_job(s, tasks):
    """The tasks kbhip_rank_victim_nodes answers for (a task without a job is refused)."""
    import kbhip
    out = []
    for t in tasks:
        try:
            s.rank_victim_nodes(t, False, 1, 0, 1)
            out.append(t)
        except kbhip.KbhipError:
            pass
    return out


def _random_case(kbgen, seed):
    feats = NO_POD_AFFINITY if seed % 2 else None
    kw = {} if feats is None else {"features": feats}
    return kbgen.gen_random(7100 + seed, n_nodes=5 + seed % 9, n_jobs=4 + seed % 5, max_tasks=1 + seed % 5, **kw)


# ---- 1. against the restatement -------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_heads_vs_oracle(engine, oracle_mod, kbgen_mod, tmp_path, seed):
    c = _random_case(kbgen_mod, seed)
    p = c.write(str(tmp_path / "s.kbs"))
    n_nodes = len(c.nodes)
    pend, _, _ = _classes(engine, p)
    assert pend
    checked = 0
    for actions in ("", "allocate"):
        with engine.Session(p) as s:
            if actions:
                s.allocate()
            todo = _still_pending(s, pend)[:64]
            if not todo:
                continue
            heads = {bs: s.rank_heads(todo, bs, 0, 64) for bs in (1, 0)}
            for i, pod in enumerate(todo):
                n_exp, k_exp = oracle_mod.ref_sweep_scores(p, pod, n_nodes, actions)
                nodes, scores, by_index = _walks(k_exp)
                assert nodes.size == n_exp
                _row_is(heads[1], i, (n_exp, nodes[:64], scores[:64], np.zeros(min(n_exp, 64), np.int32)), 64)
                _row_is(heads[0], i, (n_exp, by_index[:64], np.zeros(min(n_exp, 64), np.int32),
                                      np.zeros(min(n_exp, 64), np.int32)), 64)
                checked += 1
    assert checked


# ---- 2. against the per-task calls ----------------------------------------------
def _preempt_case(kbgen, k):
    aff, seed = [(0, 3), (0, 39), (1, 5), (1, 41)][k]
    return kbgen.gen_preempt((1500 if aff else 500) + seed, n_nodes=4 + seed % 10, n_queues=2 + seed % 3,
                             n_run_jobs=4 + seed % 9, n_pend_jobs=2 + seed % 5, max_tasks=1 + seed % 6,
                             features=("podaffinity",) if aff else ())


@pytest.mark.parametrize("case", [("rnd", 0), ("rnd", 1), ("rnd", 4), ("rnd", 7), ("pre", 0), ("pre", 1), ("pre", 2),
                                  ("pre", 3)], ids=lambda c: "%s%d" % c)
def test_heads_vs_single_calls(engine, kbgen_mod, tmp_path, case):
    kind, k = case
    c = _random_case(kbgen_mod, k) if kind == "rnd" else _preempt_case(kbgen_mod, k)
    p = c.write(str(tmp_path / "s.kbs"))
    pend, _, _ = _classes(engine, p)
    rows = 0
    for actions in ("", "allocate"):
        with engine.Session(p) as s:
            if actions:
                s.allocate()
            todo = _still_pending(s, pend)[:64]
            jobbed = _with_job(s, todo)
            for victims in (0, 1, 2, 3):
                tasks = todo if victims == 0 else jobbed
                if not tasks:
                    continue
                for cap in (1, 7, 64):
                    for by_score in (True, False):
                        _same_as_singles(s, tasks, by_score, victims, cap)
                        rows += len(tasks)
    assert rows


# ---- 3. edges of the selection --------------------------------------------------
def _edges(engine, c, p, n_pass):
    c.write(p)
    with engine.Session(p) as s:
        for by_score in (True, False):
            ref = _single(s, 0, by_score, 0, 64)
            assert ref[0] == n_pass
            for reps in (1, 2, 64):
                got = s.rank_heads([0] * reps, by_score, 0, 64)
                for i in range(reps):
                    _row_is(got, i, ref, 64)
                assert got[4][1] == 2  # the launch bound, whatever n_tasks is


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 255, 256, 257, 3001])
def test_selection_edges(engine, kbgen_mod, tmp_path, n_nodes):
    """Every node passes, few distinct scores: ties by index across wave (64),
    block (256) and multi-block boundaries; the same task 1, 2 and 64 times."""
    _edges(engine, uniform_oversized(kbgen_mod, n_nodes), str(tmp_path / "u.kbs"), n_nodes)


def test_selection_every_third_node(engine, kbgen_mod, tmp_path):
    _edges(engine, uniform_oversized(kbgen_mod, 1000, label_every=3, selector=True), str(tmp_path / "t.kbs"), 334)


def test_selection_no_node_passes(engine, kbgen_mod, tmp_path):
    _edges(engine, uniform_oversized(kbgen_mod, 300, unsched=True), str(tmp_path / "n.kbs"), 0)


# ---- 4. mixed classes in one call -----------------------------------------------
def _across_classes(tasks, cls, n):
    """n of the tasks, taken round-robin over their classes."""
    by_cls = {}
    for t in tasks:
        by_cls.setdefault(int(cls[t]), []).append(t)
    out, k = [], 0
    while len(out) < n and any(by_cls.values()):
        for lst in by_cls.values():
            if k < len(lst) and len(out) < n:
                out.append(lst[k])
        k += 1
        if k > max(len(v) for v in by_cls.values()):
            break
    return out


def test_mixed_classes_3000(engine, kbgen_mod, tmp_path):
    p = str(tmp_path / "c2.kbs")
    kbgen_mod.gen_c2(p, n_nodes=3000, n_pending=6000)
    pend, cls, _ = _classes(engine, p)
    with engine.Session(p) as s:
        tasks = _across_classes(pend, cls, 64)
        assert len(tasks) == 64 and len({int(cls[t]) for t in tasks}) > 1
        for by_score in (True, False):
            assert _same_as_singles(s, tasks, by_score, 0, 64)[4][1] == 2
        s.allocate()
        tasks = _across_classes(_still_pending(s, pend), cls, 64)
        assert tasks
        for by_score in (True, False):
            _same_as_singles(s, tasks, by_score, 0, 64)


# ---- 5. several steps per wave --------------------------------------------------
def test_several_steps_per_wave(engine, kbgen_mod, tmp_path):
    """70 000 nodes and 64 requests: every block takes several 256-node steps, the last one ragged."""
    n_nodes = 70_000
    p = str(tmp_path / "big.kbs")
    kbgen_mod.gen_c4(p, n_nodes=n_nodes, n_pending=2000, running_per_node=1)
    pend, _, _ = _classes(engine, p)
    tasks = pend[::31][:64]
    assert len(tasks) == 64
    with engine.Session(p) as s:
        got = {bs: s.rank_heads(tasks, bs, 0, 64) for bs in (True, False)}
        assert got[True][4][2] * 256 * 2 < n_nodes  # the sweep's grid x leaves every block more than one step
        for i in (0, 29, 63):
            cnt, keys = s.sweep_scores(tasks[i], n_nodes)
            nodes, scores, by_index = _walks(keys)
            assert cnt == nodes.size > 64
            zero = np.zeros(64, np.int32)
            _row_is(got[True], i, (cnt, nodes[:64], scores[:64], zero), 64)
            _row_is(got[False], i, (cnt, by_index[:64], zero, zero), 64)
        for bs in (True, False):
            for i, t in enumerate(tasks):
                _row_is(got[bs], i, _single(s, t, bs, 0, 64), 64)


# ---- 6. table lifetime ----------------------------------------------------------
def _jobs_with_big(kbgen):
    """test_gpu_victim_walk's cluster and a task of job "one" that no node holds: Pending after allocate."""
    c = _jobs(kbgen)
    c.add_pod("ns", "one-big", uid="p2", group="one", priority=5, ts=1, containers=[kbgen.res(cpu=64000, mem=GI)])
    return c


def test_table_lifetime(engine, kbgen_mod, tmp_path):
    c = _jobs_with_big(kbgen_mod)
    p = c.write(str(tmp_path / "j.kbs"))
    t_one, t_wide, t_big = len(c.pods) - 3, len(c.pods) - 2, len(c.pods) - 1
    tasks = [t_one, t_wide, t_big, t_one]
    with engine.Session(p) as s:
        assert _still_pending(s, tasks) == tasks
        assert s.rank_heads(tasks, True, 1, 64)[4][0] == 1  # the first call builds the table
        for victims in (1, 2, 3):
            assert _same_as_singles(s, tasks, True, victims, 64)[4][0] == 0
        # every candidate of node 10 for a task of queue q0, evicted through apply_ops: no rebuild
        before = s.rank_heads([t_one], False, 1, 64)
        assert 10 in before[1][0].tolist()
        names = sorted(x.name for x in c.nodes)
        pods = sorted(c.pods, key=lambda q: q.uid)
        jq = {j.name: j.queue for j in c.jobs}
        vict = [i for i, q in enumerate(pods) if q.node == names[10] and jq[q.group] == "q1"]
        assert vict
        s.apply_ops([engine.OP_EVICT] * len(vict), vict)
        for victims in (1, 2, 3):
            for by_score in (True, False):
                got = _same_as_singles(s, tasks, by_score, victims, 64)
                assert got[4][0] == 0
        assert 10 not in s.rank_heads([t_one], False, 1, 64)[1][0].tolist()
        s.allocate()
        left = _still_pending(s, tasks)
        assert t_big in left
        assert s.rank_heads(left, True, 2, 64)[4][0] == 1  # allocate left the table stale
        assert _same_as_singles(s, left, True, 2, 64)[4][0] == 0


# ---- 7. the launch bound --------------------------------------------------------
def test_launch_bound(engine, kbgen_mod, tmp_path):
    """2 launches for a batch without inter-pod classes whatever n_tasks is; one more per distinct class
    with inter-pod priority terms when the walk is scored."""
    c = _jobs_with_big(kbgen_mod)
    p = c.write(str(tmp_path / "j.kbs"))
    t_one, t_wide = len(c.pods) - 3, len(c.pods) - 2
    with engine.Session(p) as s:
        for n in (1, 2, 63, 64):
            for victims in (0, 3):
                s.rank_heads([t_one], True, victims, 64)  # (a stale table is rebuilt by a copy, not a launch)
                assert s.rank_heads(([t_one, t_wide] * 32)[:n], True, victims, 64)[4][1] == 2
    seen = 0
    for k in (2, 3):
        c = _preempt_case(kbgen_mod, k)
        p = c.write(str(tmp_path / ("a%d.kbs" % k)))
        pend, cls, ipa_n = _classes(engine, p)
        with engine.Session(p) as s:
            tasks = (_still_pending(s, pend) * 64)[:64]  # repeats: a class is counted once
            n_ipa = len({int(cls[t]) for t in tasks if ipa_n[cls[t]] > 0})
            seen += n_ipa
            assert _same_as_singles(s, tasks, True, 0, 7)[4][1] == 2 + n_ipa
            assert s.rank_heads(tasks, False, 0, 7)[4][1] == 2  # the index walk has no score to normalise
    assert seen


# ---- 8. nothing changed ---------------------------------------------------------
def test_actions_unchanged(engine, kbgen_mod, tmp_path):
    """Node rows, walk counters and the records of the actions that follow equal a twin session's
    without the calls."""
    actions = "reclaim, allocate, backfill, preempt"
    records = 0
    for seed in (900, 901, 902):
        c = kbgen_mod.gen_preempt(seed, n_nodes=24, n_queues=3, n_run_jobs=14, n_pend_jobs=5, max_tasks=5)
        p = c.write(str(tmp_path / f"a{seed}.kbs"))
        pend, _, _ = _classes(engine, p)
        with engine.Session(p) as s, engine.Session(p) as twin:
            n_nodes = s.stats()["nodes"]
            jobbed = _with_job(s, pend)
            _with_job(twin, pend)  # (the twin takes the per-task calls the filter made)
            for by_score in (1, 0):
                for victims in (0, 1, 2, 3):
                    s.rank_heads((pend if victims == 0 else jobbed)[:64], by_score, victims, 64)
            assert np.array_equal(s.read_nodes(n_nodes), twin.read_nodes(n_nodes))
            a, b = s.walk_visits(), twin.walk_visits()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            got, exp = s.run_actions(actions), twin.run_actions(actions)
            assert all(np.array_equal(x, y) for x, y in zip(got, exp)), seed
            records += got[0].size
    assert records > 0


def test_fit_deltas_stay_answerable(engine, kbgen_mod, tmp_path):
    c = uniform_oversized(kbgen_mod, 300)
    p = c.write(str(tmp_path / "u.kbs"))
    with engine.Session(p) as s, engine.Session(p) as twin:
        for x in (s, twin):
            assert x.place_job([0], 1, 1, 0)[2] == engine.STOP_UNASSIGNED
        s.rank_heads([0, 0], True, 0, 64)
        a, b = s.fit_deltas(0), twin.fit_deltas(0)
        assert a[0].size == 300 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 9. errors ------------------------------------------------------------------
def test_errors(engine, kbgen_mod, tmp_path):
    c = _jobs_with_big(kbgen_mod)
    p = c.write(str(tmp_path / "e.kbs"))
    t_one, t_wide, t_big = len(c.pods) - 3, len(c.pods) - 2, len(c.pods) - 1
    vp = __import__("ctypes").c_void_p

    def raw(s, ids, victims=0):
        ids = np.asarray(ids, np.int32)
        out = [np.full(ids.size, -7, np.int64)] + [np.full(ids.size * 64, -7, np.int32) for _ in range(3)]
        rc = engine.lib().kbhip_rank_heads(s._h, ids.ctypes.data_as(vp), ids.size, 1, victims, 64,
                                           *[a.ctypes.data_as(vp) for a in out], None)
        return rc, engine.lib().kbhip_last_error(), all((a == -7).all() for a in out)

    with engine.Session(p) as s:
        assert raw(s, [t_one, t_big])[0] == 2
        assert s.rank_heads([], True, 0, 64)[0].size == 0  # n_tasks 0: nothing to do
        for bad in (0, len(c.pods), -1):  # a Running pod, no such task
            rc, msg, untouched = raw(s, [t_one, t_big, bad, t_one])
            assert rc == -1 and b"task_ids[2]" in msg and untouched
        t = s.place_job_submit([t_wide], 0, 1, 0)
        rc, msg, untouched = raw(s, [t_big])  # a ticket is outstanding
        assert rc == -1 and untouched
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.rank_heads([t_big], True, 0, 64)
        assert s.place_job_cancel(t) == 1
        assert s.rank_heads([t_big, t_wide], True, 1, 64)[0].size == 2
        pod, _, _ = s.allocate()
        assert t_one in pod.tolist() and t_big not in pod.tolist()
        for victims in (0, 2):
            rc, msg, untouched = raw(s, [t_big, t_one], victims)  # a task the session placed
            assert rc == -1 and b"task_ids[1]" in msg and b"Pending" in msg and untouched
        assert raw(s, [t_big, t_big], 2)[0] == 2
    sh = engine.ShardedSession(p, 0, 0, 2)
    try:
        for victims in (0, 1):
            with pytest.raises(engine.KbhipError, match=EUNSUP):
                sh.rank_heads([t_one], True, victims, 64)
    finally:
        sh.close()
