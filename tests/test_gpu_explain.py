"""kbhip_explain_tasks on the device: per-node rejection reasons of up to 64
pending tasks from one sweep launch, one reduce launch and one copy.

Verdict bytes and histograms must equal the ordered restatement
(verdictedges.why over prededges.Model; tests/test_explain_model.py holds the
host compilation of the same function to it) on every prededges kind and on the
stacked snapshot at 1 to 1200 nodes, for batches of 1, 2 and 64 tasks, with and
without verdict rows, and with the sweep's grid capped to 1 and 2 blocks (the
strided path with a partial last step).  In the same session the call must
agree with kbhip_sweep_scores, kbhip_place_job, kbhip_fit_deltas and
kbhip_gang_unschedulable; pod-affinity classes are held to the faithful
restatement's sweep.  References of a snapshot are computed once and not
changed.
"""
import ctypes

import numpy as np
import pytest

import prededges as pe
import verdictedges as ve

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in pe.CASES] + [s[0] for s in ve.STACKED]
CROSS = [c for c in pe.CROSS_NAMES if c != "cross65nopred" and int(c[5:]) >= 63]
EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"
GI, MI = 1 << 30, 1 << 20
PENDING = 1
VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def cases(kbgen_mod, tmp_path_factory):
    d = tmp_path_factory.mktemp("explain")
    out = pe.write_cases(kbgen_mod, d)
    out.update(ve.write_stacked(kbgen_mod, d))
    return out


@pytest.fixture(scope="module")
def expected(cases):
    """{name: {task: (verdict row, histogram)}} of the restatement at open, computed once."""
    out = {}
    for name, (snap, _) in cases.items():
        m = snap.model()
        out[name] = {}
        for j in ve.tasks_of(snap):
            v = ve.verdicts(m, j)
            out[name][j] = (v, ve.histogram(v))
    return out


def _blocks(n_nodes, n_req, cap=0):
    need = max((n_nodes + 255) // 256, 1)
    return min(need, cap) if cap else need


@pytest.mark.parametrize("name", NAMES)
def test_verdicts_and_histograms(engine, cases, expected, name):
    snap, path = cases[name]
    n = len(snap.rows)
    js = list(expected[name])
    with engine.Session(path) as s:
        for cap in (0, 1, 2) if n == 1200 else (0,):
            s.set_option("explain_blocks", cap)
            for k in (1, 2, 64):
                order = [js[(3 * i + 1) % len(js)] for i in range(k)]   # duplicates, mixed classes
                ids = [snap.tasks[j]["pod"] for j in order]
                e_hist = np.array([expected[name][j][1] for j in order])
                h0, v0, i0 = s.explain_tasks(ids, verdicts=False)
                h1, v1, i1 = s.explain_tasks(ids, verdicts=True, n_nodes=n)
                assert v0 is None and v1.shape == (k, n)
                assert list(i0[[0, 2]]) == [2, 0] and list(i1[[0, 2]]) == [2, 1]
                assert i0[1] == i1[1] and 1 <= i1[1] <= _blocks(n, k, cap)
                if k == 1 or cap:
                    assert i1[1] == _blocks(n, k, cap)
                for i, j in enumerate(order):
                    exp = expected[name][j][0]
                    bad = np.nonzero(v1[i] != exp)[0]
                    assert bad.size == 0, (cap, k, i, j, [(int(b), snap.family(int(b)), hex(int(v1[i, b])),
                                                           hex(int(exp[b]))) for b in bad[:4]])
                assert np.array_equal(h1, e_hist), (cap, k)
                assert np.array_equal(h0, e_hist), (cap, k)


@pytest.mark.parametrize("name", NAMES)
def test_agrees_with_sweep_scores(engine, cases, expected, name):
    """In one session: a node's code is in 0..2 exactly where kbhip_sweep_scores gives it a key."""
    snap, path = cases[name]
    n = len(snap.rows)
    js = list(expected[name])[:64]
    with engine.Session(path) as s:
        hist, v, _ = s.explain_tasks([snap.tasks[j]["pod"] for j in js], verdicts=True, n_nodes=n)
        for i, j in enumerate(js):
            cnt, keys = s.sweep_scores(snap.tasks[j]["pod"], n)
            assert np.array_equal((v[i] & 15) <= ve.RESOURCES, keys != 0), j
            assert cnt == hist[i, 14] == hist[i, :3].sum()
            assert hist[i, 15] == n and hist[i, :10].sum() == n and hist[i, 10] == 0


def _fit_text(h):
    """JobInfo.FitError (job_info.go:343-372) from a histogram row."""
    if h[14] == 0:
        return "0 nodes are available"
    rs = sorted(f"{int(h[11 + k])} insufficient {r}" for k, r in enumerate(("cpu", "memory", "GPU")) if h[11 + k] > 0)
    return f"0/{int(h[14])} nodes are available, " + ", ".join(rs) + "."


@pytest.mark.parametrize("name", CROSS)
def test_along_a_gang_until_no_node_is_left(engine, cases, name):
    """The tasks of the Pipelined-capable gang and of the gang that runs out of
    nodes, placed one by one: before every placement the verdict row is the
    restatement's on the state the commits left (pod counts, Idle, Releasing
    moved), the node kbhip_place_job then picks carries code 0 where it reports
    Allocated and code 1 where it reports Pipelined, and the task that finds no
    node has the FitError numbers of kbhip_fit_deltas, which still answers
    afterwards.  (kbhip_place_job does not record a job's FitError: the text of
    kbhip_gang_unschedulable is compared after the allocate action, below.)"""
    snap, path = cases[name]
    n = len(snap.rows)
    m = snap.model()
    kinds = set()
    with engine.Session(path) as s:
        for uid in ("ns/jpipe", "ns/jgang"):
            for j in snap.jobs[uid]:
                pod = snap.tasks[j]["pod"]
                hist, v, _ = s.explain_tasks([pod], verdicts=True, n_nodes=n)
                exp = ve.verdicts(m, j)
                assert np.array_equal(v[0], exp) and np.array_equal(hist[0], ve.histogram(exp)), (uid, j)
                nodes, knd, stop = s.place_job([pod], 0, 1, 0)
                if stop == engine.STOP_UNASSIGNED:
                    assert list(nodes) == [-1] and hist[0, 0] == hist[0, 1] == 0
                    node, delta = s.fit_deltas(pod)
                    assert hist[0, 14] == node.size
                    assert list(hist[0, 11:14]) == [(delta[:, k] < 0).sum() for k in range(3)]
                    again = s.explain_tasks([pod])[0]
                    assert np.array_equal(again, hist)
                    node2, delta2 = s.fit_deltas(pod)   # still answerable
                    assert np.array_equal(node, node2) and np.array_equal(delta, delta2)
                    assert _fit_text(hist[0]) == m.fit_counts(j)
                    kinds.add(0)
                    break
                code = int(v[0, int(nodes[0])]) & 15
                assert code == (ve.FITS_IDLE if int(knd[0]) == engine.ALLOCATED else ve.FITS_RELEASING), (uid, j)
                kinds.add(int(knd[0]))
                m.commit(j, int(nodes[0]), int(knd[0]))
    assert kinds == {0, engine.ALLOCATED, engine.PIPELINED}


@pytest.mark.parametrize("name", [c for c in pe.CROSS_NAMES if c != "cross65nopred"])
def test_fit_error_text_after_allocate(engine, cases, name):
    """The allocate action records the FitError of the task a gang stopped on.
    The jobs select disjoint node families, so an unplaced task of a job left
    not Ready meets the state its job's last walk saw: the histogram's [14] and
    [11..13] are the numbers in kbhip_gang_unschedulable's text for the job."""
    snap, path = cases[name]
    compared = 0
    with engine.Session(path) as s:
        placed = set(s.allocate()[0].tolist())
        msgs = s.gang_unschedulable()
        for uid, msg in msgs.items():
            left = [j for j in snap.jobs.get(uid, []) if snap.tasks[j]["pod"] not in placed]
            if not left:   # (the Running pods' job)
                continue
            hist = s.explain_tasks([snap.tasks[left[0]]["pod"]])[0]
            assert hist[0, 0] == hist[0, 1] == 0
            assert msg.split(": ", 1)[1] == _fit_text(hist[0]), (uid, msg)
            compared += 1
    assert compared >= 1


# ---- pod (anti-)affinity ----------------------------------------------------------
N_AFF = 300


def _zone_case(kbgen):
    """300 nodes in 10 zones, every seventh unschedulable; Running pods app=db on
    nodes 0 (zone z0) and 3 (zone z3).  Pending: X with required anti-affinity to
    app=db by zone, X' its twin without the terms, Z with required affinity."""
    c = kbgen.Cluster()
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    c.add_job("ns", "run", "q1", min_member=1, ts=0)
    for n in range(N_AFF):
        c.add_node(f"n{n:05d}", 16000, 64 * GI, 0, 110, labels={"zone": f"z{n % 10}"}, unschedulable=n % 7 == 0)
    for k, n in enumerate((0, 3)):
        c.add_pod("ns", f"r{k}", uid=f"r{k}", group="run", node=f"n{n:05d}", phase="Running", labels={"app": "db"},
                  containers=[kbgen.res(cpu=1000, mem=GI)])
    term = {"selector": {"ml": {"app": "db"}}, "topology_key": "zone"}
    for k, aff in enumerate(({"anti": {"required": [term]}}, None, {"pod": {"required": [term]}})):
        c.add_job("ns", f"pj{k}", "q0", min_member=1, ts=k + 1)
        c.add_pod("ns", f"u{k}", uid=f"u{k}", group=f"pj{k}", ts=k + 1, affinity=aff,
                  containers=[kbgen.res(cpu=500, mem=GI)])
    return c


def test_pod_affinity_codes_and_the_flush(engine, oracle_mod, kbgen_mod, tmp_path):
    p = _zone_case(kbgen_mod).write(str(tmp_path / "z.kbs"))
    x, twin, z = 2, 3, 4
    zone = np.arange(N_AFF) % 10
    unsched = np.arange(N_AFF) % 7 == 0
    with engine.Session(p) as s:
        hist, v, info = s.explain_tasks([x, twin, z], verdicts=True, n_nodes=N_AFF)
        assert info[0] == 2
        code = v & 15
        for i, pod in enumerate((x, twin, z)):
            cnt, keys = oracle_mod.ref_sweep_scores(p, pod, N_AFF, "")
            assert np.array_equal(code[i] <= ve.RESOURCES, keys != 0) and cnt == hist[i, 14]
            assert not keys[code[i] == ve.POD_AFFINITY].any()
        in_db = (zone == 0) | (zone == 3)
        assert np.array_equal(code[0] == ve.POD_AFFINITY, in_db & ~unsched)
        assert np.array_equal(code[2] == ve.POD_AFFINITY, ~in_db & ~unsched)
        assert (code[0] == ve.POD_AFFINITY).sum() >= 40 and (code[2] == ve.POD_AFFINITY).sum() >= 150
        # the same pod without the terms: every code-8 node is in the walk; the earlier steps are the twin's
        assert (code[1][(code[0] == ve.POD_AFFINITY) | (code[2] == ve.POD_AFFINITY)] <= ve.RESOURCES).all()
        assert np.array_equal(code[0] == ve.UNSCHEDULABLE, unsched) and np.array_equal(code[1] == ve.UNSCHEDULABLE, unsched)
        # the db pod of zone z0 evicted: the zone opens for X and closes for Z.  (kbhip_apply_ops applies its
        # own count changes before it returns, so the call finds nothing left to flush: 2 launches or 3.)
        s.apply_ops([engine.OP_EVICT], [0])
        hist2, v2, info2 = s.explain_tasks([x, twin, z], verdicts=True, n_nodes=N_AFF)
        assert info2[0] in (2, 3)
        code2 = v2 & 15
        assert np.array_equal(code2[0] == ve.POD_AFFINITY, (zone == 3) & ~unsched)
        assert np.array_equal(code2[2] == ve.POD_AFFINITY, (zone != 3) & ~unsched)
        assert (code2[0][(zone == 0) & ~unsched] <= ve.RESOURCES).all()
        assert np.array_equal(code2[1], code[1])
        assert s.explain_tasks([x])[2][0] == 2   # nothing left to flush
        for i, pod in enumerate((x, twin, z)):
            cnt, keys = s.sweep_scores(pod, N_AFF)
            assert np.array_equal(code2[i] <= ve.RESOURCES, keys != 0) and cnt == hist2[i, 14]


@pytest.mark.parametrize("seed", range(6))
def test_random_classes_walk_set_is_the_restatements(engine, oracle_mod, kbgen_mod, tmp_path, seed):
    """gen_random with every feature (pod affinity, inter-pod terms, invalid
    selectors, init containers, host ports): the walk set of every pending task
    is the faithful restatement's, before and after allocate; a node with code
    8 has key 0; the codes 3..9 and 0..2 partition the nodes."""
    c = kbgen_mod.gen_random(8200 + seed, n_nodes=9 + 5 * seed, n_jobs=6 + seed, max_tasks=4)
    p = c.write(str(tmp_path / "r.kbs"))
    n = len(c.nodes)
    with engine.EncodedSnapshot(p) as enc:
        pend = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
    checked = 0
    for actions in ("", "allocate"):
        with engine.Session(p) as s:
            if actions:
                s.allocate()
            st = s.table("pod_status")
            todo = [t for t in pend if st[t] == PENDING][:64]
            if not todo:
                continue
            hist, v, _ = s.explain_tasks(todo, verdicts=True, n_nodes=n)
            for i, pod in enumerate(todo):
                cnt, keys = oracle_mod.ref_sweep_scores(p, pod, n, actions)
                code = v[i] & 15
                assert code.max() <= ve.SCORE_ERROR
                assert np.array_equal(code <= ve.RESOURCES, keys != 0), (actions, pod)
                assert np.array_equal(hist[i], ve.histogram(v[i])) and cnt == hist[i, 14]
                assert not (v[i][code > ve.RESOURCES] & 0x70).any()
                checked += 1
    assert checked


# ---- state and refusals -----------------------------------------------------------
def test_nothing_changes(engine, cases):
    """Node rows and the number of walk-visit records are the same before and
    after the calls (after two placements whose walks visited Backfilled nodes)."""
    snap, path = cases["stacked257"]
    n = len(snap.rows)
    pods = [t["pod"] for t in snap.tasks]
    with engine.Session(path) as s:
        for pod in (pods[0], pods[3]):
            assert s.place_job([pod], 0, 1, 0)[2] != engine.STOP_UNASSIGNED
        rows = s.read_nodes(n)
        visits = int(engine.lib().kbhip_walk_visits(s._h, None, None, 0))
        for verdicts in (False, True):
            s.explain_tasks([pods[1], pods[2], pods[1]], verdicts=verdicts, n_nodes=n)
        assert np.array_equal(s.read_nodes(n), rows)
        assert int(engine.lib().kbhip_walk_visits(s._h, None, None, 0)) == visits


def test_refusals(engine, cases):
    snap, path = cases["stacked65"]
    n = len(snap.rows)
    pods = [t["pod"] for t in snap.tasks]

    def raw(s, ids):
        ids = np.asarray(ids, np.int32)
        hist = np.full(max(ids.size, 1) * 16, -7, np.int64)
        v = np.full(max(ids.size, 1) * n, 0xA5, np.uint8)
        info = np.full(3, -7, np.int64)
        rc = engine.lib().kbhip_explain_tasks(s._h, ids.ctypes.data_as(VP), ids.size, v.ctypes.data_as(VP),
                                              hist.ctypes.data_as(VP), info.ctypes.data_as(VP))
        return rc, engine.lib().kbhip_last_error(), (hist == -7).all() and (v == 0xA5).all() and (info == -7).all()

    with engine.Session(path) as s:
        assert raw(s, pods)[0] == len(pods)
        rc, _, untouched = raw(s, [])       # n_tasks 0: nothing to do, nothing written
        assert rc == 0 and untouched
        assert s.explain_tasks([])[0].shape == (0, 16)
        for bad in (0, n + len(pods), -1):  # a Running pod, no such task
            rc, msg, untouched = raw(s, [pods[0], pods[1], bad, pods[0]])
            assert rc == -1 and b"task_ids[2]" in msg and untouched
        t = s.place_job_submit([pods[2]], 0, 1, 0)
        rc, msg, untouched = raw(s, [pods[0]])   # a ticket is outstanding
        assert rc == -1 and untouched
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.explain_tasks([pods[0]])
        assert s.place_job_cancel(t) == 1
        assert raw(s, [pods[0], pods[2]])[0] == 2
        placed = s.allocate()[0].tolist()
        assert pods[2] in placed and pods[4] not in placed
        rc, msg, untouched = raw(s, [pods[4], pods[2]])   # a task the session placed since
        assert rc == -1 and b"task_ids[1]" in msg and b"Pending" in msg and untouched
        assert raw(s, [pods[4], pods[4]])[0] == 2
    sh = engine.ShardedSession(path, 0, 0, 2)
    try:
        for verdicts in (False, True):
            with pytest.raises(engine.KbhipError, match=EUNSUP):
                sh.explain_tasks([pods[0]], verdicts=verdicts, n_nodes=n)
    finally:
        sh.close()
