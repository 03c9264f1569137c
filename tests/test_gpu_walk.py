"""Read-outs of the allocate walk on the device: kbhip_walk_visits (per-node
GetAccessibleResource visit counts) and kbhip_fit_deltas (the NodesFitDelta
records of a task that found no node), against the faithful restatement
(oracle/kbref.cpp) and against independent engine paths."""
import numpy as np
import pytest

from gohost import GoHost
from walkmodel import NodeModel, crowded_gangs, fit_delta, fit_error, uniform_oversized

pytestmark = pytest.mark.gpu
GI = 1 << 30
FEATURES = ("labels", "taints", "ports", "init", "running", "releasing", "backfill", "selector", "nodeaffinity",
            "unsched")
STATUS = {1: 4, 2: 8}
PATHS = [{}, {"batched": 0}, {"overlap": 0}, {"overlap": 2}]


def _pairs(node, count):
    return [(int(a), int(b)) for a, b in zip(node, count)]


def test_known_answer(engine, oracle_mod, kbgen_mod, tmp_path):
    """Two equal nodes, allocatable cpu 4000, each running one backfill-annotated
    pod of cpu 1000: Idle = 3000, Backfilled = 1000 at open.  Two gangs of one
    task, popped in creation order (allocate.go:149-185 per task):

    task A (cpu 4500): both nodes score alike, so the walk goes n0, n1.
      n0: GetAccessibleResource -> Idle 4000 (visit), 4500 does not fit, nothing
      Releasing; n1: Idle 4000 (visit), does not fit.  Unassigned.
    task B (cpu 4800): same order.  n0: GetAccessibleResource -> Idle 5000
      (second visit of n0), 4800 fits: Allocated on n0; n1 is not reached.

    Visits: n0 twice, n1 once."""
    c = kbgen_mod.Cluster()
    c.add_queue("q0", 1)
    for i in range(2):
        c.add_node(f"n{i}", 4000, 8 * GI, 0, 110)
        c.add_pod("run", f"r{i}", uid=f"r{i}", node=f"n{i}", phase="Running", backfill=True,
                  containers=[kbgen_mod.res(cpu=1000, mem=1 * GI)])
    for j, cpu in enumerate((4500, 4800)):
        c.add_job("ns", f"j{j}", "q0", min_member=1, ts=j)
        c.add_pod("ns", f"j{j}-0", uid=f"p{j}", group=f"j{j}", ts=j, containers=[kbgen_mod.res(cpu=cpu, mem=1 * GI)])
    p = c.write(str(tmp_path / "k.kbs"))
    with engine.Session(p) as s:
        pod, node, kind = s.allocate()
        assert [(int(a), int(b), int(k)) for a, b, k in zip(pod, node, kind)] == [(1, 0, 1)]  # p1 (task B) on n0
        assert _pairs(*s.walk_visits()) == [(0, 2), (1, 1)]
        assert _pairs(*s.walk_visits()) == []
        ns = s.read_nodes(2)
    assert ns[0, 0] == 3000 + 2 * 1000 - 4800 and ns[1, 0] == 3000 + 1000
    assert oracle_mod.ref_allocate(p).as_list() == [(1, 0, 4)]


_HITS = {}


def _visits_case(engine, oracle_mod, p, n_nodes, n_pods):
    """allocate on every path: equal (node, count) lists; the host model with
    count x Backfilled and the placement log equals the oracle's node state and
    the device's.  Returns the visited nodes that carry Backfilled."""
    exp, ons = oracle_mod.ref_allocate(p, with_nodes=True)
    open_nodes, _ = oracle_mod.ref_open_nodes(p, n_nodes)
    req = oracle_mod.ref_task_requests(p, n_pods)
    first = None
    for opts in PATHS:
        with engine.Session(p) as s:
            for k, v in opts.items():
                s.set_option(k, v)
            pod, node, kind = s.allocate()
            vis = _pairs(*s.walk_visits())
            assert _pairs(*s.walk_visits()) == []
            ns = s.read_nodes(n_nodes)
        log = [(int(a), int(b), STATUS[int(k)]) for a, b, k in zip(pod, node, kind)]
        assert log == exp.as_list(), opts
        if first is None:
            first = vis
        assert vis == first, opts
        assert [n for n, _ in vis] == sorted(n for n, _ in vis) and all(k > 0 for _, k in vis)
        m = NodeModel(open_nodes, req)
        m.visit([n for n, _ in vis], [k for _, k in vis])
        m.place(log)
        assert np.array_equal(m.state().astype(np.float64), ons[:n_nodes]), opts
        assert np.array_equal(m.state(), ns), opts
    bf = open_nodes[:, 9:12].any(axis=1)
    return sum(1 for n, _ in first if bf[n])


@pytest.mark.parametrize("seed", range(24))
def test_visits_random(engine, oracle_mod, kbgen_mod, tmp_path, seed):
    c = kbgen_mod.gen_random(7300 + seed, n_nodes=3 + seed % 13, n_jobs=5 + seed % 9, max_tasks=2 + seed % 12,
                             features=FEATURES)
    p = c.write(str(tmp_path / "r.kbs"))
    _HITS[seed] = _visits_case(engine, oracle_mod, p, len(c.nodes), len(c.pods))


def test_visits_reach_backfilled_nodes(engine, oracle_mod, kbgen_mod, tmp_path):
    """At least half of the seeds above visit a node with Backfilled != 0."""
    for seed in range(24):
        if seed not in _HITS:
            c = kbgen_mod.gen_random(7300 + seed, n_nodes=3 + seed % 13, n_jobs=5 + seed % 9,
                                     max_tasks=2 + seed % 12, features=FEATURES)
            _HITS[seed] = _visits_case(engine, oracle_mod, c.write(str(tmp_path / f"r{seed}.kbs")), len(c.nodes),
                                       len(c.pods))
    assert sum(1 for seed in range(24) if _HITS[seed] > 0) >= 12


def test_visits_c5_small(engine, oracle_mod, kbgen_mod, tmp_path):
    p = str(tmp_path / "c5.kbs")
    kbgen_mod.gen_c5(p, seed=kbgen_mod.BASE_SEED + 50, n_nodes=120, n_pending=150, best_effort=8)
    with engine.Session(p) as s:
        n_pods = len(s.table("pod_class"))
    assert _visits_case(engine, oracle_mod, p, 120, n_pods) > 0


def _per_pop(engine, oracle_mod, c, p, opts=None):
    """allocate.go's loop over kbhip_place_job; after every pop that stops
    unassigned, fit_deltas of its last task against numpy over sweep_scores
    (passing nodes), read_nodes (Idle) and the oracle's Resreq.  Returns the
    log and each job's deltas at its last pop (None: it did not stop unassigned)."""
    n_nodes, n_pods = len(c.nodes), len(c.pods)
    req = oracle_mod.ref_task_requests(p, n_pods).astype(np.int64)[:, 0:3]
    host = GoHost(c)
    last = {}
    with engine.Session(p) as s:
        for k, v in (opts or {}).items():
            s.set_option(k, v)

        def place_job(ids, gm, mn, ready):
            nodes, kinds, stop = s.place_job(ids, gm, mn, ready)
            job = host.pods[ids[0]]["job"]
            last[job] = None
            if stop == engine.STOP_UNASSIGNED:
                task = ids[len(nodes) - 1]
                node, delta = s.fit_deltas(task)
                n_pass, keys = s.sweep_scores(task, n_nodes)
                passing = np.nonzero(keys)[0]
                assert n_pass == passing.size
                assert np.array_equal(node, passing)  # ascending node index
                idle = s.read_nodes(n_nodes)[passing, 0:3]
                assert np.array_equal(delta, fit_delta(idle, req[task]))
                node2, delta2 = s.fit_deltas(task)  # read-only calls in between change nothing
                assert np.array_equal(node2, node) and np.array_equal(delta2, delta)
                last[job] = delta
            return nodes, kinds, stop
        log, _ = host.allocate(place_job)
    return log, last


@pytest.mark.parametrize("seed", range(8))
def test_fit_deltas_per_pop_random(engine, oracle_mod, kbgen_mod, tmp_path, seed):
    c = kbgen_mod.gen_random(7300 + seed, n_nodes=3 + seed % 13, n_jobs=5 + seed % 9, max_tasks=2 + seed % 12,
                             features=FEATURES)
    p = c.write(str(tmp_path / "r.kbs"))
    log, _ = _per_pop(engine, oracle_mod, c, p)
    assert log == oracle_mod.ref_allocate(p).as_list()


@pytest.mark.parametrize("eng", [1, 0])
def test_fit_error_text(engine, oracle_mod, kbgen_mod, tmp_path, eng):
    """JobInfo.FitError rebuilt from the last deltas of every job whose final
    pop stopped unassigned equals the gang plugin's close message of the
    faithful restatement."""
    c = crowded_gangs(kbgen_mod)
    p = c.write(str(tmp_path / "u.kbs"))
    log, last = _per_pop(engine, oracle_mod, c, p, {"engine": eng})
    assert log == oracle_mod.ref_allocate(p).as_list()
    close = oracle_mod.ref_gang_close(p)
    checked = 0
    for job, delta in last.items():
        if delta is None or job not in close:
            continue
        assert close[job].split(": ", 1)[1] == fit_error(delta), job
        checked += 1
    assert checked > 5


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 256, 257, 3001])
def test_compaction_edges(engine, kbgen_mod, tmp_path, n_nodes):
    """Every node passes and none fits: one record per node, in order, across
    wave (64), block (256) and multi-block boundaries."""
    c = uniform_oversized(kbgen_mod, n_nodes)
    p = c.write(str(tmp_path / "o.kbs"))
    with engine.Session(p) as s:
        pod, _, _ = s.allocate()
        assert pod.size == 0
        node, delta = s.fit_deltas(0)
        idle = s.read_nodes(n_nodes)[:, 0:3]
        msg = s.gang_unschedulable()["ns/big"]
    assert np.array_equal(node, np.arange(n_nodes))
    assert np.array_equal(delta, fit_delta(idle, np.array([64000, 2 * GI, 0])))
    assert (delta[:, 0] < 0).all() and (delta[:, 1] >= 0).all()
    assert msg.split(": ", 1)[1] == fit_error(delta) == f"0/{n_nodes} nodes are available, {n_nodes} insufficient cpu."


def test_compaction_no_node_passes(engine, kbgen_mod, tmp_path):
    c = uniform_oversized(kbgen_mod, 300, unsched=True)
    p = c.write(str(tmp_path / "n.kbs"))
    with engine.Session(p) as s:
        s.allocate()
        node, delta = s.fit_deltas(0)
        msg = s.gang_unschedulable()["ns/big"]
    assert node.size == 0 and delta.shape == (0, 3)
    assert msg.split(": ", 1)[1] == fit_error(delta) == "0 nodes are available"


def test_compaction_every_third_node(engine, kbgen_mod, tmp_path):
    n_nodes = 1000
    c = uniform_oversized(kbgen_mod, n_nodes, label_every=3, selector=True)
    p = c.write(str(tmp_path / "t.kbs"))
    with engine.Session(p) as s:
        s.allocate()
        node, delta = s.fit_deltas(0)
        idle = s.read_nodes(n_nodes)[:, 0:3]
    assert np.array_equal(node, np.arange(0, n_nodes, 3))
    assert np.array_equal(delta, fit_delta(idle[node], np.array([64000, 2 * GI, 0])))


def test_errors(engine, kbgen_mod, tmp_path):
    """One fitting job (task 0), one oversized job (task 1)."""
    c = kbgen_mod.Cluster()
    c.add_queue("q0", 1)
    for i in range(5):
        c.add_node(f"n{i}", 4000, 8 * GI, 0, 110)
    for j, cpu in enumerate((1000, 64000)):
        c.add_job("ns", f"j{j}", "q0", min_member=1, ts=j)
        c.add_pod("ns", f"j{j}-0", uid=f"p{j}", group=f"j{j}", ts=j, containers=[kbgen_mod.res(cpu=cpu, mem=GI)])
    p = c.write(str(tmp_path / "e.kbs"))
    einval, eunsup = "kbhip error -1", "kbhip error -3"
    with engine.Session(p) as s:
        with pytest.raises(engine.KbhipError, match=einval):  # no pop yet
            s.fit_deltas(1)
        nodes, _, stop = s.place_job([1], 1, 1, 0)
        assert stop == engine.STOP_UNASSIGNED and list(nodes) == [-1]
        assert s.fit_deltas(1)[0].size == 5
        with pytest.raises(engine.KbhipError, match=einval):  # another task
            s.fit_deltas(0)
        t = s.place_job_submit([0], 1, 1, 0)
        with pytest.raises(engine.KbhipError, match=einval):  # a ticket is outstanding
            s.fit_deltas(1)
        with pytest.raises(engine.KbhipError, match=einval):
            s.walk_visits()
        assert s.place_job_cancel(t) == 1
        assert s.fit_deltas(1)[0].size == 5  # the cancelled pop left the state as it was
        nodes, _, stop = s.place_job([0], 1, 1, 0)
        assert stop == engine.STOP_READY and nodes[0] >= 0
        with pytest.raises(engine.KbhipError, match=einval):  # a task that was placed
            s.fit_deltas(0)
        with pytest.raises(engine.KbhipError, match=einval):  # after a later place_job
            s.fit_deltas(1)
        assert _pairs(*s.walk_visits()) == []  # no Backfilled node: nothing is counted
    sh = engine.ShardedSession(p, 0, 0, 2)  # a shard handle: both calls are out of scope there
    try:
        with pytest.raises(engine.KbhipError, match=eunsup):
            sh.walk_visits()
        with pytest.raises(engine.KbhipError, match=eunsup):
            sh.fit_deltas(1)
    finally:
        sh.close()
