"""kbhip_rank_victim_nodes on the device: kbhip_rank_nodes' walk without the
nodes that can yield no victim set for the task.

The expected walk is restated here from the kbgen.Cluster: the walk
kbhip_rank_nodes gives on the same session, minus every node whose candidate
set (Running pods with a Running node copy, narrowed by queue / job for the
mode) is empty or whose candidates' Resreq sum is strictly below the task's
InitResreq in all three resources.  The candidate sets are kept by Model from
the pods' phase, node, job and queue and from the operations and records the
test itself applied (statement.go's evict / unevict / pipeline, and the carry
rules of tests/cachemodel.py snapshot_after_session: binds and evictions reach
the cache, the rest is session-only).

Status codes are the TaskStatus values kbhip_debug_table's pod_status gives:
1 Pending, 8 Pipelined, 64 Running, 128 Releasing."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GI = 1 << 30
EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"
PENDING, ALLOCATED, PIPELINED, BINDING, BOUND, RUNNING, RELEASING, GONE = 1, 4, 8, 16, 32, 64, 128, -1
STATUS = {1: 4, 2: 8, 3: 128}
FEATURES = ("selector", "taints", "ports", "init", "bestEffort", "unsched")
TIERS = [
    None,
    [["priority", "gang", "drf", "predicates", "proportion", "nodeorder"]],
    [["drf", "predicates", "nodeorder"], ["gang", "proportion"]],
    [["priority", "conformance"], ["drf", "proportion", "predicates", "nodeorder"]],
]
# the 17 snapshots of tests/test_gpu_apply_ops.py: (pod affinity, seed, tier layout, features on)
CASES = [(0, 3, 0, 0), (0, 6, 0, 0), (0, 5, 0, 1), (0, 34, 1, 0), (0, 50, 1, 1), (0, 118, 1, 1), (0, 107, 2, 0),
         (0, 35, 2, 1), (0, 5, 3, 0), (0, 3, 3, 1), (0, 39, 3, 1),
         (1, 3, 0, 0), (1, 5, 0, 1), (1, 113, 1, 0), (1, 41, 2, 1), (1, 2, 3, 0), (1, 5, 3, 1)]
# four of them whose reclaim pipelines at least two tasks (checked with the restatement on the CPU)
EXACT = [(0, 3, 0, 0), (0, 3, 3, 1), (0, 39, 3, 1), (1, 2, 3, 0)]


def _gen(kbgen, case):
    aff, seed, tier, feat = case
    c = kbgen.gen_preempt((1500 if aff else 500) + seed, n_nodes=4 + seed % 10, n_queues=1 + seed % 4,
                          n_run_jobs=4 + seed % 9, n_pend_jobs=2 + seed % 5, max_tasks=1 + seed % 6, tiers=TIERS[tier],
                          features=(("podaffinity",) if aff else ()) + (FEATURES if feat else ()))
    if aff and seed % 3 == 0:
        c.args = {"nodeorder": {"podaffinity.weight": str(1 + seed % 4)}}
    return c


class Model:
    """Per pod (canonical order: by UID): status, node, job, queue, Resreq, InitResreq and whether its
    node's copy stayed Releasing after an unevict."""

    def __init__(self, c):
        pods = sorted(c.pods, key=lambda q: q.uid)
        nodes = {n: i for i, n in enumerate(sorted(x.name for x in c.nodes))}
        jobs = {j.uid: i for i, j in enumerate(sorted(c.jobs, key=lambda j: j.uid))}
        jq = {j.uid: j.queue for j in c.jobs}
        queues = {q: i for i, q in enumerate(sorted(x.name for x in c.queues))}
        self.n_nodes = len(nodes)
        self.status, self.node, self.job, self.queue, self.req, self.ireq = [], [], [], [], [], []
        for q in pods:
            assert q.group is not None and not q.detached
            if q.phase == "Running":
                st = RELEASING if q.deleting else RUNNING
            elif q.phase == "Pending":
                st = RELEASING if q.deleting else (BOUND if q.node else PENDING)
            else:
                st = 0
            self.status.append(st)
            self.node.append(nodes[q.node] if q.node else -1)
            uid = "%s/%s" % (q.ns, q.group)
            self.job.append(jobs[uid])
            self.queue.append(queues.get(jq[uid], -1))
            r = [sum(x.get(k, 0) for x in q.containers) for k in ("cpu", "mem", "gpu")]
            self.req.append(r)
            self.ireq.append([max([r[i]] + [x.get(k, 0) for x in q.init_containers])
                              for i, k in enumerate(("cpu", "mem", "gpu"))])
        self.node_rel = [False] * len(pods)

    # statement.go / session.go, as kbhip_apply_ops applies them
    def evict(self, p):
        assert self.status[p] == RUNNING and not self.node_rel[p]
        self.status[p] = RELEASING

    def unevict(self, p):
        self.status[p], self.node_rel[p] = RUNNING, True

    def pipeline(self, p, n):
        self.status[p], self.node[p] = PIPELINED, n

    def unpipeline(self, p):
        self.status[p] = PENDING

    def records(self, rec):
        """Records of an action (pod, node, TaskStatus code): 128 evicted, 8 pipelined, 4 allocated."""
        for p, n, k in rec:
            if k == 128:
                self.evict(p)
            elif k == 8:
                self.pipeline(p, n)
            else:
                self.status[p], self.node[p] = ALLOCATED, n

    def carry(self, events=()):
        """kbhip_session_carry(_events): binds and evictions stay, Allocated / Pipelined tasks are Pending
        again, every node copy is its pod's again; then the cache events on existing pods."""
        for p, st in enumerate(self.status):
            if st in (ALLOCATED, PIPELINED, 2, BINDING):
                self.status[p], self.node[p] = PENDING, -1
            self.node_rel[p] = False
        for p, ev in events:
            self.status[p] = GONE if ev == 1 else 0
            if ev == 1:
                self.node[p] = -1

    def cands(self, task, mode):
        """node -> [count, cpu, memory, gpu] of the candidates the mode's loop filters for."""
        out = {}
        for p, st in enumerate(self.status):
            if st != RUNNING or self.node_rel[p] or self.node[p] < 0 or self.queue[p] < 0:
                continue
            same_q, same_j = self.queue[p] == self.queue[task], self.job[p] == self.job[task]
            if (mode == 1 and same_q) or (mode == 2 and (not same_q or same_j)) or (mode == 3 and not same_j):
                continue
            e = out.setdefault(self.node[p], [0, 0, 0, 0])
            e[0] += 1
            for k in range(3):
                e[1 + k] += self.req[p][k]
        return out

    def kept(self, task, mode):
        need = self.ireq[task]
        return {n: e[0] for n, e in self.cands(task, mode).items()
                if e[0] > 0 and not all(e[1 + k] < need[k] for k in range(3))}


def _expect(s, m, task, by_score, mode):
    _, nodes, scores = s.rank_nodes(task, by_score)
    kept = m.kept(task, mode)
    sel = [i for i, n in enumerate(nodes.tolist()) if n in kept]
    return nodes[sel], scores[sel], np.array([kept[int(n)] for n in nodes[sel]], np.int32)


def _same(got, exp, lo=0, hi=None):
    total, n, sc, cd = got[:4]
    e_n, e_s, e_c = exp
    assert total == e_n.size, (total, e_n.size)
    assert np.array_equal(n, e_n[lo:hi]), (n, e_n[lo:hi])
    assert np.array_equal(sc, e_s[lo:hi])
    assert np.array_equal(cd, e_c[lo:hi]), (cd, e_c[lo:hi])


def _check_task(s, m, task, modes=(1, 2, 3), rebuilt=None):
    """Both orders and the given modes, the full path and the head, against the restatement."""
    for by_score in (True, False):
        for mode in modes:
            exp = _expect(s, m, task, by_score, mode)
            full = s.rank_victim_nodes(task, by_score, mode, 0, max(m.n_nodes, 65))  # first + cap > 64: the full path
            _same(full, exp)
            assert full[4]["head"] == 0 and full[4]["launches"] >= 7
            assert s.rank_victim_nodes(task, by_score, mode, 0, 0)[0] == exp[0].size  # the size query
            if rebuilt is not None:
                assert full[4]["rebuilt"] == rebuilt, (task, by_score, mode)
                rebuilt = 0
            head = s.rank_victim_nodes(task, by_score, mode, 0, 64)
            _same(head, exp, 0, 64)
            assert head[4] == {"head": 1, "rebuilt": 0, "launches": head[4]["launches"]}
            assert 3 <= head[4]["launches"] <= 5


def _pending(engine, s, path):
    with engine.EncodedSnapshot(path) as enc:
        tasks = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
    st = s.table("pod_status")
    return [t for t in tasks if st[t] == PENDING]


def _model_matches(s, m):
    """The restatement's Running / Releasing / Pending pods are the session's."""
    st = s.table("pod_status")
    for code in (RUNNING, RELEASING, PENDING):
        assert [p for p, x in enumerate(m.status) if x == code] == np.nonzero(st == code)[0].tolist(), code


def _records(log):
    return [(int(p), int(n), STATUS[int(k)]) for p, n, k in zip(*log)]


@pytest.fixture(scope="module")
def snaps(oracle_mod, kbgen_mod, tmp_path_factory):
    """case -> (snapshot path, the restatement's reclaim records, the cluster): computed once, never changed."""
    d = tmp_path_factory.mktemp("victims")

    @functools.lru_cache(maxsize=None)
    def get(case):
        c = _gen(kbgen_mod, case)
        p = c.write(str(d / ("c%d_%d_%d_%d.kbs" % case)))
        return p, oracle_mod.ref_allocate(p, actions="reclaim").as_list(), c

    return get


# ---- 1. parity on the gen_preempt snapshots -----------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_parity(engine, kbgen_mod, snaps, case):
    """Every Pending task, the three modes, both orders: as opened (the first call builds the table),
    and after the restatement's reclaim went through apply_ops (no rebuild)."""
    p, rec, c = snaps(case)
    E, P = engine.OP_EVICT, engine.OP_PIPELINE
    with engine.Session(p) as s:
        m = Model(c)
        _model_matches(s, m)
        todo = _pending(engine, s, p)
        assert todo
        for i, t in enumerate(todo):
            _check_task(s, m, t, rebuilt=1 if i == 0 else 0)
        assert s.apply_ops([E if k == 128 else P for _, _, k in rec], [q for q, _, _ in rec],
                           [n for _, n, _ in rec]) <= 2
        m.records(rec)
        _model_matches(s, m)
        for t in _pending(engine, s, p):
            _check_task(s, m, t, rebuilt=0)


# ---- 2. boundaries -------------------------------------------------------------
def _uniform(kbgen, n_nodes, kept):
    """n_nodes equal nodes, one Pending task of queue q0; one Running pod of queue q1 on every node with
    n % 3 == 0 ("third"), on every node ("all"), or of the task's own queue on every third node ("none")."""
    c = kbgen.Cluster()
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    for i in range(n_nodes):
        c.add_node("n%05d" % i, 8000, 16 * GI, 0, 110)
    c.add_job("ns", "run", "q0" if kept == "none" else "q1", min_member=1)
    for i in range(n_nodes):
        if kept == "all" or i % 3 == 0:
            c.add_pod("ns", "run-%05d" % i, uid="a%05d" % i, group="run", node="n%05d" % i, phase="Running",
                      containers=[kbgen.res(cpu=1000 + (i % 5) * 500, mem=GI)])
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    c.add_pod("ns", "pend-0", uid="p00000", group="pend", priority=5, ts=1, containers=[kbgen.res(cpu=1000, mem=GI)])
    return c


SHAPES = [(n, "third") for n in (1, 63, 64, 65, 255, 256, 257, 3001)] + \
         [(n, k) for k in ("none", "all") for n in (64, 257, 3001)]


@pytest.mark.parametrize("n_nodes,kept", SHAPES, ids=lambda v: str(v))
def test_boundaries(engine, kbgen_mod, tmp_path, n_nodes, kept):
    c = _uniform(kbgen_mod, n_nodes, kept)
    p = c.write(str(tmp_path / "u.kbs"))
    m = Model(c)
    task = len(c.pods) - 1  # "p00000" sorts after the running pods' "a....."
    assert m.status[task] == PENDING
    n_kept = {"third": (n_nodes + 2) // 3, "none": 0, "all": n_nodes}[kept]
    with engine.Session(p) as s:
        for radix in (0, 1):
            s.set_option("rank_radix", radix)
            for by_score in (True, False):
                exp = _expect(s, m, task, by_score, 1)
                assert exp[0].size == n_kept and s.rank_nodes(task, by_score, 0, 0)[0] == n_nodes
                if kept == "third":
                    assert all(int(n) % 3 == 0 for n in exp[0])
                full = s.rank_victim_nodes(task, by_score, 1, 0, max(n_nodes, 65))
                _same(full, exp)
                assert full[4]["head"] == 0
                total = full[0]
                size = s.rank_victim_nodes(task, by_score, 1, 0, 0)  # the size query
                assert size[0] == total and size[1].size == 0 and size[4]["head"] == 0
                for first, cap in ((0, 64), (1, 63), (0, 65), (60, 10), (max(total - 3, 0), 10), (total, 5)):
                    got = s.rank_victim_nodes(task, by_score, 1, first, cap)
                    _same(got, exp, first, first + cap)
                    assert got[4]["head"] == (1 if first + cap <= 64 else 0), (first, cap)
                    if first + cap <= 64:  # the full path serves the same window: both agree
                        wide = s.rank_victim_nodes(task, by_score, 1, 0, 65)
                        assert wide[4]["head"] == 0
                        assert np.array_equal(wide[1][first:first + cap], got[1])
                        assert np.array_equal(wide[2][first:first + cap], got[2])
                        assert np.array_equal(wide[3][first:first + cap], got[3])


# ---- 3. the strict-less rule ---------------------------------------------------
def _strict(kbgen):
    c = kbgen.Cluster()
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    for i in range(6):
        c.add_node("n%d" % i, 16000, 64 * GI, 8000, 110)
    c.add_job("ns", "run", "q1", min_member=1)
    # candidate sums per node against the request cpu 2000, memory 2 Gi, gpu 1000
    sums = {0: [(2000, GI, 0)],                    # equal in cpu only, below in the other two: kept
            1: [(1000, GI, 0)],                    # below in all three: dropped
            2: [(500, 2 * GI, 500)],               # equal in memory only: kept
            3: [(1000, GI, 500), (500, GI // 2, 500)],  # two pods: gpu adds up to the request, cpu / memory below: kept
            4: [(1000, GI, 0), (500, GI // 2, 900)]}    # two pods, every sum below: dropped
    k = 0                                               # node 5: no candidate: dropped
    for n, pods in sums.items():
        for cpu, mem, gpu in pods:
            c.add_pod("ns", "run-%d" % k, uid="a%02d" % k, group="run", node="n%d" % n, phase="Running",
                      containers=[kbgen.res(cpu=cpu, mem=mem, gpu=gpu)])
            k += 1
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    c.add_pod("ns", "pend-0", uid="p0", group="pend", priority=5, ts=1,
              containers=[kbgen.res(cpu=2000, mem=2 * GI, gpu=1000)])
    c.add_pod("ns", "pend-1", uid="p1", group="pend", priority=5, ts=1, containers=[kbgen.res(cpu=64000, mem=64 * GI)])
    # InitResreq, not Resreq, is compared: an init container lifts the cpu request above node 0's sum
    c.add_pod("ns", "pend-2", uid="p2", group="pend", priority=5, ts=1,
              containers=[kbgen.res(cpu=2000, mem=2 * GI, gpu=1000)],
              init_containers=[kbgen.res(cpu=2001, mem=GI)])
    return c


def test_strict_less_rule(engine, kbgen_mod, tmp_path):
    c = _strict(kbgen_mod)
    p = c.write(str(tmp_path / "s.kbs"))
    m = Model(c)
    t_gpu, t_nogpu, t_init = len(c.pods) - 3, len(c.pods) - 2, len(c.pods) - 1
    with engine.Session(p) as s:
        for by_score in (True, False):
            for cap in (64, None):
                got = s.rank_victim_nodes(t_gpu, by_score, 1, 0, cap)
                assert sorted(got[1].tolist()) == [0, 2, 3]
                assert dict(zip(got[1].tolist(), got[3].tolist())) == {0: 1, 2: 1, 3: 2}
                # no gpu request: no sum is below it, so every node with a candidate stays
                got = s.rank_victim_nodes(t_nogpu, by_score, 1, 0, cap)
                assert sorted(got[1].tolist()) == [0, 1, 2, 3, 4]
                got = s.rank_victim_nodes(t_init, by_score, 1, 0, cap)
                assert sorted(got[1].tolist()) == [2, 3]
        for t in (t_gpu, t_nogpu, t_init):
            _check_task(s, m, t, modes=(1,))


# ---- 4. modes 2 and 3 ----------------------------------------------------------
def _jobs(kbgen, n_nodes=100):
    """Queue q0: job "one" (Running on node 7 only), job "wide" (Running on 70 nodes, three tasks on node 0,
    tasks on the first and the last node), job "other"; queue q1: job "far".  "one" and "wide" each have a
    Pending task."""
    c = kbgen.Cluster()
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    for i in range(n_nodes):
        c.add_node("n%03d" % i, 32000, 64 * GI, 0, 110)
    k = [0]

    def run(job, node, cpu):
        c.add_pod("ns", "%s-r%d" % (job, k[0]), uid="a%04d" % k[0], group=job, node="n%03d" % node, phase="Running",
                  containers=[kbgen.res(cpu=cpu, mem=GI)])
        k[0] += 1
    for job, q in (("one", "q0"), ("wide", "q0"), ("other", "q0"), ("far", "q1")):
        c.add_job("ns", job, q, min_member=1)
    run("one", 7, 3000)
    for n in [0, 0, 0] + list(range(1, 68)) + [n_nodes - 2, n_nodes - 1]:
        run("wide", n, 500 + (n % 4) * 500)
    for n in range(0, n_nodes, 2):
        run("other", n, 1000)
    for n in range(0, n_nodes, 5):
        run("far", n, 4000)
    c.add_pod("ns", "one-p", uid="p0", group="one", priority=5, ts=1, containers=[kbgen.res(cpu=2000, mem=GI)])
    # (a gpu request, so that the sum test can drop nodes: cpu 1500 against the own pods' 500 .. 2000)
    c.add_pod("ns", "wide-p", uid="p1", group="wide", priority=5, ts=1,
              containers=[kbgen.res(cpu=1500, mem=2 * GI, gpu=1000)])
    return c


@pytest.mark.parametrize("radix", [0, 1])
def test_modes_same_queue_and_same_job(engine, kbgen_mod, tmp_path, radix):
    c = _jobs(kbgen_mod)
    p = c.write(str(tmp_path / "j.kbs"))
    m = Model(c)
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    assert len(m.cands(t_one, 3)) == 1 and len(m.cands(t_wide, 3)) == 70 and m.cands(t_wide, 3)[0][0] == 3
    assert {0, 99} <= set(m.kept(t_wide, 3)) and len(m.kept(t_wide, 3)) < 70  # the sum test bites in mode 3 too
    with engine.Session(p) as s:
        s.set_option("rank_radix", radix)
        for t in (t_one, t_wide):
            _check_task(s, m, t)
        assert s.rank_victim_nodes(t_one, True, 3)[1].tolist() == [7]
        # evictions of the job's own tasks reach the own list as well as the table
        own0 = [q for q in range(len(c.pods)) if m.job[q] == m.job[t_wide] and m.node[q] == 0 and m.status[q] == RUNNING]
        assert len(own0) == 3
        s.apply_ops([engine.OP_EVICT] * 3, own0)
        for q in own0:
            m.evict(q)
        assert 0 not in m.kept(t_wide, 3)
        for t in (t_one, t_wide):
            _check_task(s, m, t, rebuilt=0)


# ---- 5. the table follows kbhip_apply_ops --------------------------------------
def test_table_follows_apply_ops(engine, kbgen_mod, tmp_path):
    E, P, U, UE = engine.OP_EVICT, engine.OP_PIPELINE, engine.OP_UNPIPELINE, engine.OP_UNEVICT
    c = _jobs(kbgen_mod, 600)  # more distinct nodes in one batch than one block of the apply kernel holds
    p = c.write(str(tmp_path / "a.kbs"))
    m = Model(c)
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    with engine.Session(p) as s:
        first = s.rank_victim_nodes(t_one, False, 1, 0, 64)
        assert first[4]["rebuilt"] == 1 and 10 in first[1].tolist()
        # every candidate of node 10 (queue q1's pod, for a task of q0)
        vict = [q for q in range(len(c.pods)) if m.node[q] == 10 and m.queue[q] != m.queue[t_one]
                and m.status[q] == RUNNING]
        assert vict
        assert s.apply_ops([E] * len(vict), vict) <= 2
        for q in vict:
            m.evict(q)
        got = s.rank_victim_nodes(t_one, False, 1, 0, 64)
        assert got[4]["rebuilt"] == 0 and 10 not in got[1].tolist()
        _check_task(s, m, t_one, rebuilt=0)
        # unevict: Running again, but the node keeps the Releasing copy: not a candidate
        assert s.apply_ops([UE] * len(vict), vict) <= 2
        for q in vict:
            m.unevict(q)
        got = s.rank_victim_nodes(t_one, False, 1)
        assert got[4]["rebuilt"] == 0 and 10 not in got[1].tolist()
        # a refused batch (its second operation evicts a Pending task) leaves the walk as it is
        other = [q for q in range(len(c.pods)) if m.node[q] == 20 and m.status[q] == RUNNING]
        before = s.rank_victim_nodes(t_one, True, 1)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.apply_ops([E, E], [other[0], t_wide])
        after = s.rank_victim_nodes(t_one, True, 1)
        assert after[4]["rebuilt"] == 0 and after[0] == before[0]
        assert all(np.array_equal(a, b) for a, b in zip(before[1:4], after[1:4]))
        # one batch over every node: evictions of several queues on one node, pipelines in between
        every = [q for q in range(len(c.pods)) if m.status[q] == RUNNING and not m.node_rel[q] and m.node[q] % 2 == 0]
        assert len({m.node[q] for q in every}) > 256 and len({m.queue[q] for q in every}) == 2
        ops, pods, nodes = [E] * len(every), list(every), [0] * len(every)
        ops[5:5] = [P, U, P]
        pods[5:5] = [t_wide, t_wide, t_wide]
        nodes[5:5] = [4, 4, 6]
        assert s.apply_ops(ops, pods, nodes) <= 2
        for q in every:
            m.evict(q)
        m.pipeline(t_wide, 6)
        _model_matches(s, m)
        _check_task(s, m, t_one, rebuilt=0)
        with pytest.raises(engine.KbhipError, match=EINVAL):  # a Pipelined task is not Pending
            s.rank_victim_nodes(t_wide, True, 2)
        s.apply_ops([U], [t_wide])
        m.unpipeline(t_wide)
        _check_task(s, m, t_wide, rebuilt=0)


# ---- 6. the table follows everything else --------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[9], CASES[15]], ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_table_follows_actions_and_carries(engine, kbgen_mod, snaps, case):
    p, _, c = snaps(case)
    with engine.Session(p) as s:
        m = Model(c)
        todo = _pending(engine, s, p)
        _check_task(s, m, todo[0], rebuilt=1)
        checked = 0
        for step in ("reclaim", "allocate", "carry", "carry_events"):
            if step == "reclaim":
                m.records(_records(s.reclaim()))
            elif step == "allocate":
                m.records(_records(s.allocate()))
            elif step == "carry":
                s.carry()
                m.carry()
            else:  # one Running pod deleted, one succeeded
                run = [q for q, st in enumerate(m.status) if st == RUNNING]
                assert len(run) >= 2
                ev = [(run[0], engine.EV_DELETE), (run[-1], engine.EV_SUCCEEDED)]
                s.carry_events([q for q, _ in ev], [e for _, e in ev])
                m.carry(ev)
            st = s.table("pod_status")
            assert [q for q, x in enumerate(m.status) if x == RUNNING] == np.nonzero(st == RUNNING)[0].tolist(), step
            todo = _pending(engine, s, p)
            for i, t in enumerate(todo):
                _check_task(s, m, t, rebuilt=1 if i == 0 else 0)
                checked += 1
        assert checked


def test_place_job_and_first_fit_leave_the_table_stale(engine, kbgen_mod, tmp_path):
    c = _jobs(kbgen_mod)
    p = c.write(str(tmp_path / "f.kbs"))
    m = Model(c)
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    with engine.Session(p) as s:
        assert s.rank_victim_nodes(t_one, True, 1, 0, 64)[4]["rebuilt"] == 1
        assert s.rank_victim_nodes(t_one, True, 1, 0, 64)[4]["rebuilt"] == 0
        s.place_job([t_wide], 0, 1, 0)
        assert s.rank_victim_nodes(t_one, True, 1, 0, 64)[4]["rebuilt"] == 1
        s.carry()
        assert s.rank_victim_nodes(t_one, True, 1, 0, 64)[4]["rebuilt"] == 1
        assert s.first_fit([t_wide])[0] >= 0
        got = s.rank_victim_nodes(t_one, True, 1, 0, 64)
        assert got[4]["rebuilt"] == 1
        _same(got, _expect(s, m, t_one, True, 1), 0, 64)


# ---- 7. exactness against the engine's own reclaim -----------------------------
@pytest.mark.parametrize("case", EXACT, ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_reclaim_pipelines_only_onto_walk_nodes(engine, snaps, case):
    """Every node kbhip_reclaim pipelines a task onto is in the pruned walk of that task, taken on the
    state before the evictions on that node that made room for it."""
    p, _, _ = snaps(case)
    E, P = engine.OP_EVICT, engine.OP_PIPELINE
    with engine.Session(p) as own, engine.Session(p) as s:
        rec = _records(own.reclaim())
        piped = [i for i, (_, _, k) in enumerate(rec) if k == 8]
        assert piped
        done = 0
        for i in piped:
            task, node, _ = rec[i]
            j = i
            while j > done and rec[j - 1][2] == 128 and rec[j - 1][1] == node:
                j -= 1
            assert j < i  # reclaim evicted on the node before it pipelined
            if j > done:
                part = rec[done:j]
                s.apply_ops([E if k == 128 else P for _, _, k in part], [q for q, _, _ in part],
                            [n for _, n, _ in part])
            for cap in (64, None):
                total, walk, _, cands, info = s.rank_victim_nodes(task, False, 1, 0, cap)
                assert node in walk.tolist(), (i, task, node)
                assert cands[walk.tolist().index(node)] >= i - j
            part = rec[j:i + 1]
            s.apply_ops([E if k == 128 else P for _, _, k in part], [q for q, _, _ in part], [n for _, n, _ in part])
            done = i + 1
        part = rec[done:]  # evictions that ended in no pipeline
        assert all(k == 128 for _, _, k in part)
        s.apply_ops([E] * len(part), [q for q, _, _ in part])
        assert np.array_equal(s.table("pod_status")[[q for q, _, _ in rec]],
                              own.table("pod_status")[[q for q, _, _ in rec]])


# ---- 8. kbhip_rank_nodes is unchanged; errors ----------------------------------
def test_rank_nodes_unchanged(engine, kbgen_mod, snaps):
    p, _, _ = snaps(CASES[2])
    with engine.Session(p) as s, engine.Session(p) as twin:
        n_nodes = s.stats()["nodes"]
        t = _pending(engine, s, p)[0]
        rows = s.read_nodes(n_nodes)
        for by_score in (True, False):
            for cap in (64, None):
                a = s.rank_nodes(t, by_score, 0, cap)
                for mode in (1, 2, 3):
                    s.rank_victim_nodes(t, by_score, mode, 0, cap)
                b = s.rank_nodes(t, by_score, 0, cap)
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert np.array_equal(s.read_nodes(n_nodes), rows)
        a, b = s.walk_visits(), twin.walk_visits()  # the walk counters of a session without the calls
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_errors(engine, kbgen_mod, tmp_path):
    c = _jobs(kbgen_mod)
    p = c.write(str(tmp_path / "e.kbs"))
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    with engine.Session(p) as s:
        for victims in (0, 4, -1):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.rank_victim_nodes(t_one, True, victims, 0, 64)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.rank_victim_nodes(t_one, 2, 1, 0, 64)  # by_score outside {0, 1}
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.rank_victim_nodes(0, True, 1, 0, 64)  # a Running pod: no task class
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.rank_victim_nodes(len(c.pods), True, 1, 0, 64)
        t = s.place_job_submit([t_wide], 0, 1, 0)
        with pytest.raises(engine.KbhipError, match=EINVAL):  # a ticket is outstanding
            s.rank_victim_nodes(t_one, True, 1, 0, 64)
        assert s.place_job_cancel(t) == 1
        assert s.rank_victim_nodes(t_one, True, 1, 0, 64)[0] > 0
    sh = engine.ShardedSession(p, 0, 0, 2)
    try:
        for cap in (64, None):
            with pytest.raises(engine.KbhipError, match=EUNSUP):
                sh.rank_victim_nodes(t_one, True, 1, 0, cap)
    finally:
        sh.close()
