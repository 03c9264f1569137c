"""kbhip_apply_ops on the device: evictions and pipelines a host-driven
reclaim / preempt loop decided, applied to the session's host model and node
rows as the engine's own actions apply theirs.

The oracle is the faithful restatement (oracle.ref_allocate with node state),
as in tests/test_gpu_evict.py.  Reclaim has no statements, so its records are
the complete list of its operations: replaying them through apply_ops must
leave the node state the restatement has after "reclaim", and the actions run
afterwards on that session must produce the restatement's remaining records.

The replay cases are fixed here; they were chosen on the CPU with the
restatement alone (gen_preempt in the shapes of test_gpu_evict.py's random
snapshots: 4-13 nodes, the four tier layouts, features on and off, and the
pod-affinity variant) so that every case's reclaim evicts at least one pod.
Records use the restatement's TaskStatus codes: 8 Pipelined, 128 Releasing."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATUS = {1: 4, 2: 8, 3: 128}
EINVAL = "kbhip error -1"
FEATURES = ("selector", "taints", "ports", "init", "bestEffort", "unsched")
TIERS = [
    None,                                                          # shipped kube-batch-conf.yaml
    [["priority", "gang", "drf", "predicates", "proportion", "nodeorder"]],  # one tier: drf / proportion intersect
    [["drf", "predicates", "nodeorder"], ["gang", "proportion"]],
    [["priority", "conformance"], ["drf", "proportion", "predicates", "nodeorder"]],
]
TAIL = "allocate, backfill, preempt"
FULL = "reclaim, " + TAIL
# (pod affinity, seed, tier layout, features on): shape = test_gpu_evict.py's, by seed
CASES = [(0, 3, 0, 0), (0, 6, 0, 0), (0, 5, 0, 1), (0, 34, 1, 0), (0, 50, 1, 1), (0, 118, 1, 1), (0, 107, 2, 0),
         (0, 35, 2, 1), (0, 5, 3, 0), (0, 3, 3, 1), (0, 39, 3, 1),
         (1, 3, 0, 0), (1, 5, 0, 1), (1, 113, 1, 0), (1, 41, 2, 1), (1, 2, 3, 0), (1, 5, 3, 1)]


def _gen(kbgen, case):
    aff, seed, tier, feat = case
    c = kbgen.gen_preempt((1500 if aff else 500) + seed, n_nodes=4 + seed % 10, n_queues=1 + seed % 4,
                          n_run_jobs=4 + seed % 9, n_pend_jobs=2 + seed % 5, max_tasks=1 + seed % 6, tiers=TIERS[tier],
                          features=(("podaffinity",) if aff else ()) + (FEATURES if feat else ()))
    if aff and seed % 3 == 0:
        c.args = {"nodeorder": {"podaffinity.weight": str(1 + seed % 4)}}
    return c


@pytest.fixture(scope="module")
def refs(oracle_mod, kbgen_mod, tmp_path_factory):
    """case -> (snapshot path, reclaim records, node state after reclaim, the records of the
    actions after it, the final node state): computed once per case, never changed."""
    d = tmp_path_factory.mktemp("apply_ops")

    @functools.lru_cache(maxsize=None)
    def get(case):
        p = _gen(kbgen_mod, case).write(str(d / ("c%d_%d_%d_%d.kbs" % case)))
        rec, ns = oracle_mod.ref_allocate(p, actions="reclaim", with_nodes=True)
        full, nf = oracle_mod.ref_allocate(p, actions=FULL, with_nodes=True)
        rec, full = rec.as_list(), full.as_list()
        assert full[:len(rec)] == rec
        return p, rec, ns, full[len(rec):], nf

    # Properties of the fixed inputs, asserted for every test that replays them (no filtering at
    # run time): every case's reclaim evicts, at least a third hold a pipeline, at least two are
    # pod-affinity snapshots, and the shapes span 4-13 nodes, the four tier layouts and both
    # feature settings.
    recs = [get(c)[1] for c in CASES]
    assert all(any(k == 128 for _, _, k in r) for r in recs)
    assert 3 * sum(any(k == 8 for _, _, k in r) for r in recs) >= len(CASES)
    assert sum(c[0] for c in CASES) >= 2
    assert {c[2] for c in CASES} == {0, 1, 2, 3} and {c[3] for c in CASES} == {0, 1}
    assert {4 + c[1] % 10 for c in CASES} >= {4, 13}
    assert any(any(k == 128 for _, _, k in get(c)[3]) for c in CASES)  # the later preempt evicts too
    return get


def _ops(engine, rec):
    op = [engine.OP_EVICT if k == 128 else engine.OP_PIPELINE for _, _, k in rec]
    assert all(k in (8, 128) for _, _, k in rec)
    return op, [p for p, _, _ in rec], [n for _, n, _ in rec]


def _replay(engine, s, rec, single):
    """The records through apply_ops, as one batch or one operation per call; the launches per call."""
    op, pod, node = _ops(engine, rec)
    if not single:
        return [s.apply_ops(op, pod, node)]
    return [s.apply_ops([o], [p], [n]) for o, p, n in zip(op, pod, node)]


def _records(log):
    return [(int(p), int(n), STATUS[int(k)]) for p, n, k in zip(*log)]


def _same_nodes(ns, ons):
    return np.array_equal(ns.astype(np.float64), ons[:ns.shape[0]])


def _hand(kbgen, pend_queue, pend_min, second_running=False):
    GI = 1 << 30
    c = kbgen.Cluster()
    c.add_node("n0", 4000, 8 * GI, 0, 110)
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    c.add_job("ns1", "r0", "q0", min_member=1)
    c.add_pod("ns1", "r0-0", uid="a0", group="r0", node="n0", phase="Running", containers=[kbgen.res(cpu=4000, mem=GI)])
    if second_running:  # pod 1 (UID order); the pending pod becomes pod 2
        c.add_pod("ns1", "r0-1", uid="a1", group="r0", node="n0", phase="Running",
                  containers=[kbgen.res(mem=GI)])
    c.add_job("ns2", "p0", pend_queue, min_member=pend_min)
    c.add_pod("ns2", "p0-0", uid="b0", group="p0", priority=10, containers=[kbgen.res(cpu=2000, mem=GI)])
    return c


# ---- 1. known answers ---------------------------------------------------------
@pytest.mark.parametrize("single", [False, True], ids=["batch", "per_call"])
def test_known_reclaim(engine, oracle_mod, kbgen_mod, tmp_path, single):
    p = _hand(kbgen_mod, "q1", 1).write(str(tmp_path / "h.kbs"))
    exp, ons = oracle_mod.ref_allocate(p, actions="reclaim", with_nodes=True)
    assert exp.as_list() == [(0, 0, 128), (1, 0, 8)]
    with engine.Session(p) as s:
        launches = _replay(engine, s, exp.as_list(), single)
        assert _same_nodes(s.read_nodes(1), ons)
        st = s.table("pod_status")
        assert (int(st[0]), int(st[1])) == (128, 8) and int(s.table("pod_node")[1]) == 0
    assert all(1 <= x <= 2 for x in launches)


@pytest.mark.parametrize("single", [False, True], ids=["batch", "per_call"])
def test_known_discarded_preempt(engine, oracle_mod, kbgen_mod, tmp_path, single):
    """preempt's discarded statement: evict, pipeline, unpipeline, unevict.  The victim is
    Running again in the session while its node keeps the Releasing copy (statement.go:81-105)."""
    p = _hand(kbgen_mod, "q0", 1).write(str(tmp_path / "h.kbs"))
    exp, ons = oracle_mod.ref_allocate(p, actions="preempt", with_nodes=True)
    assert exp.as_list() == []
    assert ons[0, 6] == 4000  # the Releasing quirk is in the expected state
    op = [engine.OP_EVICT, engine.OP_PIPELINE, engine.OP_UNPIPELINE, engine.OP_UNEVICT]
    pod, node = [0, 1, 1, 0], [0, 0, 0, 0]
    with engine.Session(p) as s:
        if single:
            for o, q, n in zip(op, pod, node):
                s.apply_ops([o], [q], [n])
        else:
            s.apply_ops(op, pod, node)
        assert _same_nodes(s.read_nodes(1), ons)
        st = s.table("pod_status")
        assert (int(st[0]), int(st[1])) == (64, 1)
        assert s.rank_nodes(1, True)[0] == oracle_mod.ref_sweep_scores(p, 1, 1, "preempt")[0]
        # the node copy is Releasing: the pod is no victim candidate, for the host or the engine
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.apply_ops([engine.OP_EVICT], [0])
        assert _records(s.run_actions("preempt")) == []


# ---- 2. replay parity ---------------------------------------------------------
@pytest.mark.parametrize("single", [False, True], ids=["batch", "per_call"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_replay_parity(engine, refs, case, single):
    p, rec, ons, tail, onf = refs(case)
    with engine.Session(p) as s, engine.Session(p) as own:
        n_nodes = s.stats()["nodes"]
        launches = _replay(engine, s, rec, single)
        assert all(1 <= x <= 2 for x in launches)
        assert _same_nodes(s.read_nodes(n_nodes), ons)
        # the host model and the count tables as the engine's own reclaim leaves them
        assert _records(own.reclaim()) == rec
        for name in ("pod_status", "pod_node") + (("aff_cnt", "aff_scalar") if case[0] else ()):
            assert np.array_equal(s.table(name), own.table(name)), name
        assert _records(s.run_actions(TAIL)) == tail
        assert _same_nodes(s.read_nodes(n_nodes), onf)
        assert _records(own.run_actions(TAIL)) == tail
        assert s.gang_unschedulable() == own.gang_unschedulable()


def test_replay_then_carry(engine, refs):
    """A carry-over after a replay is the carry-over after the engine's own reclaim."""
    p, rec, _, _, _ = refs(CASES[9])
    with engine.Session(p) as s, engine.Session(p) as own:
        n_nodes = s.stats()["nodes"]
        _replay(engine, s, rec, False)
        own.reclaim()
        s.carry()
        own.carry()
        assert np.array_equal(s.read_nodes(n_nodes), own.read_nodes(n_nodes))
        assert np.array_equal(s.table("pod_status"), own.table("pod_status"))
        # operations do not reach across the carry-over: the evicted pods stay evicted
        ev = [q for q, _, k in rec if k == 128]
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.apply_ops([engine.OP_UNEVICT], ev[:1])
        assert _records(s.run_actions(FULL)) == _records(own.run_actions(FULL))
        assert np.array_equal(s.read_nodes(n_nodes), own.read_nodes(n_nodes))


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[9], CASES[11], CASES[16]],
                         ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_after_an_engine_action(engine, refs, case):
    """apply_ops after the engine's own reclaim, when the session holds the NodeInfo.Tasks lists that
    action built, and an eviction action after the call.  A pipeline undone by its unpipeline leaves
    what a session without the call has; a pipeline left in place leaves what it leaves on a session
    that got the same reclaim as a replay (which never held such lists)."""
    P, U = engine.OP_PIPELINE, engine.OP_UNPIPELINE
    p, rec, _, _, _ = refs(case)
    with engine.EncodedSnapshot(p) as enc:
        tasks = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
    with engine.Session(p) as s, engine.Session(p) as plain, engine.Session(p) as kept, \
            engine.Session(p) as replayed:
        n_nodes = s.stats()["nodes"]
        for x in (s, plain, kept):
            assert _records(x.reclaim()) == rec
        _replay(engine, replayed, rec, False)
        st = s.table("pod_status")
        pend = [t for t in tasks if st[t] == 1]
        assert pend
        ops, pods, nodes = [], [], []
        for i, t in enumerate(pend):  # each still-Pending task onto a node of its walk (else node i mod N)
            walk = s.rank_nodes(t, False)[1]
            ops += [P]
            pods += [t]
            nodes += [int(walk[0]) if walk.size else i % n_nodes]
        # pipelined and unpipelined again, in the statement's order (reverse)
        s.apply_ops(ops + [U] * len(pend), pods + pods[::-1], nodes + nodes[::-1])
        assert np.array_equal(s.read_nodes(n_nodes), plain.read_nodes(n_nodes))
        assert np.array_equal(s.table("pod_status"), plain.table("pod_status"))
        for name in (("aff_cnt", "aff_scalar") if case[0] else ()):
            assert np.array_equal(s.table(name), plain.table(name)), name
        assert _records(s.run_actions("preempt, reclaim")) == _records(plain.run_actions("preempt, reclaim"))
        assert np.array_equal(s.read_nodes(n_nodes), plain.read_nodes(n_nodes))
        assert np.array_equal(s.table("pod_status"), plain.table("pod_status"))
        # the pipelines left in place
        for x in (kept, replayed):
            x.apply_ops(ops, pods, nodes)
        assert np.array_equal(kept.read_nodes(n_nodes), replayed.read_nodes(n_nodes))
        got = _records(kept.run_actions("preempt, reclaim"))
        assert got == _records(replayed.run_actions("preempt, reclaim"))
        assert not any(q in pods for q, _, _ in got)  # no longer Pending: no action places them again
        assert np.array_equal(kept.read_nodes(n_nodes), replayed.read_nodes(n_nodes))
        for name in ("pod_status", "pod_node"):
            assert np.array_equal(kept.table(name), replayed.table(name)), name


# ---- 3. the ranking sees it ------------------------------------------------------
def _walk(keys):
    nz = np.nonzero(keys)[0]
    order = nz[np.argsort(keys[nz], kind="stable")[::-1]]  # the keys are distinct
    scores = (keys[order] >> np.uint64(32)).astype(np.int64) - 2 ** 31
    return order.astype(np.int32), scores.astype(np.int32), nz.astype(np.int32)


@pytest.mark.parametrize("case", [CASES[0], CASES[9], CASES[11], CASES[16]], ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_ranking_sees_the_operations(engine, refs, case):
    p, rec, _, _, _ = refs(case)
    piped = [q for q, _, k in rec if k == 8]
    assert piped
    with engine.EncodedSnapshot(p) as enc:
        tasks = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
    with engine.Session(p) as s, engine.Session(p) as own, engine.Session(p) as fresh:
        n_nodes = s.stats()["nodes"]
        _replay(engine, s, rec, False)
        own.reclaim()
        st = s.table("pod_status")
        pend = [t for t in tasks if st[t] == 1]
        assert pend
        for t in pend:
            total, keys = s.sweep_scores(t, n_nodes)
            nodes, scores, by_index = _walk(keys)
            assert total == nodes.size
            for by_score, e_n, e_s in ((True, nodes, scores), (False, by_index, np.zeros(by_index.size, np.int32))):
                for cap in (64, None):
                    got = s.rank_nodes(t, by_score, 0, cap)
                    ref = own.rank_nodes(t, by_score, 0, cap)
                    assert got[0] == ref[0] and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
                    assert got[0] == total
                    assert np.array_equal(got[1], e_n[:64] if cap else e_n)
                    assert np.array_equal(got[2], e_s[:64] if cap else e_s)
        # a pipelined task is not Pending: refused until it is unpipelined
        t = piped[-1]
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.rank_nodes(t, True)
        s.apply_ops([engine.OP_UNPIPELINE], [t])
        total, keys = s.sweep_scores(t, n_nodes)
        got = s.rank_nodes(t, True)
        assert got[0] == total and np.array_equal(got[1], _walk(keys)[0])
        # the walk counters are those of a session that never applied anything
        a, b = s.walk_visits(), fresh.walk_visits()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 4. kernel shapes ------------------------------------------------------------
def test_many_nodes_one_launch(engine, oracle_mod, kbgen_mod, tmp_path):
    """More distinct nodes than one block of the kernel holds (256), in one batch: the node
    state is the restatement's, in as many launches as a two-operation batch takes."""
    c = kbgen_mod.gen_preempt(700, n_nodes=600, n_queues=3, n_run_jobs=300, n_pend_jobs=120, max_tasks=6,
                              tiers=TIERS[3])
    p = c.write(str(tmp_path / "m.kbs"))
    exp, ons = oracle_mod.ref_allocate(p, actions="reclaim", with_nodes=True)
    rec = exp.as_list()
    assert len({n for _, n, _ in rec}) > 256 and len(rec) > 600
    hp = _hand(kbgen_mod, "q1", 1).write(str(tmp_path / "h.kbs"))
    with engine.Session(hp) as h:
        two = h.apply_ops([engine.OP_EVICT, engine.OP_PIPELINE], [0, 1], [0, 0])
    with engine.Session(p) as s, engine.Session(p) as one:
        big = _replay(engine, s, rec, False)
        assert big == [two] and two <= 2
        assert _same_nodes(s.read_nodes(600), ons)
        _replay(engine, one, rec, True)  # the same rows one operation per call
        assert np.array_equal(s.read_nodes(600), one.read_nodes(600))
        assert np.array_equal(s.table("pod_status"), one.table("pod_status"))


def _long_segment(kbgen):
    """One node with 100 Running pods, and 10 Pending tasks of one class with a host port."""
    GI = 1 << 30
    c = kbgen.Cluster()
    c.add_node("n0", 400000, 1024 * GI, 0, 500)
    c.add_node("n1", 400000, 1024 * GI, 0, 500)
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    c.add_job("ns1", "r0", "q0", min_member=1)
    for i in range(100):
        c.add_pod("ns1", "r0-%03d" % i, uid="a%03d" % i, group="r0", node="n0", phase="Running",
                  containers=[kbgen.res(cpu=100 + i, mem=GI + i)])
    c.add_job("ns2", "p0", "q1", min_member=1)
    for i in range(10):
        c.add_pod("ns2", "p0-%d" % i, uid="b%d" % i, group="p0", priority=10,
                  containers=[kbgen.res(cpu=2000, mem=GI, ports=[{"port": 8080}])])
    return c


def test_one_long_segment(engine, kbgen_mod, tmp_path):
    """100 evictions on one node with 8 pipelines and 8 unpipelines of a host-port class
    interleaved: one lane walks the whole segment; the row is the one the same operations
    leave one per call, and Releasing is the sum of the evicted requests."""
    E, P, U = engine.OP_EVICT, engine.OP_PIPELINE, engine.OP_UNPIPELINE
    p = _long_segment(kbgen_mod).write(str(tmp_path / "l.kbs"))
    pend = list(range(100, 110))
    seq = [(E, v) for v in range(100)]
    moves = [(P, pend[0])]
    for i in range(1, 8):  # P0 P1 U0 P2 U1 ... P7 U6 U7
        moves += [(P, pend[i]), (U, pend[i - 1])]
    moves.append((U, pend[7]))
    assert sum(o == P for o, _ in moves) == 8 and sum(o == U for o, _ in moves) == 8
    for k, m in enumerate(moves):  # spread through the evictions
        seq.insert(5 + 6 * k + k, m)
    op, pod = [o for o, _ in seq], [q for _, q in seq]
    node = [0] * len(seq)
    more = ([P, P, P, U], [pend[0], pend[1], pend[2], pend[1]], [0, 0, 1, 0])  # ends with pipelines in place
    with engine.Session(p) as s, engine.Session(p) as one:
        before = s.read_nodes(2)
        assert s.apply_ops(op, pod, node) <= 2
        for o, q, n in zip(op, pod, node):
            one.apply_ops([o], [q], [n])
        for step in range(2):
            rows, rows1 = s.read_nodes(2), one.read_nodes(2)
            assert np.array_equal(rows, rows1)
            assert np.array_equal(s.table("pod_status"), one.table("pod_status"))
            for t in (pend[8], pend[9]):  # pod count, non-zero requests and host ports, as the predicates and scores read them
                a, b = s.sweep_scores(t, 2), one.sweep_scores(t, 2)
                assert a[0] == b[0] and np.array_equal(a[1], b[1])
            if step == 0:
                exp = before.copy()
                exp[0, 6] += sum(100 + i for i in range(100))
                exp[0, 7] += sum((1 << 30) + i for i in range(100))
                assert np.array_equal(rows, exp)
                s.apply_ops(*more)
                for o, q, n in zip(*more):
                    one.apply_ops([o], [q], [n])
            else:
                exp[0, 3] += 2000  # Pipelined: Used grows, Releasing shrinks (node_info.go:113-145)
                exp[0, 4] += 1 << 30
                exp[0, 6] -= 2000
                exp[0, 7] -= 1 << 30
                exp[1, 3] += 2000
                exp[1, 4] += 1 << 30
                exp[1, 6] -= 2000
                exp[1, 7] -= 1 << 30
                assert np.array_equal(rows, exp)


# ---- 5. validation is atomic -----------------------------------------------------
def test_validation_is_atomic(engine, oracle_mod, kbgen_mod, tmp_path):
    E, P, U, UE = engine.OP_EVICT, engine.OP_PIPELINE, engine.OP_UNPIPELINE, engine.OP_UNEVICT
    p = _hand(kbgen_mod, "q1", 1, second_running=True).write(str(tmp_path / "v.kbs"))
    exp, ons = oracle_mod.ref_allocate(p, actions="reclaim", with_nodes=True)
    assert exp.as_list() == [(0, 0, 128), (2, 0, 8)]
    bad = [([E, P, UE], [0, 2, 1], [0, 0, 0]),      # unevict of a pod never evicted
           ([E, E], [0, 2], [0, 0]),                # evict of a Pending pod
           ([E, P], [0, 2], [0, 1]),                # pipeline onto node N
           ([E, P], [0, 2], [0, -1]),
           ([E, E], [0, 0], [0, 0]),                # against the statuses the batch itself leaves
           ([E, UE, E], [0, 0, 0], [0, 0, 0]),      # ... the node copy stays Releasing after an unevict
           ([E, P, P], [0, 2, 2], [0, 0, 0]),
           ([E, U], [0, 2], [0, 0]),                # unpipeline of a task never pipelined
           ([E, 9], [0, 1], [0, 0]),                # unknown operation
           ([E, E], [0, 3], [0, 0]), ([E, E], [0, -1], [0, 0])]  # pod out of range
    with engine.Session(p) as s:
        rows = s.read_nodes(1)
        walk = s.rank_nodes(2, True)
        status = s.table("pod_status")
        for op, pod, node in bad:
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.apply_ops(op, pod, node)
            assert np.array_equal(s.read_nodes(1), rows)
            assert np.array_equal(s.table("pod_status"), status)
            got = s.rank_nodes(2, True)
            assert got[0] == walk[0] and np.array_equal(got[1], walk[1]) and np.array_equal(got[2], walk[2])
        assert s.apply_ops([], []) == 0  # an empty batch: nothing done, nothing launched
        assert np.array_equal(s.read_nodes(1), rows)
        t = s.place_job_submit([2], 0, 1, 0)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.apply_ops([E], [0])
        s.place_job_cancel(t)
        assert np.array_equal(s.read_nodes(1), rows)
        # the refused batches left no trace: the valid one gives the restatement's state
        s.apply_ops([P, U, E, P], [2, 2, 0, 2], [0, 0, 0, 0])
        assert _same_nodes(s.read_nodes(1), ons)
