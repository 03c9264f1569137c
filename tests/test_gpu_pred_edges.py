"""Predicates, fit and FitDelta at their thresholds on every device path
that evaluates them.

The snapshots of tests/prededges.py (req - avail at eps - 1 / eps / eps + 1 per
resource and source, pods at maxtasks, 131 taints = three taint words, 340
port triples = six port words with class windows cut to one word, label values
that parse, overflow or do not parse, gangs crossing a threshold under their
own placements; 1 to 1200 nodes) run through kbhip_sweep_scores under every
sweep_variant, kbhip_first_fit, kbhip_rank_nodes (head, full, offset; bucket
and radix), kbhip_rank_victim_nodes, kbhip_rank_heads, kbhip_place_job with
kbhip_fit_deltas, and the allocate action (batched and per-task, engine on and
off) with kbhip_read_nodes, kbhip_walk_visits and kbhip_gang_unschedulable.
Expected keys, walks and deltas come from the plain-Python reference
(prededges.Model; tests/test_pred_edges.py holds it against the faithful
restatement), whole sessions from the faithful restatement; never from another
device path.
"""
import numpy as np
import pytest

import prededges as pe
from test_gpu_pertask_abi import _variant
from test_shard import _shard_case

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in pe.CASES]
SIZE = {c[0]: c[2] for c in pe.CASES}
STATUS = {1: 4, 2: 8}


@pytest.fixture(scope="module")
def cases(kbgen_mod, tmp_path_factory):
    return pe.write_cases(kbgen_mod, tmp_path_factory.mktemp("pred_edges"))


def _tasks(snap):
    """Every task of a static case; of an allocate case the first of each job (the rest are identical)."""
    return [v[0] for v in snap.jobs.values()] if snap.kind == "cross" else list(range(len(snap.tasks)))


@pytest.fixture(scope="module")
def expected(cases):
    """{name: {task: (keys, walk, passing nodes, victim-walk mask)}} of the reference at open, computed once."""
    out = {}
    for name, (snap, _) in cases.items():
        m = snap.model()
        out[name] = {}
        for j in _tasks(snap):
            nodes, scores = m.walk(j)
            # kbhip_rank_victim_nodes drops nodes without a Running candidate of another queue
            # and nodes whose candidates are short of InitResreq in all three resources
            keep = np.array([not snap.rows[n]["pod"].get("deleting") and
                             not all(snap.rows[n]["pod"].get(r, 0) < q for r, q in zip(pe.RES, snap.tasks[j]["ireq"]))
                             for n in nodes], bool)
            out[name][j] = (m.expected_keys(j), (nodes, scores), m.passing(j), keep)
    return out


@pytest.fixture(scope="module")
def sessions(oracle_mod, cases):
    """{name: (log, node state, gang messages)} of the faithful restatement's allocate, computed once."""
    out = {}
    for name, (snap, path) in cases.items():
        pl, nstate = oracle_mod.ref_allocate(path, with_nodes=True)
        out[name] = (pl.as_list(), nstate[: len(snap.rows)].astype(np.int64), oracle_mod.ref_gang_close(path))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_sweep_scores_every_variant(engine, cases, expected, name):
    """k_score_sweep<PLAIN> at each TB x NPT (variants 0-3) and k_score_sweep_gs (4-6)."""
    snap, path = cases[name]
    n = len(snap.rows)
    with engine.Session(path) as s:
        for v in range(7):
            with _variant(s, v):
                for j, (exp, _, _, _) in expected[name].items():
                    cnt, keys = s.sweep_scores(snap.tasks[j]["pod"], n)
                    bad = np.nonzero(keys != exp)[0]
                    assert cnt == np.count_nonzero(exp) and bad.size == 0, (
                        v, j, [(int(b), snap.family(int(b)), hex(int(keys[b])), hex(int(exp[b]))) for b in bad[:4]])


@pytest.mark.parametrize("name", NAMES)
def test_first_fit(engine, cases, name):
    """eval_first_fit: the lowest passing index per task; the call places the
    task there (Session.Allocate), so the reference commits it too and the next
    task meets the changed pod counts and host ports."""
    snap, path = cases[name]
    m = snap.model()
    with engine.Session(path) as s:
        for j in _tasks(snap):
            exp = m.first_fit(j)
            got = int(s.first_fit([snap.tasks[j]["pod"]])[0])
            assert got == exp, (j, got, exp)
            if exp >= 0:
                m.commit(j, exp, pe.ALLOCATED)


@pytest.mark.parametrize("radix", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_rank_nodes(engine, cases, expected, name, radix):
    """rank_head (first + cap <= 64) and the full sort, by score and by index;
    on the 1200-node cases also a window that starts past the passing count."""
    snap, path = cases[name]
    n = len(snap.rows)
    with engine.Session(path) as s:
        s.set_option("rank_radix", radix)
        for j, (_, (e_nodes, e_scores), passing, _) in expected[name].items():
            pod, tot = snap.tasks[j]["pod"], passing.size
            for by_score, en, es in ((True, e_nodes, e_scores), (False, passing, np.zeros(tot, np.int32))):
                t, nodes, scores = s.rank_nodes(pod, by_score, 0, 64)
                assert t == tot and np.array_equal(nodes, en[:64]) and np.array_equal(scores, es[:64]), (j, by_score)
                t, nodes, scores = s.rank_nodes(pod, by_score, 0, max(n, 65))
                assert t == tot and np.array_equal(nodes, en) and np.array_equal(scores, es), (j, by_score)
                t, nodes, scores = s.rank_nodes(pod, by_score, 3, 61)
                assert t == tot and np.array_equal(nodes, en[3:64]) and np.array_equal(scores, es[3:64]), (j, by_score)
                t, nodes, scores = s.rank_nodes(pod, by_score, 60, 70)
                assert t == tot and np.array_equal(nodes, en[60:130]) and np.array_equal(scores, es[60:130]), (j, by_score)
                if n == 1200:
                    t, nodes, scores = s.rank_nodes(pod, by_score, tot + 5, 40)
                    assert t == tot and nodes.size == 0 and scores.size == 0


@pytest.mark.parametrize("name", NAMES)
def test_victim_walk_and_heads(engine, cases, expected, name):
    """Every node carries one pod of another queue: a victim candidate unless
    it is Releasing; the victim walk is the walk without the nodes whose
    candidate is short of the task's InitResreq in all three resources.
    rank_heads with 1, 2 and 64 requests, plain and pruned."""
    snap, path = cases[name]
    js = list(expected[name])
    with engine.Session(path) as s:
        for j in js:
            _, (e_nodes, e_scores), _, keep = expected[name][j]
            t, nodes, scores, cands, info = s.rank_victim_nodes(snap.tasks[j]["pod"], True, engine.VICTIMS_OTHER_QUEUES, 0, 64)
            assert t == keep.sum() and info["head"] == 1, j
            assert np.array_equal(nodes, e_nodes[keep][:64]) and np.array_equal(scores, e_scores[keep][:64]), j
            assert (cands == 1).all()
        for k in (1, 2, 64):
            order = [js[(3 * i + 1) % len(js)] for i in range(k)]
            for victims in (0, engine.VICTIMS_OTHER_QUEUES):
                totals, nodes, scores, cands, _ = s.rank_heads([snap.tasks[j]["pod"] for j in order], True, victims, 64)
                for i, j in enumerate(order):
                    _, (e_nodes, e_scores), _, keep = expected[name][j]
                    if victims:
                        e_nodes, e_scores = e_nodes[keep], e_scores[keep]
                    m = min(e_nodes.size, 64)
                    assert totals[i] == e_nodes.size, (k, victims, i)
                    assert np.array_equal(nodes[i, :m], e_nodes[:64]), (k, victims, i)
                    assert np.array_equal(scores[i, :m], e_scores[:64]), (k, victims, i)
                    assert (nodes[i, m:] == -1).all() and not scores[i, m:].any() and not cands[i, m:].any()
                    assert (cands[i, :m] == (1 if victims else 0)).all()


@pytest.mark.parametrize("opts", [dict(batched=1, engine=1), dict(batched=1, engine=0), dict(batched=0)],
                         ids=["engine", "batched", "pertask"])
@pytest.mark.parametrize("name", NAMES)
def test_allocate(engine, cases, sessions, name, opts):
    """The allocate action: placements, node rows (all twelve columns, also
    against the reference's own state after the log), walk visits and the gang
    messages are the faithful restatement's.  Which placer ran is asserted on
    the cross cases of 63 nodes and more: gangs of several tasks whose classes
    (resources, node selector) the engine accepts, except the host-port gang,
    which no engine pop serves (its pops are launched).  The static cases are
    one-task jobs: nothing is claimed about the placer there.  Per node
    Idle == Idle at open + visits x Backfilled - committed requests gives the
    visits the restatement's walks made (the fit rows with Backfilled)."""
    snap, path = cases[name]
    log, nstate, msgs = sessions[name]
    n = len(snap.rows)
    with engine.Session(path) as s:
        for k, v in opts.items():
            s.set_option(k, v)
        pod, node, kind = s.allocate()
        got = [(int(a), int(b), STATUS[int(k)]) for a, b, k in zip(pod, node, kind)]
        assert got == log
        ns = s.read_nodes(n)
        v_node, v_cnt = s.walk_visits()
        assert s.gang_unschedulable() == msgs
        st = s.stats()
    if snap.kind == "cross" and n >= 63:
        if opts.get("batched"):
            assert st["batched_pops"] > 0
            assert (st["engine_pops"] > 0) == bool(opts["engine"])
        else:
            assert st["batched_pops"] == 0 and st["engine_pops"] == 0
    for col in range(12):   # idle, used, releasing, backfilled
        bad = np.nonzero(ns[:, col] != nstate[:, col])[0]
        assert bad.size == 0, (col, [(int(b), snap.family(int(b)), int(ns[b, col]), int(nstate[b, col])) for b in bad[:4]])
    m, pod2j = snap.model(), {t["pod"]: j for j, t in enumerate(snap.tasks)}
    for p, nd, st in log:
        m.commit(pod2j[p], nd, pe.ALLOCATED if st == 4 else pe.PIPELINED)
    mine = m.node_state()   # the reference's rows: all but Idle where walks added Backfilled to it
    assert np.array_equal(ns[:, 3:], mine[:, 3:])
    quiet = ~np.array([any(b) for b in m.bf])
    assert np.array_equal(ns[quiet, :3], mine[quiet, :3])
    visits = {}
    for i in range(n):
        if m.bf[i][0]:
            extra = int(nstate[i, 0]) - m.idle[i][0]
            assert extra % m.bf[i][0] == 0
            if extra:
                visits[i] = extra // m.bf[i][0]
    assert dict(zip(v_node.tolist(), v_cnt.tolist())) == visits
    if snap.kind == "fit" and n >= 63:
        assert visits


@pytest.mark.parametrize("name", [c for c in pe.CROSS_NAMES if SIZE[c] >= 63 and c != "cross65nopred"])
def test_place_job_until_none_then_fit_deltas(engine, cases, name):
    """The gang's tasks placed one by one (the per-task kernels after commits):
    each goes where the reference's state says, the k-th at eps - 1; the one
    that finds no node reports the reference's FitDelta records, with nodes at
    delta 0 and -1."""
    snap, path = cases[name]
    m = snap.model()
    with engine.Session(path) as s:
        for j in snap.jobs["ns/jgang"]:
            exp = m.choice(j)
            nodes, kinds, stop = s.place_job([snap.tasks[j]["pod"]], 0, 1, 0)
            if exp[0] < 0:
                assert stop == engine.STOP_UNASSIGNED and list(nodes) == [-1]
                node, delta = s.fit_deltas(snap.tasks[j]["pod"])
                e_node, e_delta = m.fit_deltas(j)
                assert np.array_equal(node, e_node) and np.array_equal(delta, e_delta)
                assert (delta[:, 1] == 0).any() and (delta[:, 1] == -1).any() and (delta[:, 0] < 0).all()
                break
            assert (int(nodes[0]), int(kinds[0])) == exp, j
            m.commit(j, *exp)
        else:
            raise AssertionError("every task of the gang found a node")


@pytest.mark.parametrize("batched", [1, 0])
@pytest.mark.parametrize("name", ["cross65", "cross257"])
def test_sharded_commit_crossings(engine, oracle_mod, cases, tmp_path, name, batched):
    """Two node-array shards on one GPU give the restatement's records and
    close messages on every rank.  The boundary falls inside the families: the
    last node of shard 0 and the first of shard 1 are both threshold rows."""
    snap, _ = cases[name]
    base = engine.shard_range(len(snap.rows), 1, 2)[0]
    edge = [f for f in pe.CROSS_TYPES if not f.startswith("gang")]
    assert snap.family(base - 1) in edge and snap.family(base) in edge
    res = _shard_case(oracle_mod, tmp_path, snap.cluster, 2, batched=batched)
    if batched:
        assert all(r["batched_pops"] > 0 for r in res)
