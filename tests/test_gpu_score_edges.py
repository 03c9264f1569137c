"""Node scores at truncation ties on every device path that evaluates one.

The snapshots of tests/scoreedges.py (BRA differences of exactly k/10, whole
LeastRequested quotients up to capacities of 2^50, zero and over-committed
allocatables, unnamed requests, inter-pod spreads of 10, 49, 98 and 103; 1,
63, 64, 65, 257 and 1200 nodes; equal and unequal, partly negative weights)
run through kbhip_sweep_scores under every sweep_variant, kbhip_rank_nodes
(head and full sort, bucket and radix ranking), kbhip_rank_victim_nodes,
kbhip_rank_heads, the allocate action (batched and per-task) and a grouped
what-if batch.  Expected keys, walks and scores come from the plain-Python
reference of tests/scoreedges.py (tests/test_score_edges.py holds it against
the faithful restatement), never from another device path; expected
placements from the faithful restatement's allocate.
"""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import scoreedges as se
from test_gpu_pertask_abi import _variant
from test_gpu_whatif import _linger, _run

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in se.CASES]
ORACLE_NAMES = [c[0] for c in se.CASES if c[4]]
WHATIF_ACTIONS = "allocate, backfill, preempt"


@pytest.fixture(scope="module")
def cases(kbgen_mod, tmp_path_factory):
    return se.write_cases(kbgen_mod, tmp_path_factory.mktemp("score_edges"))


@pytest.fixture(scope="module")
def walks(cases):
    """{name: [(nodes, scores) of the by-score walk per task]}, computed once."""
    return {name: [snap.walk(j) for j in range(len(snap.tasks))] for name, (snap, _) in cases.items()}


@pytest.mark.parametrize("name", NAMES)
def test_sweep_scores_every_variant(engine, cases, name):
    """k_score_sweep<PLAIN> at each TB x NPT (variants 0-3), k_score_sweep_gs
    (4-6), and on the inter-pod snapshots the non-plain body."""
    snap, path = cases[name]
    n = len(snap.rows)
    exp = [snap.expected_keys(j) for j in range(len(snap.tasks))]
    with engine.Session(path) as s:
        for v in range(7):
            with _variant(s, v):
                for j, (pod, _, _) in enumerate(snap.tasks):
                    cnt, keys = s.sweep_scores(pod, n)
                    bad = np.nonzero(keys != exp[j])[0]
                    assert cnt == n and bad.size == 0, (
                        v, j, [(int(b), snap.family(int(b)), snap.scalars(j, int(b)),
                                int(keys[b] >> np.uint64(32)) - 2 ** 31, int(exp[j][b] >> np.uint64(32)) - 2 ** 31)
                               for b in bad[:4]])


@pytest.mark.parametrize("radix", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_rank_nodes_head_and_full(engine, cases, walks, name, radix):
    """rank_head<PLAIN> / <!PLAIN> (first + cap <= 64) and the full sort
    (rank_bucket over the class's host-computed score range, or the radix
    passes); a score outside that range fails the full call."""
    snap, path = cases[name]
    n = len(snap.rows)
    with engine.Session(path) as s:
        s.set_option("rank_radix", radix)
        for j, (pod, _, _) in enumerate(snap.tasks):
            e_nodes, e_scores = walks[name][j]
            t, nodes, scores = s.rank_nodes(pod, True, 0, 64)
            assert t == n and np.array_equal(nodes, e_nodes[:64]) and np.array_equal(scores, e_scores[:64]), j
            t, nodes, scores = s.rank_nodes(pod, True, 0, max(n, 65))
            assert t == n and np.array_equal(nodes, e_nodes) and np.array_equal(scores, e_scores), j
            t, nodes, scores = s.rank_nodes(pod, True, 3, 61)
            assert t == n and np.array_equal(nodes, e_nodes[3:64]) and np.array_equal(scores, e_scores[3:64]), j
        st = s.stats()
        assert st["rank_heads"] == 2 * len(snap.tasks) and st["rank_fulls"] == len(snap.tasks)


@pytest.mark.parametrize("name", NAMES)
def test_victim_walk_and_heads(engine, cases, walks, name):
    """Every node carries one Running pod of another queue: each is a victim
    candidate (one per node) and the victim walk is the whole walk.
    rank_heads with 1, 2 and 64 requests mixing the pending tasks."""
    snap, path = cases[name]
    n = len(snap.rows)
    pods = [t[0] for t in snap.tasks]
    with engine.Session(path) as s:
        for j, pod in enumerate(pods):
            e_nodes, e_scores = walks[name][j]
            t, nodes, scores, cands, info = s.rank_victim_nodes(pod, True, engine.VICTIMS_OTHER_QUEUES, 0, 64)
            assert t == n and info["head"] == 1
            assert np.array_equal(nodes, e_nodes[:64]) and np.array_equal(scores, e_scores[:64]), j
            assert (cands == 1).all()
        for k in (1, 2, 64):
            order = [(3 * i + 1) % len(pods) for i in range(k)]
            for victims in (0, engine.VICTIMS_OTHER_QUEUES):
                totals, nodes, scores, cands, _ = s.rank_heads([pods[j] for j in order], True, victims, 64)
                assert (totals == n).all()
                m = min(n, 64)
                for i, j in enumerate(order):
                    e_nodes, e_scores = walks[name][j]
                    assert np.array_equal(nodes[i, :m], e_nodes[:64]), (k, victims, i)
                    assert np.array_equal(scores[i, :m], e_scores[:64]), (k, victims, i)
                    assert (nodes[i, m:] == -1).all() and not scores[i, m:].any()
                    assert (cands[i, :m] == (1 if victims else 0)).all()


@pytest.fixture(scope="module")
def placements(oracle_mod, cases):
    """The faithful restatement's allocate per snapshot, computed once."""
    return {name: oracle_mod.ref_allocate(cases[name][1]).as_list() for name in ORACLE_NAMES}


@pytest.mark.parametrize("batched", [1, 0])
@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_allocate(engine, cases, placements, name, batched):
    """The engine's sweep and the per-task path: the edge scores decide the argmax."""
    snap, path = cases[name]
    with engine.Session(path) as s:
        s.set_option("batched", batched)
        pod, node, kind = s.allocate()
    got = [(int(a), int(b), 4 if k == 1 else 8) for a, b, k in zip(pod, node, kind)]
    assert got == placements[name]
    if len(snap.rows) >= 63:
        assert len(got) >= 2


def test_whatif_group_of_two(engine, oracle_mod, cases):
    """Two grouped sessions over edge snapshots (plain with unequal weights,
    inter-pod) run their actions together; each records what the faithful
    restatement records."""
    paths = [cases["plain65w"][1], cases["ipa65"][1]]
    bar = threading.Barrier(len(paths))
    with _linger(engine, paths[0]), ThreadPoolExecutor(len(paths)) as ex:
        res = list(ex.map(lambda p: _run(engine, p, 1, bar, 20000, WHATIF_ACTIONS), paths))
    for p, (got, st) in zip(paths, res):
        exp = oracle_mod.ref_allocate(p, actions=WHATIF_ACTIONS).as_list()
        assert got == exp and len(got) >= 2
    assert sum(st["rank_requests"] + st["pop_requests"] + st["sweep_requests"] for _, st in res) > 0
