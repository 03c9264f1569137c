"""kbhip_rank_nodes on the device: the ranked node walk of one pending task.

by_score = 1 is preempt.go:270-287's walk (util.SelectBestNode order of the
nodes passing PredicateFn with a NodeOrderFn score), by_score = 0 reclaim's
(passing nodes in index order).  The expected walk comes from the faithful
restatement's per-node keys (oracle.ref_sweep_scores): the non-zero keys sorted
descending, score = (key >> 32) - 2^31; for by_score = 0 their indices,
ascending.  Requests with first + cap <= 64 run the top-64 kernel
(kbhip_stats.rank_heads), all others the full device sort (rank_fulls); both
must give the same windows of the same list.

The faithful restatement takes minutes to run an allocate action over
thousands of nodes, so the 3000-node snapshot is compared with it as opened,
and after allocate with the descending sort of kbhip_sweep_scores' keys (the
per-node sweep tests/test_gpu_pertask_abi.py holds against the restatement).
"""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import NO_POD_AFFINITY
from walkmodel import uniform_oversized

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"


def _pending(path):
    import kbhip
    with kbhip.EncodedSnapshot(path) as enc:
        return [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]


def _walks(keys):
    """(nodes, scores) of the by_score walk and the nodes of the index walk from per-node keys."""
    nz = np.nonzero(keys)[0]
    order = nz[np.argsort(keys[nz], kind="stable")[::-1]]  # the keys are distinct
    scores = (keys[order] >> np.uint64(32)).astype(np.int64) - 2 ** 31
    return order.astype(np.int32), scores.astype(np.int32), nz.astype(np.int32)


def _full(s, pod, by_score, n_nodes):
    """The whole walk through the full sort (first + cap > 64 whatever the node count)."""
    return s.rank_nodes(pod, by_score, 0, max(n_nodes, 65))


def _check_task(s, pod, keys, total, n_nodes):
    """Head and full requests of both orders against the expected walks; the stats they move."""
    nodes, scores, by_index = _walks(keys)
    assert total == nodes.size
    for by_score, e_nodes, e_scores in ((1, nodes, scores), (0, by_index, np.zeros(by_index.size, np.int32))):
        st0 = s.stats()
        t_h, n_h, s_h = s.rank_nodes(pod, by_score, 0, 64)
        st1 = s.stats()
        t_f, n_f, s_f = _full(s, pod, by_score, n_nodes)
        st2 = s.stats()
        assert t_h == t_f == total, (pod, by_score)
        assert np.array_equal(n_f, e_nodes) and np.array_equal(s_f, e_scores), (pod, by_score)
        assert np.array_equal(n_h, e_nodes[:64]) and np.array_equal(s_h, e_scores[:64]), (pod, by_score)
        assert (st1["rank_heads"] - st0["rank_heads"], st1["rank_fulls"] - st0["rank_fulls"]) == (1, 0)
        assert (st2["rank_heads"] - st1["rank_heads"], st2["rank_fulls"] - st1["rank_fulls"]) == (0, 1)


def _visit_pairs(s):
    node, cnt = s.walk_visits()
    return list(zip(node.tolist(), cnt.tolist()))


@pytest.mark.parametrize("radix", [0, 1])
@pytest.mark.parametrize("seed", range(16))
def test_rank_nodes_vs_oracle(engine, oracle_mod, kbgen_mod, tmp_path, seed, radix):
    feats = NO_POD_AFFINITY if seed % 2 else None
    kw = {} if feats is None else {"features": feats}
    c = kbgen_mod.gen_random(7100 + seed, n_nodes=5 + seed % 9, n_jobs=4 + seed % 5, max_tasks=1 + seed % 5, **kw)
    p = str(tmp_path / "s.kbs")
    c.write(p)
    n_nodes = len(c.nodes)
    pend = _pending(p)
    assert pend
    for actions in ("", "allocate"):
        with engine.Session(p) as s, engine.Session(p) as twin:
            s.set_option("rank_radix", radix)
            todo = pend
            if actions:
                s.allocate()
                twin.allocate()
                st = s.table("pod_status")
                todo = [q for q in pend if st[q] == 1]  # still Pending
            rows = s.read_nodes(n_nodes)
            for pod in todo[:6]:
                n_exp, k_exp = oracle_mod.ref_sweep_scores(p, pod, n_nodes, actions)
                _check_task(s, pod, k_exp, n_exp, n_nodes)
            assert np.array_equal(s.read_nodes(n_nodes), rows)
            assert _visit_pairs(s) == _visit_pairs(twin)  # the walk counters as a session without the calls has them


def _uniform_case(engine, oracle_mod, c, p, n_nodes):
    c.write(p)
    n_exp, k_exp = oracle_mod.ref_sweep_scores(p, 0, n_nodes, "")
    with engine.Session(p) as s:
        _check_task(s, 0, k_exp, n_exp, n_nodes)
    return n_exp


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 255, 256, 257, 3001])
def test_selection_edges(engine, oracle_mod, kbgen_mod, tmp_path, n_nodes):
    """Every node passes, few distinct scores: ties by index across wave (64),
    block (256) and multi-block boundaries."""
    c = uniform_oversized(kbgen_mod, n_nodes)
    assert _uniform_case(engine, oracle_mod, c, str(tmp_path / "u.kbs"), n_nodes) == n_nodes


def test_selection_every_third_node(engine, oracle_mod, kbgen_mod, tmp_path):
    c = uniform_oversized(kbgen_mod, 1000, label_every=3, selector=True)
    assert _uniform_case(engine, oracle_mod, c, str(tmp_path / "t.kbs"), 1000) == 334


def test_selection_no_node_passes(engine, kbgen_mod, tmp_path):
    c = uniform_oversized(kbgen_mod, 300, unsched=True)
    p = c.write(str(tmp_path / "n.kbs"))
    with engine.Session(p) as s:
        for by_score in (1, 0):
            for first, cap in ((0, 64), (0, 300), (0, None)):
                total, nodes, scores = s.rank_nodes(0, by_score, first, cap)
                assert total == 0 and nodes.size == 0 and scores.size == 0
            # nothing is written either
            node = np.full(64, -7, np.int32)
            score = np.full(64, -7, np.int32)
            vp = ctypes.c_void_p
            assert engine.lib().kbhip_rank_nodes(s._h, 0, by_score, 0, node.ctypes.data_as(vp),
                                                 score.ctypes.data_as(vp), 64) == 0
            assert (node == -7).all() and (score == -7).all()


@pytest.fixture(scope="module")
def c2_3000(kbgen_mod, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("rank") / "c2.kbs")
    kbgen_mod.gen_c2(p, n_nodes=3000, n_pending=6000)
    return p


def test_distinct_scores_3000(engine, oracle_mod, c2_3000):
    """Many distinct scores over 3000 nodes (12 blocks): as opened against the
    restatement, after allocate against the per-node sweep's keys."""
    p, n_nodes = c2_3000, 3000
    pend = _pending(p)
    with engine.Session(p) as s:
        n_exp, k_exp = oracle_mod.ref_sweep_scores(p, pend[0], n_nodes, "")
        assert np.unique(k_exp[k_exp > 0] >> np.uint64(32)).size > 4
        _check_task(s, pend[0], k_exp, n_exp, n_nodes)
        s.allocate()
        st = s.table("pod_status")
        todo = [q for q in pend if st[q] == 1][:3]
        assert todo
        for pod in todo:
            n_got, k_got = s.sweep_scores(pod, n_nodes)
            _check_task(s, pod, k_got, n_got, n_nodes)


def test_path_boundary_windows(engine, c2_3000):
    """Windows on both sides of first + cap = 64, and around the end of the
    walk: each equals the slice of the full list and returns the total."""
    p, n_nodes = c2_3000, 3000
    pod = _pending(p)[0]
    with engine.Session(p) as s:
        for by_score in (1, 0):
            total, nodes, scores = _full(s, pod, by_score, n_nodes)
            assert total > 130
            wins = [(0, 64, 1), (0, 65, 0), (1, 63, 1), (1, 64, 0), (10, 54, 1), (10, 55, 0), (63, 1, 1), (64, 1, 0),
                    (100, 30, 0), (total - 1, 1, 0), (total - 1, 70, 0), (total, 1, 0), (total, 64, 0),
                    (total + 5, 64, 0), (total - 10, None, 0)]
            for first, cap, head in wins:
                st0 = s.stats()
                t, n, sc = s.rank_nodes(pod, by_score, first, cap)
                st1 = s.stats()
                end = total if cap is None else first + cap
                assert t == total, (first, cap)
                assert np.array_equal(n, nodes[first:end]) and np.array_equal(sc, scores[first:end]), (first, cap)
                if cap is not None:
                    assert st1["rank_heads"] - st0["rank_heads"] == head, (first, cap)
                    assert st1["rank_fulls"] - st0["rank_fulls"] == 1 - head, (first, cap)
            assert s.rank_nodes(pod, by_score, 0, 0)[0] == total  # the size query
    # a walk shorter than the head: windows past its end are empty, the total still comes back
    c_path = c2_3000.replace("c2.kbs", "few.kbs")
    import kbgen
    uniform_oversized(kbgen, 40).write(c_path)
    with engine.Session(c_path) as s:
        for by_score in (1, 0):
            total, nodes, _ = s.rank_nodes(0, by_score, 0, 64)
            assert total == 40 and nodes.size == 40
            for first in (39, 40, 45):
                t, n, _ = s.rank_nodes(0, by_score, first, 64 - first)
                assert t == 40 and np.array_equal(n, nodes[first:])


def test_several_nodes_per_thread(engine, kbgen_mod, tmp_path):
    """70 000 nodes: more 256-node steps than the head sweep has blocks, so
    waves take several steps (and the last is ragged)."""
    n_nodes = 70_000
    p = str(tmp_path / "big.kbs")
    kbgen_mod.gen_c4(p, n_nodes=n_nodes, n_pending=2000, running_per_node=1)
    pend = _pending(p)
    with engine.Session(p) as s:
        for pod in pend[::397][:3]:
            cnt, keys = s.sweep_scores(pod, n_nodes)
            nodes, scores, by_index = _walks(keys)
            assert cnt == nodes.size > 64
            t, n, sc = s.rank_nodes(pod, True, 0, 64)
            assert t == cnt and np.array_equal(n, nodes[:64]) and np.array_equal(sc, scores[:64])
            t, n, sc = s.rank_nodes(pod, False, 0, 64)
            assert t == cnt and np.array_equal(n, by_index[:64]) and not sc.any()


def test_errors(engine, kbgen_mod, tmp_path):
    GI = 1 << 30
    c = kbgen_mod.Cluster()
    c.add_queue("q0", 1)
    for i in range(5):
        c.add_node(f"n{i}", 4000, 8 * GI, 0, 110)
    for j in range(3):
        c.add_job("ns", f"j{j}", "q0", min_member=1, ts=j)
        c.add_pod("ns", f"j{j}-0", uid=f"p{j}", group=f"j{j}", ts=j, containers=[kbgen_mod.res(cpu=1000, mem=GI)])
    p = c.write(str(tmp_path / "e.kbs"))
    with engine.Session(p) as s:
        assert s.rank_nodes(1)[0] == 5
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.rank_nodes(1, 2)  # by_score outside {0, 1}
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.rank_nodes(99)  # no such task
        t = s.place_job_submit([2], 1, 1, 0)
        with pytest.raises(engine.KbhipError, match=EINVAL):  # a ticket is outstanding
            s.rank_nodes(1, True, 0, 64)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.rank_nodes(1)
        assert s.place_job_cancel(t) == 1
        assert s.rank_nodes(1, True, 0, 64)[0] == 5
        assert s.rank_nodes(2)[0] == 5  # the cancelled pop left its task pending
        pod, _, _ = s.allocate()
        assert 0 in pod.tolist()
        for cap in (64, None):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.rank_nodes(0, True, 0, cap)  # a task the session placed
    sh = engine.ShardedSession(p, 0, 0, 2)
    try:
        with pytest.raises(engine.KbhipError, match=EUNSUP):
            sh.rank_nodes(1, True, 0, 64)
        with pytest.raises(engine.KbhipError, match=EUNSUP):
            sh.rank_nodes(1)
    finally:
        sh.close()


def test_actions_unchanged(engine, oracle_mod, kbgen_mod, tmp_path):
    """Ranking calls in front of the actions leave their results as they are
    (the reclaim / preempt rankings share the full path's launch selection)."""
    actions = "reclaim, allocate, backfill, preempt"
    code = {1: 4, 2: 8, 3: 128}
    records = 0
    for seed in (900, 901, 902):
        c = kbgen_mod.gen_preempt(seed, n_nodes=24, n_queues=3, n_run_jobs=14, n_pend_jobs=5, max_tasks=5)
        p = c.write(str(tmp_path / f"a{seed}.kbs"))
        exp = oracle_mod.ref_allocate(p, actions=actions).as_list()
        records += len(exp)
        pend = _pending(p)
        with engine.Session(p) as s:
            s.set_option("rank_radix", seed % 2)
            for pod in pend[:4]:
                for by_score in (1, 0):
                    s.rank_nodes(pod, by_score, 0, 64)
                    s.rank_nodes(pod, by_score, 0, 100)
            pod, node, kind = s.run_actions(actions)
        got = [(int(a), int(b), code[int(k)]) for a, b, k in zip(pod, node, kind)]
        assert got == exp, seed
    assert records > 0
