"""What the task queries (kbhip_rank_nodes, kbhip_rank_victim_nodes,
kbhip_rank_heads, kbhip_explain_tasks) share on the host: the counters and
launch counts each call reports, and the staging buffers that grow between
calls of one session.

Counters: one call each on a 65-node snapshot; the expected steps are the ones
the calls had when each was a function of its own (rank_nodes: rank_heads or
rank_fulls, and sweeps; rank_victim_nodes: sweeps only; the batched calls: one
per task), and the victim walk's launch counts are the ones measured then: 3
for the head (control block, sweep, merge), 7 for the full walk (control block,
the counting sort's three kernels, the compaction's three).

Growth: a small call, then a larger one on the same session, so that the
second call meets buffers sized for the first.  Each answer is compared with
the same call on a session opened for it and with the restatement of
tests/test_gpu_victim_walk.py (Model) or tests/verdictedges.py.  The sizes are
the smallest at which the buffers grow: 257 nodes for the own list (above its
4 096-byte first allocation: 36 bytes per node of the job) and the explain
scratch, 2 048 nodes for the heads upload (above its 64 KiB first allocation).
"""
import numpy as np
import pytest

import verdictedges as ve
from test_gpu_victim_walk import GI, PENDING, Model, _expect, _same, _uniform

pytestmark = pytest.mark.gpu

KEYS = ("rank_heads", "rank_fulls", "sweeps")


def _step(s, call):
    """(the call's answer, what it added to the three counters)"""
    a = s.stats()
    out = call()
    b = s.stats()
    return out, tuple(b[k] - a[k] for k in KEYS)


def test_counters_and_launch_counts(engine, kbgen_mod, tmp_path):
    c = _uniform(kbgen_mod, 65, "third")
    p = c.write(str(tmp_path / "u65.kbs"))
    task = len(c.pods) - 1
    with engine.Session(p) as s:
        got, d = _step(s, lambda: s.rank_nodes(task, True, 0, 64))
        assert got[0] == 65 and d == (1, 0, 1)
        got, d = _step(s, lambda: s.rank_nodes(task, True, 0, 65))
        assert got[0] == 65 and got[1].size == 65 and d == (0, 1, 1)
        got, d = _step(s, lambda: s.rank_victim_nodes(task, True, 1, 0, 64))
        assert got[0] == 22 and d == (0, 0, 1)
        assert got[4] == {"head": 1, "rebuilt": 1, "launches": 3}
        got, d = _step(s, lambda: s.rank_victim_nodes(task, True, 1, 0, 65))
        assert got[0] == 22 and d == (0, 0, 1)
        assert got[4] == {"head": 0, "rebuilt": 0, "launches": 7}
        got, d = _step(s, lambda: s.rank_heads([task] * 3, True, 0, 64))
        assert got[0].tolist() == [65] * 3 and d == (3, 0, 3)
        got, d = _step(s, lambda: s.explain_tasks([task] * 3))
        assert got[0][:, 15].tolist() == [65] * 3 and d == (0, 0, 3)


def _two_jobs(kbgen, n_nodes, one_nodes, wide_nodes):
    """Equal nodes; queue q0: job "one" Running on one_nodes, job "wide" on wide_nodes (two tasks on its
    first node), job "other" on every second node; queue q1: job "far" on every fifth.  "one" and "wide"
    each have a Pending task, the last two pods in UID order."""
    c = kbgen.Cluster()
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    for i in range(n_nodes):
        c.add_node("n%05d" % i, 32000, 64 * GI, 0, 110)
    k = [0]

    def run(job, node, cpu):
        c.add_pod("ns", "%s-r%d" % (job, k[0]), uid="a%05d" % k[0], group=job, node="n%05d" % node, phase="Running",
                  containers=[kbgen.res(cpu=cpu, mem=GI)])
        k[0] += 1
    for job, q in (("one", "q0"), ("wide", "q0"), ("other", "q0"), ("far", "q1")):
        c.add_job("ns", job, q, min_member=1)
    for n in one_nodes:
        run("one", n, 3000)
    for n in [wide_nodes[0]] + list(wide_nodes):
        run("wide", n, 500 + (n % 4) * 500)
    for n in range(0, n_nodes, 2):
        run("other", n, 1000)
    for n in range(0, n_nodes, 5):
        run("far", n, 4000)
    c.add_pod("ns", "one-p", uid="p0", group="one", priority=5, ts=1, containers=[kbgen.res(cpu=2000, mem=GI)])
    c.add_pod("ns", "wide-p", uid="p1", group="wide", priority=5, ts=1,
              containers=[kbgen.res(cpu=1500, mem=2 * GI, gpu=1000)])
    return c


def _index_walk(m, task, mode):
    """The by-index walk of the restatement alone (every node passes the predicates of these snapshots)."""
    kept = m.kept(task, mode)
    nodes = sorted(kept)
    return np.array(nodes, np.int32), np.zeros(len(nodes), np.int32), np.array([kept[n] for n in nodes], np.int32)


def test_victim_own_list_grows(engine, kbgen_mod, tmp_path):
    c = _two_jobs(kbgen_mod, 257, [7], list(range(3, 253)))
    p = c.write(str(tmp_path / "own.kbs"))
    m = Model(c)
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    assert m.status[t_one] == m.status[t_wide] == PENDING
    assert len(m.cands(t_one, 3)) == 1 and len(m.cands(t_wide, 3)) == 250
    assert 1 * 36 <= 4096 < 250 * 36  # the own list's first allocation, and the list that outgrows it
    calls = [(t, by_score, mode, cap) for t in (t_one, t_wide) for mode in (3, 2) for by_score in (False, True)
             for cap in (64, 300)]
    with engine.Session(p) as live:
        for t, by_score, mode, cap in calls:
            got = live.rank_victim_nodes(t, by_score, mode, 0, cap)
            assert got[4]["head"] == (1 if cap == 64 else 0)
            _same(got, _expect(live, m, t, by_score, mode), 0, cap)
            if not by_score:
                _same(got, _index_walk(m, t, mode), 0, cap)
            with engine.Session(p) as fresh:
                ref = fresh.rank_victim_nodes(t, by_score, mode, 0, cap)
            assert got[0] == ref[0] and all(np.array_equal(a, b) for a, b in zip(got[1:4], ref[1:4]))


@pytest.fixture(scope="module")
def stacked257(kbgen_mod, tmp_path_factory):
    """(snapshot, path, {task: (verdict row, histogram)}) of the stacked snapshot at 257 nodes, computed once."""
    snap = ve.build_stacked(kbgen_mod, 257)
    path = snap.cluster.write(str(tmp_path_factory.mktemp("plumb") / "stacked257.kbs"))
    m = snap.model()
    exp = {}
    for j in ve.tasks_of(snap):
        v = ve.verdicts(m, j)
        exp[j] = (v, ve.histogram(v))
    return snap, path, exp


def test_explain_scratch_grows(engine, stacked257):
    snap, path, exp = stacked257
    js = list(exp)
    n = len(snap.rows)

    def ask(s, k, verdicts):
        order = [js[(3 * i + 1) % len(js)] for i in range(k)]
        hist, v, info = s.explain_tasks([snap.tasks[j]["pod"] for j in order], verdicts=verdicts, n_nodes=n)
        assert list(info[[0, 2]]) == [2, int(verdicts)]
        assert np.array_equal(hist, np.array([exp[j][1] for j in order])), k
        if verdicts:
            assert v.shape == (k, n) and all(np.array_equal(v[i], exp[j][0]) for i, j in enumerate(order)), k
        return hist, v

    with engine.Session(path) as live:
        for k, verdicts in ((1, False), (8, True), (16, True), (1, True)):
            hist, v = ask(live, k, verdicts)
            with engine.Session(path) as fresh:
                r_hist, r_v = ask(fresh, k, verdicts)
            assert np.array_equal(hist, r_hist) and (v is None or np.array_equal(v, r_v))


def test_heads_upload_grows(engine, kbgen_mod, tmp_path):
    c = _two_jobs(kbgen_mod, 2048, list(range(0, 1024)), list(range(1024, 2048)))
    p = c.write(str(tmp_path / "heads.kbs"))
    m = Model(c)
    t_one, t_wide = len(c.pods) - 2, len(c.pods) - 1
    own_total = len(m.cands(t_one, 3)) + len(m.cands(t_wide, 3))
    assert own_total == 2048 > 1900
    # the upload holds the control block, the descriptors and 4 x 8 + 4 bytes per own-list entry:
    # the lists alone put it above the 65 536 bytes of the first allocation
    assert own_total * (4 * 8 + 4) > 65536
    batches = [([t_one, t_wide], False, 0), ([t_one, t_wide], False, 3), ([t_wide, t_one, t_wide], True, 2),
               ([t_one, t_wide], True, 3), ([t_one], False, 0)]
    with engine.Session(p) as live:
        for tasks, by_score, mode in batches:
            got = live.rank_heads(tasks, by_score, mode, 64)
            with engine.Session(p) as fresh:
                ref = fresh.rank_heads(tasks, by_score, mode, 64)
            assert all(np.array_equal(a, b) for a, b in zip(got[:4], ref[:4])), (tasks, by_score, mode)
            assert list(got[4][1:]) == list(ref[4][1:])  # launches and grid (the fresh session also builds the table)
            for i, t in enumerate(tasks):
                if mode == 0:
                    assert got[0][i] == 2048 and (by_score or got[1][i].tolist() == list(range(64)))
                    continue
                e_n, e_s, e_c = _index_walk(m, t, mode) if not by_score else _expect(live, m, t, True, mode)
                assert got[0][i] == e_n.size and e_n.size > 64
                assert np.array_equal(got[1][i], e_n[:64]) and np.array_equal(got[2][i], e_s[:64])
                assert np.array_equal(got[3][i], e_c[:64])
