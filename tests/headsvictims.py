"""Helpers of the kbhip_heads_victims tests: the packed cluster of the node-size test (as in
tests/test_gpu_head_victims.py), and the comparison of one batched call with the per-task calls and the
restatement (tests/victimmodel.py)."""
import numpy as np

GI = 1 << 30
SIZES = (0, 1, 63, 64, 65, 129, 200, 256, 257)  # tasks per node: the 64-lane chunks, the LDS rows (256) and past them
VALID = 1


def packed(kbgen, tiers, sizes=SIZES):
    """One node per size in SIZES.  Its tasks alternate between queue q1 (job "far", and every fourth of job
    "gang3" with MinAvailable 3) and the pending tasks' own queue q0 (job "mate", every sixth of the
    pending job "pend" itself), so every mode has candidates between non-candidates and one job spans many
    candidates of a node; every seventh pod is critical, every fifth larger than the rest."""
    c = kbgen.Cluster(tiers=tiers)
    c.add_queue("q0", 1)
    c.add_queue("q1", 3)
    for i, _ in enumerate(sizes):
        c.add_node("n%02d" % i, 64000, 256 * GI, 16000, 400)
    for job, q, mm in (("far", "q1", 1), ("gang3", "q1", 3), ("mate", "q0", 2), ("pend", "q0", 1)):
        c.add_job("ns", job, q, min_member=mm, ts=1 if job == "pend" else 0)
    k = 0
    for i, size in enumerate(sizes):
        for j in range(size):
            if j % 2 == 0:
                job = "gang3" if j % 8 == 0 else "far"
            else:
                job = "pend" if j % 6 == 1 else "mate"
            c.add_pod("ns", "r%05d" % k, uid="a%05d" % k, group=job, node="n%02d" % i, phase="Running",
                      priority_class="system-node-critical" if k % 7 == 3 else "",
                      containers=[kbgen.res(cpu=20 + (k % 5 == 0) * 300, mem=GI // 64, gpu=10 * (k % 3 == 0))])
            k += 1
    c.add_pod("ns", "pend-small", uid="p0", group="pend", priority=5, ts=1, containers=[kbgen.res(cpu=500, mem=GI)])
    c.add_pod("ns", "pend-wide", uid="p1", group="pend", priority=5, ts=1,
              containers=[kbgen.res(cpu=2500, mem=2 * GI, gpu=200)])
    return c


def first_valid(flags):
    hit = np.nonzero(np.asarray(flags) & VALID)[0]
    return int(hit[0]) if hit.size else -1


def same_rows(got, i, single):
    """Request i of a batched answer equals the per-task answer `single`, element for element."""
    totals, nodes, scores, counts, evicts, flags, rows, first, _ = got
    n, s_node, s_score, s_count, s_evict, s_flags, s_rows, _ = single
    assert int(totals[i]) == n
    for a, b in ((nodes[i], s_node), (scores[i], s_score), (counts[i], s_count), (evicts[i], s_evict),
                 (flags[i], s_flags), (rows[i], s_rows)):
        assert a.shape == b.shape and np.array_equal(a, b), i
    assert int(first[i]) == first_valid(s_flags), i


def against_model(got, i, m, task, mode, cap, stride, memo=None):
    """Request i of a batched answer against the restatement: every head row, and the padding beyond the head.
    Returns the rows with victims."""
    totals, nodes, scores, counts, evicts, flags, rows, first, _ = got
    k = min(cap, int(totals[i]))
    assert (nodes[i][k:] == -1).all() and not scores[i][k:].any() and not counts[i][k:].any()
    assert not evicts[i][k:].any() and not flags[i][k:].any() and (rows[i][k:] == -1).all()
    nonempty = 0
    for j in range(k):
        key = (task, mode, int(nodes[i][j]))
        if memo is not None and key in memo:
            exp = memo[key]
        else:
            exp = m.decide(*key)
            if memo is not None:
                memo[key] = exp
        exp_v, exp_e, exp_f = exp
        assert int(counts[i][j]) == len(exp_v), key
        assert rows[i][j].tolist() == (exp_v + [-1] * stride)[:stride], key
        assert (int(evicts[i][j]), int(flags[i][j])) == (exp_e, exp_f), key
        nonempty += bool(exp_v)
    return nonempty


def check_batch(s, m, tasks, by_score, mode, cap, stride, memo=None, model=True):
    """One batched call for `tasks` (at most 64): every row equals the per-task call on the same session and
    the restatement.  Returns (the batched answer, rows with victims)."""
    got = s.heads_victims(tasks, by_score, mode, cap, stride)
    info = got[8]
    assert got[0].shape == (len(tasks),) and got[1].shape == (len(tasks), cap)
    assert got[6].shape == (len(tasks), cap, stride) and got[7].shape == (len(tasks),)
    top = nonempty = 0
    done = {}
    for i, t in enumerate(tasks):
        if t not in done:
            done[t] = s.head_victims(t, by_score, mode, cap, stride)
        single = done[t]
        same_rows(got, i, single)
        top = max(top, single[7]["max_count"])
        if model:
            nonempty += against_model(got, i, m, t, mode, cap, stride, memo)
    assert info["max_count"] == top
    return got, nonempty
