"""Hand-placed clusters where a node's victims depend on what the walk evicted
on the node before it, for the CPU and GPU tests of kbhip_walk_victims.

Each builder returns (cluster, task uid, mode, carried, stateless): the ops
[(op, pod uid, node index)] of the task's walk over all nodes in index order,
worked out by hand below — `carried` as the reference's loop gives them, each
node answered after the evictions of the nodes before it, and `stateless` as a
walk that answered every node against the opened state would give them.  The
two differ in every case: that is what the case is for.

No task here asks for a GPU, so validateVictims (strict Less in all three
resources) passes for any non-empty victim list, and every evicted prefix is
far from covering the request: each node with a victim is evicted from, and
the loop goes on."""
import kbgen

GI, MI = 1 << 30, 1 << 20
EVICT, PIPELINE = 1, 2


def _pend(c, uid, group, **res):
    c.add_pod("ns", uid, uid=uid, group=group, priority=5, ts=1, containers=[kbgen.res(**res)])


def _run(c, uid, group, node, **res):
    c.add_pod("ns", uid, uid=uid, group=group, node="n%02d" % node, phase="Running", containers=[kbgen.res(**res)])


def gang_ready_drops():
    """gang.go:107-129: job g (MinAvailable 2) has three Running tasks, one on each node.  readyTaskNum is 3
    on n00 (2 <= 3 - 1: a victim, evicted), 2 on n01 (2 <= 1 fails) and n02.  Stateless: 3 everywhere."""
    c = kbgen.Cluster(tiers=[["gang"]])
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    for n in range(3):
        c.add_node("n%02d" % n, 8000, 16 * GI, 0, 110)
    c.add_job("ns", "g", "q1", min_member=2)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    for n in range(3):
        _run(c, "a%d" % n, "g", n, cpu=100, mem=MI)
    _pend(c, "p0", "pend", cpu=1000, mem=GI)
    return c, "p0", 1, [(EVICT, "a0", 0)], [(EVICT, "a%d" % n, n) for n in range(3)]


def drf_share_crosses():
    """drf.go:84-109, mode QUEUE_OTHER_JOBS.  Ten nodes of 200 000 millicpu: a share is millicpu / 2 000 000.
    The preemptor's job holds 99 000 (n09); the task's Resreq is 1000, which is what drf adds (ls = 0.05),
    and its InitResreq 3000 through an init container, which no victim covers.  Job v holds 101 000: b0 (1000, n01), b1 (1000, n02), b2 (99 000, n08).  On n01 v keeps
    100 000 after b0: rs = ls, a victim, evicted.  On n02 v would keep 99 000 after b1: rs = 0.0495, none;
    a stateless walk still sees 101 000 there and evicts b1.  b2 leaves v far below either way."""
    c = kbgen.Cluster(tiers=[["drf"]])
    c.add_queue("q0", 1)
    for n in range(10):
        c.add_node("n%02d" % n, 200000, 100 * GI, 0, 110)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    c.add_job("ns", "v", "q0", min_member=1)
    _run(c, "a0", "pend", 9, cpu=99000, mem=MI)
    _run(c, "b0", "v", 1, cpu=1000, mem=MI)
    _run(c, "b1", "v", 2, cpu=1000, mem=MI)
    _run(c, "b2", "v", 8, cpu=99000, mem=MI)
    # Resreq 1000 (what drf adds to the job's allocation), InitResreq 3000 through an init container: not covered
    c.add_pod("ns", "p0", uid="p0", group="pend", priority=5, ts=1, containers=[kbgen.res(cpu=1000, mem=MI)],
              init_containers=[kbgen.res(cpu=3000, mem=MI)])
    return c, "p0", 2, [(EVICT, "b0", 1)], [(EVICT, "b0", 1), (EVICT, "b1", 2)]


def drf_own_job():
    """drf.go:84-109, mode SAME_JOB, behind gang in one tier.  Ten nodes of 400 000 millicpu: one millicpu
    is 2.5e-7 of a share, shareDelta is 4 of them.  The job holds 100 006: a0 (100 000, n09) and b0, b1, b2
    (2 each, n01..n03); the task asks 1.  Both sides of drf's comparison are this job: after k evictions
    ls is (100 007 - 2 k) / 4e6 and b_k would leave rs = (100 004 - 2 k) / 4e6 — three millicpu apart on
    every node, inside shareDelta, only because `la` shrinks with the job (with the opened la the distance
    on n02 would be five, and b1 no victim).  gang (MinAvailable 2, four Running) is what ends the walk:
    ready is 4 on n01, 3 on n02 (2 <= 2: evicted) and 2 on n03 (2 <= 1 fails).  Stateless: 4 everywhere."""
    c = kbgen.Cluster(tiers=[["gang", "drf"]])
    c.add_queue("q0", 1)
    for n in range(10):
        c.add_node("n%02d" % n, 400000, 100 * GI, 0, 110)
    c.add_job("ns", "pend", "q0", min_member=2, ts=1)
    _run(c, "a0", "pend", 9, cpu=100000, mem=MI)
    for k in range(3):
        _run(c, "b%d" % k, "pend", k + 1, cpu=2, mem=256 * MI)
    _pend(c, "p0", "pend", cpu=1, mem=GI)
    return c, "p0", 3, [(EVICT, "b0", 1), (EVICT, "b1", 2)], [(EVICT, "b%d" % k, k + 1) for k in range(3)]


def proportion_reaches_deserved():
    """proportion.go:159-183 at LessEqual's tolerance.  Five nodes of 20 000 millicpu / 12 Gi; q1's Running
    pods hold every millicpu and its Pending job asks for more than the cluster, so q1 deserves the cluster
    minus q0's request (p0: 1000, 1 Gi): deserved cpu 99 000, allocated 100 000.  An evictee is a victim
    while q1 keeps more than 99 000 - 10.  n00: 500 off, 99 500 left, evicted.  n01: 509 more, 98 991 left,
    nine below deserved: inside the tolerance, evicted.  n02: one more, 98 990: ten below, none.  A
    stateless walk takes the one millicpu off 100 000 there and evicts.  The large pod of each node takes
    the queue far below deserved on its own."""
    c = kbgen.Cluster(tiers=[["proportion"]])
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    for n in range(5):
        c.add_node("n%02d" % n, 20000, 12 * GI, 0, 110)
    c.add_job("ns", "run", "q1", min_member=1)
    c.add_job("ns", "more", "q1", min_member=1, ts=2)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    big = 11 * GI + 800 * MI
    small = {0: 500, 1: 509, 2: 1}
    for n in range(4):
        if n in small:
            _run(c, "a%d0" % n, "run", n, cpu=small[n], mem=MI)
        _run(c, "a%d1" % n, "run", n, cpu=20000 - small.get(n, 0), mem=big)
    last = 59 * GI + 20 * MI - 4 * big - 3 * MI
    assert 0 < last <= 12 * GI
    _run(c, "a41", "run", 4, cpu=20000, mem=last)
    _pend(c, "p0", "pend", cpu=1000, mem=GI)
    for i in range(3):
        _pend(c, "q%d" % i, "more", cpu=50000, mem=40 * GI)
    return (c, "p0", 1, [(EVICT, "a00", 0), (EVICT, "a10", 1)],
            [(EVICT, "a00", 0), (EVICT, "a10", 1), (EVICT, "a20", 2)])


BUILDERS = {"gang_ready_drops": gang_ready_drops, "drf_share_crosses": drf_share_crosses, "drf_own_job": drf_own_job,
            "proportion_reaches_deserved": proportion_reaches_deserved}


def resolve(c, task, ops_lists):
    """Pod uids -> pod indices: (task index, [ops by index, ...])."""
    idx = {p.uid: i for i, p in enumerate(sorted(c.pods, key=lambda p: p.uid))}
    return idx[task], [[(o, idx[u], n) for o, u, n in ops] for ops in ops_lists]
