"""Hand-placed clusters at the comparison edges of the victim decision, for the
CPU and GPU tests of kbhip_head_victims.  Each builder returns (cluster,
expectations): expectations maps (task uid, node index, mode) to what the
reference's arithmetic gives there, worked out by hand below — (victim uids,
evicted prefix, flags), or None where only tests/victimmodel.py decides (a
floating-point tie whose side is the double arithmetic's).

Resource.Less is strict in all three resources; Resource.LessEqual and le_tol
allow a difference below 10 millicpu, 10 MiB, 10 milligpu."""
import kbgen

GI, MI = 1 << 30, 1 << 20
VALID, COVERS = 1, 2


def _pend(c, uid, group, **res):
    c.add_pod("ns", uid, uid=uid, group=group, priority=5, ts=1, containers=[kbgen.res(**res)])


def validate_and_prefix():
    """validateVictims' strict Less, and le_tol in the eviction loop and the pipeline test.  Tier: gang and
    conformance (every job has MinAvailable 1, so gang answers every candidate; a critical pod is a
    candidate, which keeps its node in the pruned walk, but never a victim)."""
    c = kbgen.Cluster(tiers=[["gang", "conformance"]])
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    c.add_job("ns", "run", "q1", min_member=1)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    exp, k = {}, [0]

    def node(pods, gpu_task, plain_task):
        n = len(c.nodes)
        c.add_node("n%02d" % n, 64000, 64 * GI, 8000, 110)
        uids = []
        for cpu, mem, gpu, critical in pods:
            uid = "a%03d" % k[0]
            k[0] += 1
            c.add_pod("ns", uid, uid=uid, group="run", node="n%02d" % n, phase="Running",
                      priority_class="system-node-critical" if critical else "",
                      containers=[kbgen.res(cpu=cpu, mem=mem, gpu=gpu)])
            if not critical:
                uids.append(uid)
        for task, e in (("p0", gpu_task), ("p1", plain_task)):
            if e is not None:
                exp[(task, n, 1)] = (uids, e[0], e[1])

    # p0 asks (2000, 2 Gi, 100); p1 asks (1000, 1 Gi, 0) — with no gpu asked no sum is Less, so p1 is always VALID
    crit = (10, MI, 10, True)
    # victims' sum below in all three: not valid (the critical candidate lifts the node over the walk's own test)
    node([(1999, 2 * GI - 1, 99, False), crit], (0, 0), None)
    # equal in exactly one resource: not Less, valid; the other two are 1 short, inside le_tol's tolerances: covered
    node([(2000, 2 * GI - 1, 99, False), crit], (1, VALID | COVERS), None)
    node([(1999, 2 * GI, 99, False), crit], (1, VALID | COVERS), None)
    node([(1999, 2 * GI - 1, 100, False), crit], (1, VALID | COVERS), None)
    # le_tol, cpu: 1000 - 990 = 10 is not below kMinCPU — the loop goes on to the second victim and stops there
    node([(990, GI, 0, False), (500, GI, 0, False)], None, (2, VALID | COVERS))
    # 1000 - 991 = 9 is: the loop stops after one victim, and the pipeline test passes on the same tolerance
    node([(991, GI, 0, False), (500, GI, 0, False)], None, (1, VALID | COVERS))
    # a single victim 10 short in cpu: evicted, not covered; 9 short: covered
    node([(990, GI, 0, False)], None, (1, VALID))
    node([(991, GI, 0, False)], None, (1, VALID | COVERS))
    # memory: 10 MiB short is not covered, one byte less short is
    node([(1000, GI - 10 * MI, 0, False)], None, (1, VALID))
    node([(1000, GI - 10 * MI + 1, 0, False)], None, (1, VALID | COVERS))
    # gpu (p0 asks 100): 10 short, 9 short
    node([(2000, 2 * GI, 90, False)], (1, VALID), (1, VALID | COVERS))
    node([(2000, 2 * GI, 91, False)], (1, VALID | COVERS), (1, VALID | COVERS))
    _pend(c, "p0", "pend", cpu=2000, mem=2 * GI, gpu=100)
    _pend(c, "p1", "pend", cpu=1000, mem=GI)
    return c, exp


def proportion_edges():
    """proportion.go:159-183 at LessEqual's tolerance.  Five nodes of 20 000 millicpu / 12 Gi; q1's Running
    pods hold every millicpu, and its Pending job asks for more than the cluster, so the water-filling gives
    q1 the cluster minus q0's request (p0: 1000, 1 Gi): deserved = (99 000, 59 Gi), allocated = (100 000,
    59 Gi + 20 Mi).  An evictee is a victim while the evictees so far take less than 1000 + 10 millicpu and
    less than 20 Mi + 10 Mi off the queue."""
    c = kbgen.Cluster(tiers=[["proportion"]])
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    for n in range(5):
        c.add_node("n%02d" % n, 20000, 12 * GI, 0, 110)
    c.add_job("ns", "run", "q1", min_member=1)
    c.add_job("ns", "more", "q1", min_member=1, ts=2)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    layout = {0: [(500, MI), (509, MI), (1, MI), (18990, 11 * GI + 768 * MI)],           # cpu: 500, 1009 in; 1010 out
              1: [(100, 20 * MI), (100, 10 * MI - 1), (100, 1), (19700, 11 * GI + 768 * MI)],  # memory: 20 Mi, 30 Mi - 1 in; 30 Mi out
              2: [(1009, MI), (20000 - 1009, 11 * GI + 768 * MI)],                       # one evictee just inside
              3: [(1010, MI), (20000 - 1010, 11 * GI + 768 * MI)]}                       # one evictee exactly at the tolerance: none
    used = sum(m for pods in layout.values() for _, m in pods)
    layout[4] = [(20000, 59 * GI + 20 * MI - used)]
    assert 0 < layout[4][0][1] <= 12 * GI
    exp, k = {}, 0
    for n in range(5):
        uids = []
        for cpu, mem in layout[n]:
            uid = "a%03d" % k
            k += 1
            c.add_pod("ns", uid, uid=uid, group="run", node="n%02d" % n, phase="Running",
                      containers=[kbgen.res(cpu=cpu, mem=mem)])
            uids.append(uid)
        inside = {0: 2, 1: 2, 2: 1, 3: 0, 4: 0}[n]
        # p0 asks no gpu: a non-empty victim list is VALID; the victims together are far below 1000 / 1 Gi
        # except on node 2 (1009 millicpu, but 1 Mi): every victim is evicted, none covers
        exp[("p0", n, 1)] = (uids[:inside], inside, VALID if inside else 0)
    _pend(c, "p0", "pend", cpu=1000, mem=GI)
    for i in range(3):
        _pend(c, "q%d" % i, "more", cpu=50000, mem=40 * GI)
    return c, exp


def drf_share_delta():
    """drf.go:84-109 at shareDelta.  Ten nodes of 200 000 millicpu: a share is millicpu / 2 000 000.  The
    preemptor's job holds 99 000 and asks 1000 more: ls = 0.05.  Job v<d> keeps 100 000 - d after its 1000
    millicpu pod on node d + 1 is evicted, so ls - rs = d / 2 000 000: victims for d <= 1 (also d = -1,
    where ls < rs), none for d >= 3, and d = 2 is 1e-6 up to the rounding of the two quotients."""
    c = kbgen.Cluster(tiers=[["drf"]])
    c.add_queue("q0", 1)
    for n in range(10):
        c.add_node("n%02d" % n, 200000, 100 * GI, 0, 110)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    c.add_pod("ns", "a000", uid="a000", group="pend", node="n09", phase="Running",
              containers=[kbgen.res(cpu=99000, mem=MI)])
    exp = {}
    for i, d in enumerate((-1, 0, 1, 2, 3, 4)):
        job = "v%d" % i
        c.add_job("ns", job, "q0", min_member=1)
        c.add_pod("ns", "b%d0" % i, uid="b%d0" % i, group=job, node="n%02d" % (i + 1), phase="Running",
                  containers=[kbgen.res(cpu=1000, mem=MI)])
        c.add_pod("ns", "b%d1" % i, uid="b%d1" % i, group=job, node="n%02d" % (7 + i % 2), phase="Running",
                  containers=[kbgen.res(cpu=100000 - d, mem=MI)])
        if d != 2:
            # (p0 asks 1000 millicpu, 1 Mi: the one victim is evicted and covers)
            exp[("p0", i + 1, 2)] = (["b%d0" % i], 1, VALID | COVERS) if d <= 1 else ([], 0, 0)
        else:
            exp[("p0", i + 1, 2)] = None
    _pend(c, "p0", "pend", cpu=1000, mem=MI)
    return c, exp


BUILDERS = {"validate_and_prefix": validate_and_prefix, "proportion_edges": proportion_edges,
            "drf_share_delta": drf_share_delta}


def resolve(c, exp):
    """Expectations by pod and node index: {(task, node, mode): (victims, evict, flags) or None}."""
    idx = {p.uid: i for i, p in enumerate(sorted(c.pods, key=lambda p: p.uid))}
    return {(idx[t], n, mode): (None if e is None else ([idx[u] for u in e[0]], e[1], e[2]))
            for (t, n, mode), e in exp.items()}
