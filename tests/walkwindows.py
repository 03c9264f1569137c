"""Hand-placed clusters whose eviction walks are longer than one 64-entry
window, for the CPU and GPU tests of kbhip_walk_victims_from.

Every node holds at least one Running pod that is a victim candidate of the
pending task p0, and p0 asks for no GPU, so the victim test of the pruned walk
(candidates present, not strictly short in all three resources) keeps every
node: in index order the pruned walk is 0, 1, .., n - 1 by construction.  What
a node does in the walk is its kind:
  g  its pod belongs to job "blk", whose MinAvailable is its Running count:
     gang refuses every one of them (gang.go:107-129), no victim, not VALID
  c  its pod is critical: conformance refuses it (conformance.go:37-56)
  v  a small pod of job "run" (MinAvailable 1): VALID, far from covering
  C  a pod of job "big" that covers p0's InitResreq alone: the walk ends here
  L  257 small pods of job "run": VALID, not covering, longer than the 256
     records a block stages in LDS
Mode 1 (other queues) puts the Running jobs in queue q1, mode 2 (same queue,
other jobs) in p0's own queue q0.

p0 asks 1000 millicpu / 8 Gi.  Covering needs both within the tolerance; only
C pods carry memory (8 Gi), every other pod 1 Gi (L: 1 Mi each, 257 Mi), so no
prefix but C's covers.  The cpu of a node's pod is free for the score groups.

The expected protocol (expected_calls) is walkvictims.chain over window slices
of a walk ranked once, the model moved on by the ops between the calls — what
a host loop over kbhip_walk_victims_from and kbhip_apply_ops sees."""
import copy

import gohost
import kbgen
import walkvictims
from gohost import PENDING
from victimmodel import VALID
from walkvictims import ASSIGNED, CAPACITY, EXHAUSTED, HEAD_END, EVICT, PIPELINE, records

GI, MI = 1 << 30, 1 << 20
WINDOW = 64
TIER = [["gang", "conformance"]]
SCORED = [["gang", "conformance", "predicates", "nodeorder"]]
NEGATIVE = {"nodeorder": {"leastrequested.weight": "-3", "balancedresource.weight": "0"}}
LONG = 257


def build(kinds, mode=1, tiers=None, args=None, cpu=None):
    """One node per entry of `kinds` (index order = walk order by index).  cpu: per node the millicpu of its
    pod (default 500, C: 2000; L: 10 per pod).  Pod indices (UID order): node i's pod is pod i while no node is L."""
    c = kbgen.Cluster(tiers=tiers or TIER, args=args)
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    rq = "q1" if mode == 1 else "q0"
    n_blk = sum(k == "g" for k in kinds)
    assert n_blk != 1  # (MinAvailable 1 is always preemptable)
    for i, _ in enumerate(kinds):
        c.add_node("n%05d" % i, 16000, 64 * GI, 0, 400)
    c.add_job("ns", "blk", rq, min_member=max(n_blk, 2))
    c.add_job("ns", "crit", rq, min_member=1)
    c.add_job("ns", "run", rq, min_member=1)
    c.add_job("ns", "big", rq, min_member=1)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    k = 0
    for i, kind in enumerate(kinds):
        job = {"g": "blk", "c": "crit", "v": "run", "C": "big", "L": "run"}[kind]
        for j in range(LONG if kind == "L" else 1):
            c.add_pod("ns", "r%05d" % k, uid="a%05d" % k, group=job, node="n%05d" % i, phase="Running",
                      priority_class="system-node-critical" if kind == "c" else "",
                      containers=[kbgen.res(cpu=10 if kind == "L" else (cpu[i] if cpu else 2000 if kind == "C" else 500),
                                            mem=MI if kind == "L" else (8 * GI if kind == "C" else GI))])
            k += 1
    c.add_pod("ns", "pend-0", uid="p00000", group="pend", priority=5, ts=1, containers=[kbgen.res(cpu=1000, mem=8 * GI)])
    return c


def blocked(n):
    """n walk entries none of which is VALID: gang's and conformance's refusals alternate."""
    return ["g" if i % 2 == 0 else "c" for i in range(n)]


def with_kinds(n, at):
    k = blocked(n)
    for pos, kind in at.items():
        k[pos] = kind
    if sum(x == "g" for x in k) == 1:
        k[k.index("g")] = "c"
    return k


# ---- the clusters: name -> (builder(mode) -> cluster, modes, walk by index, walk by score or None (= by index)) ----
def _plain(kinds):
    return (lambda mode: build(kinds, mode)), (1, 2), list(range(len(kinds))), None


def gang_carried(mode=1):
    """gang.go:107-129 across a window edge.  Job "g" (MinAvailable 2) has four Running tasks, at walk
    positions 10, 70, 80 and 90.  readyTaskNum is 4 at position 10 (2 <= 3: evicted), 3 at 70 (2 <= 2:
    evicted) and 2 at 80 and 90 (2 <= 1 fails: passed over); a stateless walk sees 4 everywhere and evicts
    on all four.  The first eviction reaches the second window through kbhip_apply_ops, the second through
    the overlay.  Position 100 covers."""
    kinds = with_kinds(130, {100: "C"})
    c = build(kinds, mode)
    c.add_job("ns", "g", "q1" if mode == 1 else "q0", min_member=2)
    for p in c.pods:
        if p.node in ("n00010", "n00070", "n00080", "n00090"):
            p.group = "g"
            p.priority_class = ""
    return c


GANG_ACTED, GANG_STATELESS = [10, 70, 100], [10, 70, 80, 90, 100]


def drf_carried(mode=2):
    """drf.go:84-109 (preempt only: mode 2) across a window edge, walkedges.drf_share_crosses' arithmetic.
    The cluster's cpu is 2 000 000 (129 nodes of 10 000 and one of 710 000), so a share is millicpu /
    2 000 000.  The preemptor's job holds 99 000 and the task's Resreq is 1000: ls = 0.05; its InitResreq is
    3000 through an init container.  Job "v" holds 102 000: 1000 each at walk positions 10, 70 and 80 and
    99 000 on the last node.  Position 10 leaves v 101 000 (rs above ls: evicted), position 70 leaves
    100 000 (rs = ls: evicted), position 80 would leave 99 000 (rs below ls: passed over; a stateless walk
    sees 101 000 there and evicts).  Position 100 holds 3000 of job "w", whose other 150 000 keep its share
    above ls: it covers.  The fillers' jobs hold far less than ls of the cluster: drf refuses them, as gang
    and conformance do."""
    assert mode == 2
    n = 130
    c = kbgen.Cluster(tiers=[["gang", "conformance", "drf"]])
    c.add_queue("q0", 1)
    for i in range(n):
        c.add_node("n%05d" % i, 710000 if i == n - 1 else 10000, 100 * GI, 0, 110)
    kinds = blocked(n)
    c.add_job("ns", "blk", "q0", min_member=sum(k == "g" for k in kinds))
    c.add_job("ns", "crit", "q0", min_member=1)
    c.add_job("ns", "v", "q0", min_member=1)
    c.add_job("ns", "w", "q0", min_member=1)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    special = {10: ("v", 1000), 70: ("v", 1000), 80: ("v", 1000), 100: ("w", 3000)}
    for i, kind in enumerate(kinds):
        job, cpu = special.get(i, ("blk" if kind == "g" else "crit", 100))
        if i == n - 1:
            job, cpu = "v", 99000
        c.add_pod("ns", "r%05d" % i, uid="a%05d" % i, group=job, node="n%05d" % i, phase="Running",
                  priority_class="system-node-critical" if job == "crit" else "", containers=[kbgen.res(cpu=cpu, mem=MI)])
    c.add_pod("ns", "w-big", uid="b00000", group="w", node="n%05d" % (n - 1), phase="Running",
              containers=[kbgen.res(cpu=150000, mem=MI)])
    c.add_pod("ns", "pend-run", uid="b00001", group="pend", node="n%05d" % (n - 1), phase="Running",
              containers=[kbgen.res(cpu=99000, mem=MI)])
    c.add_pod("ns", "pend-0", uid="p00000", group="pend", priority=5, ts=1, containers=[kbgen.res(cpu=1000, mem=MI)],
              init_containers=[kbgen.res(cpu=3000, mem=MI)])
    return c


DRF_ACTED, DRF_STATELESS = [10, 70, 100], [10, 70, 80, 100]


def proportion_carried(mode=1):
    """proportion.go:159-183 at LessEqual's tolerance (reclaim only: mode 1) across a window edge,
    walkedges.proportion_reaches_deserved's arithmetic.  130 nodes of 20 000 millicpu / 64 Gi, T = 2 600 000
    millicpu and M = 8320 Gi in all; q1's Running pods hold every millicpu and every byte.  p0 of q0 asks 5
    millicpu / 8 Gi, which is all q0 requests, so the water-filling gives q0 its request and q1 the rest:
    deserved (T - 5, M - 8 Gi).  An evictee is a victim while q1 keeps more than T - 15 millicpu (LessEqual's
    10) and M - 8 Gi - 10 Mi.  Every node's first pod (UID order) is the one the walk is about; a second pod
    fills the node and takes q1 far below deserved on its own (proportion subtracts it after the first).
      position 10   3 millicpu off: T - 3, evicted (1 Mi: far from covering 8 Gi)
      position 70   7 more: T - 10, five below deserved, inside the tolerance: evicted
      position 80   5 more would leave T - 15, ten below: passed over; a stateless walk sees T - 5 there
                    and evicts
      position 100  4 millicpu / 8 Gi of job "big": T - 14, nine below, and M - 8 Gi - 2 Mi: a victim, and
                    it covers p0 (5 - 4 < 10 millicpu, 8 Gi)
    Had nothing been applied after the first window, position 80 would be evicted from (T - 12) and 100
    refused (T - 16).  The other nodes hold one pod that gang or conformance refuses."""
    assert mode == 1
    n, cpu, mem = 130, 20000, 64 * GI
    special = {10: ("run", 3, MI), 70: ("run", 7, MI), 80: ("run", 5, MI), 100: ("big", 4, 8 * GI)}
    kinds = blocked(n)
    c = kbgen.Cluster(tiers=[["gang", "conformance", "proportion"]])
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    for i in range(n):
        c.add_node("n%05d" % i, cpu, mem, 0, 110)
    c.add_job("ns", "blk", "q1", min_member=sum(k == "g" for i, k in enumerate(kinds) if i not in special))
    for job in ("crit", "run", "big", "fill"):
        c.add_job("ns", job, "q1", min_member=1)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)

    def run(i, k, job, pc, pm, critical=False):
        c.add_pod("ns", "r%05d-%d" % (i, k), uid="a%05d_%d" % (i, k), group=job, node="n%05d" % i, phase="Running",
                  priority_class="system-node-critical" if critical else "", containers=[kbgen.res(cpu=pc, mem=pm)])

    for i, kind in enumerate(kinds):
        if i in special:
            job, pc, pm = special[i]
            run(i, 0, job, pc, pm)
            run(i, 1, "fill", cpu - pc, mem - pm)
        else:
            run(i, 0, "blk" if kind == "g" else "crit", cpu, mem, critical=kind == "c")
    c.add_pod("ns", "pend-0", uid="p00000", group="pend", priority=5, ts=1, containers=[kbgen.res(cpu=5, mem=8 * GI)])
    return c


PROP_ACTED, PROP_STATELESS = [10, 70, 100], [10, 70, 80, 100]
# the second window answered with nothing applied after the first (see each builder)
UNAPPLIED = {"gang_carried": [70, 80, 100], "drf_carried": [70, 80, 100], "proportion_carried": [70, 80]}

# three score groups by the cpu of the node's pod (LeastRequested and BalancedResourceAllocation both fall
# with it: the groups' scores are far apart, the nodes of a group tie)
LOW, MID, HIGH = 1000, 7000, 13000


def _groups(n_low, n_mid, n_high):
    """Node indices: the MID group first, then HIGH, then LOW — the by-score walk is LOW, MID, HIGH (index
    order within a group), no prefix of it in index order."""
    cpu = [MID] * n_mid + [HIGH] * n_high + [LOW] * n_low
    mid, high, low = (list(range(n_mid)), list(range(n_mid, n_mid + n_high)),
                      list(range(n_mid + n_high, n_mid + n_high + n_low)))
    return cpu, low, mid, high


def ties(mode=1):
    """by_score: 60 nodes of the best score, then one run of 11 equal scores at walk positions 60 .. 70 —
    the window edge falls inside the run, so the index part of the resume key decides it — then 20 more.
    Positions 62 and 66 (both in the run) are VALID."""
    cpu, low, mid, high = _groups(60, 11, 20)
    walk = low + mid + high
    kinds = blocked(len(walk))
    kinds[walk[62]] = kinds[walk[66]] = "v"
    return build(kinds, mode, tiers=SCORED, cpu=cpu), walk


def negative(mode=1):
    """The same groups under a negative LeastRequested weight: every score is negative and the by-score walk
    is HIGH, MID, LOW.  Positions 5 and 70 are VALID."""
    cpu, low, mid, high = _groups(30, 11, 40)
    walk = high + mid + low
    kinds = blocked(len(walk))
    kinds[walk[5]] = kinds[walk[70]] = "v"
    return build(kinds, mode, tiers=SCORED, args=NEGATIVE, cpu=cpu), walk


def _scored(fn):
    n = len(fn()[1])
    return (lambda mode: fn(mode)[0]), (1, 2), list(range(n)), fn()[1]


CLUSTERS = {}
for _n in (64, 65, 128, 129, 130):
    CLUSTERS["len%d" % _n] = _plain(blocked(_n))
for _p in (0, 63, 64, 65, 129):
    CLUSTERS["covers_at%d" % _p] = _plain(with_kinds(130, {_p: "C"}))
    CLUSTERS["valid_at%d" % _p] = _plain(with_kinds(130, {_p: "v"}))
CLUSTERS["gang_carried"] = (gang_carried, (1, 2), list(range(130)), None)
CLUSTERS["drf_carried"] = (drf_carried, (2,), list(range(130)), None)
CLUSTERS["proportion_carried"] = (proportion_carried, (1,), list(range(130)), None)
CLUSTERS["ties"] = _scored(ties)
CLUSTERS["negative"] = _scored(negative)
CLUSTERS["long_node"] = _plain(with_kinds(90, {10: "v", 65: "L", 80: "C"}))
LENGTHS = {"len64": [(EXHAUSTED, 64, 64)], "len65": [(HEAD_END, 65, 64), (EXHAUSTED, 1, 1)],
           "len128": [(HEAD_END, 128, 64), (EXHAUSTED, 64, 64)],
           "len129": [(HEAD_END, 129, 64), (HEAD_END, 65, 64), (EXHAUSTED, 1, 1)],
           "len130": [(HEAD_END, 130, 64), (HEAD_END, 66, 64), (EXHAUSTED, 2, 2)]}  # (stop, remaining, visited) per call


def task_of(m):
    t = m.pending()
    assert len(t) == 1
    return t[0]


def walk_of(name, by_score):
    _, _, by_index, scored = CLUSTERS[name]
    return list(scored if by_score and scored is not None else by_index)


# ---- the protocol ----
def expected_calls(m, task, mode, walk, scores=None, cap=WINDOW, cap_ops=None, ov_max=0, limit=1000):
    """The calls of a host loop over kbhip_walk_victims_from and kbhip_apply_ops for a walk ranked once:
    [(ops, info)] with info = stop, remaining, visited, acted, resume_node, resume_score, last_node,
    first_valid.  walk: the whole pruned walk (nodes); scores: their scores, or None (by_score 0).  m is not
    changed."""
    m = copy.deepcopy(m)
    walk = [int(n) for n in walk]
    pos, resume, calls = 0, (-1, 0), []
    while True:
        assert len(calls) < limit
        dec = walk[pos:pos + WINDOW][:cap]
        first = next((i for i, n in enumerate(dec) if m.decide(task, mode, n)[2] & VALID), -1)
        ops, info = walkvictims.chain(m, task, mode, dec, cap_ops=cap_ops, ov_max=ov_max)
        res = info["visited"] - 1
        if info["stop"] == CAPACITY and info["last_node"] != dec[res]:
            res -= 1  # the node the walk stopped before is met again
        if info["stop"] == EXHAUSTED and len(walk) - pos > len(dec):
            info["stop"] = HEAD_END
        if res >= 0:
            resume = (dec[res], int(scores[pos + res]) if scores is not None else 0)
        info.update(remaining=len(walk) - pos, resume_node=resume[0], resume_score=resume[1], first_valid=first)
        calls.append((ops, info))
        m.records(records(ops))
        pos += res + 1
        if info["stop"] in (ASSIGNED, EXHAUSTED):
            return calls
        assert res >= 0 or ops == [] and cap_ops is not None  # (a call that cannot move asks for a larger cap_ops)
        if res < 0:
            return calls


INFO_KEYS = ("stop", "remaining", "visited", "acted", "resume_node", "resume_score", "last_node", "first_valid")


def protocol(ask, apply, limit=1000):
    """The host loop: ask(after) -> (ops, info) of kbhip_walk_victims_from, apply(ops).  Returns the calls."""
    after, calls = None, []
    while True:
        assert len(calls) < limit
        ops, info = ask(after)
        calls.append((ops, info))
        if ops:
            apply(ops)
        if info["stop"] in (ASSIGNED, EXHAUSTED):
            return calls
        nxt = (info["resume_node"], info["resume_score"])
        if not ops and nxt == (after or (-1, 0)) and info["stop"] == CAPACITY:
            return calls  # cap_ops below the next step's need
        after = nxt if nxt[0] >= 0 else None


def host_reclaim_walk_windows(m, ask, apply):
    """walkvictims.host_reclaim_walk with kbhip_walk_victims_from: reclaim.go:41-196 on gohost's ordering;
    ask(task, after) -> (ops, info) for the session as it stands, after: None or the resume point (node,
    score) of the call before; apply(ops) sends a batch back.  After a HEAD_END or CAPACITY stop the walk
    goes on from the resume point, whether or not the call acted.  Returns (the record log, the asks per
    popped task, the stops seen)."""
    h = m.h
    qheap, seen, jheaps, ptasks = gohost.GoHeap(h.queue_less), set(), {}, {}
    for k, j in enumerate(h.jobs):
        if j["queue"] not in seen:
            seen.add(j["queue"])
            qheap.push(j["queue"])
        pend = sorted((t for t in j["tasks"] if h.pods[t]["status"] == PENDING), key=h._task_key)
        if pend:
            jheaps.setdefault(j["queue"], gohost.GoHeap(h.job_less)).push(k)
            ptasks[k] = pend
    log, asks, stops = [], [], []
    while not qheap.empty():
        qn = qheap.pop()
        if h._overused(qn):
            continue
        jh = jheaps.get(qn)
        if jh is None or jh.empty():
            continue
        tq = ptasks[jh.pop()]
        if not tq:
            continue
        task = tq.pop(0)
        after, n_ask, assigned = None, 0, False
        while True:
            ops, info = ask(task, after)
            n_ask += 1
            stops.append(info["stop"])
            if ops:
                apply(ops)
                log += [(p, n, k) for p, n, k in records(ops)]
                m.records(records(ops))
            if info["stop"] in (ASSIGNED, EXHAUSTED):
                assigned = info["stop"] == ASSIGNED
                break
            nxt = (info["resume_node"], info["resume_score"])
            if not ops and nxt == (after or (-1, 0)):
                raise RuntimeError("the walk of task %d cannot move: cap_ops is below its next step" % task)
            after = nxt
        asks.append(n_ask)
        if assigned:
            qheap.push(qn)
    return log, asks, stops


def reclaim_snapshot():
    """A snapshot whose reclaim needs a walk of more than 64 entries: 70 nodes in index order, none VALID
    but position 66, which covers p0.  reclaim evicts there and pipelines p0."""
    return build(with_kinds(70, {66: "C"}), 1)
