"""The live cursor protocol (kbhip_walk_begin_live / kbhip_walk_next /
kbhip_apply_ops), restated for the CPU and GPU tests on walkvictims.chain over
victimmodel.VictimModel, and the small clusters it is checked on.

reclaim.go:115-117 tests PredicateFn at each node as the loop reaches it.  For
a task whose predicates read pod-affinity targets an eviction of the walk can
change that answer, so the live cursor keeps every node that passes the other
predicates and the victim-candidate test (index ascending) and tests the
affinity predicate (AffPred below: predicates.go:1402-1458 for a pod's own
required affinity terms) per call, on the statuses as they stand.  A call ends
behind the first node it acts on: its evictions reach the next call's tables
through kbhip_apply_ops.

The clusters are walkwindows' pods (v small victim, C covering victim, c
critical, L 257 small victims) on nodes with a zone and a hostname label; the
pending task p0 of queue q0 requires affinity to pods labelled app=y."""
import copy

import kbgen
import walkcursor as wc
import walkvictims
from gohost import ALLOCATED_STATUSES
from victimmodel import VALID
from walkvictims import ASSIGNED, CAPACITY, EXHAUSTED, HEAD_END, records
from walkwindows import GI, LONG, MI

TIER = [["gang", "conformance", "predicates"]]
HOSTNAME = "kubernetes.io/hostname"
Y = {"app": "y"}
LIVE = 2  # kbhip_walk_begin_live's out_info[3] for a live cursor


def build(spec, mode=1, topo="zone", self_match=False, affinity=True):
    """One node per entry of spec: (zone, [(kind, labelled y)]).  p0 requires affinity to app=y pods at
    topology `topo` (affinity False: no term at all) and carries the label itself with self_match.  Pod
    indices follow the nodes (UID order), p0 is the last."""
    c = kbgen.Cluster(tiers=TIER)
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    rq = "q1" if mode == 1 else "q0"
    for i, (zone, _) in enumerate(spec):
        c.add_node("n%05d" % i, 16000, 64 * GI, 0, 400, labels={"zone": zone, HOSTNAME: "n%05d" % i})
    for job in ("crit", "run", "big"):
        c.add_job("ns", job, rq, min_member=1)
    c.add_job("ns", "pend", "q0", min_member=1, ts=1)
    k = 0
    for i, (_, pods) in enumerate(spec):
        for kind, y in pods:
            for _ in range(LONG if kind == "L" else 1):
                c.add_pod("ns", "r%05d" % k, uid="a%05d" % k, group={"c": "crit", "v": "run", "C": "big", "L": "run"}[kind],
                          node="n%05d" % i, phase="Running", labels=dict(Y) if y else {},
                          priority_class="system-node-critical" if kind == "c" else "",
                          containers=[kbgen.res(cpu=10 if kind == "L" else 2000 if kind == "C" else 500,
                                                mem=MI if kind == "L" else 8 * GI if kind == "C" else GI)])
                k += 1
    aff = {"pod": {"required": [{"selector": {"ml": dict(Y)}, "topology_key": topo}]}} if affinity else None
    c.add_pod("ns", "pend-0", uid="p00000", group="pend", priority=5, ts=1, labels=dict(Y) if self_match else {},
              affinity=aff, containers=[kbgen.res(cpu=1000, mem=8 * GI)])
    return c


# leave: the only y pod of zone a is node 0's victim, too small to cover.  The reference evicts it, finds zone
# a without a target at node 1 (whose victim would cover) and assigns on node 2 in zone b, whose y pod is
# critical and stays.  A walk fixed at the start holds node 1 and assigns there.
LEAVE = [("a", [("v", 1)]), ("a", [("C", 0)]), ("b", [("c", 1), ("C", 0)]), ("b", [("c", 0)]), ("c", [])]
# enter: p0 carries the label and asks for it on its own host.  While node 0's y pod is a target only node 0
# passes; once it is evicted no target matches anywhere and p0 matches its own term (metadata.go:498-509), so
# every node passes: the reference assigns on node 1.  A walk fixed at the start holds node 0 alone.
ENTER = [("a", [("v", 1)]), ("a", [("C", 0)]), ("a", [("C", 0)]), ("a", [("c", 0)])]
# spill: a 257-task node in a zone without a target ahead of two VALID nodes of zone b
SPILL = [("a", [("L", 0)]), ("b", [("c", 1), ("v", 0)]), ("b", [("C", 0)]), ("a", [("v", 0)])]
CLUSTERS = {
    "leave": lambda mode=1: build(LEAVE, mode),
    "enter": lambda mode=1: build(ENTER, mode, topo=HOSTNAME, self_match=True),
    "control": lambda mode=1: build(LEAVE, mode, affinity=False),
    "spill": lambda mode=1: build(SPILL, mode),
}
EXPECTED_NODES = {"leave": [0, 2, 2], "enter": [0, 1, 1]}  # the nodes of the reference's records
BIG_N, BIG_GRID, BIG_FIRST = 2100, 2048, 2090


def big(mode=1):
    """2100 entries, more than one scan grid: every node holds a small victim (VALID), all in zone a, which
    has no target, but node 2090 in zone b, whose victim covers next to a critical y pod."""
    return build([("b", [("c", 1), ("C", 0)]) if i == BIG_FIRST else ("a", [("v", 0)]) for i in range(BIG_N)], mode)


class AffPred:
    """A pending pod's own required pod-affinity terms against the model's statuses: targets are the
    AllocatedStatuses tasks of session jobs on a node (plugins/predicates/predicates.go:59-94)."""

    def __init__(self, c):
        self.pods = sorted(c.pods, key=lambda p: p.uid)
        self.nodes = sorted(c.nodes, key=lambda n: n.name)
        for p in self.pods:  # what the clusters here use, and nothing else
            a = p.affinity or {}
            assert set(a) <= {"pod"} and not (a.get("pod") or {}).get("preferred")
            assert p.phase == "Running" and p.node and not a or p.phase == "Pending" and not p.node

    def terms(self, task):
        return ((self.pods[task].affinity or {}).get("pod") or {}).get("required") or []

    def _matches(self, task, p):
        q = self.pods[p]
        return all(q.ns in (t.get("namespaces") or [self.pods[task].ns]) and not t["selector"].get("me") and
                   all(q.labels.get(k) == v for k, v in t["selector"]["ml"].items()) for t in self.terms(task))

    def holds(self, m, task, node):
        terms = self.terms(task)
        if not terms:
            return True
        targets = [p for p in range(len(self.pods)) if m.status(p) in ALLOCATED_STATUSES and m.node[p] >= 0 and
                   m.job(p) is not None and self._matches(task, p)]
        if not targets:
            return self._matches(task, task)
        here = self.nodes[node].labels
        for p in targets:
            there = self.nodes[m.node[p]].labels
            if all(t["topology_key"] in here and here[t["topology_key"]] == there.get(t["topology_key"]) for t in terms):
                return True
        return False


def live_order(m, task, mode):
    """The kept order of kbhip_walk_begin_live: the nodes with victim candidates that are not strictly short
    of InitResreq in all three resources, index ascending (every node of these clusters passes the static
    predicates, pod count and host ports)."""
    out = []
    for n in range(m.n_nodes):
        cands = m.candidates(task, mode, n)
        total = [sum(m.req[v][k] for v in cands) for k in range(3)]
        if cands and not all(t < r for t, r in zip(total, m.ireq[task])):
            out.append(n)
    return out


def fixed_order(m, aff, task, mode):
    """kbhip_walk_begin(task, 0, ..)'s: the live order's nodes that pass the affinity predicate at the start."""
    return [n for n in live_order(m, task, mode) if aff.holds(m, task, n)]


def expected_live_calls(m, aff, task, mode, walk, cap=64, cap_ops=None, ov_max=0, limit=1000, spill=()):
    """The calls of a host loop over kbhip_walk_next on a live cursor and kbhip_apply_ops: [(ops, info)] with
    info as walkcursor.expected_cursor_calls gives it.  walk: the live order.  An entry can act only where
    aff.holds on the model as it stands; `first` is the lowest such entry at or behind pos that the model
    decides VALID, or a node of `spill` whatever it would answer (the scan decides neither the predicate nor
    the victims of a node longer than its LDS rows).  The serial part is chain over the entries of
    [first, first + cap) that pass the predicate, cut behind its first acting node.  m is not changed."""
    m = copy.deepcopy(m)
    walk = [int(n) for n in walk]
    total, pos, calls = len(walk), 0, []
    while True:
        assert len(calls) < limit
        ok = {n: aff.holds(m, task, n) for n in set(walk[pos:])}
        first = next((i for i in range(pos, total)
                      if walk[i] in spill or ok[walk[i]] and m.decide(task, mode, walk[i])[2] & VALID), total)
        dec = walk[first:first + cap]
        passing = [n for n in dec if ok[n]]
        ops, info = walkvictims.chain(m, task, mode, passing, cap_ops=cap_ops, ov_max=ov_max)
        if ops:  # the first acting node ends the call
            node = ops[0][2]
            ops = [o for o in ops if o[2] == node]
            k = dec.index(node)
            nxt, decided = first + k + 1, k + 1
            uncarried = info["stop"] == CAPACITY and info["acted"] == 1 and info["last_node"] == node
            stop = (ASSIGNED if ops[-1][0] == walkvictims.PIPELINE else CAPACITY if uncarried else
                    HEAD_END if nxt < total else EXHAUSTED)
        elif info["stop"] == CAPACITY:  # refused before it acted: the entry is met again
            node, k = -1, dec.index(passing[info["visited"] - 1])
            nxt, decided, stop = first + k, k + 1, CAPACITY
        else:
            node, nxt, decided = -1, first + len(dec), len(dec)
            stop = HEAD_END if nxt < total else EXHAUSTED
        info = dict(stop=stop, total=total, decided=first - pos + decided, acted=1 if ops else 0, next=nxt,
                    first=first if first < total else -1, last_node=node)
        calls.append((ops, info))
        m.records(records(ops))
        if stop in (ASSIGNED, EXHAUSTED) or nxt == pos and not ops:
            return calls
        pos = nxt


def expected_calls(m, aff, task, mode, cap=64, **kw):
    """What a host loop sees behind kbhip_walk_begin_live: the live protocol for a task whose class reads
    affinity targets, else kbhip_walk_begin(task, 0, ..)'s cursor.  -> (the kept order, the calls, live)"""
    if aff.terms(task):
        order = live_order(m, task, mode)
        return order, expected_live_calls(m, aff, task, mode, order, cap, **kw), True
    order = fixed_order(m, aff, task, mode)
    return order, wc.expected_cursor_calls(m, task, mode, order, None, cap, **kw), False


def host_reclaim_walk_live(m, begin, ask, apply):
    """reclaim on the live cursor, the counterpart of walkcursor.host_reclaim_walk_cursor: begin(task) opens
    the popped task's cursor with kbhip_walk_begin_live, ask(pos) -> (ops, info) of kbhip_walk_next,
    apply(ops) sends a batch back before the next ask.  The loop is the fixed cursor's: only the calls behind
    begin and ask differ.  Returns (the record log, the asks per popped task, the stops seen)."""
    return wc.host_reclaim_walk_cursor(m, begin, ask, apply)


def restated_reclaim(c, mode=1, live=True):
    """The record log of reclaim on cluster c with every popped task's walk restated: the live protocol, or
    the protocol over the order fixed at the start (walkcursor.expected_cursor_calls)."""
    import victimmodel
    m, aff = victimmodel.VictimModel(c), AffPred(c)
    log = []

    def walk_task(task):
        if live:
            calls = expected_live_calls(m, aff, task, mode, live_order(m, task, mode))
        else:
            calls = wc.expected_cursor_calls(m, task, mode, fixed_order(m, aff, task, mode))
        for ops, _ in calls:
            log.extend(records(ops))
            m.records(records(ops))
        return calls[-1][1]["stop"] == ASSIGNED

    wc.host_reclaim(m, walk_task)
    return log
