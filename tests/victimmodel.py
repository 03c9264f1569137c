"""The victim choice of reclaim / preempt on one node, restated from the
reference's plugin sources for the tests of kbhip_head_victims.

Session.Reclaimable / Session.Preemptable (session_plugins.go:67-148) over the
four victim functions (gang.go:107-129, conformance.go:37-56, drf.go:84-109,
proportion.go:159-183), validateVictims (preempt.go:355-370) and the eviction
loop (reclaim.go / preempt.go:300-320), on a kbgen.Cluster.  The drf /
proportion / gang state is opened as tests/gohost.py opens it (its _share, _le
and the deserved water-filling are used, not copied) and then follows the
allocate / deallocate event handlers (drf.go:134-155, proportion.go:200-227)
through evict, pipeline, unpipeline and unevict.

Indices are the snapshot's: pods by UID, nodes by name, jobs by UID."""
import gohost
from gohost import ALLOCATED, ALLOCATED_STATUSES, PENDING, PIPELINED, RELEASING, RUNNING, _le, _share

MINS = (10, 10 * 1024 * 1024, 10)
VALID, COVERS = 1, 2
GANG_READY = ALLOCATED_STATUSES + ("Succeeded", PIPELINED)  # gang.go:212-222


def _le_tol(a, b):  # Resource.LessEqual on the integer requests
    return all(x - y < m for x, y, m in zip(a, b, MINS))


class VictimModel:
    def __init__(self, c):
        self.h = gohost.GoHost(c)  # drf / proportion opened
        h = self.h
        h._job_of = {j["uid"]: j for j in h.jobs}
        self.job_index = {j["uid"]: i for i, j in enumerate(h.jobs)}
        self.queue_index = {n: i for i, n in enumerate(sorted(h.queues))}
        nodes = {n: i for i, n in enumerate(sorted(x.name for x in c.nodes))}
        self.n_nodes = len(nodes)
        pods = sorted(c.pods, key=lambda p: p.uid)
        self.node, self.critical, self.req, self.ireq, self.detached = [], [], [], [], []
        for p in pods:
            self.node.append(nodes[p.node] if p.node else -1)
            self.critical.append(p.ns == "kube-system" or
                                 p.priority_class in ("system-cluster-critical", "system-node-critical"))
            r = [sum(x.get(k, 0) for x in p.containers) for k in ("cpu", "mem", "gpu")]
            self.req.append(r)
            self.ireq.append([max([r[i]] + [x.get(k, 0) for x in p.init_containers])
                              for i, k in enumerate(("cpu", "mem", "gpu"))])
            self.detached.append(bool(p.detached))
        self.node_rel = [False] * len(pods)
        dis = {p: set(f) for p, f in c.flags.items()}
        self.codes = {}
        for preempt in (False, True):
            flag = "disablePreemptable" if preempt else "disableReclaimable"
            own = ("gang", "conformance") + (("drf",) if preempt else ("proportion",))
            self.codes[preempt] = [[p for p in t if p in own and flag not in dis.get(p, ())] for t in c.tiers]

    # ---- the state ----
    def status(self, p):
        return self.h.pods[p]["status"]

    def job(self, p):
        return self.h._job_of.get(self.h.pods[p]["job"])

    def ready(self, j):
        return sum(self.h.pods[t]["status"] in GANG_READY for t in j["tasks"])

    def pending(self):
        return [p for p in range(len(self.node)) if self.status(p) == PENDING and self.job(p) is not None]

    # ---- the event handlers and statement operations ----
    def _on_deallocate(self, p):  # drf.go:144-155, proportion.go:211-227
        j, req = self.job(p), self.h.pods[p]["req"]
        if self.h.drf_on:
            j["drf_alloc"] = [a - b for a, b in zip(j["drf_alloc"], req)]
            j["drf"] = max(_share(a, b) for a, b in zip(j["drf_alloc"], self.h.total))
        if self.h.prop_on:
            q = self.h.queues[j["queue"]]
            q["allocated"] = [a - b for a, b in zip(q["allocated"], req)]
            self.h._prop_share(q)

    def _set_status(self, p, st):  # JobInfo.UpdateTaskStatus: the allocated count, and the job takes the task's priority
        j, pod = self.job(p), self.h.pods[p]
        j["alloc_n"] += (st in ALLOCATED_STATUSES) - (pod["status"] in ALLOCATED_STATUSES)
        j["prio"] = pod["prio"]
        pod["status"] = st

    def evict(self, p):
        assert self.status(p) == RUNNING and not self.node_rel[p]
        self._set_status(p, RELEASING)
        self._on_deallocate(p)

    def unevict(self, p):
        self._set_status(p, RUNNING)
        self.node_rel[p] = True
        self.h._on_allocate(p)

    def pipeline(self, p, n):
        self._set_status(p, PIPELINED)
        self.node[p] = n
        self.h._on_allocate(p)

    def unpipeline(self, p):
        self._set_status(p, PENDING)
        self._on_deallocate(p)

    def records(self, rec):
        """Records of an action (pod, node, TaskStatus code): 128 evicted, 8 pipelined, 4 allocated."""
        for p, n, k in rec:
            if k == 128:
                self.evict(p)
            elif k == 8:
                self.pipeline(p, n)
            else:
                self._set_status(p, ALLOCATED)
                self.node[p] = n
                self.h._on_allocate(p)

    # ---- the victim choice ----
    def candidates(self, task, mode, node):
        """The node's tasks the mode's loop hands to the victim functions, in pod-index order."""
        tj = self.job(task)
        out = []
        for p in range(len(self.node)):
            if self.node[p] != node or self.status(p) != RUNNING or self.node_rel[p] or self.detached[p]:
                continue
            j = self.job(p)
            if j is None:
                continue
            same_q, same_j = j["queue"] == tj["queue"], j is tj
            if (mode == 1 and same_q) or (mode == 2 and (not same_q or same_j)) or (mode == 3 and not same_j):
                continue
            out.append(p)
        return out

    def _answer(self, name, task, evictees):
        h = self.h
        if name == "gang":
            return [e for e in evictees
                    if self.job(e)["min"] <= self.ready(self.job(e)) - 1 or self.job(e)["min"] == 1]
        if name == "conformance":
            return [e for e in evictees if not self.critical[e]]
        out = []
        if name == "drf":
            la = [a + b for a, b in zip(self.job(task)["drf_alloc"], h.pods[task]["req"])]
            ls = max(_share(a, t) for a, t in zip(la, h.total))
            alloc = {}
            for e in evictees:
                j = self.job(e)
                cur = alloc.setdefault(j["uid"], list(j["drf_alloc"]))
                cur[:] = [a - b for a, b in zip(cur, h.pods[e]["req"])]
                rs = max(_share(a, t) for a, t in zip(cur, h.total))
                if ls < rs or abs(ls - rs) <= 0.000001:
                    out.append(e)
            return out
        assert name == "proportion"
        alloc = {}
        for e in evictees:
            q = h.queues[self.job(e)["queue"]]
            cur = alloc.setdefault(q["name"], list(q["allocated"]))
            req = h.pods[e]["req"]
            if all(a < b for a, b in zip(cur, req)):  # allocated.Less(Resreq): skipped, nothing subtracted
                continue
            cur[:] = [a - b for a, b in zip(cur, req)]
            if _le(q["deserved"], cur):
                out.append(e)
        return out

    def victims(self, task, mode, node):
        evictees = self.candidates(task, mode, node)
        if not evictees:
            return []
        victims, init = [], False
        for tier in self.codes[mode != 1]:
            for name in tier:
                if name == "drf" and not self.h.drf_on or name == "proportion" and not self.h.prop_on:
                    continue
                got = set(self._answer(name, task, evictees))
                victims = [v for v in (victims if init else evictees) if v in got]
                init = True
            if victims:
                return victims
        return []

    def decide(self, task, mode, node):
        """(victims, evicted prefix, flags) as kbhip_head_victims defines them."""
        victims = self.victims(task, mode, node)
        need = self.ireq[task]
        total = [sum(self.req[v][k] for v in victims) for k in range(3)]
        if not victims or all(t < n for t, n in zip(total, need)):
            return victims, 0, 0
        left, got, evict = list(need), [0, 0, 0], 0
        for v in victims:
            evict += 1
            got = [a + b for a, b in zip(got, self.req[v])]
            if _le_tol(left, self.req[v]):
                break
            left = [a - b for a, b in zip(left, self.req[v])]
        return victims, evict, VALID | (COVERS if _le_tol(need, got) else 0)


def host_reclaim(m, ask, apply):
    """reclaim.go:41-196 on gohost's queue / job / task ordering.  ask(task, after) -> the head rows
    [(node, victims, evict, flags)] of the task's walk in walk order, for the session as it stands;
    apply(ops) sends [(kind, pod, node)] (128 evict, 8 pipeline) back.  The walk of a task is fixed when the
    task is popped (the reference evaluates the predicates once): later answers are read only for nodes of
    that walk after the node last acted on.  Returns the record log [(pod, node, kind)]."""
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
    log = []
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
        walk, at, assigned = None, -1, False
        while not assigned:
            rows = ask(task)
            if walk is None:
                walk = [r[0] for r in rows]
            rows = {r[0]: r for r in rows}
            acted = False
            for i in range(at + 1, len(walk)):
                r = rows.get(walk[i])
                if r is None or not r[3] & VALID:
                    continue
                node, victims, evict, flags = r
                ops = [(128, int(v), m.node[int(v)]) for v in victims[:evict]]
                if flags & COVERS:
                    ops.append((8, task, node))
                    assigned = True
                apply(ops)
                log += [(p, n, k) for k, p, n in ops]
                m.records([(p, n, k) for k, p, n in ops])
                at, acted = i, True
                break
            if not acted:
                break
        if assigned:
            qheap.push(qn)
    return log
