"""One task's eviction walk, restated for the tests of kbhip_walk_victims.

chain() is the node loop of preempt() (preempt.go:259-353) and of reclaim
(reclaim.go:115-189) over a node list, on a deep copy of a
victimmodel.VictimModel: decide on each node; a node whose victims pass
validateVictims is evicted from, whether or not the evicted prefix covers
InitResreq; a covering node pipelines the task and ends the loop.  The model's
own event handlers carry the evictions to the next node, so nothing of the
library's overlay is restated here — only its two capacity rules, which are
part of the call's contract (include/kbhip.h): a step needs the prefix plus one
slot of cap_ops, and a node the walk goes on from may not bring the touched
jobs or queues above the overlay's capacity.

host_reclaim_walk() is reclaim.go:41-196 on gohost's ordering with one `ask`
per popped task."""
import copy

import gohost
from gohost import PENDING
from victimmodel import COVERS, VALID

ASSIGNED, EXHAUSTED, HEAD_END, CAPACITY = 1, 2, 3, 4
EVICT, PIPELINE = 1, 2  # KBHIP_OP_*
OV_JOBS, OV_QUEUES = 256, 64


def chain(m, task, mode, nodes, cap_ops=None, ov_max=0, carried=True):
    """-> (ops [(op, pod, node)], info) with info = dict(stop, visited, acted, last_node).
    carried=False answers every node against the state before the walk (what a walk without carried state
    would give: the edge cases must differ from it)."""
    w = copy.deepcopy(m)
    base = copy.deepcopy(m) if not carried else None
    cap_j, cap_q = (min(ov_max, OV_JOBS), min(ov_max, OV_QUEUES)) if ov_max else (OV_JOBS, OV_QUEUES)
    ops, jobs, queues = [], set(), set()
    info = dict(stop=EXHAUSTED, visited=0, acted=0, last_node=-1)
    for node in nodes:
        node = int(node)
        victims, evict, flags = (w if carried else base).decide(task, mode, node)
        info["visited"] += 1
        if not flags & VALID:
            continue
        if cap_ops is not None and len(ops) + evict + 1 > cap_ops:
            info["stop"] = CAPACITY
            break
        prefix = victims[:evict]
        uncarried = False
        if not flags & COVERS:
            nj = jobs | {w.job(v)["uid"] for v in prefix}
            nq = queues | {w.job(v)["queue"] for v in prefix}
            if len(nj) > cap_j or len(nq) > cap_q:
                if info["acted"]:
                    info["stop"] = CAPACITY
                    break
                uncarried = True  # the first step of a call is taken whatever it touches; the walk stops behind it
            jobs, queues = nj, nq
        for v in prefix:
            ops.append((EVICT, v, node))
            w.evict(v)
        info["acted"] += 1
        info["last_node"] = node
        if flags & COVERS:
            ops.append((PIPELINE, task, node))
            info["stop"] = ASSIGNED
            break
        if uncarried:
            info["stop"] = CAPACITY
            break
    return ops, info


def as_ops(got):
    """(ops, pods, nodes, info) of the bindings -> [(op, pod, node)]."""
    return [(int(o), int(p), int(n)) for o, p, n in zip(got[0], got[1], got[2])]


def records(ops):
    """-> victimmodel records (pod, node, TaskStatus code)."""
    return [(p, n, 128 if o == EVICT else 8) for o, p, n in ops]


def host_reclaim_walk(m, ask, apply):
    """reclaim.go:41-196 on gohost's queue / job / task ordering.  ask(task, after) -> (ops [(op, pod,
    node)], info) of kbhip_walk_victims for the session as it stands (after: None or (node, score));
    apply(ops) sends a batch back.  One ask per popped task; another only after a CAPACITY or HEAD_END stop,
    resumed after the last acted-on node.  Returns (the record log [(pod, node, kind)], the asks per popped
    task, the stops seen)."""
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
            if info["acted"] == 0:  # nothing to resume after: the walk went past the head
                raise NotImplementedError("the walk of task %d leaves the 64-entry head" % task)
            after = (info["last_node"], info["last_score"])
        asks.append(n_ask)
        if assigned:
            qheap.push(qn)
    return log, asks, stops
