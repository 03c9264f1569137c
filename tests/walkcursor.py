"""The cursor protocol (kbhip_walk_begin / kbhip_walk_next / kbhip_apply_ops),
restated for the CPU and GPU tests on walkvictims.chain over
victimmodel.VictimModel.

A walk is ranked once.  Each call finds `first`, the lowest position at or
behind `pos` whose node the model decides VALID as it stands — what the scan
answers — passes over the entries before it, and runs chain over at most `cap`
entries from there; the model is then moved on by the ops, as kbhip_apply_ops
moves the session."""
import copy

import walkvictims
from victimmodel import VALID
from walkvictims import ASSIGNED, CAPACITY, EXHAUSTED, HEAD_END, records

INFO_KEYS = ("stop", "total", "decided", "acted", "next", "first", "last_node")


def expected_cursor_calls(m, task, mode, walk, scores=None, cap=64, cap_ops=None, ov_max=0, limit=1000, spill=()):
    """The calls of a host loop over kbhip_walk_next and kbhip_apply_ops: [(ops, info)] with info = stop,
    total, decided, acted, next, first, last_node.  walk: the whole pruned walk (nodes), ranked once; scores:
    unused (the positions carry the order).  spill: the nodes that hold more candidate records than a scan
    block stages (256, counted when the victim state was built): the scan does not decide them, they count
    as `first` whether VALID or not, and the serial chain decides them.  m is not changed."""
    m = copy.deepcopy(m)
    walk = [int(n) for n in walk]
    total, pos, calls = len(walk), 0, []
    while True:
        assert len(calls) < limit
        first = next((i for i in range(pos, total)
                      if walk[i] in spill or m.decide(task, mode, walk[i])[2] & VALID), total)
        dec = walk[first:first + cap]
        ops, info = walkvictims.chain(m, task, mode, dec, cap_ops=cap_ops, ov_max=ov_max)
        res = info["visited"] - 1
        if info["stop"] == CAPACITY and info["last_node"] != dec[res]:
            res -= 1  # the node the walk stopped before is met again
        if info["stop"] == EXHAUSTED and first + len(dec) < total:
            info["stop"] = HEAD_END
        nxt = first + res + 1
        info = dict(stop=info["stop"], total=total, decided=first - pos + info["visited"], acted=info["acted"],
                    next=nxt, first=first if first < total else -1, last_node=info["last_node"])
        calls.append((ops, info))
        m.records(records(ops))
        if info["stop"] in (ASSIGNED, EXHAUSTED):
            return calls
        assert nxt > pos or ops == [] and cap_ops is not None  # (a call that cannot move asks for a larger cap_ops)
        if nxt == pos and not ops:
            return calls
        pos = nxt


def protocol(ask, apply, limit=1000):
    """The host loop: ask(pos) -> (ops, info) of kbhip_walk_next, apply(ops).  Returns the calls."""
    pos, calls = 0, []
    while True:
        assert len(calls) < limit
        ops, info = ask(pos)
        calls.append((ops, info))
        if ops:
            apply(ops)
        if info["stop"] in (ASSIGNED, EXHAUSTED):
            return calls
        if not ops and info["next"] == pos and info["stop"] == CAPACITY:
            return calls  # cap_ops below the next step's need
        assert info["next"] > pos or ops
        pos = info["next"]


def host_reclaim(m, walk_task):
    """reclaim.go:41-196 on gohost's queue / job / task ordering, the node loop of each popped task left to
    walk_task(task) -> assigned.  (walkwindows.host_reclaim_walk_windows keeps its own copy of this pop loop.)"""
    import gohost
    from gohost import PENDING
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
    while not qheap.empty():
        qn = qheap.pop()
        if h._overused(qn):
            continue
        jh = jheaps.get(qn)
        if jh is None or jh.empty():
            continue
        tq = ptasks[jh.pop()]
        if tq and walk_task(tq.pop(0)):
            qheap.push(qn)


def host_reclaim_walk_cursor(m, begin, ask, apply):
    """reclaim on the cursor: begin(task) ranks the popped task's walk once, ask(pos) -> (ops, info) of
    kbhip_walk_next, apply(ops) sends a batch back.  Returns (the record log, the asks per popped task, the
    stops seen)."""
    log, asks, stops = [], [], []

    def walk_task(task):
        begin(task)
        pos, n_ask = 0, 0
        while True:
            ops, info = ask(pos)
            n_ask += 1
            stops.append(info["stop"])
            if ops:
                apply(ops)
                log.extend((p, n, k) for p, n, k in records(ops))
                m.records(records(ops))
            if info["stop"] in (ASSIGNED, EXHAUSTED):
                asks.append(n_ask)
                return info["stop"] == ASSIGNED
            if not ops and info["next"] == pos:
                raise RuntimeError("the walk of task %d cannot move: cap_ops is below its next step" % task)
            pos = info["next"]

    host_reclaim(m, walk_task)
    return log, asks, stops


# ---- a walk longer than two scan grids ------------------------------------------------------------------
BIG_N, BIG_GRID = 4500, 2048  # (kWalkScanBlocks, kbhip_victims.hip: a scan block takes every 2048th entry)
BIG_VALID, BIG_LONG, BIG_LONG_REFUSED, BIG_COVERS = 10, 100, 200, 4400
BIG_FIRSTS = [10, 100, 200, 4400]
# the calls start at 0, 74, 164 and 264.  Every scan but the last finds its `first` within the blocks' first
# entries, and the blocks in front of it end on their second entry, after they have decided one; the last
# call's `first` lies more than two grids behind its position (4136 entries), so the blocks of that scan
# decide two or three entries each before they meet the result.  (The walk is as short as that allows: the
# restatement's decide reads every pod of the model.)
BIG_STARTS = [0, 74, 164, 264]


def big_walk(mode=1):
    """walkwindows.build over 4500 blocked entries — more than two scan grids — with a VALID node at position
    10, a VALID 257-task node at 100, a 257-task node at 200 whose tasks are all critical (conformance
    refuses them: not VALID, and longer than the LDS rows, so the scan reports it and the serial loop passes
    it over), and a covering node at 4400.  -> (cluster, the nodes longer than the LDS rows)"""
    import walkwindows as ww
    c = ww.build(ww.with_kinds(BIG_N, {BIG_VALID: "v", BIG_LONG: "L", BIG_LONG_REFUSED: "L", BIG_COVERS: "C"}), mode)
    for p in c.pods:
        if p.node == "n%05d" % BIG_LONG_REFUSED:
            p.group, p.priority_class = "crit", "system-node-critical"
    return c, {BIG_LONG, BIG_LONG_REFUSED}
