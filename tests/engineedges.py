"""Hand-placed clusters at the edges of the persistent pop engine's structure.

The engine is exact by a structural argument: workers
sweep fixed node ranges on rows four pops old and leave out the candidates of
pops p-3 and p-2, lists of 128 keys are merged through up to three levels with
"lowest node index wins", the placer re-evaluates the last pops' candidates,
owners keep one byte per node in segments of 1 792.  The clusters here put the
deciding nodes of a session on those structures' seams and limits:

A  partition seams and tie cuts in sweep mode (engine_workers, engine_groups),
B  stale rows: pops that want the nodes the previous four pops just changed,
   until a node is exactly full (request == idle) and must vanish,
C  owner limits in list mode (segment seams, 127 / 128 score levels, a
   backlog of more than 2 x 64 pops, 254 / 255 classes),
D  run boundaries: engine runs of 1, 15, 16, 17 and 64 pops between launched
   pops, and sessions of exactly 8, 9, 16 and 17 pops (the descriptor rings).

CASES is a list of (name, builder, options, claims).  builder(kbgen) returns a
kbgen.Cluster whose `edge` attribute (Edge) describes its gangs: every job is
a gang of one task class whose MinAvailable is its size, so the session pops
the gangs in order and one chunk of up to 64 tasks is one pop.  options are
the set_option pairs the case runs under; claims are the structural facts the
case exists for, checked on a placement log by check_claims() (expectations
written down from the cluster's construction, never read from a log), plus the
engine shape a device run must report (workers, owners, all_engine).

The tiers are [priority, gang] [predicates, nodeorder]: no drf / proportion,
so the job order is the creation order whatever was placed before.
"""
import scoreedges as se

GI = 1 << 30
MI = 1 << 20
TIERS = [["priority", "gang"], ["predicates", "nodeorder"]]
# Without nodeorder every node that passes scores 0: the whole cluster is one
# tie and the key is the node index alone.  The faithful restatement's
# nodeorder is quadratic in the nodes per task (its inter-pod priority visits
# every node for every node: 0.2 s per task at 845 nodes, 4 s at 3 585, about
# 20 s at 8 193), so the clusters of more than 257 nodes run under these tiers
# and decide by fit; those up to 257 nodes decide by score.
TIERS_NOSCORE = [["priority", "gang"], ["predicates"]]
SCORED_MAX = 257
CHUNK = 64          # kMaxChunk: tasks per pop
ENG_MAX_NPB = 8192  # kEngMaxNpb
OWN_SEG = 1792      # kOwnSeg


def eng_shape(n, workers):
    """(nw, npb) as session/03_pop.cpp eng_size takes them in sweep mode."""
    nw = min(workers, max(1, (n + 63) // 64))
    return nw, (n + nw - 1) // nw


class Edge:
    """gangs[g] = dict(first, size, cls, min, eligible): pod indices first ..
    first + size - 1; req[cls] = (cpu, mem, gpu) requests; idle[n] = (cpu, mem,
    gpu) before the session; exact = {gang: expected nodes in order}."""

    def __init__(self):
        self.gangs, self.req, self.idle, self.exact = [], {}, [], {}


class _Builder:
    def __init__(self, kbgen, args=None, scored=True):
        self.c = kbgen.Cluster(tiers=TIERS if scored else TIERS_NOSCORE, actions="allocate", args=args)
        self.c.add_queue("q0", 1)
        self.e = Edge()
        self.n_run = 0
        self.classes = {}

    def node(self, cpu, mem, gpu=0, labels=None, run=None):
        """run: the containers' dict of one Running pod on the node."""
        i = len(self.c.nodes)
        name = f"n{i:05d}"
        self.c.add_node(name, cpu, mem, gpu, 110, labels=dict(labels or {}))
        idle = [cpu, mem, gpu]
        if run is not None:
            if not self.n_run:
                self.c.add_job("ns", "run", "q0", min_member=1, ts=0)
            # ("r" sorts after the gangs' "g": pending pods keep the first indices)
            self.c.add_pod("ns", f"r{i:05d}", uid=f"r{i:05d}", group="run", node=name, phase="Running",
                           containers=[dict(run)])
            self.n_run += 1
            for k, key in enumerate(("cpu", "mem", "gpu")):
                idle[k] -= run.get(key, 0)
        self.e.idle.append(tuple(idle))
        return i

    def cls(self, name, ctr, affinity=None, eligible=True):
        self.classes[name] = (dict(ctr), affinity, eligible)
        self.e.req[name] = (ctr.get("cpu", 0), ctr.get("mem", 0), ctr.get("gpu", 0))

    def gang(self, cls, size, min_member=None):
        g = len(self.e.gangs)
        ctr, aff, eligible = self.classes[cls]
        jn = f"g{g:03d}"
        self.c.add_job("ns", jn, "q0", min_member=size if min_member is None else min_member, ts=g + 1)
        first = sum(x["size"] for x in self.e.gangs)
        for k in range(size):
            self.c.add_pod("ns", f"{jn}-{k:03d}", uid=f"{jn}-{k:03d}", group=jn, ts=g + 1, affinity=aff,
                           containers=[dict(ctr)])
        self.e.gangs.append(dict(first=first, size=size, cls=cls, min=size if min_member is None else min_member,
                                 eligible=eligible))
        return g

    def done(self):
        assert len(self.e.gangs) <= 1000
        self.c.edge = self.e
        return self.c


# ----------------------------------------------------------------------------
# reading a placement log
# ----------------------------------------------------------------------------
def pops_of(edge, log):
    """The session's pops in order: (gang, class, [nodes placed]).  A gang is
    popped once (MinAvailable = size: ready only with its last task); its
    tasks go in chunks of 64, and the pop of a chunk whose task finds no node
    ends the gang.  A chunk that places nothing is still a pop."""
    by_pod = {}
    for i, (pod, node, _) in enumerate(log):
        assert pod not in by_pod, f"pod {pod} placed twice"
        by_pod[pod] = (i, node)
    pops, seen = [], 0
    for g, gang in enumerate(edge.gangs):
        placed = 0
        while placed < gang["size"] and gang["first"] + placed in by_pod:
            i, _ = by_pod[gang["first"] + placed]
            assert i == seen, f"gang {g}: task {placed} is log entry {i}, expected {seen} (gangs in order)"
            seen += 1
            placed += 1
        for k in range(placed, gang["size"]):
            assert gang["first"] + k not in by_pod, f"gang {g}: task {k} placed after task {placed} found no node"
        for start in range(0, gang["size"], CHUNK):
            if start > placed:
                break
            end = min(start + CHUNK, gang["size"], placed)
            pops.append((g, gang["cls"], [by_pod[gang["first"] + k][1] for k in range(start, end)]))
            if placed < min(start + CHUNK, gang["size"]):
                break
    assert seen == len(log), "log entries outside the gangs"
    return pops


def _fits(idle, req):
    return all(r <= i for r, i in zip(req, idle))


def lags_seen(pops):
    """{lag: pop index}: pop p places on a node that pop p - lag placed on."""
    out = {}
    for p, (_, _, nodes) in enumerate(pops):
        for lag in (1, 2, 3, 4):
            if p - lag >= 0 and lag not in out and set(nodes) & set(pops[p - lag][2]):
                out[lag] = p
    return out


def vanished(edge, pops):
    """[(pop, node)]: node was the first (best) placement of pop p-1, fitted
    pop p's class before pop p-1 and does not fit it after: on a key four pops
    stale it is still the best node of pop p's class."""
    idle = [list(x) for x in edge.idle]
    out = []
    for p, (_, cls, nodes) in enumerate(pops):
        if p + 1 < len(pops) and nodes:
            nxt = edge.req[pops[p + 1][1]]
            before = _fits(idle[nodes[0]], nxt)
        for n in nodes:
            for k in range(3):
                idle[n][k] -= edge.req[cls][k]
            assert min(idle[n]) >= 0, f"pop {p}: node {n} over-committed"
        if p + 1 < len(pops) and nodes and before and not _fits(idle[nodes[0]], nxt):
            out.append((p + 1, nodes[0]))
    return out


def exact_full(edge, pops):
    """Nodes that some placement filled exactly (request == idle in a resource it asks for)."""
    idle = [list(x) for x in edge.idle]
    out = set()
    for _, cls, nodes in pops:
        for n in nodes:
            if any(r > 0 and r == i for r, i in zip(edge.req[cls], idle[n])):
                out.add(n)
            for k in range(3):
                idle[n][k] -= edge.req[cls][k]
    return out


def engine_runs(edge, pops, backoff_max=64, short=16):
    """Engine-run lengths by the restart hysteresis of session/03_pop.cpp
    (eng_eligible / eng_stop): after a stop the engine restarts with the
    (backoff + 1)-th eligible pop in a row; a run that an ineligible pop ends
    after fewer than `short` pops sets the backoff to 8 or doubles it (at most
    backoff_max), a run of 4 x short or more clears it."""
    runs, backoff, streak, run = [], 0, 0, 0
    for g, _, _ in pops:
        if edge.gangs[g]["eligible"]:
            if run:
                run += 1
            else:
                streak += 1
                if streak > backoff:
                    run = 1
        else:
            if run:
                runs.append(run)
                if run < short:
                    backoff = min(backoff_max, max(8, 2 * backoff))
                elif run >= 4 * short:
                    backoff = 0
            run = streak = 0
    if run:
        runs.append(run)
    return runs


def check_claims(edge, claims, log):
    """Asserts the case's claims on a placement log [(pod, node, status)];
    returns what it measured."""
    pops = pops_of(edge, log)
    for g, nodes in edge.exact.items():
        got = [n for gg, _, ns in pops if gg == g for n in ns]
        assert got == list(nodes), f"gang {g}: placed {got[:8]}.. expected {list(nodes)[:8]}.."
    if "seam" in claims:  # every seam node decides, and the lower index of a tied pair first
        placed = {n for _, _, ns in pops for n in ns}
        assert set(claims["seam"]) <= placed, sorted(set(claims["seam"]) - placed)
    lags = lags_seen(pops)
    for lag in claims.get("lags", ()):
        assert lag in lags, f"no pop places on a node that the pop {lag} back changed ({lags})"
    van = vanished(edge, pops)
    if claims.get("vanish"):
        assert van, "no node goes from best to infeasible between consecutive pops"
        assert {n for _, n in van} & exact_full(edge, pops), "no vanished node was filled exactly"
    if "pops" in claims:
        assert len(pops) == claims["pops"], (len(pops), claims["pops"])
    short = [g for g, gang in enumerate(edge.gangs) if sum(len(ns) for gg, _, ns in pops if gg == g) < gang["min"]]
    if "unready" in claims:  # the gangs that stay unready, each between two gangs that place
        assert short == claims["unready"], short
        for g in short:
            assert any(ns for gg, _, ns in pops if gg < g) and any(ns for gg, _, ns in pops if gg > g), g
    if "backlog" in claims:  # that many pops of class b in a row, all on the big nodes, between two pops of a
        bs = [ns for _, cls, ns in pops[1:-1] if cls == "b" and len(ns) == 1 and set(ns) <= edge.big]
        assert len(bs) == len(pops) - 2 == claims["backlog"] > 2 * 64
        assert pops[0][1] == pops[-1][1] == "a" and not set(pops[-1][2]) & edge.big
    if "levels" in claims:  # the class's range as class_key_format computes it: LR and BRA 0..10, every term
        weights = [w for w, _ in edge.pref]
        assert 21 + sum(weights) == claims["levels"], weights
    runs = engine_runs(edge, pops)
    if "runs" in claims:
        assert runs == claims["runs"], runs
    if "eligible_pops" in claims:
        assert sum(edge.gangs[g]["eligible"] for g, _, _ in pops) == claims["eligible_pops"]
    return dict(pops=len(pops), lags=lags, vanished=van, runs=runs, unready=short)


# ----------------------------------------------------------------------------
# A. partition seams and tie cuts
# ----------------------------------------------------------------------------
A_TASK = dict(cpu=1000, mem=GI, gpu=1000)
GOOD = (8000, 8 * GI)  # balanced: LR 8 + BRA 10 for A_TASK when empty, one LR step less per task
BAD = (2000, 8 * GI)   # cpu fraction 1/2 against 1/8: LR 6 + BRA 6


def _a_score(alloc, placed):
    return se.score(1000 * (placed + 1), alloc[0], GI * (placed + 1), alloc[1])


def seam_nodes(n, workers=0, seg=0):
    """The deciding nodes: node 0, node n-1, the wave seam 63 / 64, the last
    node of worker w and the first of worker w+1 (first, middle and last seam),
    and the owner-segment seams."""
    d = {0, n - 1} | {x for x in (63, 64) if x < n}
    if workers:
        nw, npb = eng_shape(n, workers)
        for w in {0, (nw - 1) // 2, nw - 2} if nw > 1 else ():
            d |= {(w + 1) * npb - 1, (w + 1) * npb}
    if seg:
        d |= {x for k in range(seg, n, seg) for x in (k - 1, k)}
    return sorted(x for x in d if 0 <= x < n)


def seam_cluster(kbgen, n, workers=0, seg=0):
    """Seam nodes are GOOD with three accelerator slots, every other node BAD
    with one; node n-1 has a fourth slot.  Three gangs of |D| tasks: each pop
    ties all of D (a placement costs the node one LR step, so a pop takes each
    once, ascending).  Then one task that only node n-1 can take above the BAD
    score, then eight tasks on the lowest BAD nodes (all tied)."""
    if n > SCORED_MAX:
        return seam_cluster_fit(kbgen, n, workers, seg)
    d = seam_nodes(n, workers, seg)
    b = _Builder(kbgen)
    b.cls("a", A_TASK)
    for i in range(n):
        if i in d:
            b.node(*GOOD, gpu=4000 if i == n - 1 else 3000)
        else:
            b.node(*BAD, gpu=1000)
    scores = [_a_score(GOOD, t) for t in range(4)]
    assert scores[0] > scores[1] > scores[2] > scores[3] > _a_score(BAD, 0), scores
    for _ in range(3):
        b.e.exact[b.gang("a", len(d))] = d
    b.e.exact[b.gang("a", 1)] = [n - 1]
    rest = [i for i in range(n) if i not in d][:8]
    b.e.exact[b.gang("a", len(rest))] = rest
    return b.done()


def seam_cluster_fit(kbgen, n, workers=0, seg=0):
    """The seam cluster without nodeorder (more than SCORED_MAX nodes): every
    node scores 0 and only the seam nodes D fit class a (one accelerator and
    1000 m each, both taken exactly by one task; node n-1 has two of each).
    The first gang takes the lower half of D, the second the upper half, one
    task then fits node n-1 alone, and eight tasks of class c (no
    accelerator) take the lowest nodes outside D: D has no cpu left."""
    d = seam_nodes(n, workers, seg)
    b = _Builder(kbgen, scored=False)
    b.cls("a", A_TASK)
    b.cls("c", dict(cpu=1000, mem=GI))
    ds = set(d)
    for i in range(n):
        slots = 0 if i not in ds else 2 if i == n - 1 else 1
        b.node(1000 * max(slots, 1), 8 * GI, gpu=1000 * slots)
    h = (len(d) + 1) // 2
    b.e.exact[b.gang("a", h)] = d[:h]
    b.e.exact[b.gang("a", len(d) - h)] = d[h:]
    b.e.exact[b.gang("a", 1)] = [n - 1]
    rest = [i for i in range(n) if i not in ds][:8]
    b.e.exact[b.gang("c", len(rest))] = rest
    return b.done()


def tie_cluster(kbgen, n, good, gangs=5):
    """`good` nodes share the top key's score and hold one task each: every
    gang of 64 must take the 64 lowest indices still free.  (Without
    nodeorder: the tie is the score 0 of every node that fits.)"""
    good = sorted(good)
    b = _Builder(kbgen, scored=False)
    b.cls("a", A_TASK)
    gs = set(good)
    for i in range(n):
        b.node(*(GOOD if i in gs else BAD), gpu=1000 if i in gs else 0)
    assert CHUNK * gangs <= len(good)
    for g in range(gangs):
        b.e.exact[b.gang("a", CHUNK)] = good[CHUNK * g:CHUNK * (g + 1)]
    return b.done()


def tie_worker(kbgen):
    """640 nodes, two workers of 320: nodes 0..299 (300 of worker 0) and
    320..339 tie at the top, so worker 0's top-256 and its published 128 are
    cut inside the tie; the fifth gang crosses into worker 1."""
    return tie_cluster(kbgen, 640, list(range(300)) + list(range(320, 340)))


def tie_all(kbgen):
    """845 nodes, 13 workers of 65, every node tied: each worker list, each
    group's 128 and the final 128 are cut inside the tie."""
    return tie_cluster(kbgen, 845, range(845))


# ----------------------------------------------------------------------------
# B. stale rows
# ----------------------------------------------------------------------------
REFILL_ARGS = {"nodeorder": {"leastrequested.weight": "0"}}  # the score is BRA alone


def refill_cluster(kbgen, n, seq):
    """Nodes of 8000 m / 8 GiB / 3 accelerators with a Running pod of 1000 m:
    cpu is 1/8 ahead of memory.  Class a asks 2 GiB and one accelerator, class
    b 2000 m: a moves the balance by -1/4, b by +1/4, all fractions dyadic.
    On an untouched node (balance +1/8) a scores BRA 8 and b 6; once a is on it
    (-1/8) a scores 6 and b 8: a placement lowers the node for its own class
    (a gang spreads, one task per node, lowest indices first) and raises it
    for the other, so b gangs want the nodes the a gangs just took.  With a
    alone the gangs rotate over the nodes in blocks of 64.  The third a fills
    a node's accelerators exactly and it vanishes for a.
    seq: [(class, size)] or (class, size, MinAvailable)."""
    b = _Builder(kbgen, args=REFILL_ARGS)
    b.cls("a", dict(cpu=0, mem=2 * GI, gpu=1000))
    b.cls("b", dict(cpu=2000, mem=0))
    for _ in range(n):
        b.node(8000, 8 * GI, gpu=3000, run=dict(cpu=1000, mem=0))
    # the class a / class b scores by the number of (a, b) tasks on the node
    bra = lambda na, nb, da, db: se.bra_score(1000 + 2000 * (nb + db), 8000, 2 * GI * (na + da), 8 * GI)
    assert (bra(0, 0, 1, 0), bra(1, 0, 1, 0), bra(0, 0, 0, 1), bra(1, 0, 0, 1)) == (8, 6, 6, 8)
    for s in seq:
        b.gang(s[0], s[1], s[2] if len(s) > 2 else None)
    return b.done()


# per node count: the gangs.  a gangs first rotate over the nodes in blocks of
# 64 (at 192 nodes the fourth pop's nodes are all among the candidates of the
# three pops before it; at 193 and 257 one node is left over), then b and a
# take the nodes just taken, the third a fills a node's accelerators and a
# pops again right after (the filled nodes are the best of a's stale keys);
# one gang (MinAvailable one above its size) stays unready between two gangs
# that place.  The sizes 1, 63, 65 and 128 take part at 64 and 65 nodes; from
# 192 nodes on the gangs after the rotation are small, for the restatement's
# time (18 ms per task at 192 nodes, 36 ms at 257).
REFILL_SEQ = {
    64: [("a", 64), ("b", 64), ("a", 64), ("b", 63), ("a", 64), ("a", 64, 65), ("b", 65)],
    65: [("a", 64), ("a", 1), ("b", 65), ("a", 65), ("b", 128), ("a", 63), ("a", 2, 3), ("b", 1)],
    128: [("a", 64), ("a", 64), ("a", 128), ("b", 65), ("a", 64), ("a", 2, 3), ("b", 1)],
    129: [("a", 64), ("a", 64), ("a", 1), ("a", 64), ("b", 63), ("a", 65), ("a", 2, 3), ("b", 1)],
    192: [("a", 64), ("a", 64), ("a", 64), ("a", 64), ("b", 8), ("a", 8), ("a", 2, 3), ("b", 1)],
    193: [("a", 64), ("a", 64), ("a", 64), ("a", 64), ("b", 8), ("a", 8), ("a", 2, 3), ("b", 1)],
    257: [("a", 64), ("a", 64), ("a", 64), ("a", 64), ("a", 64), ("b", 8), ("a", 8), ("a", 2, 3), ("b", 1)],
}


# ----------------------------------------------------------------------------
# C. owner limits
# ----------------------------------------------------------------------------
def levels_cluster(kbgen, top_weight):
    """The class's host-computed score range (class_key_format: LR 0..10, BRA
    0..10, node affinity 0..100 + top_weight) spans 21 + 100 + top_weight
    levels.  The class asks one accelerator and names cpu and memory as zero:
    on an empty node with both labels it scores the range's top (LR 10, BRA
    10, every term), on a node whose Running pod takes all cpu and memory and
    that has no label its bottom, 0 (level 1).  One slot per node: the top
    nodes decide the first gang, the bottom nodes the last."""
    lab = ("edge/zone", "a"), ("edge/tier", "x")
    pref = [(100, {"expr": [(lab[0][0], "In", [lab[0][1]])]}), (top_weight, {"expr": [(lab[1][0], "In", [lab[1][1]])]})]
    b = _Builder(kbgen)
    b.cls("l", dict(cpu=0, mem=0, gpu=1000), affinity={"node": {"preferred": pref}})
    top, mid, bottom = [5, 40], [], []
    for i in range(64):
        if i in top:
            b.node(4000, 4 * GI, gpu=1000, labels=dict(lab))
        elif i % 2:
            mid.append(b.node(4000, 4 * GI, gpu=1000, labels=dict(lab[:1])))
        else:
            bottom.append(b.node(4000, 4 * GI, gpu=1000, run=dict(cpu=4000, mem=4 * GI)))
    assert se.score(0, 4000, 0, 4 * GI) == 20 and se.score(4000, 4000, 4 * GI, 4 * GI) == 0
    b.e.exact[b.gang("l", len(top))] = top
    b.e.exact[b.gang("l", len(mid))] = mid
    b.e.exact[b.gang("l", len(bottom))] = bottom
    b.e.pref = pref
    return b.done()


def backlog_cluster(kbgen):
    """Four big nodes (0..3) are the best of both classes; their accelerators
    hold a's first task plus exactly 134 b tasks.  a pops once, b pops 134
    times (gangs of one: more than twice the owners' 64-pop log), every one on
    nodes 0..3, the last ones filling them exactly; then a pops again and must
    take the small nodes: a stale byte for any of 0..3 would put it there."""
    b = _Builder(kbgen)
    b.cls("a", dict(cpu=1000, mem=GI, gpu=200))
    b.cls("b", dict(cpu=500, mem=512 * MI, gpu=100))
    for i in range(64):
        if i < 4:
            b.node(80000, 80 * GI, gpu=3400)
        else:
            b.node(2000, 16 * GI, gpu=200)
    # a loaded big node stays above an empty small one for both classes
    assert se.score(17500, 80000, 17500 * MI, 80 * GI) > max(se.score(1000, 2000, GI, 16 * GI),
                                                               se.score(500, 2000, 512 * MI, 16 * GI))
    b.e.exact[b.gang("a", 1)] = [0]
    n_b = 32 + 3 * 34
    for _ in range(n_b):
        b.gang("b", 1)
    b.e.exact[b.gang("a", 4)] = [4, 5, 6, 7]
    c = b.done()
    c.edge.big = {0, 1, 2, 3}
    return c


def classes_cluster(kbgen, n_classes):
    """n_classes eligible classes (cpu requests 100, 101, ..) of one task each on 64 nodes."""
    b = _Builder(kbgen)
    for _ in range(64):
        b.node(64000, 64 * GI)
    for k in range(n_classes):
        b.cls(f"c{k}", dict(cpu=100 + k, mem=100 * MI))
        b.gang(f"c{k}", 1)
    return b.done()


# ----------------------------------------------------------------------------
# D. run boundaries
# ----------------------------------------------------------------------------
PORT = dict(cpu=100, mem=100 * MI, ports=[dict(port=8080, proto="TCP")])
# eligible pops in a row between two host-port pops; with the hysteresis
# (engine_runs) they give engine runs of RUNS pops: the backoff goes 0, 8, 16,
# 16, 16, 32, 64, 64 (kEngBackoffMax) and the run of 64 clears it
STREAKS = [1, 8 + 15, 16 + 16, 16 + 17, 16 + 1, 32 + 1, 64 + 1, 64 + 64, 1]
RUNS = [1, 15, 16, 17, 1, 1, 1, 64, 1]


def runs_cluster(kbgen, streaks):
    """64 equal nodes; gangs of one task of an eligible class in streaks,
    a gang of one host-port task (a launched pop) between two streaks.  Every
    pop takes the best node on the rows all the pops before it left."""
    b = _Builder(kbgen)
    for _ in range(64):
        b.node(16000, 16 * GI)
    b.cls("e", dict(cpu=100, mem=100 * MI))
    b.cls("h", PORT, eligible=False)
    for k, s in enumerate(streaks):
        if k:
            b.gang("h", 1)
        for _ in range(s):
            b.gang("e", 1)
    return b.done()


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------
def _seam_case(n, w, groups=None, tag=""):
    nw, npb = eng_shape(n, w)
    served = npb <= ENG_MAX_NPB
    opts = dict(engine_lists=0, engine_workers=w)
    if groups is not None:
        opts["engine_groups"] = groups
    claims = dict(group="A", seam=seam_nodes(n, w), workers=nw if served else None, owners=0,
                  all_engine=served, no_engine=not served)
    return (f"seam{n}w{w}{tag}", lambda kb: seam_cluster(kb, n, w), opts, claims)


def _tie_case(name, builder, n, w, groups=None):
    opts = dict(engine_lists=0, engine_workers=w)
    if groups is not None:
        opts["engine_groups"] = groups
    return (name, builder, opts, dict(group="A", workers=eng_shape(n, w)[0], owners=0, all_engine=True))


def _refill_case(n, lists):
    unready = [g for g, s in enumerate(REFILL_SEQ[n]) if len(s) > 2]
    claims = dict(group="B", lags=(1, 2, 3, 4), vanish=True, unready=unready, all_engine=True,
                  owners=2 if lists else 0, workers=None if lists else eng_shape(n, 512)[0])
    return (f"refill{n}{'lists' if lists else 'sweep'}", lambda kb: refill_cluster(kb, n, REFILL_SEQ[n]),
            dict(engine_lists=lists), claims)


def _owner_seam_case(n):
    return (f"owner{n}", lambda kb: seam_cluster(kb, n, seg=OWN_SEG), dict(engine_lists=1),
            dict(group="C", seam=seam_nodes(n, seg=OWN_SEG), owners=2, all_engine=True))  # classes a and c


def _ring_case(pops, speculate):
    opts = dict(engine_lists=0)
    if speculate is not None:
        opts["speculate"] = speculate
    return (f"ring{pops}{'' if speculate is None else 's%d' % speculate}", lambda kb: runs_cluster(kb, [pops]), opts,
            dict(group="D", pops=pops, eligible_pops=pops, runs=[pops], all_engine=True, owners=0))


CASES = [_seam_case(64, 1), _seam_case(65, 2), _seam_case(129, 3), _seam_case(257, 5), _seam_case(4161, 66),
         _seam_case(8192, 1), _seam_case(8193, 1), _seam_case(8193, 2)]
CASES += [_tie_case("tieworker", tie_worker, 640, 2), _tie_case("tieall", tie_all, 845, 13)]
CASES += [_seam_case(845, 13, g, f"g{g}") for g in (0, 1, 3, 8)]
CASES += [_tie_case(f"tieallg{g}", tie_all, 845, 13, g) for g in (0, 1, 3, 8)]
CASES += [_seam_case(65, 2, 8, "g8"), _tie_case("tieworkerg8", tie_worker, 640, 2, 8)]
CASES += [_refill_case(n, lists) for n in sorted(REFILL_SEQ) for lists in (0, 1)]
CASES += [_owner_seam_case(n) for n in (1791, 1792, 1793, 3585)]
CASES += [
    ("levels127", lambda kb: levels_cluster(kb, 6), dict(engine_lists=1),
     dict(group="C", owners=1, all_engine=True, levels=127)),
    ("levels128", lambda kb: levels_cluster(kb, 7), dict(engine_lists=1),
     dict(group="C", owners=0, all_engine=True, levels=128)),
    ("backlog", backlog_cluster, dict(engine_lists=1),
     dict(group="C", owners=2, all_engine=True, pops=136, backlog=134)),
    ("classes254", lambda kb: classes_cluster(kb, 254), dict(engine_lists=1),
     dict(group="C", owners=(254, 0), all_engine=True, pops=254)),
    ("classes255", lambda kb: classes_cluster(kb, 255), dict(engine_lists=1),
     dict(group="C", owners=0, all_engine=True, pops=255)),
    ("runs", lambda kb: runs_cluster(kb, STREAKS), dict(engine_lists=0),
     dict(group="D", runs=RUNS, eligible_pops=sum(STREAKS), pops=sum(STREAKS) + len(STREAKS) - 1, owners=0,
          mixed=True)),
]
CASES += [_ring_case(p, s) for p in (8, 9, 16, 17) for s in (0, None)]
NAMES = [c[0] for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def write_cases(kbgen, directory):
    """{name: (cluster, path of its KBS1 file)} for CASES."""
    out = {}
    for name, builder, _, _ in CASES:
        c = builder(kbgen)
        out[name] = (c, c.write(str(directory / (name + ".kbs"))))
    return out
