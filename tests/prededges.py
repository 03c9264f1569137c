"""Predicate and fit edge snapshots and an independent reference of the
node selection key.

tests/scoreedges.py puts the *score* half of a node's selection key on its
truncation ties.  This module does the same for the other half: the predicates
kube-batch runs (predicates.go:123-203: pod count, node selector and required
node affinity, host ports, unschedulable, taints), the resource fit of
allocate.go:153-173 with the epsilon rule of resource_info.go:164-168, and the
FitDelta records (resource_info.go:134-147, job_info.go:343-372).

build() makes one cluster per *kind*; every node carries one Running pod and
has a row type (its family member), the types repeat with the node index so
that every wave / block position sees each of them:

  fit     req - avail at {eps - 1, eps, eps + 1} per resource and per source
          (Idle, Idle + Backfilled, Releasing), all three at once, the accessible
          side failing by one while Releasing passes by one and the reverse, an
          Idle of 0, an over-committed Idle of -1, a memory allocatable of 2^50
  count   pods at maxtasks - 1 / maxtasks / maxtasks + 1 (maxtasks 2 / 1 / 0)
  taints  131 (or 64, 65) distinct NoSchedule / NoExecute taints; node 0 lists
          them all in order, which pins their ids; the special ids 0, 63, 64,
          127, 128 and the last sit alone, in pairs across a word boundary, and
          next to PreferNoSchedule taints
  ports   340 distinct (protocol, port, IP) triples = 6 words; ids follow the
          engine's documented order (protocol, port, IP in first-use order):
          a specific IP and its wildcard twin at ids 63 / 64 and, the other way
          round, 127 / 128; TCP / UDP twins; classes whose window starts at
          word 0, 1, 2, 3 and at the last word (one word wide)
  labels  the label values "7", "007", "-5", "0", 2^63 - 1, 2^63, "1e3", "x" and
          no label, under Gt / Lt (right-hand sides 0, -5, 6, 7 and the int64
          extremes), In / NotIn / Exists / DoesNotExist, OR-ed terms (one of
          them empty) and metadata.name In / NotIn
  cross   the allocate cases: gangs of identical tasks whose node families
          accept exactly k of them by cpu, memory, GPU or pod count (the k-th
          at eps - 1; on the twin node the k-th misses at eps), run out of Idle
          and go on as Pipelined, take one host port each, and a gang whose last
          task finds no node among nodes at FitDelta 0 and -1

What Go does with the label values was read off strconv.ParseInt (base 10, 64
bits: a sign and digits only, so "007" is 7, "1e3" and "x" are errors, 2^63 a
range error) and labels.Requirement.Matches (selector.go:192-236): an
unparsable or absent value fails Gt / Lt; a Gt / Lt requirement whose own
value does not parse is invalid and fails the whole term, so the right-hand
sides here all parse.  kbgen expresses every value; none is dropped.

In the 1200-node cross case the gangs are sized for five repetitions of the row
types, spread over the node array (_cross_active; the other rows miss at eps): expected sessions come from the
faithful restatement, whose nodeorder is quadratic in the nodes for every task.
With disablePredicate the selectors are off, so that case makes cpu short on
every node and sizes one gang against the whole cluster (_tight_jobs).

Every static task but a few (noslot) carries a required node-affinity term
that leaves out a seventh of the nodes (_slot_terms), which keeps every pass
rate under 90 %; the noslot tasks and the cross jobs (node selector only) are
the classes without required node affinity.

taint_id / port_id are derived from the engine's documented numbering
(csrc/session/02_open.cpp), not read from it.

Model is the reference: plain Python integers over the Kubernetes objects as
they were given to kbgen.  It uses neither the oracle nor the engine's header;
the score comes from scoreedges.score.  Rules holds the comparison rules, so
that tests can bend one (a mutant) and see that rows notice.
"""
import re

import numpy as np

import scoreedges as se

MI, GI = 1 << 20, 1 << 30
EPS = (10, 10 * MI, 10)              # resource_info.go:54-56: minMilliCPU, minMemory, minMilliGPU
BASE = (1000, GI, 2000)              # avail of an edge row in its edge resource
AMPLE = (100_000, 64 * GI, 100_000)
HOSTNAME = se.HOSTNAME
NODE_COUNTS = se.NODE_COUNTS
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
ALLOCATED, PIPELINED = 1, 2
SEED = 20261020


class Rules:
    """The comparisons of the reference; a mutant changes one."""
    eps = EPS
    le_at_eps = False        # '<=' in place of '<' at eps
    taint_word0 = False      # only taints with an id below 64 are compared
    port_shift = False       # a 4-word port window pushed down instead of cut at port_words
    gt_ge = False            # '>=' in place of '>' in Gt
    unparsable_zero = False  # an unparsable label value reads as 0
    count_lt = False         # maxtasks < pods in place of <=


def parse_int64(s):
    """strconv.ParseInt(s, 10, 64): None on a syntax or range error."""
    if not re.fullmatch(r"[+-]?[0-9]+", s):
        return None
    v = int(s)
    return v if I64_MIN <= v <= I64_MAX else None


def sanitize(pt):
    return (pt.get("ip") or "0.0.0.0", pt.get("proto") or "TCP", pt["port"])


def port_conflict(used, pt):
    """HostPortInfo.CheckConflict (host_ports.go:96-125); used: a set of sanitized triples."""
    ip, proto, port = sanitize(pt)
    if port <= 0:
        return False
    if ip == "0.0.0.0":
        return any(u[1] == proto and u[2] == port for u in used)
    return ("0.0.0.0", proto, port) in used or (ip, proto, port) in used


def tolerates(tol, taint):
    """Toleration.ToleratesTaint (toleration.go:37-56)."""
    key, val, eff = taint
    if tol.get("effect") and tol["effect"] != eff:
        return False
    if tol.get("key") and tol["key"] != key:
        return False
    op = tol.get("op") or "Equal"
    if op == "Equal":
        return (tol.get("value") or "") == val
    return op == "Exists"


def req_matches(rules, req, labels):
    """labels.Requirement.Matches (selector.go:192-236)."""
    key, op, vals = req
    has = key in labels
    if op == "In":
        return has and labels[key] in vals
    if op == "NotIn":
        return not has or labels[key] not in vals
    if op == "Exists":
        return has
    if op == "DoesNotExist":
        return not has
    if not has:
        return False
    lv, rv = parse_int64(labels[key]), parse_int64(vals[0])
    if lv is None and rules.unparsable_zero:
        lv = 0
    if lv is None or rv is None or len(vals) != 1:
        return False
    if op == "Gt":
        return lv >= rv if rules.gt_ge else lv > rv
    return lv < rv


def terms_match(rules, terms, labels, name):
    """v1helper.MatchNodeSelectorTerms (helpers.go:302-333): OR of the terms,
    an empty term matches nothing; fields: metadata.name In / NotIn one value."""
    for t in terms:
        expr, fields = t.get("expr", []), t.get("fields", [])
        if not expr and not fields:
            continue
        if not all(req_matches(rules, r, labels) for r in expr):
            continue
        if not all((name == f[2][0]) == (f[1] == "In") for f in fields):
            continue
        return True
    return False


class Model:
    """The node state of a session in plain integers (node_info.go:113-145)
    and the evaluation of one pending task against it."""

    def __init__(self, snap, rules=None):
        self.snap, self.rules = snap, rules or Rules()
        self.idle, self.rel, self.bf, self.used, self.pods, self.ports, self.nz = [], [], [], [], [], [], []
        for r in snap.rows:
            p = r["pod"]
            req = [p.get("cpu", 0), p.get("mem", 0), p.get("gpu", 0)]
            self.idle.append([a - q for a, q in zip(r["alloc"], req)])
            self.rel.append(list(req) if p.get("deleting") else [0, 0, 0])
            self.bf.append(list(req) if p.get("backfill") else [0, 0, 0])
            self.used.append(list(req))
            self.pods.append(1)
            self.ports.append({sanitize(pt) for pt in p.get("ports", []) if pt["port"] > 0})
            self.nz.append(list(se.nonzero([{k: p[k] for k in ("cpu", "mem") if k in p}])))

    # -- predicates ----------------------------------------------------------
    def predicate(self, j, n, task=None):
        """task: evaluate this variant of task j (thresholds())."""
        if self.snap.pred_off:
            return True
        ru, r, t = self.rules, self.snap.rows[n], task or self.snap.tasks[j]
        if (r["maxtasks"] < self.pods[n]) if ru.count_lt else (r["maxtasks"] <= self.pods[n]):
            return False
        if any(r["labels"].get(k) != v for k, v in t.get("nsel", {}).items()):
            return False
        if t.get("terms") is not None and not terms_match(ru, t["terms"], r["labels"], r["name"]):
            return False
        if self.port_blocked(j, n):
            return False
        if r.get("unsched"):
            return False
        for taint in r.get("taints", []):
            if taint[2] not in ("NoSchedule", "NoExecute"):
                continue
            if ru.taint_word0 and self.snap.taint_id[taint] >= 64:
                continue
            if not any(tolerates(tol, taint) for tol in t.get("tols", [])):
                return False
        return True

    def port_blocked(self, j, n):
        t = self.snap.tasks[j]
        own = [pt for pt in t["ctr"].get("ports", []) if pt["port"] > 0]
        if not self.rules.port_shift:
            return any(port_conflict(self.ports[n], pt) for pt in own)
        # the mutant: the class's 4-word window, instead of being cut at
        # port_words, starts at min(pw_lo, port_words - 4) while its masks stay
        # relative to pw_lo: mask word w meets column word w + the shift
        ids = self.snap.port_id
        words = (len(ids) + 63) // 64
        conf = {ids[u] for pt in own for u in ids if port_conflict({u}, pt)}
        if not conf:
            return False
        pw_lo = min(min(conf), min(ids[sanitize(pt)] for pt in own)) // 64
        shift = min(pw_lo, max(words - 4, 0)) - pw_lo
        col = {ids[u] for u in self.ports[n]}
        return any(c + 64 * shift in col for c in conf)

    # -- fit, FitDelta ---------------------------------------------------------
    def _le(self, req, avail):
        """Resource.LessEqual with the epsilon rule, in integers."""
        ru = self.rules
        return all((q - a <= e) if ru.le_at_eps else (q - a < e) for q, a, e in zip(req, avail, ru.eps))

    def kind(self, j, n):
        """allocate.go:153-182 for one node: ALLOCATED, PIPELINED or 0."""
        req = self.snap.tasks[j]["ireq"]
        if self._le(req, [i + b for i, b in zip(self.idle[n], self.bf[n])]):
            return ALLOCATED
        return PIPELINED if self._le(req, self.rel[n]) else 0

    def fit_delta(self, j, n):
        """Idle.FitDelta(Resreq) after the walk's visit (Idle += Backfilled)."""
        req = self.snap.tasks[j]["req"]
        return [i + b - (q + e) if q > 0 else i + b
                for i, b, q, e in zip(self.idle[n], self.bf[n], req, self.rules.eps)]

    def fit_deltas(self, j):
        """(nodes, deltas) of the nodes in task j's walk, ascending index."""
        ns = [n for n in range(len(self.snap.rows)) if self.predicate(j, n)]
        return np.array(ns, np.int32), np.array([self.fit_delta(j, n) for n in ns], np.int64).reshape(-1, 3)

    def fit_counts(self, j):
        """JobInfo.FitError (job_info.go:343-372) of task j finding no node."""
        _, d = self.fit_deltas(j)
        if not len(d):
            return "0 nodes are available"
        rs = sorted(f"{int((d[:, k] < 0).sum())} insufficient {name}"
                    for k, name in enumerate(("cpu", "memory", "GPU")) if (d[:, k] < 0).any())
        return f"0/{len(d)} nodes are available, " + ", ".join(rs) + "."

    # -- score, key, walk ------------------------------------------------------
    def score(self, j, n):
        if self.snap.score_off:
            return 0
        t, r = self.snap.tasks[j], self.snap.rows[n]
        return se.score(t["nz"][0] + self.nz[n][0], r["alloc"][0], t["nz"][1] + self.nz[n][1], r["alloc"][1])

    def expected_keys(self, j, fit=False):
        """Per node the packed key of the predicate + score sweep (0: fails);
        fit=True: allocate's selection key, 0 also where neither fit holds and
        bit 0 set where the task would be Pipelined."""
        out = np.zeros(len(self.snap.rows), np.uint64)
        for n in range(len(self.snap.rows)):
            if not self.predicate(j, n):
                continue
            k = self.kind(j, n) if fit else ALLOCATED
            if k:
                out[n] = se.pack_key(self.score(j, n), n) | (1 if k == PIPELINED else 0)
        return out

    def walk(self, j):
        """(nodes, scores) of the by-score walk: score descending, then index."""
        ns = np.array([n for n in range(len(self.snap.rows)) if self.predicate(j, n)], np.int64)
        sc = np.array([self.score(j, int(n)) for n in ns], np.int64)
        order = np.lexsort((ns, -sc))
        return ns[order].astype(np.int32), sc[order].astype(np.int32)

    def passing(self, j, task=None):
        return np.array([n for n in range(len(self.snap.rows)) if self.predicate(j, n, task)], np.int32)

    def first_fit(self, j):
        """backfill.go:51-56: the lowest passing index, -1: none."""
        p = self.passing(j)
        return int(p[0]) if p.size else -1

    def choice(self, j):
        """(node, kind) allocate gives task j on this state; (-1, 0): none."""
        nodes, _ = self.walk(j)
        for n in nodes:
            k = self.kind(j, int(n))
            if k:
                return int(n), k
        return -1, 0

    def commit(self, j, n, kind):
        """NodeInfo.AddTask of task j (Allocated or Pipelined) on node n."""
        t = self.snap.tasks[j]
        tgt = self.idle[n] if kind == ALLOCATED else self.rel[n]
        for k in range(3):
            tgt[k] -= t["req"][k]
            self.used[n][k] += t["req"][k]
        self.pods[n] += 1
        self.nz[n][0] += t["nz"][0]
        self.nz[n][1] += t["nz"][1]
        self.ports[n] |= {sanitize(pt) for pt in t["ctr"].get("ports", []) if pt["port"] > 0}

    def node_state(self):
        """N x 12: idle, used, releasing, backfilled (read_nodes' layout)."""
        return np.array([i + u + r + b for i, u, r, b in zip(self.idle, self.used, self.rel, self.bf)], np.int64)


class PredSnap:
    """rows[n]: dict(fam, name, alloc, maxtasks, labels, taints, unsched, pod);
    tasks[j]: dict(pod index, job, ctr, req, ireq, nz, tols, nsel, terms, edge);
    taint_id / port_id: the ids the engine's documented numbering gives."""

    def __init__(self, kind):
        self.kind, self.cluster, self.rows, self.tasks = kind, None, [], []
        self.pred_off = self.score_off = False
        self.taint_id, self.port_id, self.jobs = {}, {}, {}

    def model(self, rules=None):
        return Model(self, rules)

    def family(self, n):
        return self.rows[n]["fam"]


# ----------------------------------------------------------------------------
# the rows and tasks of each kind
# ----------------------------------------------------------------------------
def _ample(rng, k):
    return BASE[k] + EPS[k] + AMPLE[k] // 50 * int(rng.integers(1, 40))


def _pod_ample(rng):
    return [int(rng.integers(1, 40)) * 100, int(rng.integers(1, 64)) * 64 * MI + int(rng.integers(0, 999)),
            int(rng.integers(0, 4)) * 500]


def _plain_row(rng, fam, **kw):
    pod = _pod_ample(rng)
    alloc = [pod[k] + _ample(rng, k) for k in range(3)]
    row = dict(fam=fam, alloc=alloc, maxtasks=110, labels={}, taints=[], pod=dict(cpu=pod[0], mem=pod[1], gpu=pod[2]))
    row.update(kw)
    return row


FIT_TYPES = [f"{s}_{r}" for s in ("idle", "bf", "rel") for r in ("cpu", "mem", "gpu")] + \
    ["idle_all", "acc_miss_rel_fit", "acc_fit_rel_miss", "idle_zero", "idle_neg", "idle_mem_big"]
RES = ("cpu", "mem", "gpu")


def _fit_row(rng, fam):
    avail = [_ample(rng, k) for k in range(3)]       # what the source offers
    src, _, what = fam.partition("_")
    if fam in ("acc_miss_rel_fit", "acc_fit_rel_miss"):
        a, b = list(BASE), list(BASE)
        (a if fam == "acc_miss_rel_fit" else b)[0] -= 1   # a: Idle, b: Releasing
        return dict(fam=fam, alloc=[x + y for x, y in zip(a, b)], maxtasks=110, labels={}, taints=[],
                    pod=dict(cpu=b[0], mem=b[1], gpu=b[2], deleting=True))
    if fam == "idle_zero":
        avail[0] = 0
    elif fam == "idle_neg":
        avail[0] = -1
    elif fam == "idle_mem_big":
        avail[1] = BASE[1]
    elif what == "all":
        avail = list(BASE)
    else:
        avail[RES.index(what)] = BASE[RES.index(what)]
    if src == "idle":
        pod = _pod_ample(rng)
        if fam == "idle_mem_big":
            pod[1] = (1 << 50) - BASE[1]
        alloc = [a + p for a, p in zip(avail, pod)]
        return dict(fam=fam, alloc=alloc, maxtasks=110, labels={}, taints=[], pod=dict(cpu=pod[0], mem=pod[1], gpu=pod[2]))
    if src == "bf":    # Idle + Backfilled = allocatable
        pod = [min(p, a) for p, a in zip(_pod_ample(rng), avail)]
        return dict(fam=fam, alloc=avail, maxtasks=110, labels={}, taints=[],
                    pod=dict(cpu=pod[0], mem=pod[1], gpu=pod[2], backfill=True))
    # Releasing = the deleting pod's request; Idle is a few units
    return dict(fam=fam, alloc=[a + 5 for a in avail], maxtasks=110, labels={}, taints=[],
                pod=dict(cpu=avail[0], mem=avail[1], gpu=avail[2], deleting=True))


def _fit_tasks():
    def t(d, **kw):
        c = {r: BASE[k] + EPS[k] + d[k] for k, r in enumerate(RES) if d[k] is not None}
        c.update(kw)
        return dict(ctr=c, edge=True)
    return [t((-1, -1, -1)), t((0, 0, 0)), t((1, 1, 1)), t((-1, 0, -1)), t((0, -1, -1)), t((-1, -1, 0)),
            t((1, -1, -1)), t((-1, 1, 1)),
            t((None, -1, -1), cpu=0), t((-1, -1, None)), t((-1, None, -1), mem=0),
            dict(ctr=dict(cpu=9, mem=MI), edge=True), dict(ctr=dict(cpu=10, mem=MI), edge=True),
            dict(ctr=dict(cpu=8, mem=MI), edge=True)]


COUNT_TYPES = [0, 1, 2, 3, 110]
PLAIN_TASKS = [dict(ctr=dict(cpu=100, mem=64 * MI)), dict(ctr=dict(cpu=500, mem=GI), noslot=True), dict(ctr={})]


def _taint_defs(u):
    return [(f"k{i:03d}", "" if i % 5 == 4 else f"v{i % 3}", "NoExecute" if i % 2 else "NoSchedule") for i in range(u)]


def _taint_specials(u):
    return sorted({i for i in (0, 63, 64, 127, 128, u - 1) if i < u})


def _taint_types(u):
    """Row types of the taints kind: lists of taint indices; -1 = a
    PreferNoSchedule taint (with the key and value of taint 0)."""
    sp = _taint_specials(u)
    types = [("all", list(range(u)))] + [(f"one{i}", [i]) for i in sp]
    for a, b in ((63, 64), (127, 128)):
        if b < u:
            types.append((f"pair{a}", [a, b]))
    types += [("none", []), ("prefer", [-1]), ("prefer_last", [-1, u - 1]), ("plain5", [5]), ("plain_mid", [u // 2 + 6])]
    return types


def _taint_tasks(u):
    defs, sp = _taint_defs(u), _taint_specials(u)

    def eq(i):
        k, v, e = defs[i]
        return dict(key=k, op="Equal" if v else "Exists", value=v, effect=e)
    tasks = [dict(tols=[eq(i)], edge=True) for i in sp]
    tasks += [dict(tols=[eq(i) for i in sp if i != out], edge=True) for out in sp]
    tasks += [dict(tols=[dict(key="", op="Exists", value="", effect="")]),
              dict(tols=[dict(key="", op="Exists", value="", effect="NoSchedule")], edge=True),
              dict(tols=[dict(key=defs[sp[-1]][0], op="Exists", value="", effect="NoExecute"),
                         dict(key=defs[0][0], op="Exists", value="", effect="PreferNoSchedule")], edge=True),
              dict(tols=[])]
    for t in tasks:
        t["ctr"] = dict(cpu=100, mem=64 * MI)
    tasks[0]["noslot"] = tasks[len(sp)]["noslot"] = True   # their own taints keep them under 90 %
    return tasks


# the port triples in id order: TCP ports 2000.., then UDP
PORT_BASE = 2000
PAIR_A, PAIR_B = PORT_BASE + 63, PORT_BASE + 63 + 62   # ids 63 / 64 / 65 and 127 / 128
IP_A, IP_B, IP_C = "10.0.0.0", "10.0.0.2", "10.0.0.7"   # first-use order: IP_A, 0.0.0.0, IP_B, IP_C
N_TCP_PORTS, N_UDP_PORTS = 327, 10


def _port_of_id(i):
    """The wildcard TCP triple whose id is i (not one of the pair ports' ids)."""
    assert i < 63 or 65 < i < 127 or i > 128
    return PORT_BASE + (i if i < 63 else i - 2 if i < 127 else i - 3)


def _all_ports():
    """The filler pod's ports: IP_A first (its IP is then the first seen)."""
    out = [dict(ip=IP_A, proto="TCP", port=PAIR_A)]
    out += [dict(ip="", proto="" if p % 2 else "TCP", port=p) for p in range(PORT_BASE, PORT_BASE + N_TCP_PORTS)]
    out += [dict(ip=IP_B, proto="TCP", port=PAIR_B)]
    out += [dict(ip="", proto="UDP", port=_udp_port(k)) for k in range(N_UDP_PORTS)]
    return out


def _udp_port(k):
    return [PORT_BASE, _port_of_id(191), _port_of_id(200)][k] if k < 3 else 7000 + k


def _port_types():
    w = lambda port, proto="TCP", ip="": [dict(ip=ip, proto=proto, port=port)]
    return [("filler", _all_ports()), ("none", []), ("bit0", w(PORT_BASE)), ("bit0_udp", w(PORT_BASE, "UDP")),
            ("id63_ip", w(PAIR_A, ip=IP_A)), ("id64_any", w(PAIR_A)), ("id127_any", w(PAIR_B)),
            ("id128_ip", w(PAIR_B, ip=IP_B)), ("mid200", w(_port_of_id(200))), ("bit63_w2", w(_port_of_id(191))),
            ("udp_last", w(_udp_port(1), "UDP")), ("two", w(_port_of_id(70)) + w(_port_of_id(139)))]


def _port_tasks():
    w = lambda port, proto="TCP", ip="": dict(ip=ip, proto=proto, port=port)
    sets = [[w(PORT_BASE)], [w(PORT_BASE, "UDP")], [w(PAIR_A, ip=IP_A)], [w(PAIR_A)], [w(PAIR_A, ip=IP_C)],
            [w(PAIR_B)], [w(PAIR_B, ip=IP_B)], [w(_port_of_id(200))], [w(_port_of_id(191))],
            [w(_udp_port(1), "UDP")], [w(_udp_port(2), "UDP")], [w(PORT_BASE), w(_port_of_id(2))],
            [w(_port_of_id(70)), w(_port_of_id(191))], [w(0), w(_port_of_id(139), "")]]
    # (the UDP twin of the mid-word TCP port meets only node 0's pod: no threshold of its own)
    return [dict(ctr=dict(cpu=100, mem=64 * MI, ports=p), edge=i != 10, noslot=i in (3, 12)) for i, p in enumerate(sets)]


LABEL_VALUES = ["7", "007", "-5", "0", str(I64_MAX), str(I64_MAX + 1), "1e3", "x", None, None]


def _label_tasks(n_nodes):
    LV = "lv"
    alt = {"expr": [(LV, "In", ["x", "1e3"])]}
    terms = []
    for op in ("Gt", "Lt"):
        for rhs in (0, -5, 6, 7, I64_MAX, I64_MIN):
            t = [{"expr": [(LV, op, [str(rhs)])]}]
            if sum(v is not None and req_matches(Rules, t[0]["expr"][0], {LV: v}) for v in LABEL_VALUES) < 2:
                t.append(alt)  # (next to) nothing is beyond it: an OR-ed term keeps some nodes passing
            terms.append(t)
    quiet = []  # tasks that (nearly) every node passes: no threshold of their own
    terms += [[{"expr": [(LV, "In", ["7", "0"])]}], [{"expr": [(LV, "NotIn", ["7", "x"])]}],
              [{"expr": [(LV, "Exists", [])]}], [{"expr": [(LV, "DoesNotExist", [])]}],
              [{"expr": [("nokey", "NotIn", ["7"]), ("nokey", "DoesNotExist", [])]}],
              [{}, {"expr": [(LV, "In", ["-5", "0"])]}],
              [{"expr": [(LV, "Gt", ["6"]), (LV, "Lt", [str(I64_MAX)])]}, {"expr": [(LV, "Lt", ["-4"])]}]]
    for n in sorted({0, 63, 64, n_nodes - 1, 10 ** 6}):
        if n < n_nodes or n == 10 ** 6:
            name = f"n{n:05d}"
            terms.append([{"fields": [("metadata.name", "In", [name])]}, {"expr": [(LV, "In", ["7", "0"])]}])
            terms.append([{"fields": [("metadata.name", "NotIn", [name])]}])
            quiet.append(len(terms) - 1)
    quiet.append(next(i for i, t in enumerate(terms) if t[0].get("expr", [("", )])[0][0] == "nokey"))
    return [dict(ctr=dict(cpu=100, mem=64 * MI), terms=t, edge=i not in quiet) for i, t in enumerate(terms)]


def _slot_terms(terms, j):
    """Every task leaves out the nodes of one slot (a seventh of them), by a
    requirement AND-ed into each of its terms."""
    ex = ("slot", "NotIn", [str(j % 7)])
    if terms is None:
        return [{"expr": [ex]}]
    return [dict(t, expr=list(t.get("expr", [])) + [ex]) if (t.get("expr") or t.get("fields")) else t for t in terms]


# --- the allocate kind --------------------------------------------------------
CROSS_TYPES = ["pipe_a", "cpu_a", "cpu_b", "mem_a", "mem_b", "gpu_a", "gpu_b", "pods_a", "port_a", "gang_fit",
               "gang_d0", "gang_d1", "pods_b", "pipe_b", "port_b"]
CROSS_ACTIVE_MAX = 5   # repetitions the gangs select in a cluster above 257 nodes, spread over it
CROSS_REQ = (1000, GI, 1000)
CROSS_PORT = 9000


def _cross_active(n_nodes):
    """{repetition: its index among the repetitions the gangs select}.  Up to
    257 nodes every whole repetition of the types; above, CROSS_ACTIVE_MAX of
    them at equal distances, so that the gangs stay small (the faithful
    restatement is quadratic in the nodes for every task) and still cross
    their thresholds in every part of the node array.  The other rows are in
    the same walks and miss the first task at exactly eps."""
    reps = max(1, n_nodes // len(CROSS_TYPES))
    act = reps if n_nodes <= 257 else CROSS_ACTIVE_MAX
    stride = reps // act
    return {i * stride: i for i in range(act)}


def _cross_row(rng, fam, rep, idx, tight):
    k = 2 + (rep if idx is None else idx) % 2
    row = _plain_row(rng, fam)
    row["labels"]["fam"] = fam.split("_")[0]
    pod, alloc = [row["pod"][r] for r in RES], row["alloc"]

    def idle(r, v):
        alloc[r] = pod[r] + v
    if idx is None and not tight:
        # a repetition the gangs are not sized for: in their walks, and the first task
        # already misses at exactly eps in the family's resource
        if fam.startswith("gang_d"):
            return _cross_row(rng, fam, rep, 0, tight)
        r = RES.index(fam[:3]) if fam[:3] in ("mem", "gpu") else 0
        idle(r, (100 if fam[:3] in ("pod", "por") else CROSS_REQ[r]) - EPS[r])
    elif fam[:3] in ("cpu", "mem", "gpu") and fam[3] == "_":
        r = RES.index(fam[:3])
        idle(r, CROSS_REQ[r] * k - (EPS[r] - 1 if fam.endswith("_a") else EPS[r]))
    elif fam.startswith("pods"):
        row["maxtasks"] = 1 + k
    elif fam.startswith("pipe"):   # Idle holds k tasks by cpu, the deleting pod's Releasing three more
        row["pod"] = dict(cpu=3 * CROSS_REQ[0], mem=3 * CROSS_REQ[1] + 5, gpu=0, deleting=True)
        pod = [row["pod"][r] for r in RES]
        for r in range(3):
            idle(r, AMPLE[r])
        idle(0, CROSS_REQ[0] * k - (EPS[0] - 1))
    elif fam == "gang_fit":  # holds exactly one task of the gang, by cpu
        idle(0, CROSS_REQ[0] - (EPS[0] - 1))
    elif fam in ("gang_d0", "gang_d1"):  # cpu misses; memory / GPU FitDelta 0 or -1
        d = 0 if fam == "gang_d0" else 1
        idle(0, CROSS_REQ[0] - EPS[0] - rep)
        idle(1, CROSS_REQ[1] + EPS[1] - d)
        idle(2, CROSS_REQ[2] + EPS[2] - d)
    if tight and fam[:3] not in ("cpu", "pip", "gan"):  # predicates off: cpu is short on every node
        idle(0, CROSS_REQ[0] * k - (EPS[0] - 1))
    return row


def _tight_jobs(rows):
    """disablePredicate: every job meets every node, so one gang is sized
    against the whole cluster (what Idle holds by cpu, then the Releasing of
    the pipe rows, and two tasks more); a second, small gang competes for the
    same nodes."""
    cap = 0
    for r in rows:
        idle = r["alloc"][0] - r["pod"]["cpu"]
        cap += 0 if idle <= CROSS_REQ[0] - EPS[0] else (idle - (CROSS_REQ[0] - EPS[0] + 1)) // CROSS_REQ[0] + 1
        cap += 3 if r["pod"].get("deleting") else 0
    return [("jall", "cpu", cap + 2, max(2, cap // 2), dict(cpu=CROSS_REQ[0], mem=64 * MI)),
            ("jlate", "gang", 3, 3, dict(cpu=CROSS_REQ[0], mem=65 * MI))]


def _cross_jobs(reps):
    """(job name, node-selector family, tasks, minMember, container)."""
    per = {0: 2, 1: 3}
    cap_a = sum(per[r % 2] for r in range(reps))          # what the _a rows hold
    cap_b = sum(per[r % 2] - 1 for r in range(reps))      # the _b rows: one fewer each
    base = dict(cpu=CROSS_REQ[0], mem=64 * MI)
    jobs = []
    for r, res in enumerate(RES):
        c = dict(cpu=500, mem=64 * MI)
        c[res] = CROSS_REQ[r]
        n = cap_a + cap_b + 2
        jobs.append((f"j{res}", res, n, max(2, n // 2), c))
    jobs.append(("jpods", "pods", 2 * cap_a + 2, max(2, cap_a), dict(cpu=100, mem=64 * MI)))
    jobs.append(("jpipe", "pipe", 2 * cap_a + 6 * reps + 2, max(2, cap_a), dict(base)))
    jobs.append(("jport", "port", 2 * reps + 2, max(2, reps),
                 dict(cpu=100, mem=64 * MI, ports=[dict(ip="", proto="", port=CROSS_PORT)])))
    jobs.append(("jgang", "gang", reps + 1, reps + 1, dict(cpu=CROSS_REQ[0], mem=CROSS_REQ[1], gpu=CROSS_REQ[2])))
    return jobs


# ----------------------------------------------------------------------------
# build
# ----------------------------------------------------------------------------
def _requests(ctr):
    return [ctr.get("cpu", 0), ctr.get("mem", 0), ctr.get("gpu", 0)]


def build(kbgen, kind, n_nodes, seed=SEED, taints=131, flags=None) -> PredSnap:
    rng = np.random.default_rng(seed)
    snap = PredSnap(kind)
    tight = bool(flags) and "disablePredicate" in flags.get("predicates", [])
    active = _cross_active(n_nodes) if kind == "cross" else {}
    if kind == "fit":
        types, tasks = FIT_TYPES, _fit_tasks()
    elif kind == "count":
        types, tasks = COUNT_TYPES, [dict(t, edge=True) for t in PLAIN_TASKS]
    elif kind == "taints":
        types, tasks = _taint_types(taints), _taint_tasks(taints)
        defs = _taint_defs(taints)
    elif kind == "ports":
        types, tasks = _port_types(), _port_tasks()
    elif kind == "labels":
        types, tasks = LABEL_VALUES, _label_tasks(n_nodes)
    else:
        types = CROSS_TYPES
    T = len(types)
    for n in range(n_nodes):
        ty, rep = types[n % T], n // T
        if kind == "fit":
            row = _fit_row(rng, ty)
        elif kind == "count":
            row = _plain_row(rng, f"maxtasks{ty}", maxtasks=ty)
        elif kind == "taints":
            row = _plain_row(rng, ty[0], taints=[defs[i] if i >= 0 else (defs[0][0], defs[0][1], "PreferNoSchedule")
                                                 for i in ty[1]])
        elif kind == "ports":
            row = _plain_row(rng, ty[0] if n == 0 or ty[0] != "filler" else "none")
            row["pod"]["ports"] = ty[1] if n == 0 or ty[0] != "filler" else []  # one pod lists them all: node 0's
        elif kind == "labels":
            row = _plain_row(rng, f"lv_{ty}")
            if ty is not None:
                row["labels"]["lv"] = ty
        else:
            row = _cross_row(rng, ty, rep, active.get(rep), tight)
        row["name"] = f"n{n:05d}"
        row["labels"].update({HOSTNAME: row["name"], "slot": str((n + rep) % 7)})
        snap.rows.append(row)

    c = kbgen.Cluster(flags=flags)
    snap.pred_off = bool(flags) and "disablePredicate" in flags.get("predicates", [])
    snap.score_off = bool(flags) and "disableNodeOrder" in flags.get("nodeorder", [])
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    c.add_job("ns", "run", "q1", min_member=1, ts=0)
    for n, r in enumerate(snap.rows):
        c.add_node(r["name"], r["alloc"][0], r["alloc"][1], r["alloc"][2], r["maxtasks"], labels=r["labels"],
                   taints=r["taints"], unschedulable=bool(r.get("unsched")))
        p = r["pod"]
        ctr = {k: p[k] for k in ("cpu", "mem", "gpu", "ports") if k in p}
        c.add_pod("ns", f"r{n:05d}", uid=f"r{n:05d}", group="run", node=r["name"], phase="Running",
                  deleting=bool(p.get("deleting")), backfill=bool(p.get("backfill")), containers=[ctr])
    if kind == "cross":
        tasks = []
        for ji, (jn, fam, cnt, mm, ctr) in enumerate(_tight_jobs(snap.rows) if tight else _cross_jobs(len(active))):
            c.add_job("ns", jn, "q0", min_member=mm, ts=ji + 1)
            snap.jobs["ns/" + jn] = []
            for k in range(cnt):
                snap.jobs["ns/" + jn].append(len(tasks))
                tasks.append(dict(ctr=ctr, nsel={"fam": fam}, job=jn))
    for j, t in enumerate(tasks):
        t.setdefault("job", f"pj{j:02d}")
        if kind != "cross":
            c.add_job("ns", t["job"], "q0", min_member=1, ts=j + 1)
            if not t.get("noslot"):
                t["terms"] = _slot_terms(t.get("terms"), j)
        t["req"] = t["ireq"] = _requests(t["ctr"])
        t["nz"] = se.nonzero([{k: t["ctr"][k] for k in ("cpu", "mem") if k in t["ctr"]}])
        t["pod"] = n_nodes + j
        aff = {"node": {"required": t["terms"]}} if t.get("terms") is not None else None
        c.add_pod("ns", f"u{j:04d}", uid=f"u{j:04d}", group=t["job"], ts=j + 1, affinity=aff,
                  containers=[dict(t["ctr"])], node_selector=dict(t.get("nsel", {})), tolerations=list(t.get("tols", [])))
    snap.tasks, snap.cluster = tasks, c
    # the ids the engine's numbering gives: taints by first appearance over the
    # nodes; port triples by (protocol, port, IP), protocols and IPs in the
    # order the pods (Running first) first use them
    for r in snap.rows:
        for t in r["taints"]:
            if t[2] in ("NoSchedule", "NoExecute"):
                snap.taint_id.setdefault(t, len(snap.taint_id))
    ips, protos, seen = {}, {}, []
    for ctr in [r["pod"] for r in snap.rows] + [t["ctr"] for t in tasks]:
        for pt in ctr.get("ports", []):
            if pt["port"] > 0:
                u = sanitize(pt)
                ips.setdefault(u[0], len(ips))
                protos.setdefault(u[1], len(protos))
                seen.append(u)
    for i, u in enumerate(sorted(set(seen), key=lambda u: (protos[u[1]], u[2], ips[u[0]]))):
        snap.port_id[u] = i
    return snap


# (name, kind, nodes, taints in the universe, plugin flags)
CASES = [(f"{k}{n}", k, n, 131, None) for k in ("fit", "count", "taints", "ports", "labels") for n in NODE_COUNTS] + \
        [("taints64u", "taints", 65, 64, None), ("taints65u", "taints", 65, 65, None)] + \
        [(f"cross{n}", "cross", n, 131, None) for n in NODE_COUNTS] + \
        [("cross65nopred", "cross", 65, 131, {"predicates": ["disablePredicate"]})]
CROSS_NAMES = [c[0] for c in CASES if c[1] == "cross"]


def write_cases(kbgen, directory, names=None):
    """{name: (PredSnap, path of its KBS1 file)} for CASES."""
    out = {}
    for name, kind, n, taints, flags in CASES:
        if names is None or name in names:
            snap = build(kbgen, kind, n, taints=taints, flags=flags)
            out[name] = (snap, snap.cluster.write(str(directory / (name + ".kbs"))))
    return out


# ----------------------------------------------------------------------------
# conditions on the snapshots themselves
# ----------------------------------------------------------------------------
def thresholds(snap):
    """[(threshold, rows on the passing side, rows on the failing side)] of the
    snapshot's family, from the reference; a row counts for a task only where
    the task's other predicates pass."""
    m, out, N = snap.model(), [], len(snap.rows)
    live = {j: set(m.passing(j).tolist()) for j in range(len(snap.tasks))}
    if snap.kind == "fit":
        for k, res in enumerate(RES):
            for src in ("idle", "bf", "rel"):
                sides = {-1: set(), 0: set(), 1: set()}
                for n in range(N):
                    if src == "rel":
                        if not any(m.rel[n]):
                            continue
                        avail = m.rel[n][k]
                    else:
                        if bool(any(m.bf[n])) != (src == "bf") or any(m.rel[n]):
                            continue
                        avail = m.idle[n][k] + m.bf[n][k]
                    for j, t in enumerate(snap.tasks):
                        d = t["ireq"][k] - avail - EPS[k]
                        if n in live[j] and d in sides:
                            sides[d].add(n)
                out.append((f"{res} {src} eps-1|eps", sides[-1], sides[0]))
                out.append((f"{res} {src} eps-1|eps+1", sides[-1], sides[1]))
        return out
    if snap.kind == "cross":
        # the rows a job selects (every row with predicates off): a k-th task of the job
        # meets req - Idle = eps - 1 on one side and eps on the other; pods: the node
        # accepts 2 or 3 tasks; gang: memory FitDelta of its last task 0 or -1
        for uid, js in snap.jobs.items():
            t = snap.tasks[js[0]]
            rows = m.passing(js[0]).tolist()
            for k, res in enumerate(RES):
                if uid == f"ns/j{res}" or (uid == "ns/jall" and k == 0):
                    side = {d: {n for n in rows if m.idle[n][k] >= 0 and (t["req"][k] - m.idle[n][k]) % t["req"][k] == d}
                            for d in (EPS[k] - 1, EPS[k])}
                    out.append((f"{uid} {res} k-th at eps-1|eps", side[EPS[k] - 1], side[EPS[k]]))
            if uid == "ns/jpipe":   # Idle gives out after 2 or 3 tasks, then Releasing takes over
                k2 = {n for n in rows if (m.idle[n][0] + EPS[0] - 1) // CROSS_REQ[0] == 2}
                out.append(("pipe k 2|3", k2, set(rows) - k2))
            if uid == "ns/jpods":
                out.append(("pods k 2|3", {n for n in rows if snap.rows[n]["maxtasks"] == 3},
                            {n for n in rows if snap.rows[n]["maxtasks"] == 4}))
            if uid == "ns/jgang":
                d = {n: m.fit_delta(js[0], n)[1] for n in rows}
                out.append(("gang memory delta 0|-1", {n for n in rows if d[n] == 0}, {n for n in rows if d[n] == -1}))
        return out
    for j, t in enumerate(snap.tasks):
        if not t.get("edge"):
            continue
        # the family's own verdict: the task without its slot requirement
        terms = t.get("terms")
        if terms is not None:
            terms = [dict(x, expr=[e for e in x.get("expr", []) if e[0] != "slot"]) for x in terms]
            terms = None if all(not x.get("expr") and not x.get("fields") for x in terms) and snap.kind != "labels" else terms
        ok = set(m.passing(j, dict(t, terms=terms)).tolist())
        out.append((f"task {j}", ok, set(range(N)) - ok))
    return out
