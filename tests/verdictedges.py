"""Why a node is lost to a task: the ordered restatement and a snapshot whose
rows fail several steps at once.

kbhip_explain_tasks gives every (task, node) pair the code of the first step
that rejects the node, in the reference's order: predicates.go:123-203 (pod
count, node selector / required node affinity, host ports, unschedulable,
taints, pod (anti-)affinity), then NodeOrderFn's error, then the fit of
allocate.go:153-173.  why() restates that order over prededges.Model's own
pieces (terms_match, port_blocked, tolerates, _le, fit_delta): plain Python
integers over the objects given to kbgen, neither the oracle nor the engine's
header.  The pod-affinity and NodeOrderFn steps are not part of that model; no
snapshot here has a class they reject (the device tests take those from the
faithful restatement's sweep).

prededges' kinds put one predicate at a time on its edges, so the order of the
steps never shows there.  build_stacked() makes the rows where it does: the 32
subsets of {full, selector mismatch, port conflict, unschedulable, untolerated
taint} crossed with six fit families (fits Idle; fits only Releasing; fits
neither, short by exactly eps in cpu, memory or GPU; Idle short but Backfilled
making it fit), plus one plain row without the selector's label: 193 types, a
count prime to the wave and block sizes, repeating with the node index so that
every lane, wave and block position sees each of them.  The tasks: A (init
containers: InitResreq = Resreq + 200 units, so a row short by eps against
InitResreq is not short against Resreq), B (no init containers, the same
InitResreq: the short bits are set there), C (a small request and the other
selector value), D (a host port with an IP against the wildcard, a toleration
with the wrong value), E (tolerates everything, asks for more cpu than any
node has: Pending after every action).
"""
import numpy as np

import prededges as pe
import scoreedges as se

MI = pe.MI
(FITS_IDLE, FITS_RELEASING, RESOURCES, POD_COUNT, NODE_SELECTOR, HOST_PORTS, UNSCHEDULABLE, TAINTS, POD_AFFINITY,
 SCORE_ERROR) = range(10)
SHORT = (0x10, 0x20, 0x40)
BINS = 16
STEPS = ("count", "selector", "ports", "unsched", "taints")
CODE = dict(count=POD_COUNT, selector=NODE_SELECTOR, ports=HOST_PORTS, unsched=UNSCHEDULABLE, taints=TAINTS)
NODE_COUNTS = se.NODE_COUNTS


def _rejects(m, step, j, n):
    ru, r, t = m.rules, m.snap.rows[n], m.snap.tasks[j]
    if step == "count":                                   # predicates.go:127
        return r["maxtasks"] <= m.pods[n]
    if step == "selector":                                # predicates.go:132-143
        if any(r["labels"].get(k) != v for k, v in t.get("nsel", {}).items()):
            return True
        return t.get("terms") is not None and not pe.terms_match(ru, t["terms"], r["labels"], r["name"])
    if step == "ports":                                   # predicates.go:146-157
        return m.port_blocked(j, n)
    if step == "unsched":                                 # predicates.go:160-171
        return bool(r.get("unsched"))
    return any(taint[2] in ("NoSchedule", "NoExecute") and not any(pe.tolerates(tol, taint) for tol in t.get("tols", []))
               for taint in r.get("taints", []))          # predicates.go:174-185


def why(m, j, n, order=STEPS, short_from="req"):
    """The verdict byte of task j on node n of the model's state.  order and
    short_from exist for the mutants: another step order; the short bits from
    InitResreq in place of Resreq."""
    t = m.snap.tasks[j]
    if not m.snap.pred_off:
        for step in order:
            if _rejects(m, step, j, n):
                return CODE[step]
    avail = [i + b for i, b in zip(m.idle[n], m.bf[n])]
    code = FITS_IDLE if m._le(t["ireq"], avail) else FITS_RELEASING if m._le(t["ireq"], m.rel[n]) else RESOURCES
    if short_from == "req":
        delta = m.fit_delta(j, n)
    else:   # resource_info.go:134-147 with another request
        delta = [a - (q + e) if q > 0 else a for a, q, e in zip(avail, t[short_from], m.rules.eps)]
    return code | sum(bit for bit, d in zip(SHORT, delta) if d < 0)


def verdicts(m, j, **kw):
    return np.array([why(m, j, n, **kw) for n in range(len(m.snap.rows))], np.uint8)


def histogram(v):
    """The 16 bins of a verdict row (include/kbhip.h)."""
    v = np.asarray(v, np.uint8)
    code, walk = v & 15, (v & 15) <= RESOURCES
    h = np.zeros(BINS, np.int64)
    for c in range(10):
        h[c] = int((code == c).sum())
    for k, bit in enumerate(SHORT):
        h[11 + k] = int((walk & ((v & bit) != 0)).sum())
    h[14], h[15] = int(walk.sum()), v.size
    return h


# ----------------------------------------------------------------------------
# the stacked snapshot
# ----------------------------------------------------------------------------
REQ = (1000, 1024 * MI, 1000)             # task A's Resreq
IREQ = (1200, 1224 * MI, 1200)            # ... and InitResreq (an init container)
FLAGS = ("full", "selmis", "port", "unsched", "taint")
FAMS = ("idle", "rel", "short_cpu", "short_mem", "short_gpu", "bf")
PORT = 9100
TAINT = ("dedicated", "x", "NoSchedule")
TYPES = [(s, f) for s in range(32) for f in FAMS] + [(None, "nolabel")]
assert len(TYPES) == 193


def _stacked_row(rng, subset, fam):
    ample = [IREQ[k] + pe.EPS[k] + pe.AMPLE[k] // 50 * int(rng.integers(1, 40)) for k in range(3)]
    pod = dict(cpu=100 * int(rng.integers(1, 9)), mem=64 * MI * int(rng.integers(1, 9)), gpu=0)
    idle = list(ample)
    if fam == "rel":          # Idle misses by cpu at exactly eps; the deleting pod's request fits by one
        idle[0] = IREQ[0] - pe.EPS[0]
        pod = dict(cpu=IREQ[0] - pe.EPS[0] + 1, mem=IREQ[1] - pe.EPS[1] + 1, gpu=IREQ[2] - pe.EPS[2] + 1, deleting=True)
    elif fam.startswith("short_"):
        k = pe.RES.index(fam[6:])
        idle[k] = IREQ[k] - pe.EPS[k]
    elif fam == "bf":         # Idle short by 100 in cpu, Backfilled 300
        idle[0] = IREQ[0] - pe.EPS[0] - 100
        pod = dict(cpu=300, mem=64 * MI, gpu=0, backfill=True)
    on = {f: subset is not None and bool(subset >> i & 1) for i, f in enumerate(FLAGS)}
    if on["port"]:
        pod["ports"] = [dict(ip="", proto="TCP", port=PORT)]
    labels = {} if subset is None else {"vz": "b" if on["selmis"] else "a"}
    taints = [TAINT] if on["taint"] else [("soft", "y", "PreferNoSchedule")] if subset is None else []
    return dict(fam=f"{fam}+" + "+".join(f for f in FLAGS if on[f]), maxtasks=1 if on["full"] else 110,
                alloc=[i + pod.get(r, 0) for i, r in zip(idle, pe.RES)], labels=labels, taints=taints,
                unsched=on["unsched"], pod=pod)


def _stacked_tasks():
    full = dict(cpu=REQ[0], mem=REQ[1], gpu=REQ[2])
    init = [dict(cpu=IREQ[0], mem=IREQ[1], gpu=IREQ[2])]
    return [
        dict(ctr=dict(full, ports=[dict(ip="", proto="TCP", port=PORT)]), init=init, nsel={"vz": "a"}, tols=[]),
        dict(ctr=dict(cpu=IREQ[0], mem=IREQ[1], gpu=IREQ[2], ports=[dict(ip="", proto="UDP", port=PORT)]), init=[],
             terms=[{"expr": [("vz", "In", ["a", "b"])]}], tols=[dict(key="dedicated", op="Exists", value="", effect="")]),
        dict(ctr=dict(cpu=100, mem=64 * MI), init=[], nsel={"vz": "b"}, tols=[]),
        dict(ctr=dict(full, ports=[dict(ip="10.0.0.1", proto="TCP", port=PORT)]), init=init,
             tols=[dict(key="dedicated", op="Equal", value="y", effect="NoSchedule")]),
        dict(ctr=dict(cpu=10_000_000, mem=64 * MI), init=[], tols=[dict(key="", op="Exists", value="", effect="")]),
    ]


def build_stacked(kbgen, n_nodes, seed=pe.SEED) -> pe.PredSnap:
    rng = np.random.default_rng(seed)
    snap = pe.PredSnap("stacked")
    for n in range(n_nodes):
        row = _stacked_row(rng, *TYPES[n % len(TYPES)])
        row["name"] = f"n{n:05d}"
        row["labels"][pe.HOSTNAME] = row["name"]
        snap.rows.append(row)
    c = kbgen.Cluster()
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)
    c.add_job("ns", "run", "q1", min_member=1, ts=0)
    for n, r in enumerate(snap.rows):
        c.add_node(r["name"], r["alloc"][0], r["alloc"][1], r["alloc"][2], r["maxtasks"], labels=r["labels"],
                   taints=r["taints"], unschedulable=bool(r["unsched"]))
        p = r["pod"]
        c.add_pod("ns", f"r{n:05d}", uid=f"r{n:05d}", group="run", node=r["name"], phase="Running",
                  deleting=bool(p.get("deleting")), backfill=bool(p.get("backfill")),
                  containers=[{k: p[k] for k in ("cpu", "mem", "gpu", "ports") if k in p}])
    tasks = _stacked_tasks()
    for j, t in enumerate(tasks):
        t["job"] = f"pj{j:02d}"
        c.add_job("ns", t["job"], "q0", min_member=1, ts=j + 1)
        t["req"] = [t["ctr"].get(r, 0) for r in pe.RES]
        t["ireq"] = [max([q] + [ic.get(r, 0) for ic in t["init"]]) for q, r in zip(t["req"], pe.RES)]
        t["nz"] = se.nonzero([{k: t["ctr"][k] for k in ("cpu", "mem") if k in t["ctr"]}])
        t["pod"] = n_nodes + j
        aff = {"node": {"required": t["terms"]}} if t.get("terms") is not None else None
        c.add_pod("ns", f"u{j:04d}", uid=f"u{j:04d}", group=t["job"], ts=j + 1, affinity=aff,
                  containers=[dict(t["ctr"])], init_containers=[dict(ic) for ic in t["init"]],
                  node_selector=dict(t.get("nsel", {})), tolerations=list(t["tols"]))
    snap.tasks, snap.cluster = tasks, c
    return snap


STACKED = [(f"stacked{n}", n) for n in NODE_COUNTS]


def write_stacked(kbgen, directory):
    """{name: (PredSnap, path of its KBS1 file)} for STACKED."""
    out = {}
    for name, n in STACKED:
        snap = build_stacked(kbgen, n)
        out[name] = (snap, snap.cluster.write(str(directory / (name + ".kbs"))))
    return out


def tasks_of(snap):
    """Every task of a static or stacked case; of an allocate case the first of each job."""
    return [v[0] for v in snap.jobs.values()] if snap.kind == "cross" else list(range(len(snap.tasks)))
