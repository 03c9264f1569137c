"""Score-edge snapshots and an independent reference of the node score.

Every placement, ranking and walk rests on the nodeorder arithmetic
(nodeorder.go:281-313): LeastRequested (least_requested.go:44-53),
BalancedResourceAllocation (balanced_resource_allocation.go:41-77) and the
inter-pod affinity normalisation (interpod_affinity.go:228-237).  The
generators of kbgen draw from round numbers, at which the truncations of that
arithmetic sit far from any integer.  build() makes clusters that sit on them.

Every node carries one Running pod.  A row is designed for one of the pending
tasks (EdgeSnap.design): for that task the scalars the score reads,
rc = task non-zero cpu + node non-zero cpu, acpu, rm, amem, are the row's
(rc, acpu, rm, amem); for the other tasks the same node is an ordinary row.

score() / expected_keys() write the Go formulas out in Python floats (IEEE
double, one rounding per operation, as Go) and Python integers.  They use
neither the oracle nor the engine's header.  bra_exact() is the same BRA in
exact rationals: not an expected value, a guard that the rows are adversarial.
"""
from fractions import Fraction

import numpy as np

MI = 1 << 20
# k8s priorities/util/non_zero.go:29-33: what a container that names no cpu /
# memory request counts as in the nodeorder sums
DEFAULT_NZ_CPU, DEFAULT_NZ_MEM = 100, 200 * MI
HOSTNAME = "kubernetes.io/hostname"
NODE_COUNTS = (1, 63, 64, 65, 257, 1200)
UNEQUAL_WEIGHTS = {"leastrequested.weight": "3", "balancedresource.weight": "-2"}

# pending tasks of the plain snapshots: (cpu, mem); None = the container names neither
TASKS = [(1, 1), (333, 300_000_001), (1000, 3 * (1 << 30) + 7), None, (7, 12_345_678)]
# pending tasks of the inter-pod snapshot: requests, preferred pod-affinity
# weights on the pod labels b0.., preferred anti-affinity weights; the spread
# hi - lo of the weighted counts is the sum of all of them
IPA_TASKS = [((333, 300_000_001), {0: 1, 1: 2, 2: 3, 3: 4}, {}),                        # 10
             ((1, 1), {0: 1, 1: 2, 2: 4, 3: 8, 4: 16, 5: 18}, {}),                       # 49
             ((1000, 3 * (1 << 30) + 7), {0: 1, 1: 2, 2: 4, 3: 8, 4: 16, 5: 32, 6: 35}, {}),  # 98
             ((7, 12_345_678), {0: 1, 1: 2, 2: 4, 3: 8, 4: 16, 5: 32}, {6: 40})]         # 103, lo = -40
IPA_SPREADS = (10, 49, 98, 103)
IPA_BITS = 7


# ----------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------
def nonzero(containers, d_cpu=DEFAULT_NZ_CPU, d_mem=DEFAULT_NZ_MEM):
    """GetNonzeroRequests summed over the containers (non_zero.go:37-52)."""
    return (sum(c["cpu"] if "cpu" in c else d_cpu for c in containers),
            sum(c["mem"] if "mem" in c else d_mem for c in containers))


def lr_score(req: int, cap: int) -> int:
    """least_requested.go:44-53, Go int64."""
    if cap == 0 or req > cap:
        return 0
    return ((cap - req) * 10) // cap


def fraction(req: int, cap: int) -> float:
    """balanced_resource_allocation.go:72-77."""
    return 1.0 if cap == 0 else float(req) / float(cap)


def bra_score(rc: int, acpu: int, rm: int, amem: int) -> int:
    """balanced_resource_allocation.go:41-70 (no volumes), IEEE double."""
    cpu_f, mem_f = fraction(rc, acpu), fraction(rm, amem)
    if cpu_f >= 1 or mem_f >= 1:
        return 0
    diff = abs(cpu_f - mem_f)
    return int((1 - diff) * 10.0)


def bra_exact(rc: int, acpu: int, rm: int, amem: int) -> int:
    """bra_score in exact rational arithmetic."""
    cpu_f = Fraction(1) if acpu == 0 else Fraction(rc, acpu)
    mem_f = Fraction(1) if amem == 0 else Fraction(rm, amem)
    if cpu_f >= 1 or mem_f >= 1:
        return 0
    return int((1 - abs(cpu_f - mem_f)) * 10)


def ipa_score(cnt: int, lo: int, hi: int) -> int:
    """interpod_affinity.go:228-237: the counts are float64 in Go."""
    if hi - lo > 0:
        return int(10.0 * ((float(cnt) - float(lo)) / (float(hi) - float(lo))))
    return 0


def score(rc, acpu, rm, amem, ipa=0, w_lr=1, w_bra=1, w_pa=1) -> int:
    """nodeorder.go:281-313 without node affinity."""
    lr = (lr_score(rc, acpu) + lr_score(rm, amem)) // 2
    return lr * w_lr + bra_score(rc, acpu, rm, amem) * w_bra + ipa * w_pa


def pack_key(s: int, node: int) -> int:
    """The selection key of a node that passes: score, then lowest index."""
    return ((s + (1 << 31)) << 32) | ((0x7FFFFFFF - node) << 1)


# ----------------------------------------------------------------------------
# the rows
# ----------------------------------------------------------------------------
def _bra_ties(rng, n):
    """cpuF - memF = +-k/10 exactly: acpu = 10a, amem = acpu T; the tie and its
    four neighbours rc +- 1, rm +- 1."""
    rows = []
    for i in range(n):
        k = 1 + i % 9
        a = int(rng.integers(1, 6400)) if i % 4 else int(rng.integers(1, 40))
        kind = i % 3
        T = (1 << int(rng.integers(0, 21))) if kind == 0 else 999_983 if kind == 1 else int(rng.integers(1, 1 << 21))
        acpu, amem = 10 * a, 10 * a * T
        if (i // 9) % 2 == 0:  # cpu ahead of memory
            if k * a + 1 > 10 * a - 1:
                continue
            rc = int(rng.integers(k * a + 1, 10 * a))
            rm = (rc - k * a) * T
        else:                  # memory ahead of cpu
            if 10 * a - k * a - 1 < 1:
                continue
            rc = int(rng.integers(1, 10 * a - k * a))
            rm = (rc + k * a) * T
        rows.append(("bra_tie", rc, acpu, rm, amem))
        for drc, drm in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            rows.append(("bra_near", rc + drc, acpu, rm + drm, amem))
    return rows


LR_CAPS = [1, 2, 3, 7, 10, 20, 1000, 4000, 96000, (1 << 20) + 10, 10 ** 7 + 30, (1 << 31) - 1, 1 << 31,
           5 * ((1 << 32) + 1), 10 ** 12 + 10, 10 * ((1 << 44) - 1), 3 * (1 << 48), (1 << 50) - 1, 1 << 50]


def _lr_rows(which):
    """(cap - req) * 10 divisible by cap and req +- 1 around it, req = 1,
    cap, cap + 1, for cap = 1 .. 2^50 in one resource; the other resource sits
    in the middle of the LR step of the same parity, so that the halved sum
    moves with an off-by-one in either."""
    rows = []
    for cap in LR_CAPS:
        reqs = {1: "lr_one", cap: "lr_full", cap + 1: "lr_over"}
        for q in range(0, 10):
            if (cap * (10 - q)) % 10 == 0:
                r = cap * (10 - q) // 10
                for d, fam in ((0, "lr_tie"), (-1, "lr_near"), (1, "lr_near")):
                    if r + d >= 1:
                        reqs.setdefault(r + d, fam)
        for req, fam in sorted(reqs.items()):
            m = lr_score(req, cap)
            m = m if m <= 9 else 8         # the partner's LR score: same parity, mid-step
            if which == "cpu":
                M = (1 << 26) + 3
                rows.append((fam + "_cpu", req, cap, M * (2 * (10 - m) - 1), 20 * M))
            else:
                M = 401
                rows.append((fam + "_mem", M * (2 * (10 - m) - 1), 20 * M, req, cap))
    return rows


def _degenerate(rng, n):
    rows = []
    for i in range(n):
        a = int(rng.integers(2, 5000))
        T = int(rng.integers(1 << 24, 1 << 30))
        rc = int(rng.integers(8, 10 * a))
        # a zero allocatable: the Running pod leaves that resource out (rc / rm is not the row's)
        rows.append(("acpu_zero", 0, 0, int(rng.integers(1, 10 * a * T)), 10 * a * T))
        rows.append(("amem_zero", rc, 10 * a, 0, 0))
        rows.append(("over_cpu", 10 * a + 1 + (i % 3) * 3, 10 * a, rc * T, 10 * a * T))
        rows.append(("over_mem", rc, 10 * a, 10 * a * T + 1 + (i % 2) * 1000, 10 * a * T))
        rows.append(("equal", rc, 10 * a, rc * T, 10 * a * T))
    return rows


# rows whose Running pod and designed task name neither cpu nor memory: with
# the defaults 100 m / 200 MiB each, rc = 200 and rm = 400 MiB, and
# acpu = 10a, amem = acpu T make cpuF - memF = -+k/10 exactly
def _unnamed():
    rows = []
    for k, a in ((1, 100), (2, 60), (3, 50), (4, 40), (5, 35), (6, 30), (7, 25), (8, 24), (9, 22)):
        rc, rm = 2 * DEFAULT_NZ_CPU, 2 * DEFAULT_NZ_MEM
        assert rm % (rc - k * a) == 0
        T = rm // (rc - k * a)
        rows.append(("unnamed", rc, 10 * a, rm, 10 * a * T))
        rows.append(("unnamed", rc, 10 * a + 10, rm, 10 * a * T))
    return rows


def _random_rows(rng, n):
    rows = []
    for _ in range(n):
        acpu = int(rng.integers(100, 128_000))
        amem = int(rng.integers(1 << 28, 1 << 40))
        rows.append(("random", int(rng.integers(1, acpu)), acpu, int(rng.integers(1, amem)), amem))
    return rows


def _pool(seed):
    rng = np.random.default_rng(seed)
    fams = [_bra_ties(rng, 120), _lr_rows("cpu"), _lr_rows("mem"), _degenerate(rng, 16), _unnamed(),
            _random_rows(rng, 120)]
    fams = [[r for r in f if r[0] in ("acpu_zero", "amem_zero") or (r[1] >= 1 and r[3] >= 1)] for f in fams]
    # interleave the families, so that a prefix of any length holds some of each
    out, i = [], 0
    while any(fams):
        f = fams[i % len(fams)]
        if f:
            out.extend(f[:5])
            del f[:5]
        i += 1
    return out


class EdgeSnap:
    """cluster: the kbgen.Cluster; rows[n] = (family, design task, acpu, amem,
    node nz cpu, node nz mem); tasks[j] = (pod index, nz cpu, nz mem);
    counts[j][n]: the raw inter-pod count of node n for task j (None: plain)."""

    def __init__(self):
        self.cluster, self.rows, self.tasks, self.counts = None, [], [], None
        self.w_lr = self.w_bra = self.w_pa = 1

    def scalars(self, j, n):
        fam, _, acpu, amem, nzc, nzm = self.rows[n]
        return self.tasks[j][1] + nzc, acpu, self.tasks[j][2] + nzm, amem

    def family(self, n):
        return self.rows[n][0]

    def designed(self, n):
        return self.rows[n][1]

    def ipa_range(self, j):
        c = self.counts[j]
        return min(0, min(c)), max(0, max(c))

    def scores(self, j, fn=score):
        out = []
        lo, hi = self.ipa_range(j) if self.counts else (0, 0)
        for n in range(len(self.rows)):
            ipa = ipa_score(self.counts[j][n], lo, hi) if self.counts else 0
            out.append(fn(*self.scalars(j, n), ipa, self.w_lr, self.w_bra, self.w_pa))
        return out

    def expected_keys(self, j):
        """Every node passes the predicates: one packed key per node."""
        return np.array([pack_key(s, n) for n, s in enumerate(self.scores(j))], np.uint64)

    def walk(self, j):
        """(nodes, scores) of the by-score walk: score descending, then index."""
        sc = np.array(self.scores(j), np.int64)
        order = np.lexsort((np.arange(sc.size), -sc))
        return order.astype(np.int32), sc[order].astype(np.int32)


def build(kbgen, seed: int, n_nodes: int, ipa: bool = False, weights=None) -> EdgeSnap:
    """The score-edge cluster of n_nodes nodes (<= ~1200).  ipa: the inter-pod
    snapshot (pod labels, hostname topology, tasks with preferred terms);
    weights: nodeorder plugin arguments."""
    pool = _pool(seed)
    assert n_nodes <= len(pool), (n_nodes, len(pool))
    rng = np.random.default_rng(seed + 1)
    tasks = [t[0] for t in IPA_TASKS] if ipa else TASKS
    tnz = [nonzero([{}] if t is None else [dict(cpu=t[0], mem=t[1])]) for t in tasks]
    snap = EdgeSnap()
    c = kbgen.Cluster(args={"nodeorder": dict(weights)} if weights else None)
    if weights:
        snap.w_lr, snap.w_bra = int(weights["leastrequested.weight"]), int(weights["balancedresource.weight"])
    c.add_queue("q0", 1)
    c.add_queue("q1", 1)  # the Running pods' queue: victim candidates of the pending tasks' walks
    c.add_job("ns", "run", "q1", min_member=1, ts=0)
    bits = []
    for n in range(n_nodes):
        fam, rc, acpu, rm, amem = pool[n]
        # the design task: one whose requests leave the Running pod a request
        # in [0, allocatable]; the tiny task (1, 1) fits every row
        if fam == "unnamed":  # (the inter-pod snapshot has no unnamed task: a plain row there)
            d = tasks.index(None) if None in tasks else tasks.index((1, 1))
            ctr = dict(cpu=DEFAULT_NZ_CPU) if n % 2 else {}  # odd: memory takes its default alone
        else:
            d = None
            for t in range(len(tasks)):
                j = (n + t) % len(tasks)
                if tasks[j] is not None and (fam == "acpu_zero" or 0 <= rc - tnz[j][0] <= acpu) and \
                        (fam == "amem_zero" or 0 <= rm - tnz[j][1] <= amem):
                    d = j
                    break
            assert d is not None, pool[n]
            ctr = dict(cpu=rc - tnz[d][0], mem=rm - tnz[d][1])
            if fam == "acpu_zero":
                ctr.pop("cpu")
            if fam == "amem_zero":
                ctr.pop("mem")
            if fam in ("acpu_zero", "amem_zero") and n % 2:  # or names it as zero
                ctr["cpu" if fam == "acpu_zero" else "mem"] = 0
        nzc, nzm = nonzero([ctr])
        name = f"n{n:05d}"
        labels, plabels = {}, {}
        if ipa:
            labels = {HOSTNAME: name}
            b = [0b0111111, 0b1111111, 0b1000000, 0][n] if n < 4 else int(rng.integers(0, 1 << IPA_BITS))
            bits.append(b)
            plabels = {f"b{k}": "1" for k in range(IPA_BITS) if b >> k & 1}
        c.add_node(name, acpu, amem, 0, 110, labels=labels)
        c.add_pod("ns", f"r{n:05d}", uid=f"r{n:05d}", group="run", node=name, phase="Running",
                  labels=plabels, containers=[ctr])
        snap.rows.append((fam, d, acpu, amem, nzc, nzm))
    for j, t in enumerate(tasks):
        c.add_job("ns", f"pj{j}", "q0", min_member=1, ts=j + 1)
        aff = None
        if ipa:
            def terms(ws):
                return [(w, {"selector": {"ml": {f"b{k}": "1"}}, "topology_key": HOSTNAME}) for k, w in ws.items()]
            aff = {"pod": {"preferred": terms(IPA_TASKS[j][1])}}
            if IPA_TASKS[j][2]:
                aff["anti"] = {"preferred": terms(IPA_TASKS[j][2])}
        c.add_pod("ns", f"u{j:02d}", uid=f"u{j:02d}", group=f"pj{j}", ts=j + 1, affinity=aff,
                  containers=[{} if t is None else dict(cpu=t[0], mem=t[1])])
        snap.tasks.append((n_nodes + j, tnz[j][0], tnz[j][1]))
    if ipa:
        snap.counts = []
        for _, pa, paa in IPA_TASKS:
            snap.counts.append([sum(w for k, w in pa.items() if b >> k & 1) - sum(w for k, w in paa.items() if b >> k & 1)
                                for b in bits])
    snap.cluster = c
    return snap


# (name, nodes, inter-pod snapshot, nodeorder weights, compared with the
# faithful restatement: its inter-pod sweep is quadratic in the nodes)
CASES = [(f"plain{n}", n, False, None, True) for n in NODE_COUNTS] + \
        [("plain65w", 65, False, UNEQUAL_WEIGHTS, True), ("plain1200w", 1200, False, UNEQUAL_WEIGHTS, True)] + \
        [(f"ipa{n}", n, True, None, True) for n in NODE_COUNTS[:-1]] + \
        [("ipa257w", 257, True, UNEQUAL_WEIGHTS, True), ("ipa1200", 1200, True, None, False)]
SEED = 20261020


def write_cases(kbgen, directory):
    """{name: (EdgeSnap, path of its KBS1 file)} for CASES."""
    out = {}
    for name, n, ipa, weights, _ in CASES:
        snap = build(kbgen, SEED, n, ipa=ipa, weights=weights)
        out[name] = (snap, snap.cluster.write(str(directory / (name + ".kbs"))))
    return out
