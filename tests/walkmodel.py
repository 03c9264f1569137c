"""Host-side models for the walk read-outs (kbhip_walk_visits,
kbhip_fit_deltas): what a Go host keeps in its own NodeInfo / JobInfo objects
and updates from the engine's answers, restated in Python for the tests.

NodeModel is api.NodeInfo's resource bookkeeping (node_info.go:113-145,
209-211): Idle / Used / Releasing / Backfilled per node, GetAccessibleResource
applied `count` times per reported node, then the placement log through
AddTask.  fit_error is JobInfo.FitError (job_info.go:343-372) over a
NodesFitDelta given as an [k, 3] array of (cpu, memory, GPU) deltas.
"""
import numpy as np

MIN_CPU, MIN_MEM, MIN_GPU = 10, 10 * 1024 * 1024, 10
ALLOCATED_ST, PIPELINED_ST = 4, 8
GI = 1 << 30


class NodeModel:
    def __init__(self, open_nodes: np.ndarray, requests: np.ndarray):
        """open_nodes: [N, 12] idle, used, releasing, backfilled (cpu, mem, gpu
        each) at session open; requests: [P, 6] Resreq, InitResreq per pod."""
        st = np.asarray(open_nodes, np.float64).astype(np.int64)
        self.idle, self.used = st[:, 0:3].copy(), st[:, 3:6].copy()
        self.releasing, self.backfilled = st[:, 6:9].copy(), st[:, 9:12].copy()
        self.resreq = np.asarray(requests, np.float64)[:, 0:3].astype(np.int64)

    def visit(self, nodes, counts) -> None:
        """node.GetAccessibleResource() counts[i] times on node nodes[i]:
        Idle.Add(Backfilled) mutates Idle in place each time."""
        for n, k in zip(nodes, counts):
            self.idle[int(n)] += int(k) * self.backfilled[int(n)]

    def place(self, log) -> None:
        """ssn.Allocate / ssn.Pipeline -> NodeInfo.AddTask for (pod, node, status) records."""
        for pod, node, status in log:
            r = self.resreq[int(pod)]
            if status == PIPELINED_ST:
                self.releasing[int(node)] -= r
            else:
                self.idle[int(node)] -= r
            self.used[int(node)] += r

    def state(self) -> np.ndarray:
        return np.concatenate([self.idle, self.used, self.releasing, self.backfilled], axis=1)


def fit_delta(idle: np.ndarray, resreq: np.ndarray) -> np.ndarray:
    """Idle.Clone().FitDelta(Resreq) per row of idle [k, 3] (resource_info.go:134-147)."""
    mins = np.array([MIN_CPU, MIN_MEM, MIN_GPU], np.int64)
    r = np.asarray(resreq, np.int64)
    return np.where(r > 0, idle - (r + mins), idle)


def fit_error(deltas: np.ndarray) -> str:
    """JobInfo.FitError (job_info.go:343-372) for NodesFitDelta = the rows of deltas."""
    d = np.asarray(deltas, np.int64).reshape(-1, 3)
    if d.shape[0] == 0:
        return "0 nodes are available"
    reasons = []
    for k, name in enumerate(("cpu", "memory", "GPU")):
        c = int((d[:, k] < 0).sum())
        if c:
            reasons.append(f"{c} insufficient {name}")
    return f"0/{d.shape[0]} nodes are available, {', '.join(sorted(reasons))}."


def crowded_gangs(kbgen):
    """The crowded 160-node, 40-gang cluster of tests/test_gpu_engine.py's
    unplaceable-gangs test (same generator stream): many pops end on a task
    without a node."""
    rng = np.random.default_rng(9400)
    c = kbgen.Cluster()
    c.add_queue("q0", 1)
    for i in range(160):
        c.add_node(f"n{i:04d}", int(rng.choice([4000, 8000])), int(rng.choice([8, 16])) * GI,
                   int(rng.choice([0, 0, 4000])), 110)
    uid = 0
    for j in range(40):
        size = int(rng.integers(4, 30))
        jn = f"j{j:03d}"
        c.add_job("ns", jn, "q0", min_member=size, ts=j)
        req = kbgen.res(cpu=int(rng.choice([1000, 2000, 3000])), mem=int(rng.choice([2, 4, 6])) * GI,
                        gpu=int(rng.choice([0, 0, 0, 1000])))
        for k in range(size):
            c.add_pod("ns", f"{jn}-{k}", uid=f"p{uid:05d}", group=jn, ts=j, containers=[dict(req)])
            uid += 1
    return c


def uniform_oversized(kbgen, n_nodes: int, label_every: int = 0, selector: bool = False, unsched: bool = False):
    """n_nodes equal nodes and one gang of one task that asks for more cpu than
    any node has: every node that passes the predicates is a FitDelta record.
    label_every = k labels every k-th node pool=a (the task selects it when
    selector is set); unsched marks every node unschedulable (no node passes)."""
    c = kbgen.Cluster()
    c.add_queue("q0", 1)
    for i in range(n_nodes):
        labels = {"pool": "a"} if label_every and i % label_every == 0 else {}
        c.add_node(f"n{i:05d}", 4000 + (i % 7) * 100, (8 + i % 3) * GI, 0, 110, labels=labels, unschedulable=unsched)
    c.add_job("ns", "big", "q0", min_member=1, ts=0)
    c.add_pod("ns", "big-0", uid="p00000", group="big", ts=0, containers=[kbgen.res(cpu=64000, mem=2 * GI)],
              node_selector={"pool": "a"} if selector else {})
    return c
