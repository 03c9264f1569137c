"""Predicates, fit and FitDelta at their thresholds, without a GPU.

tests/prededges.py builds clusters whose rows sit on the edges of the
predicates and of the resource fit (req - avail at eps - 1 / eps / eps + 1 per
resource and source, pods at maxtasks, 131 taints in three words, 340 port
triples in six words with pairs across word boundaries, label values that
parse, overflow or do not parse under Gt / Lt, gangs that cross a threshold
under their own placements) and restates kube-batch's rules in plain Python.
Here three parties must agree, key for key:

* the Python reference (prededges.Model),
* the faithful restatement (oracle.ref_sweep_scores / ref_allocate /
  ref_gang_close),
* the host compilation of the device header (check_keys of
  tests/test_device_math.py: fit and kind bit included).

The device compilation is held to the same reference by
tests/test_gpu_pred_edges.py.
"""
import numpy as np
import pytest

import prededges as pe
from test_device_math import check_keys

NAMES = [c[0] for c in pe.CASES]
STATIC = [c[0] for c in pe.CASES if c[1] != "cross"]
CROSS = [n for n in pe.CROSS_NAMES if n != "cross65nopred"]
SIZE = {c[0]: c[2] for c in pe.CASES}


@pytest.fixture(scope="module")
def cases(kbgen_mod, tmp_path_factory):
    return pe.write_cases(kbgen_mod, tmp_path_factory.mktemp("pred_edges"))


@pytest.fixture(scope="module")
def sessions(oracle_mod, cases):
    """{name: (placement log, gang messages)} of the faithful restatement's allocate."""
    return {n: (oracle_mod.ref_allocate(cases[n][1]).as_list(), oracle_mod.ref_gang_close(cases[n][1]))
            for n in pe.CROSS_NAMES}


def _tasks(snap):
    """Every task of a static case; of an allocate case the first of each job (the rest are identical)."""
    return [v[0] for v in snap.jobs.values()] if snap.kind == "cross" else list(range(len(snap.tasks)))


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_restatement(oracle_mod, cases, name):
    snap, path = cases[name]
    n, m = len(snap.rows), snap.model()
    for j in _tasks(snap):
        cnt, keys = oracle_mod.ref_sweep_scores(path, snap.tasks[j]["pod"], n, "")
        exp = m.expected_keys(j)
        bad = np.nonzero(keys != exp)[0]
        assert cnt == np.count_nonzero(exp) and bad.size == 0, (
            j, [(int(b), snap.family(int(b)), hex(int(keys[b])), hex(int(exp[b]))) for b in bad[:4]])


@pytest.mark.parametrize("name", NAMES)
def test_host_header_agrees(engine_lib, oracle_mod, cases, name):
    """check_keys: the engine's replayed keys equal the hoisted restatement's
    before every task of an allocate + backfill session; before the first, when
    every row is still as built, they are the reference's, zero / non-zero and
    kind bit included."""
    snap, path = cases[name]
    tr = check_keys(path, oracle_mod)
    assert len(tr["pod"]) >= 1
    j = [t["pod"] for t in snap.tasks].index(int(tr["pod"][0]))
    got, exp = tr["key"][0], snap.model().expected_keys(j, fit=True)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, [(int(b), snap.family(int(b)), hex(int(got[b])), hex(int(exp[b]))) for b in bad[:4]]


def _replay(snap, log):
    """The reference's node state after the log; per job the first placement
    checked against the reference's own choice on the state before it."""
    m, pod2j, seen, firsts = snap.model(), {t["pod"]: j for j, t in enumerate(snap.tasks)}, set(), []
    for pod, node, status in log:
        j, kind = pod2j[pod], pe.ALLOCATED if status == 4 else pe.PIPELINED
        if snap.tasks[j]["job"] not in seen:
            seen.add(snap.tasks[j]["job"])
            firsts.append((j, m.choice(j), (node, kind)))
        m.commit(j, node, kind)
    return m, firsts


@pytest.mark.parametrize("name", CROSS)
def test_first_placements_and_gang_messages(cases, sessions, name):
    """Jobs select disjoint node families, so each job's first task meets its
    family as built: the reference's Allocated / Pipelined / none per node at
    open decides the same node and kind as the restatement.  The messages of
    the jobs left not Ready are the reference's FitError histogram of one of
    their unplaced tasks on the reference's own state after the log."""
    snap, _ = cases[name]
    log, msgs = sessions[name]
    m, firsts = _replay(snap, log)
    assert firsts and all(mine == theirs for _, mine, theirs in firsts), firsts
    placed = {p for p, _, _ in log}
    if SIZE[name] >= 63:
        assert "ns/jgang" in msgs
    for uid, msg in msgs.items():
        if uid not in snap.jobs:   # the Running pods' job, where its only counted pod is Releasing
            continue
        left = [j for j in snap.jobs[uid] if snap.tasks[j]["pod"] not in placed]
        assert left and msg.split(": ", 1)[1] == m.fit_counts(left[0]), (uid, msg)
    if SIZE[name] >= 63:   # nodes at FitDelta 0 and -1 are told apart
        _, d = m.fit_deltas(snap.jobs["ns/jgang"][-1])
        assert (d[:, 1] == 0).sum() >= 4 and (d[:, 1] == -1).sum() >= 4
        assert (d[:, 2] == 0).sum() >= 4 and (d[:, 2] == -1).sum() >= 4


def test_first_placement_without_predicates(cases, sessions):
    """disablePredicate: every node is in every walk; the very first placement
    is the reference's choice on the clusters as built."""
    snap, _ = cases["cross65nopred"]
    _, firsts = _replay(snap, sessions["cross65nopred"][0])
    assert firsts[0][1] == firsts[0][2]
    assert snap.model().passing(0).size == 65


@pytest.mark.parametrize("name", NAMES)
def test_conditions(cases, sessions, name):
    """Conditions on the inputs, from the reference alone: in every case of at
    least 63 nodes each threshold of the family has 4 rows or more on either
    side, and each task's predicates pass on 10 % to 90 % of the nodes; each
    allocate case, the one-node one and the one with disablePredicate included,
    places at least 2 tasks as Allocated, 1 as Pipelined and leaves 1 unplaced.
    (With disablePredicate no predicate runs, so there is no pass rate.)"""
    snap, _ = cases[name]
    if snap.kind == "cross":
        log = sessions[name][0]
        alloc, pipe = sum(s == 4 for _, _, s in log), sum(s == 8 for _, _, s in log)
        assert alloc >= 2 and pipe >= 1 and len(log) < len(snap.tasks), (alloc, pipe, len(log))
    if SIZE[name] < 63:
        return
    th = pe.thresholds(snap)
    assert len(th) >= (1 if snap.pred_off else 3)
    low = [(t, len(a), len(b)) for t, a, b in th if min(len(a), len(b)) < 4]
    assert not low, low
    m = snap.model()
    for j in ([] if snap.pred_off else _tasks(snap)):
        rate = m.passing(j).size / len(snap.rows)
        assert 0.10 <= rate <= 0.90, (j, rate)


def test_ids_sit_where_the_rows_aim(cases):
    """The engine numbers taints by first appearance over the nodes and port
    triples by (protocol, port, IP in first-use order) (02_open.cpp); under that
    numbering the special rows sit on the word boundaries.  The ids here are
    derived from that rule by prededges, not read from the engine: only the word
    counts (131 taints = 3 words, 340 triples = 6) hold whatever the order."""
    snap, _ = cases["taints65"]
    defs = pe._taint_defs(131)
    assert [snap.taint_id[defs[i]] for i in (0, 63, 64, 127, 128, 130)] == [0, 63, 64, 127, 128, 130]
    assert len(cases["taints64u"][0].taint_id) == 64 and len(cases["taints65u"][0].taint_id) == 65
    snap, _ = cases["ports65"]
    ids = snap.port_id
    assert len(ids) == 340
    assert ids[(pe.IP_A, "TCP", pe.PAIR_A)] == 63 and ids[("0.0.0.0", "TCP", pe.PAIR_A)] == 64
    assert ids[("0.0.0.0", "TCP", pe.PAIR_B)] == 127 and ids[(pe.IP_B, "TCP", pe.PAIR_B)] == 128
    assert ids[("0.0.0.0", "TCP", pe.PORT_BASE)] == 0 and ids[("0.0.0.0", "TCP", pe._port_of_id(191))] == 191
    assert ids[("0.0.0.0", "TCP", pe._port_of_id(200))] == 200
    assert min(i for u, i in ids.items() if u[1] == "UDP") == 330   # the last word, one word wide


def _changed(snap, **bent):
    """Rows (task, node pairs) whose allocate key differs under a bent rule."""
    rules = pe.Rules()
    for k, v in bent.items():
        setattr(rules, k, v)
    a, b = snap.model(), snap.model(rules)
    return sum(int((a.expected_keys(j, fit=True) != b.expected_keys(j, fit=True)).sum()) for j in _tasks(snap))


MUTANTS = [("fit65", dict(le_at_eps=True), 138), ("fit65", dict(eps=(9, 9 * pe.MI, 9)), 282),
           ("fit65", dict(eps=(11, 11 * pe.MI, 11)), 168), ("taints65", dict(taint_word0=True), 281),
           ("ports65", dict(port_shift=True), 17), ("labels65", dict(gt_ge=True), 30),
           ("labels65", dict(unparsable_zero=True), 79), ("count65", dict(count_lt=True), 36)]


@pytest.mark.parametrize("name,bent,measured", MUTANTS, ids=[next(iter(m[1])) + str(i) for i, m in enumerate(MUTANTS)])
def test_mutants_are_caught(cases, name, bent, measured):
    """Each bent rule changes allocate keys in its family's 65-node case: the
    guard that the rows are adversarial.  Measured (task, node) pairs whose key
    changes: '<=' at eps 138; eps 9: 282; eps 11: 168; only taint word 0
    compared 281; the port window pushed down instead of cut at port_words 17
    (without the cut the engine would read past its columns: the mutant models
    the in-bounds alternative, a 4-word window starting at port_words - 4 with
    masks still relative to pw_lo); '>=' in Gt 30; an unparsable value read as
    0: 79; maxtasks < pods 36."""
    assert _changed(cases[name][0], **bent) == measured
