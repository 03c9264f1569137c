"""kbhip_explain_tasks' verdict logic without a GPU.

kbhip_debug_explain runs node_verdict (kbhip_eval.h), the function the
k_explain kernel runs, over the host tables of an encode-only session.  Here
its verdict bytes and histograms must equal the ordered restatement
(verdictedges.why over prededges.Model) on every prededges kind and on the
stacked snapshot, whose rows fail several steps at once.  The device
compilation is held to the same restatement by tests/test_gpu_explain.py.
"""
import numpy as np
import pytest

import prededges as pe
import verdictedges as ve

NAMES = [c[0] for c in pe.CASES] + [s[0] for s in ve.STACKED]


@pytest.fixture(scope="module")
def cases(kbgen_mod, tmp_path_factory):
    d = tmp_path_factory.mktemp("explain_model")
    out = pe.write_cases(kbgen_mod, d)
    out.update(ve.write_stacked(kbgen_mod, d))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_debug_explain_equals_the_restatement(engine_lib, cases, name):
    import kbhip
    snap, path = cases[name]
    m = snap.model()
    with kbhip.EncodedSnapshot(path) as enc:
        for j in ve.tasks_of(snap):
            got, hist = enc.explain(snap.tasks[j]["pod"])
            exp = ve.verdicts(m, j)
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, (j, [(int(b), snap.family(int(b)), hex(int(got[b])), hex(int(exp[b]))) for b in bad[:4]])
            assert np.array_equal(hist, ve.histogram(exp)), (j, hist)
            # the restatement against the model's own conjunction: in the walk exactly where every predicate passes
            assert np.array_equal(np.nonzero((exp & 15) <= ve.RESOURCES)[0], m.passing(j)), j


def test_stacked_rows_hold_every_code_and_every_short_bit(cases):
    """Conditions on the input, from the restatement alone: at 257 and 1200
    nodes every predicate code, the three fit codes and each short bit occur
    for task A or B, nodes that fail several steps exist for every pair of
    steps, and task A has rows that are short against InitResreq only."""
    for name in ("stacked257", "stacked1200"):
        snap, _ = cases[name]
        m = snap.model()
        seen, bits = set(), 0
        for j in (0, 1):
            v = ve.verdicts(m, j)
            seen |= set((v & 15).tolist())
            bits |= int(np.bitwise_or.reduce(v[(v & 15) <= ve.RESOURCES] & 0x70))
        assert seen == set(range(8)) and bits == 0x70, (name, seen, hex(bits))
        for a in range(len(ve.STEPS)):
            for b in range(a + 1, len(ve.STEPS)):
                both = [n for n in range(len(snap.rows)) if ve._rejects(m, ve.STEPS[a], 0, n) and ve._rejects(m, ve.STEPS[b], 0, n)]
                assert len(both) >= 4, (name, ve.STEPS[a], ve.STEPS[b])
        a_req, a_ireq = ve.verdicts(m, 0), ve.verdicts(m, 0, short_from="ireq")
        assert (a_req != a_ireq).sum() >= 4


def _differs(cases, name, **kw):
    """(task, node) pairs of the case whose verdict changes under a bent restatement."""
    snap, _ = cases[name]
    m = snap.model()
    return sum(int((ve.verdicts(m, j) != ve.verdicts(m, j, **kw)).sum()) for j in ve.tasks_of(snap))


SWAPS = [("selector", "count", "ports", "unsched", "taints"), ("count", "selector", "ports", "taints", "unsched"),
         ("count", "ports", "selector", "unsched", "taints")]


@pytest.mark.parametrize("order", SWAPS, ids=["count-selector", "unsched-taints", "selector-ports"])
def test_a_swapped_order_is_noticed(engine_lib, cases, order):
    """Two neighbouring steps swapped: many stacked rows change their code, and
    the engine's bytes are the unswapped ones on each of them."""
    import kbhip
    assert _differs(cases, "stacked257", order=order) >= 16
    snap, path = cases["stacked257"]
    m = snap.model()
    with kbhip.EncodedSnapshot(path) as enc:
        for j in ve.tasks_of(snap):
            got, _ = enc.explain(snap.tasks[j]["pod"])
            bent = ve.verdicts(m, j, order=order)
            rows = np.nonzero(bent != ve.verdicts(m, j))[0]
            assert (got[rows] != bent[rows]).all()


def test_short_bits_from_initresreq_are_noticed(engine_lib, cases):
    """The short bits come from Resreq (allocate.go:164-167 stores
    Idle.FitDelta(task.Resreq)): taken from InitResreq they change on the rows
    that miss InitResreq by exactly eps, where task A's Resreq is 200 units
    smaller.  The prededges kinds have InitResreq == Resreq and cannot tell."""
    import kbhip
    assert _differs(cases, "stacked257", short_from="ireq") >= 8
    assert _differs(cases, "fit65", short_from="ireq") == 0
    snap, path = cases["stacked257"]
    m = snap.model()
    with kbhip.EncodedSnapshot(path) as enc:
        got, _ = enc.explain(snap.tasks[0]["pod"])
    bent = ve.verdicts(m, 0, short_from="ireq")
    rows = np.nonzero(bent != ve.verdicts(m, 0))[0]
    assert rows.size >= 8 and (got[rows] != bent[rows]).all()
