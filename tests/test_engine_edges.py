"""The engine-edge clusters against the restatements, without a GPU.

tests/engineedges.py places the deciding nodes of small sessions on the pop
engine's structural seams (worker, group and owner-segment boundaries, tie
cuts, the last four pops' candidate sets, the owners' limits, run
boundaries).  A case is only worth running on the device if the reference
really does what the case was built for, so here, for every case:

* the faithful restatement (oracle.ref_allocate) runs, and its time is printed;
* the hoisted restatement (oracle.fast_allocate) gives the same log;
* the case's claims hold on that log (engineedges.check_claims): the expected
  nodes gang by gang where the construction fixes them (seam nodes ascending,
  the 64 lowest indices of a tie), every seam node deciding, a pop placing on
  nodes that the pops 1, 2, 3 and 4 back changed, a node going from best to
  infeasible between consecutive pops after being filled exactly, the unready
  gang, the pop counts, the engine-run lengths the restart hysteresis gives.

A case whose claims fail here is a broken case.  The device runs are in
tests/test_gpu_engine_edges.py.
"""
import hashlib
import time

import pytest

import engineedges as ee


@pytest.fixture(scope="module")
def cases(kbgen_mod, tmp_path_factory):
    return ee.write_cases(kbgen_mod, tmp_path_factory.mktemp("engine_edges"))


_REF = {}


def reference(oracle_mod, path):
    """The faithful restatement's (log, node state, seconds), once per distinct snapshot."""
    with open(path, "rb") as f:
        key = hashlib.sha256(f.read()).hexdigest()
    if key not in _REF:
        t0 = time.time()
        pl, nodes = oracle_mod.ref_allocate(path, with_nodes=True)
        _REF[key] = (pl.as_list(), nodes, time.time() - t0)
    return _REF[key]


@pytest.mark.parametrize("name", ee.NAMES)
def test_case_claims_hold_on_the_restatement(oracle_mod, cases, name):
    claims = ee.CASES[ee.NAMES.index(name)][3]
    cluster, path = cases[name]
    log, _, secs = reference(oracle_mod, path)
    print(f"{name}: {len(cluster.nodes)} nodes, {len(log)} placements, ref_allocate {secs:.2f} s")
    assert oracle_mod.fast_allocate(path, threads=4).as_list() == log
    m = ee.check_claims(cluster.edge, claims, log)
    print(f"{name}: {m['pops']} pops, lags {m['lags']}, vanished {m['vanished'][:4]}, runs {m['runs']}, "
          f"unready {m['unready']}")
    assert len(log) >= 2


def test_shapes_reach_the_limits():
    """The partition the builders assume is the one the issue's shapes name."""
    assert ee.eng_shape(64, 1) == (1, 64) and ee.eng_shape(65, 2) == (2, 33)
    assert ee.eng_shape(129, 3) == (3, 43) and ee.eng_shape(257, 5) == (5, 52)
    assert ee.eng_shape(4161, 66) == (66, 64) and 4161 - 65 * 64 == 1  # the last worker holds one node
    assert ee.eng_shape(8192, 1) == (1, ee.ENG_MAX_NPB) and ee.eng_shape(8193, 1)[1] > ee.ENG_MAX_NPB
    assert ee.eng_shape(8193, 2) == (2, 4097) and ee.eng_shape(845, 13) == (13, 65)
    assert ee.eng_shape(65, 8)[0] == 2  # 64 nodes per worker at least
    assert ee.seam_nodes(4161, 66)[-2:] == [4159, 4160] and 4160 in ee.seam_nodes(4161, 66)
    assert {1791, 1792, 3583, 3584} <= set(ee.seam_nodes(3585, seg=ee.OWN_SEG))
    assert ee.RUNS == [1, 15, 16, 17, 1, 1, 1, 64, 1]


def test_run_lengths_follow_the_hysteresis():
    """engine_runs on hand-made pop sequences: the backoff starts at 8,
    doubles to 64 and a run of 64 clears it."""
    class E:
        gangs = [dict(eligible=True), dict(eligible=False)]
    seq = lambda streaks: [(0, "e", [0]) if k else (1, "h", [0]) for s in streaks for k in [1] * s + [0]]
    assert ee.engine_runs(E, seq([1, 8, 9])) == [1, 1]           # 8 pops under a backoff of 8: none served
    assert ee.engine_runs(E, seq([1, 9, 17, 33, 65, 65, 128, 1])) == [1, 1, 1, 1, 1, 1, 64, 1]
    assert ee.engine_runs(E, seq([64, 1])) == [64, 1] and ee.engine_runs(E, seq([16, 1])) == [16, 1]
    assert ee.engine_runs(E, seq([15, 8, 9])) == [15, 1]
