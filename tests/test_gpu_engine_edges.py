"""The persistent pop engine at the edges of its own structure.

The clusters of tests/engineedges.py (partition seams and tie cuts under
engine_workers / engine_groups, stale rows in both modes, the owners' limits
in list mode, run boundaries; tests/test_engine_edges.py holds every case's
claims against the restatements) run through the engine under the case's
options.  The placement log, read_nodes (all columns) and gang_unschedulable()
must equal the faithful restatement's, never another device path's, and
stats() must show that the structure under test really ran: engine_workers
is the partition the case was built for, engine_owners as stated, every pop
served by the engine where every pop is eligible and none where the node
range per worker is too large.  Every case also runs with engine_quick = 0,
the stale-row cases also with speculate = 0.
"""
import numpy as np
import pytest

import engineedges as ee
from test_engine_edges import reference

pytestmark = pytest.mark.gpu

VARIANTS = [(name, v) for name, _, _, claims in ee.CASES
            for v in ("default", "levels") + (("nospec",) if claims["group"] == "B" else ())]
EXTRA = {"default": {}, "levels": {"engine_quick": 0}, "nospec": {"speculate": 0}}


@pytest.fixture(scope="module")
def cases(kbgen_mod, tmp_path_factory):
    return ee.write_cases(kbgen_mod, tmp_path_factory.mktemp("engine_edges"))


@pytest.mark.parametrize("name,variant", VARIANTS)
def test_engine_edge(engine, oracle_mod, cases, name, variant):
    _, _, options, claims = ee.CASES[ee.NAMES.index(name)]
    cluster, path = cases[name]
    exp, exp_nodes, _ = reference(oracle_mod, path)
    exp_close = oracle_mod.ref_gang_close(path)
    with engine.Session(path) as s:
        for k, v in {**options, **EXTRA[variant]}.items():
            s.set_option(k, v)
        pod, node, kind = s.allocate()
        st = s.stats()
        ns = s.read_nodes(st["nodes"])
        close = s.gang_unschedulable()
    got = [(int(p), int(n), 4 if k == 1 else 8) for p, n, k in zip(pod, node, kind)]
    print(f"{name}[{variant}]: workers {st['engine_workers']} owners {st['engine_owners']} launches "
          f"{st['engine_launches']} engine pops {st['engine_pops']} of {st['batched_pops']}")
    if got != exp:
        bad = next(i for i in range(max(len(got), len(exp))) if i >= min(len(got), len(exp)) or got[i] != exp[i])
        assert False, f"log differs at entry {bad}: engine {got[bad:bad + 4]} restatement {exp[bad:bad + 4]}"
    assert st["nodes"] == len(cluster.nodes)
    assert np.array_equal(ns.astype(np.float64), exp_nodes[:ns.shape[0]])
    assert close == exp_close
    # the structure under test ran
    owners = claims["owners"]
    if isinstance(owners, tuple):  # as many owners as the limit admits, or sweep mode: the device's resident blocks
        assert st["engine_owners"] in owners
        assert st["engine_owners"] > 0 or st["engine_workers"] > 0
    else:
        assert st["engine_owners"] == owners
    if claims.get("workers") is not None:
        assert st["engine_workers"] == claims["workers"]
    if st["engine_owners"] > 0:
        assert st["engine_workers"] == 0
    if claims.get("all_engine"):
        assert st["engine_pops"] == st["batched_pops"] >= claims.get("pops", 1)
        assert st["engine_launches"] >= 1
    if claims.get("no_engine"):
        assert st["engine_pops"] == 0 and st["batched_pops"] > 0
    if claims.get("mixed"):
        assert st["engine_launches"] >= 2
        assert 0 < st["engine_pops"] < st["batched_pops"]
        # the runs the restart hysteresis gives (engineedges.engine_runs; an idle end only adds launches)
        assert st["engine_pops"] == sum(claims["runs"]) and st["engine_launches"] >= len(claims["runs"])
