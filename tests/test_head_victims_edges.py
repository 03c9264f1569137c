"""The victim decision at its comparison edges, on the CPU: kbhip_debug_victims
(the functions the kernel runs) on the hand-placed clusters of
tests/victimedges.py, against the expectations worked out by hand there and
against tests/victimmodel.py, and the staging boundary of 256 tasks."""
import numpy as np
import pytest

import victimedges
import victimmodel


@pytest.mark.parametrize("name", sorted(victimedges.BUILDERS))
def test_edges_on_the_host_tables(engine_lib, tmp_path, name):
    import kbhip
    c, exp = victimedges.BUILDERS[name]()
    exp = victimedges.resolve(c, exp)
    m = victimmodel.VictimModel(c)
    if name == "proportion_edges":  # the state the edges are placed against
        q1 = m.h.queues["q1"]
        assert q1["deserved"] == [99000.0, float(59 * victimedges.GI), 0.0]
        assert q1["allocated"] == [100000.0, float(59 * victimedges.GI + 20 * victimedges.MI), 0.0]
    enc = kbhip.EncodedSnapshot(c.write(str(tmp_path / "e.kbs")))
    try:
        for (task, node, mode), e in sorted(exp.items()):
            model = m.decide(task, mode, node)
            if e is not None:
                assert model == e, (task, node, mode)  # the restatement agrees with the hand calculation
            count, evict, flags, row = enc.victims(task, mode, node)
            assert (row.tolist(), evict, flags) == model and count == len(model[0]), (task, node, mode)
        # every other (task, node, mode) of the cluster against the restatement
        for task in m.pending():
            for mode in (1, 2, 3):
                for node in range(m.n_nodes):
                    v, e, f = m.decide(task, mode, node)
                    count, evict, flags, row = enc.victims(task, mode, node)
                    assert (count, row.tolist(), evict, flags) == (len(v), v, e, f), (task, node, mode)
    finally:
        enc.close()


def test_share_delta_tie_is_decided_by_the_doubles(tmp_path):
    """The d = 2 case of drf_share_delta sits at 1e-6 up to rounding: whichever side the two quotients fall
    on, one unit either way is decided by the integers."""
    c, _ = victimedges.drf_share_delta()
    m = victimmodel.VictimModel(c)
    task = m.pending()[0]
    got = [len(m.decide(task, 2, n)[0]) for n in range(1, 7)]
    assert got[:3] == [1, 1, 1] and got[4:] == [0, 0] and got[3] in (0, 1)
    ls, rs = 100000 / 2000000, (100000 - 2) / 2000000
    assert got[3] == int(abs(ls - rs) <= 0.000001)


@pytest.mark.parametrize("size", [255, 256, 257])
def test_staging_boundary_on_the_host_tables(engine_lib, kbgen_mod, tmp_path, size):
    import kbhip
    from test_gpu_head_victims import _packed
    c = _packed(kbgen_mod, None, sizes=(size,))
    m = victimmodel.VictimModel(c)
    enc = kbhip.EncodedSnapshot(c.write(str(tmp_path / "s.kbs")))
    try:
        seen = 0
        for task in m.pending():
            for mode in (1, 2, 3):
                v, e, f = m.decide(task, mode, 0)
                count, evict, flags, row = enc.victims(task, mode, 0, stride=300)
                assert (count, row.tolist(), evict, flags) == (len(v), v, e, f)
                seen += bool(v)
        assert seen
    finally:
        enc.close()
