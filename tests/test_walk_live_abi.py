"""kbhip_walk_begin_live without a device: the declaration and the bindings,
every refusal on an encode-only session, and the live protocol's restatement
(tests/walklive.py) against the oracle's reclaim records on clusters where an
eviction of the walk changes the pod-affinity predicate of a later node — on
each of which the restatement over the order fixed at the start
(tests/walkcursor.py) gives another log."""
import ctypes
import os
import re

import numpy as np
import pytest

import victimmodel
import walkcursor as wc
import walklive as wl
import walkwindows as ww
from walkvictims import ASSIGNED, EVICT, HEAD_END, PIPELINE, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
vp = ctypes.c_void_p
MODES = (1,)  # reclaim's victims are the other queues' tasks: the oracle's reclaim log is KBHIP_VICTIMS_OTHER_QUEUES'


def _p(a):
    return a.ctypes.data_as(vp)


def test_declared_exported_and_bound(engine_lib):
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    assert re.search(r"\bint64_t\s+kbhip_walk_begin_live\s*\(\s*kb_session\*\s*s,\s*int32_t\s+task_id,\s*int32_t\s+victims", src)
    assert "kbhip_walk_begin_live" in kbhip.EXPORTS and hasattr(engine_lib, "kbhip_walk_begin_live")
    assert callable(getattr(kbhip.Session, "walk_begin_live", None))
    go = open(os.path.join(ROOT, "go", "kbhip", "kbhip.go")).read()
    assert "C.kbhip_walk_begin_live(" in go and "func (e *Engine) WalkBeginLive(" in go


def test_argument_validation(engine_lib, tmp_path):
    """Every refusal, on an encode-only session (no device needed): KBHIP_EINVAL, and no output written."""
    import kbhip
    L = engine_lib
    info = np.full(4, 77, np.int64)
    begin = L.kbhip_walk_begin_live
    assert begin(None, 0, 1, _p(info)) == EINVAL and b"null session" in L.kbhip_last_error()
    enc = kbhip.EncodedSnapshot(wl.CLUSTERS["leave"]().write(str(tmp_path / "v.kbs")))
    try:
        t = int(np.nonzero(enc.table("pod_class") >= 0)[0][0])
        assert begin(enc._h, t, 1, _p(info)) == EINVAL and b"encode-only" in L.kbhip_last_error()
        for mode in (0, 4, -1):
            assert begin(enc._h, t, mode, _p(info)) == EINVAL
            assert b"kbhip_walk_begin_live" in L.kbhip_last_error() and b"KBHIP_VICTIMS" in L.kbhip_last_error()
        assert begin(enc._h, t, 1, None) == EINVAL
        assert L.kbhip_walk_end(enc._h) == 0
        assert (info == 77).all()
    finally:
        enc.close()


# ---- the restatement ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_log(oracle_mod, tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_live_abi")
    return lambda name, mode: [tuple(r) for r in oracle_mod.ref_allocate(
        wl.CLUSTERS[name](mode).write(str(d / ("%s_%d.kbs" % (name, mode)))), actions="reclaim").as_list()]


@pytest.mark.parametrize("name", ["leave", "enter"])
def test_live_restatement_equals_the_oracle_and_the_fixed_order_does_not(name, oracle_log):
    for mode in MODES:
        ref = oracle_log(name, mode)
        assert [n for _, n, _ in ref] == wl.EXPECTED_NODES[name] and ref[-1][2] == 8
        assert wl.restated_reclaim(wl.CLUSTERS[name](mode), mode, live=True) == ref
        # the condition: a cluster on which the fixed order gave the oracle's log would prove nothing
        assert wl.restated_reclaim(wl.CLUSTERS[name](mode), mode, live=False) != ref


def test_leave_and_enter_call_by_call():
    """leave: node 1 is in both orders and the live walk passes it over once zone a has lost its target;
    enter: nodes 1 .. 3 are in the live order only and pass once no target is left anywhere."""
    for name, orders, second in (("leave", ([0, 1, 2, 3], [0, 1, 2, 3]), dict(first=2, decided=2, next=3)),
                                 ("enter", ([0, 1, 2, 3], [0]), dict(first=1, decided=1, next=2))):
        c = wl.CLUSTERS[name](1)
        m, aff = victimmodel.VictimModel(c), wl.AffPred(c)
        task = ww.task_of(m)
        live, fixed = wl.live_order(m, task, 1), wl.fixed_order(m, aff, task, 1)
        assert (live, fixed) == orders and set(fixed) <= set(live)
        for cap in (1, 2, 64):
            calls = wl.expected_live_calls(m, aff, task, 1, live, cap)
            assert [i["stop"] for _, i in calls] == [HEAD_END, ASSIGNED], (name, cap)
            assert calls[0][0] == [(EVICT, 0, 0)] and calls[0][1]["next"] == 1
            assert {k: calls[1][1][k] for k in second} == second, (name, cap)
            assert all(i["acted"] == 1 and i["total"] == 4 for _, i in calls)
            assert calls[1][0][-1][0] == PIPELINE and calls[1][0][-1][1] == task


def test_control_live_and_fixed_agree_call_by_call(oracle_log):
    """No affinity term: the two orders are one, and the one-node-per-call cut is all that separates the live
    restatement from the fixed cursor's — which kbhip_walk_begin_live does not apply to such a class: there
    the call is kbhip_walk_begin, so the fixed restatement is what the device test holds it to.  With cap 1
    the fixed cursor also returns behind each acting node, and the two agree call by call."""
    c = wl.CLUSTERS["control"](1)
    m, aff = victimmodel.VictimModel(c), wl.AffPred(c)
    task = ww.task_of(m)
    live = wl.live_order(m, task, 1)
    assert live == wl.fixed_order(m, aff, task, 1) == [0, 1, 2, 3]
    a = wl.expected_live_calls(m, aff, task, 1, live, 1)
    b = wc.expected_cursor_calls(m, task, 1, live, None, 1)
    assert a == b and len(a) == 2
    for cap in (1, 2, 64):  # the call as the library makes it for this class
        order, calls, is_live = wl.expected_calls(m, aff, task, 1, cap)
        assert not is_live and order == live and calls == wc.expected_cursor_calls(m, task, 1, live, None, cap)
    log = [r for ops, _ in a for r in records(ops)]
    assert log == oracle_log("control", 1) == wl.restated_reclaim(c, 1, live=False)


def test_spill_and_big_restatements():
    """The device tests' other two clusters: a long node that fails the predicate counts as `first` and is
    passed over by the serial part; a `first` more than one scan grid behind the position."""
    c = wl.CLUSTERS["spill"](1)
    m, aff = victimmodel.VictimModel(c), wl.AffPred(c)
    task = ww.task_of(m)
    assert len(m.candidates(task, 1, 0)) == ww.LONG > 256 and not aff.holds(m, task, 0)
    calls = wl.expected_live_calls(m, aff, task, 1, wl.live_order(m, task, 1), spill={0})
    assert [(i["first"], i["decided"], i["next"], i["stop"], i["last_node"]) for _, i in calls] == [
        (0, 2, 2, HEAD_END, 1), (2, 1, 3, ASSIGNED, 2)]
    c = wl.big(1)
    m, aff = victimmodel.VictimModel(c), wl.AffPred(c)
    task = ww.task_of(m)
    assert m.decide(task, 1, 7)[2] & 1 and not aff.holds(m, task, 7)  # victims-VALID, and the predicate fails
    calls = wl.expected_live_calls(m, aff, task, 1, list(range(wl.BIG_N)))
    assert len(calls) == 1 and calls[0][1] == dict(stop=ASSIGNED, total=wl.BIG_N, decided=wl.BIG_FIRST + 1, acted=1,
                                                   next=wl.BIG_FIRST + 1, first=wl.BIG_FIRST, last_node=wl.BIG_FIRST)
    assert wl.BIG_FIRST > wl.BIG_GRID
