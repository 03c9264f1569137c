"""kbhip_walk_begin / kbhip_walk_next / kbhip_walk_order / kbhip_walk_end
without a device: the declarations and the bindings, every argument refusal on
an encode-only session, and the cursor protocol's restatement
(tests/walkcursor.py) checked against the uncut chain and against the window
protocol's restatement (walkwindows.expected_calls) on every cluster of
tests/walkwindows.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import victimmodel
import walkcursor as wc
import walkvictims
import walkwindows as ww
from walkvictims import ASSIGNED, CAPACITY, EXHAUSTED, HEAD_END, EVICT, PIPELINE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
vp = ctypes.c_void_p
CALLS = ("kbhip_walk_begin", "kbhip_walk_next", "kbhip_walk_order", "kbhip_walk_end")


def _p(a):
    return a.ctypes.data_as(vp)


def test_declared_exported_and_bound(engine_lib):
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    for name in CALLS[:3]:
        assert re.search(r"\bint64_t\s+%s\s*\(" % name, src), name
    assert re.search(r"\bint\s+kbhip_walk_end\s*\(", src)
    go = open(os.path.join(ROOT, "go", "kbhip", "kbhip.go")).read()
    for name, method, go_name in zip(CALLS, ("walk_begin", "walk_next", "walk_order", "walk_end"),
                                     ("WalkBegin", "WalkNext", "WalkOrder", "WalkEnd")):
        assert name in kbhip.EXPORTS and hasattr(engine_lib, name), name
        assert callable(getattr(kbhip.Session, method, None)), method
        assert "C.%s(" % name in go and "func (e *Engine) %s(" % go_name in go, name
    info = kbhip._walk_next_info(np.array([3, 130, 71, 2, 75, 10, 2, 1 | 2 | (9 << 8), 70, 66], np.int64))
    assert info == dict(stop=3, total=130, decided=71, acted=2, next=75, first=10, launches=2, rebuilt=1,
                        state_rebuilt=1, patched=9, last_node=70, scanned=66)


def test_argument_validation(engine_lib, tmp_path):
    """Every refusal, on an encode-only session (no device needed): KBHIP_EINVAL, and no output written."""
    import kbhip
    L = engine_lib
    o = [np.full(8, 77, np.uint8), np.full(8, 77, np.int32), np.full(8, 77, np.int32), np.full(10, 77, np.int64)]
    ptr = [_p(a) for a in o]
    begin, nxt, order, end = (getattr(L, n) for n in CALLS)
    assert begin(None, 0, 1, 1, ptr[3]) == EINVAL and b"null session" in L.kbhip_last_error()
    assert nxt(None, 0, 4, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL and b"null session" in L.kbhip_last_error()
    assert order(None, 0, ptr[1], ptr[2], 8) == EINVAL and b"null session" in L.kbhip_last_error()
    assert end(None) == EINVAL and b"null session" in L.kbhip_last_error()
    enc = kbhip.EncodedSnapshot(ww.build(ww.blocked(4)).write(str(tmp_path / "v.kbs")))
    try:
        t = int(np.nonzero(enc.table("pod_class") >= 0)[0][0])
        # kbhip_walk_begin
        assert begin(enc._h, t, 1, 1, ptr[3]) == EINVAL and b"encode-only" in L.kbhip_last_error()
        for by_score in (2, -1):
            assert begin(enc._h, t, by_score, 1, ptr[3]) == EINVAL
            assert b"kbhip_walk_begin" in L.kbhip_last_error() and b"by_score" in L.kbhip_last_error()
        for mode in (0, 4, -1):
            assert begin(enc._h, t, 1, mode, ptr[3]) == EINVAL
            assert b"kbhip_walk_begin" in L.kbhip_last_error() and b"KBHIP_VICTIMS" in L.kbhip_last_error()
        assert begin(enc._h, t, 1, 1, None) == EINVAL
        # kbhip_walk_next
        assert nxt(enc._h, 0, 4, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL and b"encode-only" in L.kbhip_last_error()
        for cap, cap_ops, word in ((0, 8, b"cap is"), (65, 8, b"cap is"), (-1, 8, b"cap is"), (4, 0, b"cap_ops"),
                                   (4, -1, b"cap_ops")):
            assert nxt(enc._h, 0, cap, ptr[0], ptr[1], ptr[2], cap_ops, ptr[3]) == EINVAL
            assert b"kbhip_walk_next" in L.kbhip_last_error() and word in L.kbhip_last_error()
        for k in range(3):  # a null required output (out_info is optional)
            q = list(ptr)
            q[k] = None
            assert nxt(enc._h, 0, 4, q[0], q[1], q[2], 8, q[3]) == EINVAL
            assert b"null out_op" in L.kbhip_last_error()
        for pos in (-1, -(1 << 40)):
            assert nxt(enc._h, pos, 4, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
            assert b"pos is" in L.kbhip_last_error()
        assert nxt(enc._h, 0, 4, ptr[0], ptr[1], ptr[2], 8, None) == EINVAL
        # kbhip_walk_order
        assert order(enc._h, 0, ptr[1], ptr[2], 8) == EINVAL and b"encode-only" in L.kbhip_last_error()
        for first, cap, node in ((-1, 8, ptr[1]), (0, -1, ptr[1]), (0, 8, None)):
            assert order(enc._h, first, node, ptr[2], cap) == EINVAL
            assert b"kbhip_walk_order" in L.kbhip_last_error()
        # kbhip_walk_end: no cursor was ever open
        assert end(enc._h) == 0
        assert all((a == 77).all() for a in o)  # a refused call writes nothing
    finally:
        enc.close()


# ---- the restatement ------------------------------------------------------------------------------
def _model(name, mode):
    c = ww.CLUSTERS[name][0](mode)
    m = victimmodel.VictimModel(c)
    return c, m, ww.task_of(m)


def _cat(calls):
    return [op for ops, _ in calls for op in ops]


@pytest.mark.parametrize("name", sorted(ww.CLUSTERS))
def test_cursor_protocol_equals_the_chain_and_the_windows(name):
    """Every cluster, mode and order at cap 1, 7 and 64: the concatenated ops are chain's over the uncut walk
    and the window protocol's; the positions advance and end at an ASSIGNED or EXHAUSTED call."""
    for mode in ww.CLUSTERS[name][1]:
        c, m, task = _model(name, mode)
        for by_score in (False, True):
            walk = ww.walk_of(name, by_score)
            ops, info = walkvictims.chain(m, task, mode, walk)
            windows = _cat(ww.expected_calls(m, task, mode, walk))
            for cap in (1, 7, 64):
                calls = wc.expected_cursor_calls(m, task, mode, walk, None, cap)
                where = (name, mode, by_score, cap)
                assert _cat(calls) == ops == windows, where
                assert calls[-1][1]["stop"] == info["stop"], where
                assert all(i["stop"] in (HEAD_END, CAPACITY) for _, i in calls[:-1]), where
                nxt = [i["next"] for _, i in calls]
                assert nxt == sorted(nxt) and all(i["total"] == len(walk) for _, i in calls), where
                assert sum(i["acted"] for _, i in calls) == info["acted"], where
                # every entry is decided once, but a serial entry behind a call's last acted-on node that the
                # next call's scan decides again
                assert sum(i["decided"] for _, i in calls) >= info["visited"], where
                for _, i in calls:
                    assert i["first"] == -1 or i["first"] < i["next"] or i["stop"] == CAPACITY, where


@pytest.mark.parametrize("name", sorted(ww.LENGTHS))
def test_walks_that_act_on_nothing_take_one_call(name):
    for mode in ww.CLUSTERS[name][1]:
        c, m, task = _model(name, mode)
        walk = ww.walk_of(name, False)
        for cap in (1, 7, 64):
            calls = wc.expected_cursor_calls(m, task, mode, walk, None, cap)
            assert calls == [([], dict(stop=EXHAUSTED, total=len(walk), decided=len(walk), acted=0, next=len(walk),
                                       first=-1, last_node=-1))]
        assert len(ww.expected_calls(m, task, mode, walk)) == len(ww.LENGTHS[name])


@pytest.mark.parametrize("name,acted,stateless", [("gang_carried", ww.GANG_ACTED, ww.GANG_STATELESS),
                                                  ("drf_carried", ww.DRF_ACTED, ww.DRF_STATELESS),
                                                  ("proportion_carried", ww.PROP_ACTED, ww.PROP_STATELESS)])
def test_carried_state(name, acted, stateless):
    """The walk acts at the *_ACTED positions and never at the further *_STATELESS ones: with cap 1 the
    evictions reach the next call through the model (three calls, each starting at its `first`), with cap 64
    the eviction at position 10 is carried to 70 by the overlay inside one call."""
    extra = sorted(set(stateless) - set(acted))
    assert extra
    for mode in ww.CLUSTERS[name][1]:
        c, m, task = _model(name, mode)
        walk = ww.walk_of(name, False)
        one = wc.expected_cursor_calls(m, task, mode, walk, None, 1)
        assert [i["first"] for _, i in one] == acted and [i["acted"] for _, i in one] == [1, 1, 1]
        assert [i["stop"] for _, i in one] == [HEAD_END, HEAD_END, ASSIGNED]
        assert [i["next"] for _, i in one] == [a + 1 for a in acted]
        assert [i["decided"] for _, i in one] == [acted[0] + 1, acted[1] - acted[0], acted[2] - acted[1]]
        whole = wc.expected_cursor_calls(m, task, mode, walk, None, 64)
        assert [i["first"] for _, i in whole] == [acted[0], acted[2]]
        assert [i["acted"] for _, i in whole] == [2, 1] and [i["stop"] for _, i in whole] == [HEAD_END, ASSIGNED]
        assert whole[0][1]["next"] == acted[0] + 64 and whole[0][1]["last_node"] == acted[1]
        for calls in (one, whole):
            on = [n for o, _, n in _cat(calls) if o == EVICT]
            assert on == acted and not set(on) & set(extra)
            assert _cat(calls)[-1] == (PIPELINE, task, acted[-1])
        capped = wc.expected_cursor_calls(m, task, mode, walk, None, 64, cap_ops=2, ov_max=1)
        assert _cat(capped) == _cat(whole) and CAPACITY in [i["stop"] for _, i in capped]
        k = [i["stop"] for _, i in capped].index(CAPACITY)
        # the node refused with CAPACITY is the next call's `first` and its first act
        assert capped[k + 1][1]["first"] == capped[k][1]["next"] and capped[k + 1][0][0][2] == walk[capped[k][1]["next"]]


def test_first_positions_and_long_node():
    for name, first in (("valid_at129", 129), ("covers_at129", 129)):
        for mode in ww.CLUSTERS[name][1]:
            c, m, task = _model(name, mode)
            calls = wc.expected_cursor_calls(m, task, mode, ww.walk_of(name, False), None, 64)
            assert len(calls) == 1 and calls[0][1]["first"] == first and calls[0][1]["decided"] == 130
            assert calls[0][1]["stop"] == (ASSIGNED if name.startswith("covers") else EXHAUSTED)
    for mode in ww.CLUSTERS["long_node"][1]:
        c, m, task = _model("long_node", mode)
        walk = ww.walk_of("long_node", False)
        calls = wc.expected_cursor_calls(m, task, mode, walk, None, 1)
        assert [i["first"] for _, i in calls] == [10, 65, 80] and calls[1][1]["decided"] == 65 - 11 + 1
        assert sum(n == 65 for _, _, n in calls[1][0]) == ww.LONG


def test_big_walk():
    """The device test's long walk: four calls whose `first` are the VALID node, the VALID long node, the
    refused long node (reported, passed over, nothing written) and the covering node more than two scan
    grids behind the last call's position."""
    c, spill = wc.big_walk(1)
    m = victimmodel.VictimModel(c)
    task = ww.task_of(m)
    for n in spill:
        assert len(m.candidates(task, 1, n)) == ww.LONG > 256
    assert m.decide(task, 1, wc.BIG_LONG)[2] & 1 and not m.decide(task, 1, wc.BIG_LONG_REFUSED)[2] & 1
    calls = wc.expected_cursor_calls(m, task, 1, list(range(wc.BIG_N)), None, 64, spill=spill)
    assert [i["first"] for _, i in calls] == wc.BIG_FIRSTS
    assert [0] + [i["next"] for _, i in calls[:-1]] == wc.BIG_STARTS
    assert wc.BIG_FIRSTS[-1] - wc.BIG_STARTS[-1] > 2 * wc.BIG_GRID  # a scan block decides up to three entries
    assert [i["stop"] for _, i in calls] == [HEAD_END] * 3 + [ASSIGNED]
    assert calls[2][0] == [] and calls[2][1]["acted"] == 0 and calls[2][1]["next"] == wc.BIG_LONG_REFUSED + 64
    # the log: one eviction on the VALID node, the long node's 257, the covering node's and the pipeline there
    assert [n for _, _, n in _cat(calls)] == [wc.BIG_VALID] + [wc.BIG_LONG] * ww.LONG + [wc.BIG_COVERS] * 2
    assert _cat(calls)[-1] == (PIPELINE, task, wc.BIG_COVERS)
