"""kbhip_walk_victims / kbhip_debug_walk_victims without a device: the node loop
(vict_stage_walk / vict_link / walk_step of kbhip_eval.h, the functions the
kernel runs) on the host tables of an encode-only session against the
restatement's chain (tests/walkvictims.py), the hand-placed carried-state
cases (tests/walkedges.py), the prefix property of the capacity stop, and
argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest

import victimmodel
import walkedges
import walkvictims
from test_gpu_victim_walk import CASES, EXACT, TIERS, _gen
from test_head_victims_abi import FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
vp = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(vp)


def test_declared_and_exported(engine_lib):
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    assert re.search(r"\bint64_t\s+kbhip_walk_victims\s*\(", src)
    assert re.search(r"\bint64_t\s+kbhip_debug_walk_victims\s*\(", src)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(KBHIP_WALK_[A-Z_]+)\s+(\d+)", src)}
    assert defs == {"KBHIP_WALK_ASSIGNED": kbhip.WALK_ASSIGNED, "KBHIP_WALK_EXHAUSTED": kbhip.WALK_EXHAUSTED,
                    "KBHIP_WALK_HEAD_END": kbhip.WALK_HEAD_END, "KBHIP_WALK_CAPACITY": kbhip.WALK_CAPACITY}
    assert (walkvictims.ASSIGNED, walkvictims.EXHAUSTED, walkvictims.HEAD_END, walkvictims.CAPACITY) == (
        kbhip.WALK_ASSIGNED, kbhip.WALK_EXHAUSTED, kbhip.WALK_HEAD_END, kbhip.WALK_CAPACITY)
    assert (walkvictims.EVICT, walkvictims.PIPELINE) == (kbhip.OP_EVICT, kbhip.OP_PIPELINE)
    for name in ("kbhip_walk_victims", "kbhip_debug_walk_victims"):
        assert name in kbhip.EXPORTS and hasattr(engine_lib, name)


def _same(got, exp, where):
    ops, info = walkvictims.as_ops(got), got[3]
    assert ops == exp[0], where
    assert {k: info[k] for k in exp[1]} == exp[1], where


def _compare(kbhip, c, path, prefixes=False):
    """Every pending task and mode over all nodes in index order; prefixes: every cap_ops as well.
    Returns (walks compared, walks that acted on more than one node, capacity stops)."""
    m = victimmodel.VictimModel(c)
    enc = kbhip.EncodedSnapshot(path)
    nodes = list(range(m.n_nodes))
    walks = multi = capped = 0
    try:
        cls = enc.table("pod_class")
        tasks = [t for t in m.pending() if cls[t] >= 0]
        assert tasks
        for t in tasks:
            for mode in (1, 2, 3):
                full = walkvictims.chain(m, t, mode, nodes)
                _same(enc.walk_victims(t, mode, nodes), full, (t, mode))
                walks += 1
                multi += full[1]["acted"] > 1
                if not prefixes:
                    continue
                for cap_ops in range(1, len(full[0]) + 1):
                    exp = walkvictims.chain(m, t, mode, nodes, cap_ops=cap_ops)
                    got = enc.walk_victims(t, mode, nodes, cap_ops=cap_ops)
                    _same(got, exp, (t, mode, cap_ops))
                    # the uncapped answer cut at a step boundary, CAPACITY exactly when cut
                    ops = walkvictims.as_ops(got)
                    assert ops == full[0][:len(ops)]
                    assert (got[3]["stop"] == walkvictims.CAPACITY) == (len(ops) < len(full[0]))
                    capped += len(ops) < len(full[0])
    finally:
        enc.close()
    return walks, multi, capped


@pytest.mark.parametrize("case", CASES, ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_debug_walk_equals_the_chain(engine_lib, kbgen_mod, tmp_path, case):
    import kbhip
    c = _gen(kbgen_mod, case)
    walks, _, _ = _compare(kbhip, c, c.write(str(tmp_path / "w.kbs")), prefixes=True)
    assert walks


def test_the_snapshots_carry_state(engine_lib, kbgen_mod, tmp_path):
    """Over the 17 snapshots together some walk acts on more than one node (every non-empty walk is cut by
    cap_ops 1: a step needs its prefix and one slot more)."""
    import kbhip
    multi = 0
    for case in CASES:
        c = _gen(kbgen_mod, case)
        multi += _compare(kbhip, c, c.write(str(tmp_path / ("w%d_%d_%d_%d.kbs" % case))))[1]
    assert multi


@pytest.mark.parametrize("tier", [1, 2, 3])
@pytest.mark.parametrize("flags", range(len(FLAGS)))
def test_tier_layouts_and_disabled_plugins(engine_lib, kbgen_mod, tmp_path, tier, flags):
    import kbhip
    total = 0
    for seed in (3, 34, 39):
        c = _gen(kbgen_mod, (0, seed, tier, 0))
        c.flags = {p: f for p, f in FLAGS[flags].items() if any(p in t for t in TIERS[tier])}
        walks, _, _ = _compare(kbhip, c, c.write(str(tmp_path / ("f%d.kbs" % seed))))
        total += walks
    assert total


@pytest.mark.parametrize("name", sorted(walkedges.BUILDERS))
def test_edges(engine_lib, tmp_path, name):
    """The hand answers: carried differs from stateless, the restatement gives both, the library the first."""
    import kbhip
    c, task, mode, carried, stateless = walkedges.BUILDERS[name]()
    task, (carried, stateless) = walkedges.resolve(c, task, [carried, stateless])
    assert carried != stateless
    m = victimmodel.VictimModel(c)
    nodes = list(range(m.n_nodes))
    assert walkvictims.chain(m, task, mode, nodes)[0] == carried
    assert walkvictims.chain(m, task, mode, nodes, carried=False)[0] == stateless
    enc = kbhip.EncodedSnapshot(c.write(str(tmp_path / "e.kbs")))
    try:
        got = enc.walk_victims(task, mode, nodes)
        assert walkvictims.as_ops(got) == carried
        assert got[3]["stop"] == walkvictims.EXHAUSTED and got[3]["acted"] == len({n for _, _, n in carried})
        # an overlay of one job and one queue holds each of these walks; the prefix property at every cap_ops
        enc.set_option("walk_overlay_max", 1)
        assert walkvictims.as_ops(enc.walk_victims(task, mode, nodes)) == carried
        enc.set_option("walk_overlay_max", 0)
        for cap_ops in range(1, len(carried) + 2):
            exp = walkvictims.chain(m, task, mode, nodes, cap_ops=cap_ops)
            _same(enc.walk_victims(task, mode, nodes, cap_ops=cap_ops), exp, cap_ops)
            assert exp[0] == carried[:len(exp[0])]
    finally:
        enc.close()


def test_overlay_capacity(engine_lib, kbgen_mod, tmp_path):
    """"walk_overlay_max" = k: a walk that would go on from a node touching more than k jobs or queues stops
    before it with CAPACITY, as the chain with the same bound does; some walk of the snapshots is cut."""
    import kbhip
    cut = 0
    for case in CASES[:11]:
        c = _gen(kbgen_mod, case)
        m = victimmodel.VictimModel(c)
        enc = kbhip.EncodedSnapshot(c.write(str(tmp_path / ("o%d_%d_%d_%d.kbs" % case))))
        nodes = list(range(m.n_nodes))
        try:
            cls = enc.table("pod_class")
            for k in (1, 2):
                enc.set_option("walk_overlay_max", k)
                for t in [t for t in m.pending() if cls[t] >= 0]:
                    for mode in (1, 2):
                        exp = walkvictims.chain(m, t, mode, nodes, ov_max=k)
                        _same(enc.walk_victims(t, mode, nodes), exp, (case, k, t, mode))
                        full = walkvictims.chain(m, t, mode, nodes)[0]
                        assert exp[0] == full[:len(exp[0])]
                        cut += exp[1]["stop"] == walkvictims.CAPACITY
        finally:
            enc.close()
    assert cut


def test_exact_snapshots_need_one_ask_per_task(engine_lib, kbgen_mod, tmp_path):
    """What the device test of host_reclaim_walk relies on, checked with the restatement alone: on the four
    EXACT snapshots every popped task's walk ends ASSIGNED or EXHAUSTED (no walk is longer than the head)."""
    for case in EXACT:
        c = _gen(kbgen_mod, case)
        m = victimmodel.VictimModel(c)

        def ask(task, after):
            assert after is None
            nodes = [n for n in range(m.n_nodes) if m.candidates(task, 1, n)]
            assert len(nodes) <= 64
            ops, info = walkvictims.chain(m, task, 1, nodes)
            return ops, dict(info, last_score=0)

        log, asks, stops = walkvictims.host_reclaim_walk(m, ask, lambda ops: None)
        assert asks and set(asks) == {1} and set(stops) <= {walkvictims.ASSIGNED, walkvictims.EXHAUSTED}
        assert sum(k == 8 for _, _, k in log) >= 2


def test_argument_validation(engine_lib, kbgen_mod, tmp_path):
    import kbhip
    L = engine_lib
    o = [np.full(8, 77, np.uint8), np.full(8, 77, np.int32), np.full(8, 77, np.int32), np.full(8, 77, np.int64)]
    ptr = [_p(a) for a in o]
    wv, dw = L.kbhip_walk_victims, L.kbhip_debug_walk_victims
    assert wv(None, 0, 1, 1, 4, -1, 0, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
    assert b"null session" in L.kbhip_last_error()
    p = _gen(kbgen_mod, CASES[0]).write(str(tmp_path / "v.kbs"))
    enc = kbhip.EncodedSnapshot(p)
    try:
        t = int(np.nonzero(enc.table("pod_class") >= 0)[0][0])
        n_nodes = int(enc.table("dims")[0])
        assert wv(enc._h, t, 1, 1, 4, -1, 0, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
        assert b"encode-only" in L.kbhip_last_error()
        for cap, cap_ops, word in ((0, 8, b"cap is"), (65, 8, b"cap is"), (4, 0, b"cap_ops"), (4, -1, b"cap_ops")):
            assert wv(enc._h, t, 1, 1, cap, -1, 0, ptr[0], ptr[1], ptr[2], cap_ops, ptr[3]) == EINVAL
            assert word in L.kbhip_last_error()
        for k in range(3):  # a null required output (out_info is optional)
            q = list(ptr)
            q[k] = None
            assert wv(enc._h, t, 1, 1, 4, -1, 0, q[0], q[1], q[2], 8, q[3]) == EINVAL
            assert b"null out_op" in L.kbhip_last_error()
        assert wv(enc._h, t, 2, 1, 4, -1, 0, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
        for mode in (0, 4, -1):
            assert wv(enc._h, t, 1, mode, 4, -1, 0, ptr[0], ptr[1], ptr[2], 8, ptr[3]) == EINVAL
            assert b"KBHIP_VICTIMS" in L.kbhip_last_error()
        # kbhip_debug_walk_victims
        nodes = np.arange(n_nodes, dtype=np.int32)
        ok = (enc._h, t, 1, _p(nodes), n_nodes, 8, ptr[0], ptr[1], ptr[2], ptr[3])

        def bad(k, v):
            a = list(ok)
            a[k] = v
            return dw(*a)

        assert bad(0, None) == EINVAL
        running = int(np.nonzero(enc.table("pod_class") < 0)[0][0])
        assert bad(1, running) == EINVAL and bad(1, len(enc.table("pod_class"))) == EINVAL
        assert bad(2, 0) == EINVAL and bad(2, 4) == EINVAL
        assert bad(3, None) == EINVAL and bad(4, -1) == EINVAL
        assert bad(5, 0) == EINVAL
        assert bad(6, None) == EINVAL and bad(7, None) == EINVAL and bad(8, None) == EINVAL
        for wrong in (-1, n_nodes):
            assert dw(enc._h, t, 1, _p(np.array([wrong], np.int32)), 1, 8, *ptr) == EINVAL
        assert all((a == 77).all() for a in o)  # a refused call writes nothing
        with pytest.raises(kbhip.KbhipError):
            enc.set_option("walk_overlay_max", -1)
        with pytest.raises(kbhip.KbhipError):
            enc.set_option("walk_overlay_max", 257)
        assert dw(enc._h, t, 1, None, 0, 8, *ptr) == 0  # an empty list: nothing visited
        assert o[3][0] == walkvictims.EXHAUSTED and o[3][2] == 0
        assert dw(*ok[:9], None) >= 0  # out_info is optional
    finally:
        enc.close()
