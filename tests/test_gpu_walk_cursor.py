"""kbhip_walk_begin / kbhip_walk_next / kbhip_walk_order / kbhip_walk_end on the
device: a task's eviction walk over an order ranked once and kept.

The yardsticks: kbhip_rank_victim_nodes' full-sort walk for the kept order, the
restatement of the protocol (tests/walkcursor.py over walkvictims.chain and
victimmodel) call by call, the oracle's reclaim records for the host loop, and
twin sessions for what the calls must leave alone."""
import functools

import numpy as np
import pytest

import victimmodel
import walkcursor as wc
import walkvictims
import walkwindows as ww
from test_gpu_victim_walk import CASES, EXACT, _gen
from walkvictims import ASSIGNED, CAPACITY, EXHAUSTED, HEAD_END

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = "kbhip error -1", "kbhip error -3"


def _send(engine, s, ops):
    assert (engine.OP_EVICT, engine.OP_PIPELINE) == (walkvictims.EVICT, walkvictims.PIPELINE)
    assert s.apply_ops([o for o, _, _ in ops], [p for _, p, _ in ops], [n for _, _, n in ops]) <= 2


def _full_walk(s, task, by_score, mode):
    """The whole pruned walk of the session as it stands, from the full-sort path: (nodes, scores, launches)."""
    total, nodes, scores, _, info = s.rank_victim_nodes(task, by_score, mode, 0, 1 << 16)
    assert info["head"] == 0 and len(nodes) == total
    return [int(n) for n in nodes], [int(x) for x in scores], info["launches"]


def _order(s):
    total, nodes, scores = s.walk_order()
    assert total == len(nodes) == len(scores)
    return [int(n) for n in nodes], [int(x) for x in scores]


def _check_scan(info, pos):
    """out_info[9] within its bounds, and the launch count of a call with nothing pending."""
    room = info["total"] - pos
    if info["first"] >= 0:
        assert info["first"] - pos + 1 <= info["scanned"] <= room, info
    else:
        assert info["scanned"] == room, info
    assert info["launches"] == 2 + bool(info["patched"]), info


def _loop(engine, s, cap=64, cap_ops=4096, after_apply=None):
    def ask(pos):
        got = s.walk_next(pos, cap, cap_ops)
        assert len(got[0]) <= cap_ops
        _check_scan(got[3], pos)
        return walkvictims.as_ops(got), got[3]

    def apply(ops):
        _send(engine, s, ops)
        if after_apply:
            after_apply()

    return wc.protocol(ask, apply)


def _same_calls(got, exp, where):
    assert len(got) == len(exp), where
    for k, ((g_ops, g), (e_ops, e)) in enumerate(zip(got, exp)):
        assert g_ops == e_ops, (where, k)
        assert {x: g[x] for x in wc.INFO_KEYS} == {x: e[x] for x in wc.INFO_KEYS}, (where, k)


def _run(engine, path, m, task, mode, by_score, cap=64, cap_ops=None, ov_max=0, interleave=False, expected=None):
    """One protocol loop on a fresh session against expected_cursor_calls.  The kept order equals the full-sort
    walk at the start and after every kbhip_apply_ops (interleave: a full-sort ranking and a window call of
    the old protocol run between the cursor's calls, on the scratch the cursor must not live in).
    -> (calls, walk)"""
    with engine.Session(path) as s:
        if ov_max:
            s.set_option("walk_overlay_max", ov_max)
        nodes, scores, rank_launches = _full_walk(s, task, by_score, mode)
        total, info = s.walk_begin(task, by_score, mode)
        assert total == len(nodes) and info["affinity_targets"] == 0 and not info["rebuilt"]
        assert info["launches"] == rank_launches and info["bytes"] >= 8 * total
        kept = (nodes, scores if by_score else [0] * total)
        assert _order(s) == kept
        assert s.walk_order(3, 2)[1].tolist() == nodes[3:5] and s.walk_order(total, 4)[1].size == 0

        def still_kept():
            if interleave and s.table("pod_status")[task] == 1:  # (the queries take a Pending task)
                _full_walk(s, task, not by_score, mode)
                s.walk_victims_from(task, by_score, mode, 64, (nodes[0], scores[0]))
                s.head_victims(task, not by_score, mode, 64, 4)
            assert _order(s) == kept

        still_kept()
        exp = (expected(nodes) if expected else
               wc.expected_cursor_calls(m, task, mode, nodes, None, cap, cap_ops=cap_ops, ov_max=ov_max))
        got = _loop(engine, s, cap, cap_ops or 4096, still_kept)
        _same_calls(got, exp, (mode, by_score, cap, cap_ops, ov_max))
        if got[-1][1]["stop"] == ASSIGNED:  # its own PIPELINE was applied: the task is no longer Pending
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.walk_next(got[-1][1]["next"])
            assert _order(s) == kept and s.walk_end() is True
        else:
            assert s.walk_end() is True
        assert s.walk_end() is False
        return got, nodes


@pytest.fixture(scope="module")
def clusters(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_cursor")

    @functools.lru_cache(maxsize=None)
    def get(name, mode):
        c = ww.CLUSTERS[name][0](mode)
        m = victimmodel.VictimModel(c)
        return c.write(str(d / ("%s_%d.kbs" % (name, mode)))), m, ww.task_of(m)

    return get


# ---- 1. the kept order and the protocol, call by call ------------------------------------------------
@pytest.mark.parametrize("name", sorted(ww.CLUSTERS))
def test_protocol(engine, clusters, name):
    for mode in ww.CLUSTERS[name][1]:
        path, m, task = clusters(name, mode)
        for by_score in (False, True):
            for cap in (1, 7, 64):
                got, nodes = _run(engine, path, m, task, mode, by_score, cap, interleave=cap == 7)
                assert nodes == ww.walk_of(name, by_score), (name, mode, by_score)
                assert got[-1][1]["stop"] in (ASSIGNED, EXHAUSTED)
                if name in ww.LENGTHS:  # one call, EXHAUSTED, N decided, no ops
                    assert len(got) == 1 and got[0][0] == []
                    assert [got[0][1][k] for k in ("stop", "decided", "first", "next")] == [EXHAUSTED, len(nodes), -1,
                                                                                            len(nodes)]
    if name == "negative":
        with engine.Session(clusters(name, 1)[0]) as s:
            s.walk_begin(clusters(name, 1)[2], True, 1)
            assert max(_order(s)[1]) < 0
    if name == "ties":
        with engine.Session(clusters(name, 1)[0]) as s:
            s.walk_begin(clusters(name, 1)[2], True, 1)
            sc = _order(s)[1]
            assert len(set(sc[60:71])) == 1 and sc[59] > sc[60] and sc[70] > sc[71]


@pytest.mark.parametrize("name", ["gang_carried", "drf_carried", "proportion_carried", "long_node"])
def test_capacity(engine, clusters, name):
    """cap_ops of one step and walk_overlay_max 1: the same log, and a node refused with CAPACITY is met again."""
    mode = ww.CLUSTERS[name][1][-1]
    path, m, task = clusters(name, mode)
    for by_score in (False, True):
        full, nodes = _run(engine, path, m, task, mode, by_score)
        log = [op for ops, _ in full for op in ops]
        assert full[-1][1]["stop"] == ASSIGNED and sum(i["acted"] for _, i in full) == 3
        steps = [sum(1 for o in log if o[2] == n and o[0] == walkvictims.EVICT) for n in dict.fromkeys(o[2] for o in log)]
        for cap in (1, 7, 64):
            capped, _ = _run(engine, path, m, task, mode, by_score, cap, cap_ops=max(steps) + 1, ov_max=1)
            assert [op for ops, _ in capped for op in ops] == log
            stops = [i["stop"] for _, i in capped]
            if cap == 64:
                assert CAPACITY in stops
            for k, st in enumerate(stops[:-1]):
                nxt = capped[k][1]["next"]
                if st == CAPACITY and (nxt == 0 or capped[k][1]["last_node"] != nodes[nxt - 1]):
                    # refused before it acted: the entry at the next position, the next call's first act
                    assert capped[k + 1][1]["first"] == capped[k][1]["next"]
                    assert capped[k + 1][0][0][2] == nodes[capped[k][1]["next"]]


def test_first_far_down(engine, clusters):
    """valid_at129 / covers_at129: `first` = 129 from position 0 in one call.  long_node: the 257-task node at
    position 65 is `first` from position 11 and decided by the serial loop, which owns the spill row."""
    for name in ("valid_at129", "covers_at129"):
        for mode in ww.CLUSTERS[name][1]:
            path, m, task = clusters(name, mode)
            with engine.Session(path) as s:
                assert s.walk_begin(task, False, mode)[0] == 130
                got = s.walk_next(0)
                _check_scan(got[3], 0)
                assert (got[3]["first"], got[3]["decided"], got[3]["acted"], got[3]["last_node"]) == (129, 130, 1, 129)
                assert got[3]["stop"] == (ASSIGNED if name.startswith("covers") else EXHAUSTED)
                assert got[3]["next"] == 130 and got[3]["scanned"] == 130
    for mode in ww.CLUSTERS["long_node"][1]:
        path, m, task = clusters("long_node", mode)
        with engine.Session(path) as s:
            s.walk_begin(task, False, mode)
            a = s.walk_next(0, 1)
            assert (a[3]["first"], a[3]["next"], a[3]["stop"]) == (10, 11, HEAD_END)
            _send(engine, s, walkvictims.as_ops(a))
            b = s.walk_next(11, 1)
            _check_scan(b[3], 11)
            assert (b[3]["first"], b[3]["next"], b[3]["acted"], b[3]["last_node"]) == (65, 66, 1, 65)
            assert len(b[0]) == ww.LONG and set(b[2].tolist()) == {65}
            exp = wc.expected_cursor_calls(m, task, mode, list(range(90)), None, 1)
            assert walkvictims.as_ops(b) == exp[1][0]


def test_walk_longer_than_two_scan_grids(engine, tmp_path):
    """4500 entries: a scan block takes entries pos + b, pos + b + 2048, ..  In the first three calls the
    blocks in front of `first` end on their second entry, after they have decided one; in the last `first`
    (4400) lies more than two grids behind the position (264), so a block decides two or three entries,
    stages again behind its barrier each time and adds them to the counter in one atomic.  `first` is also a
    VALID long node (100) and a long node that is not VALID (200: reported by the scan, passed over by the
    serial loop).  Call by call against the restatement, which is computed once for both orders (no nodeorder
    plugin: the by-score walk is the index walk); _loop checks first - pos + 1 <= out_info[9] <= T - pos on
    every call."""
    c, spill = wc.big_walk(1)
    m = victimmodel.VictimModel(c)
    task = ww.task_of(m)
    path = c.write(str(tmp_path / "big.kbs"))

    @functools.lru_cache(maxsize=None)
    def exp_of(nodes):
        return wc.expected_cursor_calls(m, task, 1, list(nodes), None, 64, spill=spill)

    for by_score in (False, True):
        got, nodes = _run(engine, path, m, task, 1, by_score, expected=lambda n: exp_of(tuple(n)))
        assert nodes == list(range(wc.BIG_N))
        assert [i["first"] for _, i in got] == wc.BIG_FIRSTS and got[-1][1]["stop"] == ASSIGNED
        assert got[2][0] == [] and (got[2][1]["acted"], got[2][1]["next"]) == (0, wc.BIG_LONG_REFUSED + 64)
        assert sum(n == wc.BIG_LONG for _, _, n in got[1][0]) == ww.LONG
        # the call whose `first` is behind two grids: every entry up to it was decided, by blocks on their
        # second and third entry
        starts = [0] + [i["next"] for _, i in got[:-1]]
        assert starts == wc.BIG_STARTS
        gap = got[3][1]["first"] - starts[3]
        assert gap > 2 * wc.BIG_GRID and gap + 1 <= got[3][1]["scanned"] <= wc.BIG_N - starts[3], got[3][1]


# ---- 2. end to end ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snaps(oracle_mod, kbgen_mod, tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_cursor_snaps")

    @functools.lru_cache(maxsize=None)
    def get(case):
        c = _gen(kbgen_mod, case)
        p = c.write(str(d / ("c%d_%d_%d_%d.kbs" % case)))
        return p, oracle_mod.ref_allocate(p, actions="reclaim").as_list(), c

    return get


def _host_loop(engine, p, c):
    m = victimmodel.VictimModel(c)
    with engine.Session(p) as s:
        def ask(pos):
            got = s.walk_next(pos)
            return walkvictims.as_ops(got), got[3]

        flags = []
        out = wc.host_reclaim_walk_cursor(m, lambda task: flags.append(s.walk_begin(task, False, 1)[1]["affinity_targets"]),
                                          ask, lambda ops: _send(engine, s, ops))
        return out + (flags,)


def test_host_reclaim_walk_equals_the_oracle(engine, snaps, oracle_mod, tmp_path):
    for case in EXACT:
        p, reclaim, c = snaps(case)
        log, asks, stops, flags = _host_loop(engine, p, c)
        assert log == [tuple(r) for r in reclaim], case
        # kbhip_walk_begin's out_info[3]: only the pod-affinity snapshot has classes that read affinity targets
        assert (1 in flags) == bool(case[0]) and set(flags) <= {0, 1}, (case, flags)
        assert sum(k == 8 for _, _, k in log) >= 2 and asks and stops[-1] in (ASSIGNED, EXHAUSTED), case
    c = ww.reclaim_snapshot()
    p = c.write(str(tmp_path / "r.kbs"))
    reclaim = [tuple(r) for r in oracle_mod.ref_allocate(p, actions="reclaim").as_list()]
    assert any(k == 128 and n > 64 for _, n, k in reclaim)  # an eviction beyond walk position 64
    log, asks, stops, _ = _host_loop(engine, p, c)
    assert log == reclaim and asks == [1] and stops == [ASSIGNED]  # one call where the windows take two


# ---- 3. launch accounting and read-only ------------------------------------------------------------------
def test_launches_and_read_only(engine, snaps):
    p, _, c = snaps(CASES[2])
    m = victimmodel.VictimModel(c)
    t = m.pending()[0]
    with engine.Session(p) as s, engine.Session(p) as twin:
        n_nodes = s.stats()["nodes"]
        combos = [(b, mode) for b in (True, False) for mode in (1, 2, 3)]
        old = [(twin.walk_victims(t, b, mode), twin.walk_victims_from(t, b, mode), twin.head_victims(t, b, mode, 64, 8))
               for b, mode in combos]
        tables = ("pod_status", "job_ready", "pod_job", "pod_queue")
        raw = ("job_drf_alloc", "queue_allocated", "queue_deserved")
        s.walk_victims(t, True, 1)  # (builds the two tables, as the twin's first call did)
        rows = s.read_nodes(n_nodes)
        tab0 = [s.table(n).copy() for n in tables] + [s.table_raw(n, np.float64).copy() for n in raw]
        sweeps = s.stats()["sweeps"]
        acted, k = 0, 0
        for b, mode in combos:
            full = twin.rank_victim_nodes(t, b, mode, 0, 1 << 16)
            total, info = s.walk_begin(t, b, mode)
            assert total == full[0] and info["launches"] == full[4]["launches"] and not info["rebuilt"]
            assert s.walk_order()[1].tolist() == full[1].tolist()
            pos = 0
            while True:
                got = s.walk_next(pos, 3)
                _check_scan(got[3], pos)
                assert got[3]["launches"] == 2 and not got[3]["patched"]
                acted += got[3]["acted"]
                k += 1
                if got[3]["stop"] in (ASSIGNED, EXHAUSTED):
                    break
                # read-only: nothing was applied, so the evictions are not carried to the next call and the
                # walk is moved on by hand, behind the last entry the call dealt with
                assert got[3]["next"] > pos
                pos = got[3]["next"]
            k += 1  # (kbhip_walk_begin counts as one sweep)
        assert acted and s.stats()["sweeps"] == sweeps + k
        tab1 = [s.table(n) for n in tables] + [s.table_raw(n, np.float64) for n in raw]
        assert all(np.array_equal(a, b) for a, b in zip(tab0, tab1))
        assert np.array_equal(s.read_nodes(n_nodes), rows)
        a, b = s.walk_visits(), twin.walk_visits()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # the existing calls on the same session, after the new ones ran: what they returned on the twin
        for (b, mode), (w0, f0, h0) in zip(combos, old):
            w1, f1, h1 = s.walk_victims(t, b, mode), s.walk_victims_from(t, b, mode), s.head_victims(t, b, mode, 64, 8)
            for x, y in ((w0, w1), (f0, f1)):
                assert walkvictims.as_ops(x) == walkvictims.as_ops(y)
                keys = [q for q in x[3] if q not in ("rebuilt", "state_rebuilt", "launches")]
                assert {q: x[3][q] for q in keys} == {q: y[3][q] for q in keys}
            assert h0[0] == h1[0] and all(np.array_equal(x, y) for x, y in zip(h0[1:7], h1[1:7]))
        assert s.walk_order()[0] >= 0  # the cursor outlived all of them
        # an allocate leaves walk counters and a FitDelta answer: neither moves under the calls
        s.allocate()
        left = [q for q in m.pending() if s.table("pod_status")[q] == 1]
        size = lambda: int(engine.lib().kbhip_walk_visits(s._h, None, None, 0))  # (a full read clears the counters)
        v0 = size()
        assert left and v0 >= 0
        try:
            d0 = s.fit_deltas(left[0])
        except engine.KbhipError:
            d0 = None
        s.walk_begin(left[0], True, 1)
        s.walk_next(0)
        s.walk_order()
        assert size() == v0
        if d0 is not None:
            assert all(np.array_equal(x, y) for x, y in zip(d0, s.fit_deltas(left[0])))


def test_pending_changes_are_counted(engine, clusters):
    """The patch launch is counted: after a kbhip_apply_ops the next kbhip_walk_next patches the victim state."""
    path, m, task = clusters("gang_carried", 1)
    with engine.Session(path) as s:
        s.walk_begin(task, False, 1)
        a = s.walk_next(0, 1)
        assert a[3]["launches"] == 2 and a[3]["state_rebuilt"] and not a[3]["patched"]
        _send(engine, s, walkvictims.as_ops(a))
        b = s.walk_next(a[3]["next"], 1)
        assert b[3]["patched"] > 0 and b[3]["launches"] == 3 and not b[3]["state_rebuilt"] and not b[3]["rebuilt"]


# ---- 4. the cursor's lifetime and the refusals ---------------------------------------------------------------
def test_lifetime(engine, clusters):
    path, m, task = clusters("valid_at63", 1)

    def opened():
        s = engine.Session(path)
        assert s.walk_begin(task, False, 1)[0] == 130
        return s

    def gone(s):
        for call in (lambda: s.walk_next(0), lambda: s.walk_order()):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                call()
        assert s.walk_end() is False
        s.close()

    with engine.Session(path) as s:  # no cursor yet
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_next(0)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_order()
    s = opened()
    s.first_fit([task])
    gone(s)
    s = opened()
    s.place_job([task], 0, 1, 0)
    gone(s)
    s = opened()
    s.carry()
    gone(s)
    s = opened()
    assert s.walk_end() is True
    gone(s)
    s = opened()  # a refused kbhip_apply_ops changes nothing, the cursor included
    with pytest.raises(engine.KbhipError, match=EINVAL):
        s.apply_ops([engine.OP_UNEVICT], [0], [0])
    assert s.walk_order()[0] == 130
    s.close()
    # the applied PIPELINE
    path_c, _, task_c = clusters("covers_at0", 1)
    with engine.Session(path_c) as s:
        s.walk_begin(task_c, False, 1)
        got = s.walk_next(0)
        assert got[3]["stop"] == ASSIGNED
        _send(engine, s, walkvictims.as_ops(got))
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_next(got[3]["next"])
    # a second begin replaces the first
    path_t, _, task_t = clusters("ties", 1)
    with engine.Session(path_t) as s:
        n = s.walk_begin(task_t, True, 1)[0]
        by_score = s.walk_order()[1].tolist()
        assert by_score == ww.walk_of("ties", True)
        assert s.walk_begin(task_t, False, 1)[0] == n
        total, nodes, scores = s.walk_order()
        assert nodes.tolist() == list(range(n)) != by_score and not scores.any()
        assert s.walk_end() is True


def test_errors(engine, clusters):
    path, m, task = clusters("valid_at63", 1)
    with engine.Session(path) as s:
        for kw in (dict(victims=0), dict(victims=4), dict(by_score=2)):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.walk_begin(task, **kw)
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_begin(0, True, 1)  # a Running pod: no task class
        with pytest.raises(engine.KbhipError, match=EINVAL):
            s.walk_begin(len(m.h.pods), True, 1)
        with pytest.raises(engine.KbhipError, match=EINVAL):  # no cursor is open after refused begins
            s.walk_order()
        assert s.walk_begin(task, False, 1)[0] == 130
        for pos, cap, cap_ops in ((-1, 4, 4), (131, 4, 4), (0, 0, 4), (0, 65, 4), (0, 4, 0)):
            with pytest.raises(engine.KbhipError, match=EINVAL):
                s.walk_next(pos, cap, cap_ops)
        last = s.walk_next(130)  # the end of the order is a position
        assert len(last[0]) == 0 and (last[3]["stop"], last[3]["decided"], last[3]["first"], last[3]["next"]) == (
            EXHAUSTED, 0, -1, 130)
        t = s.place_job_submit([task], 0, 1, 0)
        with pytest.raises(engine.KbhipError, match=EINVAL):  # a ticket is outstanding
            s.walk_next(0)
        assert s.place_job_cancel(t) == 1
        # a refused call on a device session writes nothing
        outs = [np.full(4, 77, np.uint8), np.full(4, 77, np.int32), np.full(4, 77, np.int32), np.full(10, 77, np.int64)]
        ptr = [a.ctypes.data for a in outs]
        L = engine.lib()
        for pos, cap, cap_ops in ((131, 4, 4), (-1, 4, 4), (0, 65, 4), (0, 4, 0)):
            assert L.kbhip_walk_next(s._h, pos, cap, *ptr[:3], cap_ops, ptr[3]) == -1
        assert L.kbhip_walk_begin(s._h, task, 1, 0, ptr[3]) == -1 and L.kbhip_walk_begin(s._h, 0, 1, 1, ptr[3]) == -1
        assert L.kbhip_walk_order(s._h, -1, ptr[1], ptr[2], 4) == -1
        assert all((a == 77).all() for a in outs)
        assert s.walk_order()[0] == 130  # refused calls leave the cursor open
    sh = engine.ShardedSession(path, 0, 0, 2)
    try:
        for call in (lambda: sh.walk_begin(task, True, 1), lambda: sh.walk_next(0), lambda: sh.walk_order()):
            with pytest.raises(engine.KbhipError, match=EUNSUP):
                call()
    finally:
        sh.close()
