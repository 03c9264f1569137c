"""kbhip_head_victims / kbhip_debug_victims without a device: argument
validation, and the per-node decision (vict_stage / vict_link / vict_decide of
kbhip_eval.h, the functions the kernel runs) on the host tables of an
encode-only session against tests/victimmodel.py at the opened state."""
import ctypes
import os
import re

import numpy as np
import pytest

import victimmodel
from test_gpu_victim_walk import CASES, TIERS, _gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
vp = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(vp)


def test_declared_and_exported(engine_lib):
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    assert re.search(r"\bint64_t\s+kbhip_head_victims\s*\(", src)
    assert re.search(r"\bint\s+kbhip_debug_victims\s*\(", src)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(KBHIP_HEAD_VICTIMS_[A-Z]+)\s+(\d+)", src)}
    assert defs == {"KBHIP_HEAD_VICTIMS_VALID": kbhip.HEAD_VICTIMS_VALID,
                    "KBHIP_HEAD_VICTIMS_COVERS": kbhip.HEAD_VICTIMS_COVERS}
    assert (victimmodel.VALID, victimmodel.COVERS) == (kbhip.HEAD_VICTIMS_VALID, kbhip.HEAD_VICTIMS_COVERS)
    for name in ("kbhip_head_victims", "kbhip_debug_victims"):
        assert name in kbhip.EXPORTS and hasattr(engine_lib, name)


def _outs(cap=4, stride=3):
    return [np.full(cap, 77, np.int32), np.full(cap, 77, np.int32), np.full(cap, 77, np.int32),
            np.full(cap, 77, np.int32), np.full(cap, 77, np.uint8), np.full(cap * stride, 77, np.int32),
            np.full(5, 77, np.int64)]


def test_argument_validation(engine_lib, kbgen_mod, tmp_path):
    import kbhip
    L = engine_lib
    o = _outs()
    ptr = [_p(a) for a in o]
    assert L.kbhip_head_victims(None, 0, 1, 1, 4, 3, *ptr) == EINVAL
    assert b"null session" in L.kbhip_last_error()
    p = _gen(kbgen_mod, CASES[0]).write(str(tmp_path / "v.kbs"))
    enc = kbhip.EncodedSnapshot(p)
    try:
        t = int(np.nonzero(enc.table("pod_class") >= 0)[0][0])
        assert L.kbhip_head_victims(enc._h, t, 1, 1, 4, 3, *ptr) == EINVAL
        assert b"encode-only" in L.kbhip_last_error()
        for cap, stride, word in ((0, 3, b"cap"), (65, 3, b"cap"), (4, 0, b"stride"), (4, -1, b"stride")):
            assert L.kbhip_head_victims(enc._h, t, 1, 1, cap, stride, *ptr) == EINVAL
            assert word in L.kbhip_last_error()
        for k in (0, 2, 3, 4, 5):  # a null required output (out_score and out_info are optional)
            q = list(ptr)
            q[k] = None
            assert L.kbhip_head_victims(enc._h, t, 1, 1, 4, 3, *q) == EINVAL
            assert b"null out_node" in L.kbhip_last_error()
        assert L.kbhip_head_victims(enc._h, t, 2, 1, 4, 3, *ptr) == EINVAL
        for mode in (0, 4, -1):
            assert L.kbhip_head_victims(enc._h, t, 1, mode, 4, 3, *ptr) == EINVAL
            assert b"KBHIP_VICTIMS" in L.kbhip_last_error()
        assert all((a == 77).all() for a in o)  # a refused call writes nothing
        # kbhip_debug_victims
        c1, e1, f1, row = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(4, np.int32)
        dv = L.kbhip_debug_victims
        assert dv(None, t, 1, 0, 4, _p(c1), _p(e1), _p(f1), _p(row)) == EINVAL
        assert dv(enc._h, t, 1, 0, 4, None, _p(e1), _p(f1), _p(row)) == EINVAL
        assert dv(enc._h, t, 1, 0, 0, _p(c1), _p(e1), _p(f1), _p(row)) == EINVAL
        assert dv(enc._h, t, 0, 0, 4, _p(c1), _p(e1), _p(f1), _p(row)) == EINVAL
        assert dv(enc._h, t, 1, -1, 4, _p(c1), _p(e1), _p(f1), _p(row)) == EINVAL
        assert dv(enc._h, t, 1, int(enc.table("dims")[0]), 4, _p(c1), _p(e1), _p(f1), _p(row)) == EINVAL
        running = int(np.nonzero(enc.table("pod_class") < 0)[0][0])
        assert dv(enc._h, running, 1, 0, 4, _p(c1), _p(e1), _p(f1), _p(row)) == EINVAL
        assert dv(enc._h, t, 1, 0, 4, _p(c1), _p(e1), _p(f1), _p(row)) == 0
    finally:
        enc.close()


def _compare(kbhip, c, path):
    m = victimmodel.VictimModel(c)
    enc = kbhip.EncodedSnapshot(path)
    checked = nonempty = 0
    try:
        cls = enc.table("pod_class")
        tasks = [t for t in m.pending() if cls[t] >= 0]
        assert tasks
        # the plugin state the library opened is the restatement's
        assert np.array_equal(enc.table("pod_job"),
                              [m.job_index.get(m.h.pods[p]["job"], -1) for p in range(len(m.node))])
        assert np.array_equal(enc.table("job_ready"), [m.ready(j) for j in m.h.jobs])
        if m.h.drf_on:
            assert np.array_equal(enc.table_raw("job_drf_alloc", np.float64).reshape(-1, 3),
                                  np.array([j["drf_alloc"] for j in m.h.jobs]))
        if m.h.prop_on:
            names = sorted(m.h.queues)
            for tab, key in (("queue_allocated", "allocated"), ("queue_deserved", "deserved")):
                assert np.array_equal(enc.table_raw(tab, np.float64).reshape(-1, 3),
                                      np.array([m.h.queues[n][key] for n in names])), tab
        for t in tasks:
            for mode in (1, 2, 3):
                for node in range(m.n_nodes):
                    exp_v, exp_e, exp_f = m.decide(t, mode, node)
                    count, evict, flags, row = enc.victims(t, mode, node)
                    assert (count, row.tolist(), evict, flags) == (len(exp_v), exp_v, exp_e, exp_f), (t, mode, node)
                    if count > 1:  # a stride below the count truncates the row only
                        c2, e2, f2, r2 = enc.victims(t, mode, node, stride=count - 1)
                        assert (c2, e2, f2, r2.tolist()) == (count, evict, flags, exp_v[:count - 1])
                    checked += 1
                    nonempty += bool(exp_v)
    finally:
        enc.close()
    return checked, nonempty


@pytest.mark.parametrize("case", CASES, ids=lambda c: "a%d_s%d_t%d_f%d" % c)
def test_debug_victims_equals_the_restatement(engine_lib, kbgen_mod, tmp_path, case):
    import kbhip
    c = _gen(kbgen_mod, case)
    checked, _ = _compare(kbhip, c, c.write(str(tmp_path / "v.kbs")))
    assert checked


FLAGS = [{"gang": ["disablePreemptable"]}, {"gang": ["disableReclaimable"], "drf": ["disablePreemptable"]},
         {"proportion": ["disableReclaimable"], "conformance": ["disablePreemptable"]},
         {"conformance": ["disableReclaimable", "disablePreemptable"], "gang": ["disableJobReady"]}]


@pytest.mark.parametrize("tier", [1, 2, 3])
@pytest.mark.parametrize("flags", range(len(FLAGS)))
def test_tier_layouts_and_disabled_plugins(engine_lib, kbgen_mod, tmp_path, tier, flags):
    import kbhip
    total = 0
    for seed in (3, 34, 39):
        c = _gen(kbgen_mod, (0, seed, tier, 0))
        c.flags = {p: f for p, f in FLAGS[flags].items() if any(p in t for t in TIERS[tier])}
        _, nonempty = _compare(kbhip, c, c.write(str(tmp_path / ("f%d.kbs" % seed))))
        total += nonempty
    assert total  # the layouts decide something
