"""kbhip_explain_tasks without a GPU: the declaration, the export, the binding,
the constants, and the argument checks that need no device — each refused with
KBHIP_EINVAL and with every output array left as it was.  The verdict logic is
tests/test_explain_model.py, the device path tests/test_gpu_explain.py."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1
VP = ctypes.c_void_p


def _p(a):
    return None if a is None else a.ctypes.data_as(VP)


def test_declared_exported_and_bound(engine_lib):
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    assert re.search(r"\bint64_t\s+kbhip_explain_tasks\s*\(", src)
    assert re.search(r"\bint\s+kbhip_debug_explain\s*\(", src)
    for name in ("kbhip_explain_tasks", "kbhip_debug_explain"):
        assert name in kbhip.EXPORTS and hasattr(engine_lib, name)
    for cls in (kbhip.Session, kbhip.ShardedSession):
        assert callable(getattr(cls, "explain_tasks", None))
    assert callable(getattr(kbhip.EncodedSnapshot, "explain", None))


def test_constants_match_the_header():
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    defs = {k: int(v, 0) for k, v in re.findall(r"^#define\s+(KBHIP_(?:WHY|EXPLAIN)_[A-Z_]+)\s+(0x[0-9a-fA-F]+|\d+)", src, re.M)}
    names = ["FITS_IDLE", "FITS_RELEASING", "RESOURCES", "POD_COUNT", "NODE_SELECTOR", "HOST_PORTS", "UNSCHEDULABLE",
             "TAINTS", "POD_AFFINITY", "SCORE_ERROR"]
    assert [defs["KBHIP_WHY_" + n] for n in names] == list(range(10))
    assert [getattr(kbhip, "WHY_" + n) for n in names] == list(range(10))
    assert (defs["KBHIP_WHY_SHORT_CPU"], defs["KBHIP_WHY_SHORT_MEM"], defs["KBHIP_WHY_SHORT_GPU"]) == \
        (kbhip.WHY_SHORT_CPU, kbhip.WHY_SHORT_MEM, kbhip.WHY_SHORT_GPU) == (0x10, 0x20, 0x40)
    assert defs["KBHIP_EXPLAIN_MAX"] == kbhip.EXPLAIN_MAX == 64
    assert defs["KBHIP_EXPLAIN_BINS"] == kbhip.EXPLAIN_BINS == 16


def test_null_session(engine_lib):
    ids = np.zeros(2, np.int32)
    hist = np.full(32, -7, np.int64)
    assert engine_lib.kbhip_explain_tasks(None, _p(ids), 2, None, _p(hist), None) == EINVAL
    assert b"null session" in engine_lib.kbhip_last_error()
    assert (hist == -7).all()
    assert engine_lib.kbhip_debug_explain(None, 0, None, _p(hist)) == EINVAL
    assert (hist == -7).all()


# (n_tasks, null argument) -> a word of the message
REFUSED = [(-1, None, b"n_tasks"), (65, None, b"n_tasks"), (2, "task_ids", b"null"), (2, "out_hist", b"null"),
           # well-formed arguments: an encode-only session has no device state, also for an empty batch
           (2, None, b"encode-only"), (64, None, b"encode-only"), (0, None, b"encode-only")]


@pytest.mark.parametrize("n_tasks,null,word", REFUSED, ids=lambda v: v.decode() if isinstance(v, bytes) else str(v))
def test_argument_checks(engine_lib, kbgen_mod, tmp_path, n_tasks, null, word):
    import kbhip
    p = kbgen_mod.gen_random(7, n_nodes=4, n_jobs=2, max_tasks=2).write(str(tmp_path / "e.kbs"))
    with kbhip.EncodedSnapshot(p) as enc:
        pend = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
        assert pend
        ids = np.full(65, pend[0], np.int32)
        hist = np.full(65 * 16, -7, np.int64)
        verdict = np.full(65 * 4, 0xA5, np.uint8)
        info = np.full(3, -7, np.int64)
        args = {"task_ids": ids, "out_hist": hist}
        if null:
            args[null] = None
        rc = engine_lib.kbhip_explain_tasks(enc._h, _p(args["task_ids"]), n_tasks, _p(verdict), _p(args["out_hist"]),
                                            _p(info))
        assert rc == EINVAL
        assert word in engine_lib.kbhip_last_error(), engine_lib.kbhip_last_error()
        assert (hist == -7).all() and (verdict == 0xA5).all() and (info == -7).all()


def test_debug_twin_checks(engine_lib, kbgen_mod, tmp_path):
    """The twin refuses a task without a class and a null histogram, writing nothing."""
    import kbhip
    p = kbgen_mod.gen_random(7, n_nodes=4, n_jobs=2, max_tasks=2).write(str(tmp_path / "e.kbs"))
    with kbhip.EncodedSnapshot(p) as enc:
        cls = enc.table("pod_class")
        no_class = [int(i) for i in np.nonzero(cls < 0)[0]] + [-1, int(cls.size)]
        hist = np.full(16, -7, np.int64)
        verdict = np.full(4, 0xA5, np.uint8)
        for pod in no_class:
            assert engine_lib.kbhip_debug_explain(enc._h, pod, _p(verdict), _p(hist)) == EINVAL
            assert b"task class" in engine_lib.kbhip_last_error()
        assert engine_lib.kbhip_debug_explain(enc._h, int(np.nonzero(cls >= 0)[0][0]), _p(verdict), None) == EINVAL
        assert (hist == -7).all() and (verdict == 0xA5).all()
        v, h = enc.explain(int(np.nonzero(cls >= 0)[0][0]))
        assert v.size == 4 and h[15] == 4 and h[:10].sum() == 4 and h[10] == 0 and h[14] == h[:3].sum()
