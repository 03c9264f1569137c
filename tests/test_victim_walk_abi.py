"""kbhip_rank_victim_nodes without a GPU: the declaration, the export, the
victim-kind codes and the argument checks that need no device.  The device
paths are tests/test_gpu_victim_walk.py."""
import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "kbhip.h")).read()


def test_declared_and_exported(engine_lib):
    import kbhip
    assert re.search(r"\bint64_t\s+kbhip_rank_victim_nodes\s*\(", _header())
    assert "kbhip_rank_victim_nodes" in kbhip.EXPORTS
    assert hasattr(engine_lib, "kbhip_rank_victim_nodes")
    assert hasattr(kbhip.Session, "rank_victim_nodes")


def test_victim_codes_match_binding():
    import kbhip
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(KBHIP_VICTIMS_[A-Z_]+)\s+(\d+)", _header())}
    assert defs == {"KBHIP_VICTIMS_OTHER_QUEUES": kbhip.VICTIMS_OTHER_QUEUES,
                    "KBHIP_VICTIMS_QUEUE_OTHER_JOBS": kbhip.VICTIMS_QUEUE_OTHER_JOBS,
                    "KBHIP_VICTIMS_SAME_JOB": kbhip.VICTIMS_SAME_JOB}
    assert sorted(defs.values()) == [1, 2, 3]


def test_null_session(engine_lib):
    f = engine_lib.kbhip_rank_victim_nodes
    vp = ctypes.c_void_p
    node = np.full(4, -7, np.int32)
    info = np.full(3, -7, np.int64)
    assert f(None, 0, 1, 1, 0, None, None, None, 0, None) == EINVAL
    assert b"null session" in engine_lib.kbhip_last_error()
    assert f(None, 0, 0, 1, 0, node.ctypes.data_as(vp), None, None, 4, info.ctypes.data_as(vp)) == EINVAL
    assert (node == -7).all() and (info == -7).all()  # nothing written on a refused call


def test_argument_checks(engine_lib, kbgen_mod, tmp_path):
    """On an encode-only session every call is refused: a well-formed one
    because the session has no device state; a negative first or cap, a null
    out_node with cap > 0 and a victims value outside 1..3 whatever the
    session is."""
    import kbhip
    p = kbgen_mod.gen_random(7, n_nodes=4, n_jobs=2, max_tasks=2).write(str(tmp_path / "e.kbs"))
    node = np.zeros(4, np.int32)
    vp = ctypes.c_void_p
    nd = node.ctypes.data_as(vp)
    f = engine_lib.kbhip_rank_victim_nodes
    with kbhip.EncodedSnapshot(p) as enc:
        pend = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
        assert pend
        t = pend[0]
        for by_score in (0, 1):
            for victims in (1, 2, 3):
                assert f(enc._h, t, by_score, victims, 0, None, None, None, 0, None) == EINVAL
                assert b"encode-only" in engine_lib.kbhip_last_error()
                assert f(enc._h, t, by_score, victims, 0, nd, None, None, 4, None) == EINVAL
                assert b"encode-only" in engine_lib.kbhip_last_error()
                assert f(enc._h, t, by_score, victims, -1, nd, None, None, 4, None) == EINVAL
                assert b"first" in engine_lib.kbhip_last_error()
                assert f(enc._h, t, by_score, victims, 0, nd, None, None, -1, None) == EINVAL
                assert b"cap" in engine_lib.kbhip_last_error()
                assert f(enc._h, t, by_score, victims, 0, None, None, None, 4, None) == EINVAL
                assert b"out_node" in engine_lib.kbhip_last_error()
            for victims in (0, 4):
                assert f(enc._h, t, by_score, victims, 0, nd, None, None, 4, None) == EINVAL
                assert b"victims" in engine_lib.kbhip_last_error()
                assert f(enc._h, t, by_score, victims, 0, None, None, None, 0, None) == EINVAL
                assert b"victims" in engine_lib.kbhip_last_error()
