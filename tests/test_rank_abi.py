"""kbhip_rank_nodes without a GPU: the declaration, the export, the argument
checks that need no device, and the two stats fields of its device paths.
The device paths are tests/test_gpu_rank_nodes.py."""
import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_rank_nodes_declared_and_exported(engine_lib):
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    assert re.search(r"\bint64_t\s+kbhip_rank_nodes\s*\(", src)
    assert "kbhip_rank_nodes" in kbhip.EXPORTS
    assert hasattr(engine_lib, "kbhip_rank_nodes")


def test_rank_nodes_null_session(engine_lib):
    node = np.zeros(4, np.int32)
    vp = ctypes.c_void_p
    assert engine_lib.kbhip_rank_nodes(None, 0, 1, 0, None, None, 0) == -1  # KBHIP_EINVAL
    assert b"null session" in engine_lib.kbhip_last_error()
    assert engine_lib.kbhip_rank_nodes(None, 0, 0, 0, node.ctypes.data_as(vp), None, 4) == -1


def test_rank_nodes_argument_checks(engine_lib, kbgen_mod, tmp_path):
    """On an encode-only session every call is refused: the size query because
    the session has no device state, and a negative first or a null out_node
    with cap > 0 whatever the session is."""
    import kbhip
    p = kbgen_mod.gen_random(7, n_nodes=4, n_jobs=2, max_tasks=2).write(str(tmp_path / "e.kbs"))
    node = np.zeros(4, np.int32)
    vp = ctypes.c_void_p
    with kbhip.EncodedSnapshot(p) as enc:
        pend = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
        assert pend
        t = pend[0]
        for by_score in (0, 1):
            assert engine_lib.kbhip_rank_nodes(enc._h, t, by_score, 0, None, None, 0) == -1
            assert b"encode-only" in engine_lib.kbhip_last_error()
            assert engine_lib.kbhip_rank_nodes(enc._h, t, by_score, 0, node.ctypes.data_as(vp), None, 4) == -1
            assert engine_lib.kbhip_rank_nodes(enc._h, t, by_score, -1, node.ctypes.data_as(vp), None, 4) == -1
            assert b"first" in engine_lib.kbhip_last_error()
            assert engine_lib.kbhip_rank_nodes(enc._h, t, by_score, 0, None, None, 4) == -1
            assert b"out_node" in engine_lib.kbhip_last_error()
            assert engine_lib.kbhip_rank_nodes(enc._h, t, by_score, 0, node.ctypes.data_as(vp), None, -1) == -1


def test_rank_stats_fields_last():
    import kbhip
    assert [n for n, _ in kbhip.Stats._fields_[-2:]] == ["rank_heads", "rank_fulls"]
    assert all(t is ctypes.c_int64 for _, t in kbhip.Stats._fields_[-2:])
