"""kbhip_rank_heads without a GPU: the declaration, the export, the binding,
the batch limit, and the argument checks that need no device — each refused
with KBHIP_EINVAL and with every output array left as it was.
The device paths are tests/test_gpu_rank_heads.py."""
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


def test_rank_heads_declared_exported_and_bound(engine_lib):
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    assert re.search(r"\bint64_t\s+kbhip_rank_heads\s*\(", src)
    assert "kbhip_rank_heads" in kbhip.EXPORTS
    assert hasattr(engine_lib, "kbhip_rank_heads")
    assert callable(getattr(kbhip.Session, "rank_heads", None))
    for cls in (kbhip.Session, kbhip.ShardedSession):
        assert hasattr(cls, "rank_heads")


def test_rank_heads_max_matches_the_header():
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    m = re.search(r"^#define\s+KBHIP_RANK_HEADS_MAX\s+(\d+)\s*$", src, re.M)
    assert m and int(m.group(1)) == kbhip.RANK_HEADS_MAX == 64


def test_rank_heads_null_session(engine_lib):
    ids = np.zeros(2, np.int32)
    total = np.full(2, -7, np.int64)
    node = np.full(8, -7, np.int32)
    assert engine_lib.kbhip_rank_heads(None, _p(ids), 2, 1, 0, 4, _p(total), _p(node), None, None, None) == EINVAL
    assert b"null session" in engine_lib.kbhip_last_error()
    assert (total == -7).all() and (node == -7).all()


# (n_tasks, by_score, victims, cap, null argument) -> a word of the message
REFUSED = [(2, 1, 0, 0, None, b"cap"), (2, 1, 0, 65, None, b"cap"), (2, 1, 0, -1, None, b"cap"),
           (-1, 1, 0, 4, None, b"n_tasks"), (65, 1, 0, 4, None, b"n_tasks"),
           (2, 1, -1, 4, None, b"victims"), (2, 1, 4, 4, None, b"victims"),
           (2, 2, 0, 4, None, b"by_score"),
           (2, 1, 0, 4, "task_ids", b"null"), (2, 1, 0, 4, "out_total", b"null"), (2, 1, 0, 4, "out_node", b"null"),
           # well-formed arguments: an encode-only session has no device state, whatever victims is
           (2, 1, 0, 4, None, b"encode-only"), (2, 0, 3, 64, None, b"encode-only"), (0, 1, 0, 4, None, b"encode-only")]


@pytest.mark.parametrize("n_tasks,by_score,victims,cap,null,word", REFUSED,
                         ids=lambda v: v.decode() if isinstance(v, bytes) else str(v))
def test_rank_heads_argument_checks(engine_lib, kbgen_mod, tmp_path, n_tasks, by_score, victims, cap, null, word):
    import kbhip
    p = kbgen_mod.gen_random(7, n_nodes=4, n_jobs=2, max_tasks=2).write(str(tmp_path / "e.kbs"))
    with kbhip.EncodedSnapshot(p) as enc:
        pend = [int(i) for i in np.nonzero(enc.table("pod_class") >= 0)[0]]
        assert pend
        ids = np.full(65, pend[0], np.int32)
        total = np.full(65, -7, np.int64)
        node, score, cands = (np.full(65 * 65, -7, np.int32) for _ in range(3))
        info = np.full(3, -7, np.int64)
        args = {"task_ids": ids, "out_total": total, "out_node": node}
        if null:
            args[null] = None
        rc = engine_lib.kbhip_rank_heads(enc._h, _p(args["task_ids"]), n_tasks, by_score, victims, cap,
                                         _p(args["out_total"]), _p(args["out_node"]), _p(score), _p(cands), _p(info))
        assert rc == EINVAL
        assert word in engine_lib.kbhip_last_error(), engine_lib.kbhip_last_error()
        for a in (total, node, score, cands, info):
            assert (a == -7).all()
