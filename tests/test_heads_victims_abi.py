"""kbhip_heads_victims without a device: the declaration, the binding's constants and the argument
validation on an encode-only session — a refused call writes nothing."""
import ctypes
import os
import re

import numpy as np

from test_gpu_victim_walk import CASES, _gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
vp = ctypes.c_void_p
N, CAP, STRIDE = 3, 4, 3


def _p(a):
    return a.ctypes.data_as(vp)


def test_declared_and_exported(engine_lib):
    import kbhip
    src = open(os.path.join(ROOT, "include", "kbhip.h")).read()
    assert re.search(r"\bint64_t\s+kbhip_heads_victims\s*\(", src)
    defs = dict(re.findall(r"#define\s+(KBHIP_HEADS_VICTIMS_[A-Z]+)\s+(\d+)", src))
    assert defs == {"KBHIP_HEADS_VICTIMS_MAX": str(kbhip.HEADS_VICTIMS_MAX)}
    assert kbhip.HEADS_VICTIMS_MAX == 64 == kbhip.RANK_HEADS_MAX
    assert "kbhip_heads_victims" in kbhip.EXPORTS and hasattr(engine_lib, "kbhip_heads_victims")
    assert callable(getattr(kbhip.Session, "heads_victims"))


def _outs():
    """total, node, score, count, evict, flags, victim, first, info: every buffer at its sentinel."""
    rows = N * CAP
    return [np.full(N, 77, np.int64), np.full(rows, 77, np.int32), np.full(rows, 77, np.int32),
            np.full(rows, 77, np.int32), np.full(rows, 77, np.int32), np.full(rows, 77, np.uint8),
            np.full(rows * STRIDE, 77, np.int32), np.full(N, 77, np.int32), np.full(6, 77, np.int64)]


def test_argument_validation(engine_lib, kbgen_mod, tmp_path):
    import kbhip
    L = engine_lib
    o = _outs()
    ptr = [_p(a) for a in o]
    untouched = lambda: all((a == 77).all() for a in o)
    p = _gen(kbgen_mod, CASES[0]).write(str(tmp_path / "v.kbs"))
    enc = kbhip.EncodedSnapshot(p)
    try:
        pend = np.nonzero(enc.table("pod_class") >= 0)[0]
        ids = np.ascontiguousarray(np.resize(pend, N), np.int32)
        call = lambda h, n=N, by_score=1, victims=1, cap=CAP, stride=STRIDE, tasks=_p(ids), outs=ptr: \
            L.kbhip_heads_victims(h, tasks, n, by_score, victims, cap, stride, *outs)
        assert call(None) == EINVAL
        assert b"null session" in L.kbhip_last_error() and untouched()
        assert call(enc._h) == EINVAL  # an otherwise valid call
        assert b"encode-only" in L.kbhip_last_error() and untouched()
        assert call(enc._h, n=0) == EINVAL  # (an empty batch still needs a device session)
        assert b"encode-only" in L.kbhip_last_error() and untouched()
        for kw, word in ((dict(n=-1), b"n_tasks"), (dict(n=65), b"n_tasks"), (dict(cap=0), b"cap"),
                         (dict(cap=65), b"cap"), (dict(stride=0), b"stride"), (dict(by_score=2), b"by_score"),
                         (dict(victims=0), b"KBHIP_VICTIMS"), (dict(victims=4), b"KBHIP_VICTIMS")):
            assert call(enc._h, **kw) == EINVAL, kw
            assert word in L.kbhip_last_error(), kw
            assert untouched(), kw
        assert call(enc._h, tasks=None) == EINVAL
        assert b"null task_ids" in L.kbhip_last_error() and untouched()
        for k in (0, 1, 3, 4, 5, 6):  # a null required output (out_score, out_first and out_info are optional)
            q = list(ptr)
            q[k] = None
            assert call(enc._h, outs=q) == EINVAL, k
            assert b"null task_ids" in L.kbhip_last_error(), k
            assert untouched(), k
        for k in (2, 7, 8):  # without an optional output the call gets as far as the session check
            q = list(ptr)
            q[k] = None
            assert call(enc._h, outs=q) == EINVAL
            assert b"encode-only" in L.kbhip_last_error() and untouched()
    finally:
        enc.close()
