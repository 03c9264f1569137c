"""kbhip_apply_ops without a GPU: the declaration, the export, the operation
codes and the argument checks that need no device.  The device path is
tests/test_gpu_apply_ops.py."""
import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "kbhip.h")).read()


def _arrays(n):
    vp = ctypes.c_void_p
    op = np.full(n, 1, np.uint8)
    pod = np.zeros(n, np.int32)
    node = np.zeros(n, np.int32)
    return op, pod, node, [a.ctypes.data_as(vp) for a in (op, pod, node)]


def test_apply_ops_declared_and_exported(engine_lib):
    import kbhip
    assert re.search(r"\bint64_t\s+kbhip_apply_ops\s*\(", _header())
    assert "kbhip_apply_ops" in kbhip.EXPORTS
    assert hasattr(engine_lib, "kbhip_apply_ops")


def test_operation_codes_match_binding():
    import kbhip
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(KBHIP_OP_[A-Z]+)\s+(\d+)", _header())}
    assert defs == {"KBHIP_OP_EVICT": kbhip.OP_EVICT, "KBHIP_OP_PIPELINE": kbhip.OP_PIPELINE,
                    "KBHIP_OP_UNPIPELINE": kbhip.OP_UNPIPELINE, "KBHIP_OP_UNEVICT": kbhip.OP_UNEVICT}
    assert sorted(defs.values()) == [1, 2, 3, 4]


def test_apply_ops_null_session(engine_lib):
    _, _, _, (op, pod, node) = _arrays(2)
    launches = ctypes.c_int64(-7)
    assert engine_lib.kbhip_apply_ops(None, None, None, None, 0, None) == EINVAL
    assert b"null session" in engine_lib.kbhip_last_error()
    assert engine_lib.kbhip_apply_ops(None, op, pod, node, 2, ctypes.byref(launches)) == EINVAL
    assert launches.value == -7  # nothing written on a refused call


def test_apply_ops_argument_checks(engine_lib, kbgen_mod, tmp_path):
    """An encode-only session has no device state: every call on it is refused,
    and a negative n or a null array with n > 0 is refused whatever the session
    is."""
    import kbhip
    p = kbgen_mod.gen_random(7, n_nodes=4, n_jobs=2, max_tasks=2).write(str(tmp_path / "e.kbs"))
    _, _, _, (op, pod, node) = _arrays(2)
    f = engine_lib.kbhip_apply_ops
    with kbhip.EncodedSnapshot(p) as enc:
        assert f(enc._h, op, pod, node, 2, None) == EINVAL
        assert b"encode-only" in engine_lib.kbhip_last_error()
        assert f(enc._h, None, None, None, 0, None) == EINVAL
        assert b"encode-only" in engine_lib.kbhip_last_error()
        assert f(enc._h, op, pod, node, -1, None) == EINVAL
        assert b"negative n" in engine_lib.kbhip_last_error()
        for args in ((None, pod, node), (op, None, node), (op, pod, None), (None, None, None)):
            assert f(enc._h, *args, 2, None) == EINVAL
            assert b"null" in engine_lib.kbhip_last_error()
