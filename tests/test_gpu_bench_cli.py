"""bench.py's command line: a plain run prints the headline line and nothing
that takes runs of its own; --dump-outputs writes the last timed session's
placement log, equal to what a caller of Session.allocate() receives."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_options():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(engine, tmp_path):
    cache, out = tmp_path / "cache", tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--nodes", "3000",
                        "--pending", "20000", "--cache", str(cache), "--dump-outputs", str(out)],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "placements/s" and d["higher_is_better"] is True and d["dtype"] == "int64"
    assert d["ms_per_step"] > 0 and d["value"] > 0
    # value = placements of the timed steps / their wall time
    assert d["value"] == pytest.approx(2 * d["config"]["placements_per_session"] / (2 * d["ms_per_step"] * 1e-3))
    assert "cpu_baseline" not in d and d["roofline"]["sweep"] is None and d["roofline"]["traffic"] is None
    got = {n: np.load(out / f"{n}.npy") for n in ("pod", "node", "kind")}
    assert sorted(os.listdir(out)) == ["kind.npy", "node.npy", "pod.npy"]
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in got.values())
    snaps = os.listdir(cache)
    assert len(snaps) == 1
    with open(cache / snaps[0], "rb") as f, engine.Session(f.read(), device=0) as s:
        pod, node, kind = s.allocate()
    assert len(pod) == d["config"]["placements_per_session"] > 0
    for n, a in zip(("pod", "node", "kind"), (pod, node, kind)):
        assert np.array_equal(got[n], a.astype(np.float64)), n
