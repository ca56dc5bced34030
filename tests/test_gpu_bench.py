"""bench.py on one GPU: a plain run prints the headline line without the measurements that take runs of their own (--full), the timed
region runs exactly --steps iterations, and --dump-outputs writes float32 / float64 arrays that are the same on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_WINDOW = ["--scans", "2", "--rings", "32", "--az", "256", "--static", "2000"]


def _bench(cwd, *argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv], capture_output=True, text=True, timeout=600, env=env,
                       cwd=str(cwd))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_steps_and_dumped_outputs(tmp_path):
    runs = [_bench(tmp_path, "--steps", "3", "--warmup", "1", *SMALL_WINDOW, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for out in runs:
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(out)
        assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
        assert out["stage_ms_per_step"] is None and out["pcie_inclusive"] is None and out["keyframe_pass"] is None and out["small_window"] is None
        assert "cpu_baseline" not in out
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["global_points", "rel_orientations", "rel_translations", "report"]
    assert a["rel_orientations"].dtype == np.float64 and a["rel_orientations"].shape == (runs[0]["config"]["control_poses_or_frames"], 3)
    assert a["global_points"].dtype == np.float32 and a["global_points"].shape == (runs[0]["config"]["points"], 4)
    assert np.all(np.isfinite(a["global_points"])) and np.all(np.isfinite(a["rel_translations"]))
    assert a["report"][0] == 3 and a["report"][2] == runs[0]["config"]["gaussians"]
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_keyframe_workload_dumps_every_neighbourhood(tmp_path):
    out = _bench(tmp_path, "--workload", "keyframes", "--steps", "2", "--warmup", "1", "--map-frames", "17", "--neighbourhoods", "4",
                 "--dump-outputs", str(tmp_path / "kf"))
    assert out["steps"] == 2 and out["value"] > 0 and out["stage_ms_per_step"] is None and "cpu_baseline" not in out
    d = _load(tmp_path / "kf")
    assert sorted(d) == sorted(["rel_orientations", "rel_translations"] + [f"nb{n}_{k}" for n in range(4) for k in ("global_points", "report")])
    assert d["rel_orientations"].shape == (17, 3) and d["rel_translations"].dtype == np.float64
    assert all(d[f"nb{n}_report"][0] == 2 and d[f"nb{n}_global_points"].dtype == np.float32 for n in range(4))
