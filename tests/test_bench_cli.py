"""bench.py's own contract on the HIP stepper: a plain run times exactly --steps steps and prints the headline fields without the side measurements,
--full adds those, and --dump-outputs writes what the last timed step returned -- the same arrays whichever of the two runs computed them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3", "--envs-per-gpu", str(N), "--preroll-steps", "40",
           "--clock-warm-s", "0", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.timeout(900)
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain = _bench(tmp_path / "plain")
    assert plain["steps"] == 12 and plain["warmup"] == 3 and plain["unit"] == "env-steps/s" and plain["higher_is_better"] is True
    assert plain["value"] > 0 and abs(plain["value"] - N * 1e3 / plain["ms_per_step"]) < 1e-6 * plain["value"]
    assert plain["dtype"] and plain["metric"]
    for k in ("roofline", "kernels", "repeats", "long_window", "step_us", "workload_rates", "extra_workloads", "cpu_baseline"):
        assert k not in plain, k
    assert "cold_start" not in plain["preroll"]

    full = _bench(tmp_path / "full", "--full", "--no-extra", "--no-cpu-baseline")
    assert full["steps"] == 12 and full["value"] > 0
    assert full["roofline"]["kernel"] in ("k_step", "k_obs", "k_render") and len(full["repeats"]["ms_per_step"]) == 5
    assert full["long_window"]["steps"] == 1000 and full["step_us"]["step"]["p50"] > 0 and full["preroll"]["cold_start"]["steps"] == 12

    size = 0
    for name, shape in (("obs", (N, 1, 16, 32)), ("reward", (N,)), ("done", (N,))):
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape, (name, a.dtype, a.shape)
        assert np.array_equal(a, b), name
        size += os.path.getsize(tmp_path / "plain" / (name + ".npy"))
    assert size <= 64 << 20
    obs = np.load(tmp_path / "plain" / "obs.npy")
    assert obs.min() >= 0 and obs.max() <= 1 and obs.std() > 0
