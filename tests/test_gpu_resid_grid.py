"""The fix-up pass on any grid (rg_obs.hip k_obs_resid, rgk_obs_resid_blocks): a wave of a grid smaller than the runs loops over runs gridDim.x apart, one
run ahead with the flag words and masks, and must serve every env exactly as a wave per run does.  The development library takes the grid from
RG_OBS_RESID_BLOCKS; tests/prestream_child.py (unchanged) compares images, flag words, reward and done with a twin on the two-pass path after each of 60
steps, fills the tensor with -1 before every step -- an env no wave serves shows -- and asserts that flagged Redraw, changed and unchanged envs all occurred.

Shapes: 80 envs (20 runs), 82 (21 runs, the last of 2 envs: the `base + lane < n` guard of a looping wave -- every other shape of the suite is a multiple
of 4) and 4 160 (1 040 runs).  Grids: 1 (one wave walks every run; its last prefetch lies past the batch), 3 (odd: unequal trip counts, and a wave whose
last iteration prefetches nothing), runs - 1 (exactly one wave loops twice), runs + 5 (must clamp to the runs)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "rogue-gym_amd", "variants", "librogue_gym_hip_dev.so")
SHAPES = [80, 82, 4160]
GRIDS = ["one", "three", "runs-1", "runs+5"]
CHILD_SECONDS = 240   # a child takes seconds; the limit only ends one that hangs
pytestmark = pytest.mark.gpu


def grid_of(name, n):
    nruns = -(-n // 4)
    return {"one": 1, "three": 3, "runs-1": nruns - 1, "runs+5": nruns + 5}[name]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", SHAPES)
def test_twin_on_the_two_pass_path_for_any_grid(n, grid):
    assert os.path.exists(DEV), "the development library is missing: __graft_entry__.build() makes it"
    g = grid_of(grid, n)
    env = dict(os.environ, ROGUE_GYM_HIP_EPW="64", ROGUE_GYM_HIP_LIB=DEV, RG_OBS_RESID_BLOCKS=str(g))
    for k in ("ROGUE_GYM_HIP_NO_TAIL_ENCODE", "ROGUE_GYM_HIP_ENC_CUT", "ROGUE_GYM_HIP_ENC_DELAY", "ROGUE_GYM_HIP_ENC_HELPERS"):
        env.pop(k, None)
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.join(ROOT, "tests", "prestream_child.py"), str(n)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_SECONDS + 30)
    print(r.stdout[-400:])
    assert r.returncode == 0, (n, g, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK"), r.stdout[-2000:]
