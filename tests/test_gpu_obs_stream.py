"""k_obs_stream (the gray encode of <= 512-cell grids without status / history planes) against the encode it replaced, k_obs<0, false>: same image for
every env and every pixel, same mirrors, same flag words.  Both run in one process of the development library (-DRG_DEV_KNOBS, built by
__graft_entry__.build()), where RG_OBS_STREAM=0 selects the old kernel per call -- tests/obs_stream_child.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "rogue-gym_amd", "variants", "librogue_gym_hip_dev.so")

CASES = [
    ("mini", 65536, 200, ""),              # the headline batch
    ("mini", 65536 - 37, 200, ""),         # a batch that is not a whole number of runs
    ("mini", 65536 - 37, 120, "no_mirror"),  # every Redraw drawn from the tiles by the pass (ROGUE_GYM_HIP_NO_MIRROR_UPDATE: ~43 % of the envs)
    ("default", 16384, 200, ""),           # 80x24: served by k_obs as before
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,steps,mode", CASES, ids=["%s-%d-%s" % (c[0], c[1], c[3] or "mirror") for c in CASES])
def test_stream_encode_equals_the_previous_encode(name, n, steps, mode):
    """Prefix steps, steps whose Redraw flags stay pending into the next pass, and the first pass after rg_reset included (see the child)."""
    assert os.path.exists(DEV), "the development library is missing: __graft_entry__.build() makes it"
    env = dict(os.environ, ROGUE_GYM_HIP_LIB=DEV)
    args = [sys.executable, os.path.join(ROOT, "tests", "obs_stream_child.py"), name, str(n), str(steps)] + ([mode] if mode else [])
    r = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("OK"), r.stdout[-2000:]
