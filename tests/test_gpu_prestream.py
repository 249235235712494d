"""The pre-streamed encode (rg_kernels.hip enc_helper, rg_obs.hip k_obs_resid): rg_step_obs_gray on the mini config streams every env's gray image from the
screen mirror in helper blocks of the step launch, beside the turns, and the pass behind the launch re-encodes the image lines the turns touched
(RgState::enc_rows) and draws the Redraw envs.  Which mirror bytes a helper happened to see must never show: a twin on the two-pass path gets the same keys,
and images, flag words, reward and done are compared after every step -- tests/prestream_child.py, one process per batch shape: 80 envs at 64 per wave (a
full wave and a 16-lane one, 20 runs for the helpers) and 4 160 envs at 64 per wave.  With the development library the helpers start at once, or only after
every turn has ended and rewritten its mirror, or there is one helper that streams every run."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "rogue-gym_amd", "variants", "librogue_gym_hip_dev.so")
SHAPES = [80, 4160]
pytestmark = pytest.mark.gpu


def child(n, **extra):
    env = dict(os.environ, ROGUE_GYM_HIP_EPW="64", **extra)
    for k in ("ROGUE_GYM_HIP_NO_TAIL_ENCODE", "ROGUE_GYM_HIP_ENC_CUT", "ROGUE_GYM_HIP_ENC_DELAY", "ROGUE_GYM_HIP_ENC_HELPERS"):
        if k not in extra:
            env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "prestream_child.py"), str(n)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK"), r.stdout[-2000:]
    return r.stdout


@pytest.mark.parametrize("n", SHAPES)
def test_twin_on_the_two_pass_path(n):
    child(n)


@pytest.mark.parametrize("delay", [0, 20000], ids=["helpers-start-at-once", "helpers-start-after-every-turn"])
@pytest.mark.parametrize("n", SHAPES)
def test_twin_whatever_the_helpers_see(n, delay):
    """The helper start delay of the development library (ROGUE_GYM_HIP_ENC_DELAY, ticks of the 100 MHz clock; capped at 200 us in the kernel): with 20 000 the
    helpers read mirrors the turns of these small batches have long rewritten, with 0 the ones the previous step left or a turn is writing."""
    assert os.path.exists(DEV), "the development library is missing: __graft_entry__.build() makes it"
    child(n, ROGUE_GYM_HIP_LIB=DEV, ROGUE_GYM_HIP_ENC_DELAY=str(delay))


@pytest.mark.parametrize("n", SHAPES)
def test_one_helper_streams_every_run(n):
    assert os.path.exists(DEV), "the development library is missing: __graft_entry__.build() makes it"
    child(n, ROGUE_GYM_HIP_LIB=DEV, ROGUE_GYM_HIP_ENC_HELPERS="1")
