"""k_step_enc (rg_step_enc.hip, librogue_gym_stepenc.so): the step kernel of the headline class -- 32 x 16 cells, at most 32 rooms, the launch that pre-streams
the gray images -- is k_step_w32<false, true>'s turn code compiled with the grid as a constant.  It must compute what the generic instance computes:
tests/step_enc_child.py plays the mini config with max_steps = 30 for 120 steps, '>' for every env on the stairs, and after every step compares the observation,
reward, done, status, flag bits and both mirrors of every env with the oracle, and -- in the development library -- everything, the saved state records
included, with a twin handle forced onto the generic instance (ROGUE_GYM_HIP_STEP_GENERIC, a knob of that library alone).

Shapes: 1 env (a lone lane), 65 (a partial last wave), 130 (several 16-env waves, stair blocks and helper blocks).  Once more at 130 envs without helper blocks
(ROGUE_GYM_HIP_ENC_CUT=0: every line mask all ones) and with the helpers' start delay at 0.  The product library against the oracle alone.  And the launch the
dispatch keeps on the generic instance (step_enc_child.py `narrow`: a 16 x 32 grid is refused by the config parser, so it is a handle without next-level
structures -- rgk_step_enc_takes: one of the things the kernel's text takes for granted about a handle; the others are switched by suites of their own, the
action history and the no-stair-waves and kept-spares knobs among them, which all step through the same call)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "rogue-gym_amd", "variants", "librogue_gym_hip_dev.so")
SHAPES = [1, 65, 130]
CHILD_SECONDS = 240   # a child takes seconds; the limit only ends one that hangs
KNOBS = ("ROGUE_GYM_HIP_NO_TAIL_ENCODE", "ROGUE_GYM_HIP_ENC_CUT", "ROGUE_GYM_HIP_ENC_DELAY", "ROGUE_GYM_HIP_ENC_HELPERS", "ROGUE_GYM_HIP_STEP_GENERIC", "ROGUE_GYM_HIP_NO_NEXT_LEVELS",
         "ROGUE_GYM_HIP_EPW", "RG_OBS_RESID_BLOCKS", "ROGUE_GYM_HIP_LIB")
pytestmark = pytest.mark.gpu


def child(mode, n, **extra):
    env = dict(os.environ, **extra)
    for k in KNOBS:
        if k not in extra:
            env.pop(k, None)
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.join(ROOT, "tests", "step_enc_child.py"), mode, str(n)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_SECONDS + 30)
    print(r.stdout[-600:])
    assert r.returncode == 0, (mode, n, extra, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK"), r.stdout[-2000:]
    return r.stdout


def dev_library():
    assert os.path.exists(DEV), "the development library is missing: __graft_entry__.build() makes it"
    return DEV


@pytest.mark.parametrize("n", SHAPES)
def test_the_oracle_and_a_twin_on_the_generic_instance(n):
    child("twin", n, ROGUE_GYM_HIP_LIB=dev_library())


def test_without_helper_blocks():
    child("twin", 130, ROGUE_GYM_HIP_LIB=dev_library(), ROGUE_GYM_HIP_ENC_CUT="0")


def test_helpers_that_start_at_once():
    child("twin", 130, ROGUE_GYM_HIP_LIB=dev_library(), ROGUE_GYM_HIP_ENC_DELAY="0")


def test_the_product_library_against_the_oracle():
    child("oracle", 130)


def test_a_launch_outside_the_class_stays_on_the_generic_instance():
    child("narrow", 65)
