"""The group-wise fix-up pass (rg_obs_fix.hip k_obs_fix, librogue_gym_obsfix.so): behind a step launch that pre-streamed the gray images, one wave per group of
consecutive envs (OBS_FIX_GROUP: 8, the sweep's choice among 8, 16 and 32 -- profiles/r12_experiments.txt) re-encodes the image lines the turns touched --
packed into a list, eight lines per wave instruction -- and draws the group's Redraw envs.  It must leave exactly what k_obs_resid left: tests/prestream_child.py and tests/tail_encode_child.py (both unchanged) compare images, flag words, mirrors,
reward and done with a twin on the two-pass path after every step, fill the tensor with -1 before each step -- an env no wave serves shows -- and assert that
Redraw, changed and unchanged envs all occurred.

Shapes chosen around a group of 16, none the workload's own, and as good around the group of 8: 15 (a full group and a short one), 16 (full groups and
nothing behind them), 17 (a group of one env behind full ones), 82 (full groups and two envs: the `base + lane < n` guard) and 4 160 (520 groups).  Every
child runs with 64 envs per step wave.

With the development library: ROGUE_GYM_HIP_ENC_CUT=0 -- no helper blocks, every mask all ones, so a full group fills its list (16 entries per env: 128, four
trips of the pass loop; with groups of 16 it was 256 and eight) -- the helpers starting at once or after every turn, and one helper for every run.
tests/obs_fix_child.py counts what the groups held, for the kernel's groups of 8 and for 16 consecutive envs (two groups side by side): a step with a
Redraw pending in every env of a group, and a step with a Redraw beside masked envs in one group."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "rogue-gym_amd", "variants", "librogue_gym_hip_dev.so")
GROUPS = [8, 16]   # the kernel's group (csrc/rg_obs_fix.hip OBS_FIX_GROUP; tests/test_obs_fix_resources.py pins it to the source), and 16 consecutive envs
SHAPES = [15, 16, 17, 82, 4160]
CHILD_SECONDS = 240   # a child takes seconds; the limit only ends one that hangs
pytestmark = pytest.mark.gpu


def child(script, *args, **extra):
    env = dict(os.environ, ROGUE_GYM_HIP_EPW="64", **extra)
    for k in ("ROGUE_GYM_HIP_NO_TAIL_ENCODE", "ROGUE_GYM_HIP_ENC_CUT", "ROGUE_GYM_HIP_ENC_DELAY", "ROGUE_GYM_HIP_ENC_HELPERS", "RG_OBS_RESID_BLOCKS", "ROGUE_GYM_HIP_LIB"):
        if k not in extra:
            env.pop(k, None)   # (RG_OBS_RESID_BLOCKS would select k_obs_resid in the development library)
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.join(ROOT, "tests", script)] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_SECONDS + 30)
    print(r.stdout[-400:])
    assert r.returncode == 0, (args, extra, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK"), r.stdout[-2000:]
    return r.stdout


def dev_library():
    assert os.path.exists(DEV), "the development library is missing: __graft_entry__.build() makes it"
    return DEV


@pytest.mark.parametrize("n", SHAPES)
def test_twin_on_the_two_pass_path(n):
    child("prestream_child.py", n)


@pytest.mark.parametrize("n", SHAPES)
def test_every_mask_all_ones_fills_the_list(n):
    """ENC_CUT = 0: every env without a Redraw has all 16 lines in the list -- 16 entries per env, 128 in a full group, 16 passes of eight lines."""
    child("prestream_child.py", n, ROGUE_GYM_HIP_LIB=dev_library(), ROGUE_GYM_HIP_ENC_CUT="0")


@pytest.mark.parametrize("delay", [0, 20000], ids=["helpers-start-at-once", "helpers-start-after-every-turn"])
@pytest.mark.parametrize("n", [82, 4160])
def test_twin_whatever_the_helpers_see(n, delay):
    child("prestream_child.py", n, ROGUE_GYM_HIP_LIB=dev_library(), ROGUE_GYM_HIP_ENC_DELAY=str(delay))


@pytest.mark.parametrize("n", [82, 4160])
def test_one_helper_streams_every_run(n):
    child("prestream_child.py", n, ROGUE_GYM_HIP_LIB=dev_library(), ROGUE_GYM_HIP_ENC_HELPERS="1")


@pytest.mark.parametrize("check", ["nokey", "nolive", "cadence"])
def test_keys_that_do_not_play_and_a_mixed_cadence(check):
    child("tail_encode_child.py", check, 82)


@pytest.mark.parametrize("group", GROUPS)
def test_a_group_of_nothing_but_redraws_and_a_redraw_beside_masked_envs(group):
    child("obs_fix_child.py", 82, group)
