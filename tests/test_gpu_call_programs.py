"""Interleaved C-ABI call sequences against the CPU oracle, call by call (tests/call_programs.py: the programs; tests/call_model.py: the model;
tests/call_runner.py: the harness; tests/test_call_programs_host.py: the CPU proof of all three).

Every program walks every ordered pair of the thirteen call classes and six named triples on one _Handle of 82 envs -- not on HipVecRogueEnv, which encodes
after every call and so hides these orders -- and every call's own outputs are held against the model with tolerance 0; at the end the internals and
mirrors of every env, rg_sync and the workload counters.  Profiles: the mini grid (k_step_w32, the pre-streamed encode and k_obs_fix) with a plain and
with a bound standing tensor, the default 80x24 dungeon (k_step<2>, partial dist maps in the records, the 256-thread k_obs), a 33x17 grid (H*W = 561: the
unfused k_render and the scalar encode; the typed passes, the compact record and rg_step_fetch are refused there, and the program asserts the refusal), and
the mini grid once more at 64 envs per step wave in a child process (the knob is read once per process)."""
import os
import subprocess
import sys

import pytest

import call_programs as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", cp.SEEDS)
@pytest.mark.parametrize("profile", sorted(cp.PROFILES))
def test_program_against_the_model(profile, seed):
    from call_runner import run_program

    print("%s seed %d: %s" % (profile, seed, run_program(profile, seed)))


@pytest.mark.parametrize("seed", cp.SEEDS)
def test_vec_env_program_against_the_model(seed):
    """The shorter program over HipVecRogueEnv's public methods (call_programs.vec_program: step_keys, reset, reset_envs with ids or a mask and with seeds,
    seed, save_state / load_state / clone_state, archive_update / archive_restore, cut_episodes; all 100 ordered pairs of its ten classes), mini only, with
    episodes, novelty, an added crop view and the legal-action mask on: obs, the crop view, the mask, reward, done, episode returns and lengths after every
    call -- the _refresh / _after_step lists of device.py in every order."""
    from call_runner import run_vec_program

    print("vec seed %d: %s" % (seed, run_vec_program(seed)))


def test_program_at_64_envs_per_wave():
    """The plain mini program of seed 1 with ROGUE_GYM_HIP_EPW=64: one full 64-env step wave and a short one."""
    env = dict(os.environ, ROGUE_GYM_HIP_EPW="64")
    env.pop("ROGUE_GYM_HIP_NO_TAIL_ENCODE", None)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "call_programs_child.py"), "mini_plain", "1"], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK"), r.stdout[-2000:]
    print(r.stdout.strip())
