"""The tail encode (rg_kernels.hip tail_encode, rg_obs.hip k_obs_resid): rg_step_obs_gray on the mini config lets every step wave write the gray images of the
envs it leaves without a pending Redraw, and a residual pass serves the others.  Checked against the CPU oracle at every step, against the two-pass path
(ROGUE_GYM_HIP_NO_TAIL_ENCODE=1) and against rg_step + rg_obs_gray as separate calls, through a mixed cadence of calls, and with keys that do not play --
tests/tail_encode_child.py, one process per batch shape: 48 envs (three waves of 16 lanes), 80 envs at 64 per wave (a full wave and a 16-lane one) and
4 160 envs at 64 per wave (65 waves and 260 runs of the residual pass).  Handles the tail encode does not apply to must take the path they took."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(48, None), (80, 64), (4160, 64)]
pytestmark = pytest.mark.gpu


DEV = os.path.join(ROOT, "rogue-gym_amd", "variants", "librogue_gym_hip_dev.so")


def child(check, n, epw, **extra):
    env = dict(os.environ, **extra)
    env.pop("ROGUE_GYM_HIP_NO_TAIL_ENCODE", None)
    if epw:
        env["ROGUE_GYM_HIP_EPW"] = str(epw)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tail_encode_child.py"), check, str(n)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("OK"), r.stdout[-2000:]
    return r.stdout


@pytest.mark.parametrize("n,epw", SHAPES, ids=["n%d-epw%s" % s for s in SHAPES])
def test_every_step_against_the_oracle(n, epw):
    child("oracle", n, epw)


@pytest.mark.parametrize("n,epw", SHAPES, ids=["n%d-epw%s" % s for s in SHAPES])
def test_twin_handles_are_bit_identical(n, epw):
    child("twins", n, epw)


@pytest.mark.parametrize("cut", [0, 1 << 30], ids=["every-wave-late", "no-wave-late"])
def test_twin_handles_whichever_waves_are_late(cut):
    """A step wave that reaches its tail late leaves its envs to the residual pass (RgState::enc_cut), and which waves do changes from run to run.  The
    development library (-DRG_DEV_KNOBS, built by __graft_entry__.build()) takes the threshold from ROGUE_GYM_HIP_ENC_CUT: with 0 every wave is late and the
    pass streams every env that is not drawn, with 2^30 ticks none is.  Bit-identical to the two-pass path and to separate calls either way."""
    assert os.path.exists(DEV), "the development library is missing: __graft_entry__.build() makes it"
    child("twins", 4160, 64, ROGUE_GYM_HIP_LIB=DEV, ROGUE_GYM_HIP_ENC_CUT=str(cut))


@pytest.mark.parametrize("n,epw", SHAPES, ids=["n%d-epw%s" % s for s in SHAPES])
def test_mixed_cadence_on_one_handle(n, epw):
    child("cadence", n, epw)


@pytest.mark.parametrize("n,epw", SHAPES, ids=["n%d-epw%s" % s for s in SHAPES])
def test_keys_that_do_not_play(n, epw):
    child("nokey", n, epw)


@pytest.mark.parametrize("n,epw", SHAPES, ids=["n%d-epw%s" % s for s in SHAPES])
def test_envs_past_max_steps_without_auto_reset(n, epw):
    child("nolive", n, epw)


def residual_launches(env, keys, steps=3):
    """(k_step launches, observation-pass launches) rg_timing saw over `steps` step_keys calls."""
    L, h = env._h.L, env._h.h
    env._h.check(L.rg_timing_enable(h, 1))
    for _ in range(steps):
        env.step_keys(keys)
    env.check_errors()
    ms, launches = (C.c_double * 4)(), (C.c_uint64 * 4)()
    env._h.check(L.rg_timing_read(h, ms, launches))
    env._h.check(L.rg_timing_enable(h, 0))
    return int(launches[0]), int(launches[2])


def test_ineligible_handles_take_the_old_path(goldens):
    """A 33x17 grid, status planes, a bound tensor and a bf16 image: the same images as the two-pass build of the same handle (nothing observable tells
    the launches apart: rg_timing counts one step and one observation launch per call on either path)."""
    import torch

    from rogue_gym.envs.device import HipVecRogueEnv
    from rogue_gym.envs.rogue_env import DungeonType, ImageSetting, StatusFlag

    mini = goldens["configs"]["mini"]
    cases = {
        "33x17": ({"width": 33, "height": 17, "dungeon": {"style": "rogue", "room_num_x": 2, "room_num_y": 2, "min_room_size": {"x": 4, "y": 4}}}, {}),
        "status planes": (mini, {"image_setting": ImageSetting(DungeonType.GRAY, StatusFlag.DUNGEON_LEVEL | StatusFlag.HP_CURRENT, False)}),
        "persistent_obs": (mini, {"persistent_obs": True}),
        "bf16": (mini, {"obs_dtype": torch.bfloat16}),
    }
    n = 80
    rng = np.random.RandomState(3)
    table = np.frombuffer(b".hjklnbuy>s", np.uint8)
    for name, (cfg, kw) in cases.items():
        cfgs = [json.dumps(dict(cfg, seed=i)) for i in range(n)]
        a = HipVecRogueEnv(cfgs, max_steps=9, **kw)
        os.environ["ROGUE_GYM_HIP_NO_TAIL_ENCODE"] = "1"
        try:
            b = HipVecRogueEnv(cfgs, max_steps=9, **kw)
        finally:
            del os.environ["ROGUE_GYM_HIP_NO_TAIL_ENCODE"]
        for t in range(1, 31):
            keys = table[rng.randint(0, len(table), n)].copy()
            if t % 4 == 0:
                keys[:] = ord(">")
            k = torch.as_tensor(keys, device=a.device)
            a.step_keys(k)
            b.step_keys(k)
            assert torch.equal(a.obs, b.obs), "%s: step %d" % (name, t)
            assert torch.equal(a.flags, b.flags) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), "%s: step %d" % (name, t)
        assert residual_launches(a, k) == residual_launches(b, k) == (3, 3), name
        a.close()
        b.close()
