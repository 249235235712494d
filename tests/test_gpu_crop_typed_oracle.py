"""Crop views (HipVecRogueEnv.add_crop -> rg_obs_crop_typed) against the CPU oracle at every step, in the pattern of test_crop_every_step of
tests/test_gpu_obs_oracle.py: the oracle's image gathered at the oracle's player cell (parity_util.crop_window) and rounded with typed_util; the ids
are Symbol::from_tile of the oracle's screen (typed_util.SYMBOL_OF_TILE)."""
import numpy as np
import pytest

import typed_util as tu
from oracle.pyoracle import OracleEnv
from parity_util import crop_window
from test_crop_typed_abi import typed_crop_reference
from test_gpu_obs_oracle import FULL, device_keys, fail, image, seeker_keys, vec_env

pytestmark = pytest.mark.gpu

# (seeds for which the oracles alone stay within the cap: checked on the CPU)
N, STEPS, MAX_STEPS, RADII, SEED0, KEY_SEED = 96, 20, 25, (3, 5), 0, 305
SKIP_CAP = 0.05  # of all (env, step) pairs: those whose oracle one-hot image raises (a 'Z' on screen), for the one kind that cannot express them


def configs(goldens):
    mini, nohide = goldens["configs"]["mini"], goldens["configs"]["nohide"]
    return [dict(nohide if i % 3 == 2 else mini, seed=SEED0 + i) for i in range(N)]


@pytest.mark.timeout(150)
def test_crop_views_against_the_oracle_every_step(goldens):
    """96 envs, mini and nohide 80x24 in one batch (mixed sizes: a crop env), 20 seeker-policy steps with 25-step episodes; an id view, an f16 gray view with
    every status plane and the history plane and a bf16 one-hot view with the history plane, all of radii (3, 5): every window and every centre at every
    step.  The one-hot view is skipped where the oracle's one-hot image raises; at most 5 % of the pairs."""
    import torch
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag

    ry, rx = RADII
    cfgs = configs(goldens)
    env = vec_env(cfgs, 0, 0, False, crop=0, max_steps=MAX_STEPS)
    ids = env.add_crop(RADII, image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, True), symbol_ids=True)
    gray = env.add_crop(RADII, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.FULL, True), obs_dtype=torch.float16)
    onehot = env.add_crop(RADII, image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, True), obs_dtype=torch.bfloat16)
    oracles = [OracleEnv(c, max_steps=MAX_STEPS) for c in cfgs]
    rng = np.random.RandomState(KEY_SEED)
    skipped = pairs = 0
    for t in range(0, STEPS + 1):
        if t:
            keys = seeker_keys(oracles, rng)
            env.step_keys(device_keys(env, keys))
            for i, o in enumerate(oracles):
                o.step_autoreset(int(keys[i]))
        got_ids, got_gray, got_oh = ids.obs.cpu().numpy(), gray.obs.view(torch.int16).cpu().numpy().view(np.uint16), onehot.obs.view(torch.int16).cpu().numpy().view(np.uint16)
        cens = [v.center.cpu().numpy() for v in (ids, gray, onehot)] + [env.crop_center.cpu().numpy()]
        for i, o in enumerate(oracles):
            sc = o.scalars()
            py, px = sc["py"], sc["px"]
            for c in cens:
                assert (int(c[i, 0]), int(c[i, 1])) == (py, px), "step %d env %d: centre %s, oracle player (%d, %d)" % (t, i, c[i], py, px)
            pairs += 1
            idimg = np.stack([tu.symbol_ids(o.screen()), np.asarray(o.hist(), np.uint8)]).astype(np.float32)
            exp = typed_crop_reference(idimg, py, px, ry, rx, 2, 1, True, tu.RG_OBS_U8)
            if not np.array_equal(got_ids[i], exp):
                fail("id view", t, i, got_ids[i], exp, env._h, o.screen())
            exp = typed_crop_reference(image(o, 0, FULL, True), py, px, ry, rx, 0, 1, True, tu.RG_OBS_F16)
            if not np.array_equal(got_gray[i], exp):
                fail("f16 gray view", t, i, got_gray[i], exp, env._h, o.screen())
            try:
                img = image(o, 1, 0, True)
            except RuntimeError:  # (a 'Z' on the screen: the library raises only if it lies inside the window -- tests/test_gpu_crop_typed.py)
                skipped += 1
                continue
            exp = tu.bits16(crop_window(img, py, px, ry, rx, 1, env.symbols, True), tu.RG_OBS_BF16)
            if not np.array_equal(got_oh[i], exp):
                fail("bf16 one-hot view", t, i, got_oh[i], exp, env._h, o.screen())
        env._h.L.rg_sync(env._h.h)  # (drains a possible tile error of such a window)
    print("skipped %d of %d (env, step) pairs of the one-hot view" % (skipped, pairs))
    assert skipped <= SKIP_CAP * pairs, (skipped, pairs)
    env.close()
