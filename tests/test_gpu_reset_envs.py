"""Resetting chosen envs on the device (rg_reset_envs / rg_reset_mask / rg_seed_envs; HipVecRogueEnv.reset_envs, HipVecFirstFloor): the state records of
rebuilt and of untouched envs, the three ways of naming the envs, lock step with the CPU oracle through partial resets (stair set, dist cache, next-level
structures, spares), a list of every env of a 4 096-env handle, per-env seeds, `seed: None` envs, every observation mode, the key log, the
FirstFloorEnv convention and the refusals."""
import ctypes as C
import json
import types

import numpy as np
import pytest

from oracle.pyoracle import OracleEnv
from parity_util import ACTION_KEYS, ALL_KEYS, HipBatch, compare_internal, compare_mirrors, crop_window, make_oracles

pytestmark = pytest.mark.gpu

def torch_mod():
    import torch

    return torch


def seeded(cfg, seeds):
    out = []
    for s in seeds:
        d = dict(cfg)
        d["seed"] = int(s)
        out.append(d)
    return out


def vec_env(cfg, seeds, **kw):
    from rogue_gym.envs.device import HipVecRogueEnv

    return HipVecRogueEnv(seeded(cfg, seeds), **kw)


def random_keys(env, rng, table=ALL_KEYS):
    return torch_mod().as_tensor(table[rng.randint(0, len(table), env.num_envs)], device=env.device)


def mask_of(env, ids):
    torch = torch_mod()
    m = torch.zeros(env.num_envs, dtype=torch.bool)
    m[list(ids)] = True
    return m.to(env.device)


SEEK_TABLE = np.frombuffer(b"yku" b"h>l" b"bjn", np.uint8)


def seeker_key(screen, rng):
    """The stair-seeking policy of tests/test_gpu_crop.py on one screen (u8 [H, W]): '>' where no stairs are in sight (the player may stand on them), a
    greedy step towards a '%' in sight, one key in four at random."""
    if rng.randint(4) == 0:
        return int(ACTION_KEYS[rng.randint(len(ACTION_KEYS))])
    st, at = np.argwhere(screen == ord("%")), np.argwhere(screen == ord("@"))
    if len(st) == 0 or len(at) == 0:
        return ord(">")
    dy, dx = int(np.sign(st[0][0] - at[0][0])), int(np.sign(st[0][1] - at[0][1]))
    return int(SEEK_TABLE[(dy + 1) * 3 + dx + 1])


def subset_mirrors(handle, oracles, where):
    """compare_mirrors over a dict env -> OracleEnv."""
    screen, hist, status, flags = handle.fetch()
    for i, o in oracles.items():
        assert np.array_equal(screen[i], o.screen()), "%s env %d screen\nHIP:\n%s\nORACLE:\n%s" % (
            where, i, "\n".join(bytes(r).decode() for r in screen[i]), "\n".join(bytes(r).decode() for r in o.screen()))
        assert np.array_equal(hist[i], o.hist()), "%s env %d hist" % (where, i)
        assert [int(v) & 0xFFFFFFFF for v in status[i]] == [int(v) for v in o.status_arr()], "%s env %d status" % (where, i)
        f = o.flags()
        assert bool(flags[i] & 1) == f["is_terminal"] and bool(flags[i] & 2) == f["dead"], "%s env %d terminal / dead" % (where, i)


# ---------------------------------------------------------------------------------------------
# 1. records: rebuilt envs equal a newly created handle's, every other env keeps every byte
# ---------------------------------------------------------------------------------------------
def _records_case(cfg, n, seed):
    torch = torch_mod()
    seeds = [300 + i for i in range(n)]
    env, twin, new = vec_env(cfg, seeds), vec_env(cfg, seeds), vec_env(cfg, seeds)
    fresh = new.save_state().clone()
    new.close()
    rng = np.random.RandomState(seed)
    for _ in range(60):
        k = random_keys(env, rng)
        env.step_keys(k)
        twin.step_keys(k)
    gen = torch.Generator().manual_seed(seed)
    masks = [("empty", mask_of(env, [])), ("env 0", mask_of(env, [0])), ("last env", mask_of(env, [n - 1])), ("one per 16", mask_of(env, range(5, n, 16))),
             ("a random third", (torch.rand(n, generator=gen) < 1.0 / 3).to(env.device)), ("all", mask_of(env, range(n)))]
    for name, m in masks:
        before = env.save_state().clone()
        obs = env.reset_envs(mask=m)
        assert obs is env.obs
        after = env.save_state()
        torch.cuda.synchronize()
        assert torch.equal(after[~m], before[~m]), "%s: an env outside the mask changed" % name
        diff = (after[m] != fresh[m]).any(1).nonzero().reshape(-1).tolist()
        assert not diff, "%s: rebuilt envs %s differ from a newly created handle's (first byte %d)" % (
            name, [int(m.nonzero().reshape(-1)[i]) for i in diff[:8]], int((after[m][diff[0]] != fresh[m][diff[0]]).nonzero()[0]))
        if name != "all":
            for _ in range(6):  # (played on between the masks: the next mask meets envs in every state, rebuilt ones included)
                env.step_keys(random_keys(env, rng))
    twin.reset()
    assert torch.equal(env.save_state(), twin.save_state()), "the all-ones mask and rg_reset leave different records"
    env.step_keys(random_keys(env, rng))  # still steppable
    env.check_errors()
    env.close()
    twin.close()


def test_records_changed_and_unchanged_mini(goldens):
    _records_case(goldens["configs"]["mini"], 200, 1)   # 200: a multiple of neither 16 (envs per build wave) nor 64


def test_records_changed_and_unchanged_default(goldens):
    _records_case(goldens["configs"]["default"], 96, 2)


# ---------------------------------------------------------------------------------------------
# 2. host ids, device ids and the mask name the same envs
# ---------------------------------------------------------------------------------------------
def test_ids_and_mask_agree(goldens):
    torch = torch_mod()
    cfg, n = goldens["configs"]["mini"], 150
    envs = [vec_env(cfg, range(n)) for _ in range(3)]
    rng = np.random.RandomState(3)
    for _ in range(40):
        k = ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)]
        for e in envs:
            e.step_keys(torch.as_tensor(k, device=e.device))
    ids = sorted(int(i) for i in rng.permutation(n)[:41])
    shuffled = [ids[i] for i in rng.permutation(len(ids))]
    envs[0].reset_envs(env_ids=shuffled)
    envs[1].reset_envs(env_ids=torch.tensor(ids, dtype=torch.int64, device=envs[1].device))
    envs[2].reset_envs(mask=mask_of(envs[2], ids).to(torch.uint8))
    recs = [e.save_state() for e in envs]
    assert torch.equal(recs[0], recs[1]) and torch.equal(recs[0], recs[2])
    assert torch.equal(envs[0].obs, envs[1].obs) and torch.equal(envs[0].obs, envs[2].obs)
    for _ in range(10):  # ... and play on alike (the stair set each of them produced)
        k = ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)]
        for e in envs:
            e.step_keys(torch.as_tensor(k, device=e.device))
    recs = [e.save_state() for e in envs]
    assert torch.equal(recs[0], recs[1]) and torch.equal(recs[0], recs[2])
    for e in envs:
        e.check_errors()
        e.close()


# ---------------------------------------------------------------------------------------------
# 3. lock step with the oracle through partial resets
# ---------------------------------------------------------------------------------------------
LOCKSTEP_STEPS = 150


def partial_reset_scenario(cfg, n, seed, max_steps, hip=None):
    """150 steps of the stair-seeking policy (keys from the ORACLE's screens, so the scenario is the same with and without a GPU); after every 7th step a
    pseudo-random quarter of the envs is reset on both sides.  Returns (descents by untouched envs in the step right after a partial reset, '>' keys of
    freshly rebuilt envs in that step)."""
    rng = np.random.RandomState(seed)
    seeds = [7000 + 13 * i for i in range(n)]
    oracles = make_oracles(cfg, seeds, max_steps=max_steps)
    if hip is not None:
        compare_mirrors(hip, oracles, "t=0")
    fresh, untouched_descents, fresh_stairs_keys = set(), 0, 0
    for t in range(LOCKSTEP_STEPS):
        keys = np.array([seeker_key(o.screen(), rng) for o in oracles], np.uint8)
        levels = [int(o.status_arr()[0]) for o in oracles]
        if hip is not None:
            hip.step(keys)
        for i, o in enumerate(oracles):
            o.step_autoreset(int(keys[i]))
            if fresh:  # the step right after a partial reset
                if i in fresh:
                    fresh_stairs_keys += int(keys[i] == ord(">"))
                elif int(o.status_arr()[0]) > levels[i] and not o.flags()["is_terminal"]:
                    untouched_descents += 1
        fresh = set()
        if t % 7 == 6:
            fresh = set(int(i) for i in np.nonzero(rng.randint(0, 4, n) == 0)[0])
            ids = np.array(sorted(fresh), np.int32)
            if hip is not None:
                hip.h.check(hip.h.L.rg_reset_envs(hip.h.h, ids.ctypes.data, len(ids), 0))
            for i in fresh:
                oracles[i].reset()
        if hip is not None:
            compare_mirrors(hip, oracles, "t=%d" % (t + 1))
            if t % 8 == 7:
                compare_internal(hip, oracles, range(n), "t=%d" % (t + 1))
    return untouched_descents, fresh_stairs_keys


LOCKSTEP_CASES = {"mini": (128, 11, 40), "default": (64, 14, 60)}   # envs, scenario seed, max_steps (short episodes: auto-resets of rebuilt envs)


@pytest.mark.parametrize("name", sorted(LOCKSTEP_CASES))
def test_lockstep_with_oracle_through_partial_resets(goldens, name):
    """The scenario was run on the oracle alone first (no GPU): mini gives 13 descents by untouched envs in the step right after a partial reset and
    423 '>' keys of freshly rebuilt envs, the default dungeon 4 and 232."""
    n, seed, max_steps = LOCKSTEP_CASES[name]
    cfg = goldens["configs"][name]
    hip = HipBatch(cfg, [7000 + 13 * i for i in range(n)], max_steps=max_steps)
    untouched_descents, fresh_stairs_keys = partial_reset_scenario(cfg, n, seed, max_steps, hip)
    hip.sync()
    assert untouched_descents >= 1 and fresh_stairs_keys >= 1, (untouched_descents, fresh_stairs_keys)
    out = (C.c_uint64 * 9)()
    hip.h.check(hip.h.L.rg_counters_ex(hip.h.h, out, 9, 0))
    assert int(out[0]) > 0 and int(out[1]) > 0, list(out)   # auto-resets (every env, rebuilt ones included: max_steps is short) and descents


# ---------------------------------------------------------------------------------------------
# 4. a list of every env of a larger handle
# ---------------------------------------------------------------------------------------------
def test_every_env_listed_4096(goldens):
    """The list-driven build launches ceil(n_env / 16) one-wave blocks, enough for a list of every env: its grid is NOT capped and there is no stride
    loop to outrun.  So: 4 096 envs (256 blocks), all set."""
    torch = torch_mod()
    cfg, n = goldens["configs"]["mini"], 4096
    env = vec_env(cfg, range(n))
    fresh = env.save_state().clone()
    rng = np.random.RandomState(4)
    for _ in range(30):
        env.step_keys(random_keys(env, rng))
    played = env.save_state().clone()
    assert int((played != fresh).any(1).sum()) > n // 2
    env.reset_envs(mask=torch.ones(n, dtype=torch.bool, device=env.device))
    assert torch.equal(env.save_state(), fresh)
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------
# 5. seeds for chosen envs
# ---------------------------------------------------------------------------------------------
def test_seeds_for_chosen_envs(goldens):
    cfg, n, max_steps = goldens["configs"]["mini"], 136, 25
    s1, s2 = (0x1234ABCD << 64) | 0xDEADBEEF12345678, 987654321
    seeds = [900 + i for i in range(n)]
    env = vec_env(cfg, seeds, max_steps=max_steps)
    oracles = make_oracles(cfg, seeds, max_steps=max_steps)
    rng = np.random.RandomState(5)

    def play(steps, where):
        for t in range(steps):
            k = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)]
            env.step_keys(torch_mod().as_tensor(k, device=env.device))
            for i, o in enumerate(oracles):
                o.step_autoreset(int(k[i]))
            compare_mirrors(hb, oracles, "%s t=%d" % (where, t))

    hb = types.SimpleNamespace(fetch=env._h.fetch, debug=env._h.debug_state)   # (what parity_util's comparisons ask of a batch)
    play(10, "before")
    env.reset_envs(env_ids=[5, 130], seeds=[s1, s2])
    direct = {5: OracleEnv(cfg, max_steps=max_steps, seed=s1), 130: OracleEnv(cfg, max_steps=max_steps, seed=s2)}
    subset_mirrors(env._h, direct, "after reset_envs(seeds=)")
    buf = C.create_string_buffer(1 << 16)
    env._h.check(env._h.L.rg_dump_config(env._h.h, 5, buf, len(buf)))
    assert json.loads(buf.value.decode())["seed"] == s1
    env._h.check(env._h.L.rg_dump_config(env._h.h, 6, buf, len(buf)))
    assert json.loads(buf.value.decode())["seed"] == seeds[6]
    for i, s in ((5, s1), (130, s2)):
        oracles[i].set_seed(s)
        oracles[i].reset()
    compare_mirrors(hb, oracles, "after reset")
    play(3 * max_steps, "after")   # every env auto-resets at least twice: 5 and 130 into s1 / s2 again, every other one into its own seed
    compare_internal(hb, oracles, [4, 5, 6, 129, 130, 131], "end")
    assert env.counters()["resets"] >= 2 * n
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------
# 6. `seed: None` envs draw a new seed per rebuild
# ---------------------------------------------------------------------------------------------
def test_seedless_envs_get_new_levels(goldens):
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv

    cfg = dict(goldens["configs"]["mini"])
    cfg["seed"] = None
    n = 64
    env = HipVecRogueEnv([cfg] * n)
    start_status = env.status.clone()
    rng = np.random.RandomState(6)
    for _ in range(10):
        env.step_keys(random_keys(env, rng))
    rec0 = env.save_state().clone()
    env.reset_envs(env_ids=list(range(n)))
    rec1 = env.save_state().clone()
    assert torch.equal(env.status, start_status) and int(env.status[:, 0].max()) == 1   # level 1, the status of a new game
    assert not env.done.any() and not env.reward.any()
    assert all(env._h.debug_state(i)[0].steps == 0 for i in range(0, n, 7))
    assert int((rec1 != rec0).any(1).sum()) == n
    env.reset_envs(mask=torch.ones(n, dtype=torch.uint8, device=env.device))
    rec2 = env.save_state()
    hw2 = 2 * env.height * env.width
    assert int((rec2[:, 64:64 + hw2] != rec1[:, 64:64 + hw2]).any(1).sum()) >= 60   # the cell section: another level
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------
# 7. every observation mode after a partial reset
# ---------------------------------------------------------------------------------------------
def test_every_observation_mode(goldens):
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv
    from rogue_gym.envs.rogue_env import DungeonType, ImageSetting, StatusFlag

    cfg, n = goldens["configs"]["mini"], 64
    cfgs = seeded(cfg, range(40, 40 + n))
    gray, sym = ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False)
    plain_gray, plain_sym = HipVecRogueEnv(cfgs, image_setting=gray), HipVecRogueEnv(cfgs, image_setting=sym)
    full = HipVecRogueEnv(cfgs, image_setting=gray)
    bound = HipVecRogueEnv(cfgs, image_setting=gray, persistent_obs=True)
    crop = HipVecRogueEnv(cfgs, image_setting=gray, crop=2)
    bf16 = HipVecRogueEnv(cfgs, image_setting=gray, obs_dtype=torch.bfloat16)
    ids = HipVecRogueEnv(cfgs, image_setting=sym, symbol_ids=True)
    envs = [plain_gray, plain_sym, full, bound, crop, bf16, ids]
    rng = np.random.RandomState(7)

    def check(where):
        g, s = plain_gray.obs, plain_sym.obs
        assert torch.equal(full.obs, g), where
        assert torch.equal(bound.obs, g), where
        assert torch.equal(bf16.obs, g.to(torch.bfloat16)), where
        assert torch.equal(ids.obs[:, 0], s.argmax(1).to(torch.uint8)), where
        gn, cen, win = g.cpu().numpy(), crop.crop_center.cpu().numpy(), crop.obs.cpu().numpy()
        for i in range(n):
            assert np.array_equal(win[i], crop_window(gn[i], int(cen[i, 0]), int(cen[i, 1]), 2, 2, 0, 1, False)), (where, i)

    check("t=0")
    for t in range(30):
        k = ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)]
        for e in envs:
            e.step_keys(torch.as_tensor(k, device=e.device))
        if t % 5 == 4:
            chosen = [int(i) for i in np.nonzero(rng.randint(0, 3, n) == 0)[0]]
            for j, e in enumerate(envs):  # (the plain twins by ids, the others by mask and ids in turn)
                if j < 2 or (j + t) % 2:
                    e.reset_envs(env_ids=chosen)
                else:
                    e.reset_envs(mask=mask_of(e, chosen))
        check("t=%d" % (t + 1))
    for e in envs:
        e.check_errors()
        e.close()


# ---------------------------------------------------------------------------------------------
# 8. the key log
# ---------------------------------------------------------------------------------------------
def test_key_log_is_rolled(goldens):
    cfg, n = goldens["configs"]["mini"], 40
    env = vec_env(cfg, range(n))
    env.enable_history(64)
    rng = np.random.RandomState(8)
    for _ in range(20):
        env.step_keys(random_keys(env, rng, ACTION_KEYS))
    run = {i: env.history_keys(i) for i in (3, 4, 39)}
    prev = {i: env.history_keys(i, previous=True) for i in (3, 4, 39)}
    assert len(run[3]) > 0 and len(run[39]) > 0
    env.reset_envs(env_ids=[39, 3])
    for i in (3, 39):
        assert env.history_keys(i) == b"" and env.history_keys(i, previous=True) == run[i]
    assert env.history_keys(4) == run[4] and env.history_keys(4, previous=True) == prev[4]
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------
# 9. HipVecFirstFloor against FirstFloorEnv(RogueEnv)
# ---------------------------------------------------------------------------------------------
FIRST_FLOOR_SEEDS = [21, 39, 41, 56, 57, 64, 100, 23]
FIRST_FLOOR_STEPS = 120


def first_floor_keys(cfg, seed, step_fn, screen_fn):
    """The stair-seeking key sequence of one single env, recorded while it is played through step_fn(key) -> done; it ends with the first `done`."""
    rng = np.random.RandomState(1000 + seed)
    keys = []
    for _ in range(FIRST_FLOOR_STEPS):
        keys.append(seeker_key(screen_fn(), rng))
        if step_fn(keys[-1]):
            break
    return keys


def test_first_floor_wrapper(goldens):
    """On the CPU oracle the recorded sequences reach level 2 for 7 of the 8 seeds, after 7 to 14 keys; seed 23 dies on level 1 at its 26th key (the
    episode then ends the ordinary way, on both sides)."""
    torch = torch_mod()
    from rogue_gym.envs import FirstFloorEnv, HipVecFirstFloor, RogueEnv

    cfg = goldens["configs"]["mini"]
    singles = []
    for s in FIRST_FLOOR_SEEDS:
        env = FirstFloorEnv(RogueEnv(config_dict=dict(cfg, seed=s), max_steps=1000), stair_reward=50.0)
        trace = []

        def step_fn(key, env=env, trace=trace):
            _, reward, done, _ = env.step(chr(key))
            trace.append((float(reward), bool(done)))
            return done

        keys = first_floor_keys(cfg, s, step_fn, lambda env=env: np.array([list(r.encode()) for r in env.unwrapped.get_dungeon()], np.uint8))
        singles.append((keys, trace, env.unwrapped.result.dungeon_level))
    assert sum(1 for _, trace, level in singles if trace[-1][1] and level == 2) >= 6
    vec = HipVecFirstFloor(seeded(cfg, FIRST_FLOOR_SEEDS), max_steps=1000, stair_reward=50.0)
    longest = max(len(k) for k, _, _ in singles)
    for t in range(longest + 1):
        # a lane whose sequence is over searches on the spot ('s'): the step after its `done` must pay nothing and report level 1
        k = np.array([ks[t] if t < len(ks) else ord("s") for ks, _, _ in singles], np.uint8)
        _, reward, done = vec.step_keys(torch.as_tensor(k, device=vec.device))
        reward, done, level = reward.cpu().numpy(), done.cpu().numpy(), vec.status[:, 0].cpu().numpy()
        for i, (ks, trace, _) in enumerate(singles):
            if t < len(ks):
                assert (float(reward[i]), bool(done[i])) == trace[t], (i, t, reward[i], done[i], trace[t])
                if trace[t][1] and singles[i][2] == 2:
                    assert reward[i] >= 50.0 and level[i] == 1, (i, t, reward[i], level[i])   # the bonus of the descent, the post-reset state
            elif t == len(ks) and trace[-1][1]:
                assert reward[i] == 0.0 and not done[i] and level[i] == 1, (i, t, reward[i], done[i], level[i])
    vec.check_errors()
    vec.close()


# ---------------------------------------------------------------------------------------------
# 10. refusals: each names its argument and launches nothing
# ---------------------------------------------------------------------------------------------
def test_refusals(goldens):
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv

    cfg, n = goldens["configs"]["mini"], 48
    env = vec_env(cfg, range(n))
    rng = np.random.RandomState(10)
    for _ in range(10):
        env.step_keys(random_keys(env, rng))
    before = env.save_state().clone()
    L, h = env._h.L, env._h.h

    def refused(what, match, fn, exc=RuntimeError):
        with pytest.raises(exc, match=match):
            fn()
        assert torch.equal(env.save_state(), before), "%s: a refused call changed the state" % what

    refused("id out of range", "env_ids", lambda: env.reset_envs(env_ids=[3, n]))
    refused("negative id", "env_ids", lambda: env.reset_envs(env_ids=[-1]))
    refused("duplicate ids", "env_ids.*twice", lambda: env._h.check(L.rg_reset_envs(h, np.array([7, 9, 7], np.int32).ctypes.data, 3, 0)))
    refused("duplicate device ids", "env_ids", lambda: env.reset_envs(env_ids=torch.tensor([7, 7], device=env.device)), ValueError)
    refused("null mask", "mask_dev", lambda: env._h.check(L.rg_reset_mask(h, None)))
    refused("mask dtype", "mask", lambda: env.reset_envs(mask=torch.zeros(n, dtype=torch.int32, device=env.device)), ValueError)
    refused("mask device", "mask", lambda: env.reset_envs(mask=torch.zeros(n, dtype=torch.bool)), ValueError)
    refused("mask length", "mask", lambda: env.reset_envs(mask=torch.zeros(n + 1, dtype=torch.bool, device=env.device)), ValueError)
    refused("both", "env_ids and mask", lambda: env.reset_envs(env_ids=[1], mask=torch.zeros(n, dtype=torch.bool, device=env.device)), ValueError)
    refused("neither", "env_ids and mask", lambda: env.reset_envs(), ValueError)
    refused("seeds with a mask", "seeds", lambda: env.reset_envs(mask=torch.zeros(n, dtype=torch.bool, device=env.device), seeds=[1]), ValueError)
    refused("seed count", "seeds", lambda: env.reset_envs(env_ids=[1, 2], seeds=[1]), ValueError)
    refused("seed id out of range", "env_ids", lambda: env._h.check(L.rg_seed_envs(h, np.array([n], np.int32).ctypes.data, (C.c_uint64 * 1)(1), None, 1)))
    # an empty list is a valid no-op, and a device-side id out of range is skipped and reported
    env.reset_envs(env_ids=[])
    env.reset_envs(env_ids=torch.zeros(0, dtype=torch.int32, device=env.device))
    assert torch.equal(env.save_state(), before)
    bad = torch.tensor([2, n + 5, -3], dtype=torch.int32, device=env.device)
    env._h.check(L.rg_reset_envs(h, C.c_void_p(bad.data_ptr()), 3, 1))
    after = env.save_state()
    keep = [i for i in range(n) if i != 2]
    assert torch.equal(after[keep], before[keep]) and not torch.equal(after[2], before[2])
    with pytest.raises(RuntimeError):
        env.check_errors()
    env.step_keys(random_keys(env, rng))
    env.check_errors()
    env.close()
    # a handle with config groups
    other = dict(goldens["configs"]["mini"], seed=1, enemies={"enemies": []})
    mixed = HipVecRogueEnv([dict(cfg, seed=1), other])
    for fn in (lambda: mixed.reset_envs(env_ids=[0]), lambda: mixed.reset_envs(mask=torch.zeros(2, dtype=torch.bool, device=mixed.device)),
               lambda: mixed.reset_envs(env_ids=[0], seeds=[3])):
        with pytest.raises(RuntimeError, match="config groups"):
            fn()
    mixed.close()
