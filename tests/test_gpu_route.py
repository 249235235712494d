"""rg_route on the GPU (rogue-gym_amd/csrc/rg_route.hip k_route): mode 0 against rg_path, every (goals, fallback, mode) against the host entry on states
reached by play, in lock-step with the CPU oracle following the device's own keys, a batch of three sizes, no side effects, the refusals and the Python
surface.  The grids play does not reach -- secrets and holes in the map at word seams, borders and group boundaries -- are tests/test_gpu_route_grids.py's."""
import ctypes as C
import json

import numpy as np
import pytest

import mask_util as mu
import path_util as pu
import route_util as ru
from parity_util import HipBatch, compare_internal, compare_mirrors, make_oracles
from path_util import path_call, ptr
from route_util import GOAL_CELL, GOAL_FRONTIER, GOAL_GOLD, GOAL_STAIRS, KNOWN, NO_TIER, SECRETS, route_call
from test_gpu_path import env_states, grid_cfg, torch_mod

pytestmark = pytest.mark.gpu

NO_ENEMIES = {"enemies": []}
EXPLORE = (GOAL_STAIRS, GOAL_FRONTIER, KNOWN)
WITH_SECRETS = (GOAL_STAIRS, 0, SECRETS)
# 70 envs each: a ragged last wave at four, two and one env per wave
SHAPES = {
    "32x16": lambda g: dict(g["configs"]["mini"], enemies=mu.ENEMIES),
    "80x24": lambda g: mu.DEFAULT_SIZE,
    "160x48": lambda g: grid_cfg(160, 48, 4, 4),
    "50x21": lambda g: grid_cfg(50, 21, 3, 2),
    "64x16": lambda g: grid_cfg(64, 16, 2, 2),
}


@pytest.fixture(scope="module")
def lib():
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def check_host(lib, states, combo, cells, got, where):
    goals, fb, mode = combo
    d, k, t = got
    for i, (grid, px, py, dead) in enumerate(states):
        cell = (-1, -1) if cells is None else (int(cells[i][0]), int(cells[i][1]))
        _, hd_, hk, ht = ru.host(lib, grid, px, py, goals, fb, mode, dead, cell, want=(False, True, True, True))
        assert (d[i], k[i], t[i]) == (hd_, hk, ht), "%s goals %d fallback %d mode %d env %d player (%d, %d) cell %s: kernel dist %d key %r tier %d, host entry dist %d key %r tier %d" % (
            where, goals, fb, mode, i, px, py, cell, d[i], chr(k[i]), t[i], hd_, chr(hk), ht)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_rg_path_and_the_host_entry(goldens, lib, shape):
    """70 envs after 40 random steps.  Mode 0 without fallback equals rg_path, keys and distances, for every goal word of rg_path; every legal (goals,
    fallback, mode) -- 592 -- equals the host entry on dist, key and tier, with the bytes behind the last env left alone (route_call)."""
    torch_mod()
    n = 70
    hip = HipBatch(SHAPES[shape](goldens), [7300 + i for i in range(n)], max_steps=1000, auto_reset=True)
    hd = hip.h
    table = mu.key_table(3, 40, n)
    for t in range(40):
        hip.step(table[t])
    hip.sync()
    states = env_states(hd)
    rng = np.random.RandomState(len(shape))
    cells = np.stack([rng.randint(-1, hd.height + 1, n), rng.randint(-1, hd.width + 1, n)], axis=1).astype(np.int32)
    for i in range(0, n, 5):  # ... now and then the player's own cell
        cells[i] = (states[i][2], states[i][1])
    for goals in range(1, 8):
        cc = cells if goals & GOAL_CELL else None
        _, pd, pk = path_call(hd, goals, cc, field=False)
        d, k, t = route_call(hd, goals, 0, 0, cc)
        assert np.array_equal(d, pd) and np.array_equal(k, pk) and np.array_equal(t, np.where(pd < 0, NO_TIER, 0)), "%s goals %d: mode 0 vs rg_path" % (shape, goals)
    seen, tiers = set(), set()
    for combo in ru.combos():
        cc = cells if (combo[0] | combo[1]) & GOAL_CELL else None
        got = route_call(hd, combo[0], combo[1], combo[2], cc)
        check_host(lib, states, combo, cc, got, shape)
        seen |= set(bytes(got[1]).decode())
        tiers |= set(got[2].tolist())
    assert tiers == {0, 1, NO_TIER} and len(seen & set("kjhlyubn")) >= 4 and "s" in seen, (seen, tiers)


@pytest.mark.parametrize("teacher", [EXPLORE, WITH_SECRETS], ids=["explore", "stairs+secrets"])
@pytest.mark.parametrize("size", ["mini", "80x24"])
def test_lock_step_with_the_oracle(goldens, lib, size, teacher):
    """256 mini envs / 64 envs of 80 x 24 without enemies, 80 steps: both engines play the DEVICE's keys.  Before every step the device's dist, key and tier
    equal the host entry's on the ORACLE's state; mirrors match every 8th step and the internal state every 16th and at the end."""
    torch = torch_mod()
    cfg, n = (dict(goldens["configs"]["mini"], enemies=NO_ENEMIES), 256) if size == "mini" else ({"width": 80, "height": 24, "enemies": NO_ENEMIES}, 64)
    seeds = [8100 + i for i in range(n)]
    hip = HipBatch(cfg, seeds, max_steps=1000, auto_reset=True)
    hd = hip.h
    oracles = make_oracles(cfg, seeds, max_steps=1000)
    dev = "cuda:%d" % hd.device
    d, k, tr = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    descents = searches = 0
    for t in range(80):
        hd.check(hd.L.rg_route(hd.h, teacher[0], teacher[1], teacher[2], None, ptr(d), ptr(k), ptr(tr)))
        hip.sync()
        dv, kv, tv = d.cpu().numpy(), k.cpu().numpy(), tr.cpu().numpy()
        for i, o in enumerate(oracles):
            sc = o.scalars()
            _, hd_, hk, ht = ru.host(lib, mu.cell_words(*o.grid()), sc["px"], sc["py"], teacher[0], teacher[1], teacher[2], int(o.flags()["dead"]), want=(False, True, True, True))
            assert (dv[i], kv[i], tv[i]) == (hd_, hk, ht), "t=%d env %d: device dist %d key %r tier %d, host entry on the oracle's state dist %d key %r tier %d" % (
                t, i, dv[i], chr(kv[i]), tv[i], hd_, chr(hk), ht)
            o.step_autoreset(int(kv[i]))
        descents += int((kv == ord(">")).sum())
        searches += int((kv == ord("s")).sum())
        hd.check(hd.L.rg_step(hd.h, ptr(k), 1))
        if (t + 1) % 8 == 0:
            compare_mirrors(hip, oracles, "t=%d" % (t + 1))
        if (t + 1) % 16 == 0:
            compare_internal(hip, oracles, range(n), "t=%d" % (t + 1))
    hip.sync()
    print("%s %s: %d descents, %d searches in %d rows" % (size, teacher, descents, searches, 80 * n))
    assert descents >= n // 8 and searches > 0


def test_a_batch_of_three_sizes(goldens, lib):
    """96 envs cycling mini / 80 x 24 / 48 x 20: three config groups of different sizes; every group's answers land in the caller's env order (ext), and
    the cells of RG_GOAL_CELL are read in that order."""
    torch_mod()
    from rogue_gym_python import _rogue_gym as inner
    enemies = {"enemies": list(range(10))}
    shapes = [dict(goldens["configs"]["mini"], enemies=enemies), {"width": 80, "height": 24, "enemies": enemies},
              {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": enemies}]
    n, steps = 96, 24
    cfgs = [dict(shapes[i % 3], seed=6300 + i) for i in range(n)]
    dims = [(c["height"], c["width"]) for c in cfgs]
    hd = inner._Handle([json.dumps(c) for c in cfgs], 1000, auto_reset=True)
    assert hd.mixed_sizes
    rng = np.random.RandomState(4)
    for t in range(steps + 1):
        if t % 8 == 0:
            states = env_states(hd, dims)
            cells = np.stack([rng.randint(0, 16, n), rng.randint(0, 32, n)], axis=1).astype(np.int32)
            for combo, cc in ((EXPLORE, None), (WITH_SECRETS, None), ((GOAL_CELL | GOAL_GOLD, GOAL_FRONTIER, KNOWN | SECRETS), cells), ((GOAL_GOLD, GOAL_CELL, 0), cells)):
                check_host(lib, states, combo, cc, route_call(hd, combo[0], combo[1], combo[2], cc), "mixed t=%d" % t)
        if t < steps:
            _, teach, _ = route_call(hd, *EXPLORE)
            hd.check(hd.L.rg_step(hd.h, np.ascontiguousarray(teach).ctypes.data, 0))
    hd.check(hd.L.rg_sync(hd.h))
    kv, dv, tv = hd.route_keys("stairs", "frontier", known=True)  # the value form serves the groups too
    d1, k1, t1 = route_call(hd, *EXPLORE)
    assert np.array_equal(kv, k1) and np.array_equal(dv, d1) and np.array_equal(tv, t1)
    hd.close()


def test_guides_and_route_have_no_side_effects(goldens):
    """Twin envs on the same seeds and keys, one plain, one with guide="explore" and a route() call every step, one with guide_secrets: the same observations,
    rewards and dones at every step, the same mirrors, flag words, status and state records (RNG words included) at the end."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    n, steps = 128, 40
    cfgs = [dict(goldens["configs"]["mini"], seed=800 + i) for i in range(n)]
    setting = ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, True)
    table = torch.as_tensor(mu.key_table(7, steps, n))
    trace = []
    for kw in ({}, dict(guide="explore"), dict(guide="stairs+gold", guide_secrets=True)):
        env = HipVecRogueEnv(cfgs, max_steps=30, image_setting=setting, **kw)
        per_step = [env.obs.cpu().clone()]
        for t in range(steps):
            if kw:
                env.route("gold", "frontier", secrets=True, known=True)
            obs, reward, done = env.step_keys(table[t].to(env.device).contiguous())
            per_step.append((obs.cpu().clone(), reward.cpu().clone(), done.cpu().clone()))
        end = (env.screen.cpu().clone(), env.flags.cpu().clone(), env.status.cpu().clone(), env.save_state().cpu())
        env.check_errors()
        env.close()
        trace.append((per_step, end))
    (a_steps, a_end) = trace[0]
    for b_steps, b_end in trace[1:]:
        assert torch.equal(a_steps[0], b_steps[0])
        for t in range(1, steps + 1):
            for x, y, what in zip(a_steps[t], b_steps[t], ("obs", "reward", "done")):
                assert torch.equal(x, y), "t=%d %s differs" % (t, what)
        for x, y, what in zip(a_end, b_end, ("screen", "flags", "status", "state records")):
            assert torch.equal(x, y), what + " differs at the end"


def test_refusals_launch_nothing(goldens):
    torch = torch_mod()
    hip = HipBatch(goldens["configs"]["mini"], [1 + i for i in range(70)], max_steps=60, auto_reset=True)
    hd, L = hip.h, hip.h.L
    dev = "cuda:%d" % hd.device
    d = torch.full((70,), -7, dtype=torch.int32, device=dev)
    k = torch.full((70,), 0xAA, dtype=torch.uint8, device=dev)
    t = torch.full((70,), 0xAA, dtype=torch.uint8, device=dev)
    c = torch.zeros((70, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    dp, kp, tp, cp = d.data_ptr(), k.data_ptr(), t.data_ptr(), c.data_ptr()
    cases = [((0, 0, 0, None, dp, kp, tp), ("goals", "got 0")), ((16, 0, 0, cp, dp, kp, tp), ("goals", "got 16")), ((0x10001, 0, 0, cp, dp, kp, tp), ("goals",)),
             ((1, 16, 0, cp, dp, kp, tp), ("fallback_goals", "got 16")), ((1, 0, 4, cp, dp, kp, tp), ("mode", "got 4")), ((1, 0, 0x80000001, cp, dp, kp, tp), ("mode",)),
             ((8, 0, 0, None, dp, kp, tp), ("RG_GOAL_FRONTIER", "RG_ROUTE_KNOWN", "goals")), ((1, 8, SECRETS, None, dp, kp, tp), ("RG_GOAL_FRONTIER", "RG_ROUTE_KNOWN", "fallback_goals")),
             ((4, 0, 0, None, dp, kp, tp), ("cells_dev", "RG_GOAL_CELL", "goals")), ((1, 5, 0, None, dp, None, None), ("cells_dev", "fallback_goals")),
             ((1, 0, 0, None, None, None, None), ("dist_dev", "key_dev", "tier_dev"))]
    for (goals, fb, mode, cc, dd, kk, tt), words in cases:
        rc = L.rg_route(hd.h, goals, fb, mode, *(None if p is None else C.c_void_p(p) for p in (cc, dd, kk, tt)))
        msg = L.rg_last_error(hd.h).decode()
        assert rc != 0 and "rg_route" in msg and all(w in msg for w in words), (goals, fb, mode, msg)
        hip.sync()
        assert bool((d == -7).all()) and bool((k == 0xAA).all()) and bool((t == 0xAA).all()), "a refused call wrote: " + msg
    # and the same buffers are written by a call that is not refused; any subset of the outputs
    assert L.rg_route(hd.h, 1, 8, KNOWN, None, C.c_void_p(dp), None, None) == 0
    hip.sync()
    assert bool((d >= -1).all()) and bool((k == 0xAA).all()) and bool((t == 0xAA).all())
    assert L.rg_route(hd.h, 1, 8, KNOWN, None, None, C.c_void_p(kp), C.c_void_p(tp)) == 0
    hip.sync()
    assert bool((k != 0xAA).all()) and bool(((t == 0) | (t == 1) | (t == NO_TIER)).all())


class Counting:
    """A library whose calls of rg_path and rg_route are counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {"rg_path": 0, "rg_route": 0}

    def __getattr__(self, name):
        if name in self.calls:
            self.calls[name] += 1
        return getattr(self._lib, name)


def test_python_surface(goldens):
    torch = torch_mod()
    from rogue_gym.envs import ParallelRogueEnv, RogueEnv
    from rogue_gym.envs.device import HipVecRogueEnv

    n = 72
    cfg = dict(goldens["configs"]["mini"], enemies=NO_ENEMIES)
    cfgs = [dict(cfg, seed=9100 + i) for i in range(n)]
    for kw, args in ((dict(guide="explore"), dict(goal="stairs", fallback="frontier", known=True)),
                     (dict(guide="stairs+gold", guide_secrets=True), dict(goal="stairs+gold", secrets=True))):
        env = HipVecRogueEnv(cfgs, max_steps=1000, **kw)
        explore = kw["guide"] == "explore"
        assert (env.guide_tier is not None) == explore and env.guide_keys.dtype == torch.uint8 and env.guide_dist.dtype == torch.int32
        if explore:
            assert env.guide_tier.dtype == torch.uint8 and tuple(env.guide_tier.shape) == (n,)

        def fresh(where):
            keys, dist, tier = env.route(**args)
            assert torch.equal(env.guide_keys, keys) and torch.equal(env.guide_dist, dist) and (not explore or torch.equal(env.guide_tier, tier)), where
            return keys.clone()

        at_reset = fresh("constructor")
        for _ in range(12):
            env.step_keys(env.guide_keys.clone())
        after_steps = fresh("after step_keys")
        assert not torch.equal(after_steps, at_reset)
        env.step(torch.zeros(n, dtype=torch.int64, device=env.device))
        fresh("after step")
        records, saved = env.save_state(), env.guide_keys.clone()
        env.reset_envs(env_ids=list(range(1, n, 2)))
        now = fresh("after reset_envs")
        assert torch.equal(now[1::2], at_reset[1::2]) and torch.equal(now[0::2], saved[0::2])
        env.reset_envs(mask=torch.arange(n, device=env.device) % 3 == 0)
        fresh("after reset_envs(mask)")
        env.load_state(records)
        assert torch.equal(fresh("after load_state"), saved)
        env.clone_state([0] * n, list(range(n)))
        assert bool((fresh("after clone_state") == saved[0]).all())
        env.reset()
        assert torch.equal(fresh("after reset"), at_reset)
        env._h.L = counted = Counting(env._h.L)  # the guides of this change go through rg_route alone
        env.step_keys(env.guide_keys.clone())
        assert counted.calls == {"rg_path": 0, "rg_route": 1}
        env._h.L = counted._lib
        env.reset()
        if explore:
            # mode 0 of route() is path(); a caller's cells; the refusals of the arguments
            kp, dp, _ = env.path("stairs+gold")
            kr, dr, tr = env.route("stairs+gold")
            assert torch.equal(kp, kr) and torch.equal(dp, dr) and torch.equal(tr == 255, dp < 0)
            cells = torch.tensor([[3, 5]] * n, dtype=torch.int32, device=env.device)
            kc, dc, tc = env.route(None, cells=cells, secrets=True)
            kq, dq, _ = env.path(None, cells=cells)
            assert bool(((dq < 0) | ((dc >= 0) & (dc <= dq))).all()) and bool((dc[3::7] >= -1).all())  # (a secret can only shorten the way)
            for bad in (dict(goal="amulet"), dict(goal=None), dict(goal=3), dict(goal="frontier"), dict(goal="stairs", fallback="frontier"), dict(goal="stairs", fallback="amulet"),
                        dict(cells=cells.long()), dict(cells=cells[:5]), dict(cells=cells.cpu())):
                with pytest.raises(ValueError):
                    env.route(**bad)
            # the value forms agree with the tensor form
            penv = ParallelRogueEnv(cfgs[:8], max_steps=1000)
            for a in (args, dict(goal="gold", fallback="stairs", secrets=True), dict(goal="stairs", secrets=True, known=True)):
                keys, dist, tier = penv.route_keys(**a)
                tk, td, tt = env.route(**a)
                assert keys.dtype == np.uint8 and dist.dtype == np.int32 and tier.dtype == np.uint8
                assert np.array_equal(keys, tk[:8].cpu().numpy()) and np.array_equal(dist, td[:8].cpu().numpy()) and np.array_equal(tier, tt[:8].cpu().numpy()), a
            with pytest.raises(ValueError):
                penv.route_keys("frontier")
            penv.close()
            one = RogueEnv(config_dict=cfg, max_steps=1000, seed=9100)
            key, dist, tier = one.route_key("stairs", "frontier", known=True)
            assert key == chr(int(env.guide_keys[0])) and dist == (None if int(env.guide_dist[0]) < 0 else int(env.guide_dist[0])) and tier == (None if int(env.guide_tier[0]) == 255 else int(env.guide_tier[0]))
            assert key in RogueEnv.ACTIONS
            for _ in range(400):  # the single env explores its way down the first stairs
                key, dist, tier = one.route_key("stairs", "frontier", known=True)
                one.step(key)
                if key == ">":
                    break
            assert key == ">" and dist == 0 and tier == 0
        env.check_errors()
        env.close()
    # guide=None launches nothing; the default guides still call rg_path and never rg_route; the arguments' refusals
    for kw, want in ((dict(), {"rg_path": 0, "rg_route": 0}), (dict(guide="stairs"), {"rg_path": 4, "rg_route": 0})):
        plain = HipVecRogueEnv(cfgs, max_steps=1000, **kw)
        assert plain.guide_tier is None and not plain.guide_secrets
        plain._h.L = counted = Counting(plain._h.L)
        plain.reset()
        plain.step(torch.zeros(n, dtype=torch.int64, device=plain.device))
        plain.reset_envs(env_ids=[0, 5])
        plain.load_state(plain.save_state())
        assert counted.calls == want, (kw, counted.calls)
        plain.route("stairs", secrets=True)
        assert counted.calls == dict(want, rg_route=1)
        plain._h.L = counted._lib
        plain.close()
    for bad in ("amulet", "", "stairs,gold", 3, True, b"stairs", "frontier"):
        with pytest.raises(ValueError, match="guide"):
            HipVecRogueEnv(cfgs[:2], guide=bad)
    with pytest.raises(ValueError, match="guide_secrets"):
        HipVecRogueEnv(cfgs[:2], guide_secrets=True)
