"""rg_path on the GPU (rogue-gym_amd/csrc/rg_path.hip k_path): field, distance and teacher key against the host entry and the numpy rule on states reached by
play, config groups and mixed sizes, no side effects, the teacher judged by what the step then does, the Python surface and the refusals.  Play reaches
seven grid shapes and walks of about a hundred moves; every wave shape, row-word count and store alignment, walkable borders and the high distance planes
are reached by tests/test_gpu_constructed_grids.py, on grids of its own making."""
import ctypes as C
import json

import numpy as np
import pytest

import mask_util as mu
import path_util as pu
from parity_util import HipBatch
from path_util import GOAL_CELL, GOAL_GOLD, GOAL_STAIRS, path_call, ptr

pytestmark = pytest.mark.gpu


def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def grid_cfg(w, h, rx, ry):
    return {"width": w, "height": h, "dungeon": {"style": "rogue", "room_num_x": rx, "room_num_y": ry, "min_room_size": {"x": 4, "y": 4}}}


def env_states(hd, dims=None):
    """[(cells u16 [H][W], px, py, dead)] of every env, from rg_debug_fetch and the flag words."""
    from rogue_gym_python._rogue_gym import RgDebugState
    flags = np.empty(hd.n, np.uint32)
    hd.check(hd.L.rg_fetch_states(hd.h, None, None, None, flags.ctypes.data))
    out = []
    for i in range(hd.n):
        h, w = (hd.height, hd.width) if dims is None else dims[i]
        st, cells = RgDebugState(), np.empty((h, w), np.uint16)
        hd.check(hd.L.rg_debug_fetch(hd.h, i, C.byref(st), cells.ctypes.data))
        out.append((cells, int(st.px), int(st.py), int((flags[i] & 2) != 0)))
    return out


def check_all(lib, hd, states, goals, cells, got, where, numpy_too=True, graphs=None):
    """kernel == host entry (== numpy rule) for every env."""
    f, d, k = got
    for i, (grid, px, py, dead) in enumerate(states):
        cell = (-1, -1) if cells is None else (int(cells[i][0]), int(cells[i][1]))
        hf, hd_, hk = pu.host(lib, grid, px, py, goals, dead, cell)
        tag = "%s goals %d env %d player (%d, %d) cell %s" % (where, goals, i, px, py, cell)
        assert d[i] == hd_ and k[i] == hk, "%s: kernel dist %d key %r, host entry dist %d key %r" % (tag, d[i], chr(k[i]), hd_, chr(hk))
        if f is not None and not np.array_equal(f[i], hf):
            bad = np.argwhere(f[i] != hf)
            raise AssertionError("%s: %d field cells differ, first (y, x) = %s: kernel %d, host entry %d" % (tag, len(bad), tuple(bad[0]), f[i][tuple(bad[0])], hf[tuple(bad[0])]))
        if numpy_too:
            ef, ed, ek = graphs[i].answer(px, py, dead, goals, cell)
            assert np.array_equal(hf, ef) and hd_ == ed and hk == ek, tag + ": host entry vs numpy rule"


SHAPES = {
    "mini": (lambda g: dict(g["configs"]["mini"], enemies=mu.ENEMIES), 135),  # four envs per wave; the last wave holds three
    "80x24": (lambda g: mu.DEFAULT_SIZE, 71),                                 # two envs per wave; the last wave is half full
    "160x48": (lambda g: grid_cfg(160, 48, 4, 4), 9),                         # one env per wave, widest rows (five words)
    "40x20": (lambda g: grid_cfg(40, 20, 2, 2), 13),                          # 33..64 columns (two words)
    "50x21": (lambda g: grid_cfg(50, 21, 3, 2), 13),                          # env bases of the field not 16-byte aligned, rows loaded cell by cell
    "32x48": (lambda g: grid_cfg(32, 48, 1, 3), 5),                           # tallest grid
    "64x16": (lambda g: grid_cfg(64, 16, 2, 2), 7),
}


@pytest.fixture(scope="module")
def lib():
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_host_entry_equals_numpy(goldens, lib, shape):
    """n envs x 40 steps; half the envs follow the teacher (stairs + gold), half the uniform policy.  Field, distance and key for ALL envs every 4th step and
    after the last, for goals 1, 2, 3, 4 + a random cell (outside the grid now and then) and 5 + that cell; and the keys-only pass against the field pass."""
    torch_mod()
    make, n = SHAPES[shape]
    cfg = make(goldens)
    hip = HipBatch(cfg, [7000 + i for i in range(n)], max_steps=1000, auto_reset=True)
    hd = hip.h
    H, W = hd.height, hd.width
    rng = np.random.RandomState(len(shape) + n)
    table = mu.key_table(2, 40, n)
    seen, far, unreachable = set(), 0, 0
    for t in range(41):
        if t % 4 == 0 or t == 40:
            states = env_states(hd)
            graphs = [pu.Graph(s[0]) for s in states]
            cells = np.stack([rng.randint(-1, H + 1, n), rng.randint(-1, W + 1, n)], axis=1).astype(np.int32)
            own = rng.rand(n) < 0.2  # ... and now and then the player's own cell
            for i in np.flatnonzero(own):
                cells[i] = (states[i][2], states[i][1])
            for goals, cc in ((1, None), (2, None), (3, None), (GOAL_CELL, cells), (GOAL_CELL | GOAL_STAIRS, cells)):
                got = path_call(hd, goals, cc)
                check_all(lib, hd, states, goals, cc, got, "%s t=%d" % (shape, t), True, graphs)
                _, d2, k2 = path_call(hd, goals, cc, field=False)  # the pass that stops at the player's cell
                assert np.array_equal(d2, got[1]) and np.array_equal(k2, got[2]), "%s t=%d goals %d: keys-only pass vs field pass" % (shape, t, goals)
                seen |= set(bytes(got[2]).decode())
                far = max(far, int(got[1].max()))
                unreachable += int((got[1] < 0).sum())
        if t < 40:
            _, _, teach = path_call(hd, GOAL_STAIRS | GOAL_GOLD, field=False)
            hip.step(np.where(np.arange(n) % 2 == 0, teach, table[t]).astype(np.uint8))
    hip.sync()
    print("%s: keys seen %s, largest distance %d, unreachable answers %d" % (shape, "".join(sorted(seen)), far, unreachable))
    assert far >= 10 and len(seen & set("kjhlyubn")) >= 4, (seen, far)


def test_groups_and_mixed_sizes(goldens, lib):
    """96 envs cycling mini / 80 x 24 / 48 x 20: three config groups of different sizes (four, two and two envs per wave), every group's answers scattered
    into the caller's env order (ext), the cells of RG_GOAL_CELL read in that order.  field_dev is refused on such a handle."""
    torch = torch_mod()
    from rogue_gym_python import _rogue_gym as inner

    enemies = {"enemies": list(range(10))}
    shapes = [dict(goldens["configs"]["mini"], enemies=enemies), {"width": 80, "height": 24, "enemies": enemies},
              {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": enemies}]
    n, steps = 96, 40
    cfgs = [dict(shapes[i % 3], seed=6000 + i) for i in range(n)]
    dims = [(c["height"], c["width"]) for c in cfgs]
    hd = inner._Handle([json.dumps(c) for c in cfgs], 1000, auto_reset=True)
    assert hd.mixed_sizes
    table = mu.key_table(1, steps, n)
    rng = np.random.RandomState(3)
    far = 0
    for t in range(steps + 1):
        if t % 4 == 0:
            states = env_states(hd, dims)
            cells = np.stack([rng.randint(0, 16, n), rng.randint(0, 32, n)], axis=1).astype(np.int32)
            for goals, cc in ((1, None), (3, None), (GOAL_CELL | GOAL_GOLD, cells)):
                got = path_call(hd, goals, cc, field=False)
                check_all(lib, hd, states, goals, cc, (None,) + got[1:], "mixed t=%d" % t, False)
                far = max(far, int(got[1].max()))
        if t < steps:
            _, _, teach = path_call(hd, GOAL_STAIRS, field=False)
            keys = np.ascontiguousarray(np.where(np.arange(n) % 2 == 0, teach, table[t]).astype(np.uint8))
            hd.check(hd.L.rg_step(hd.h, keys.ctypes.data, 0))
    hd.check(hd.L.rg_sync(hd.h))
    assert far >= 10
    dev = "cuda:%d" % hd.device
    f = torch.full((n * 80 * 24,), 0x2AAA, dtype=torch.int16, device=dev)
    d = torch.full((n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert hd.L.rg_path(hd.h, 1, None, ptr(f), ptr(d), None) != 0
    msg = hd.L.rg_last_error(hd.h).decode()
    assert "rg_path" in msg and "field_dev" in msg and "config groups" in msg, msg
    hd.check(hd.L.rg_sync(hd.h))
    assert bool((f == 0x2AAA).all()) and bool((d == -7).all())
    kv, dv = hd.path_keys("stairs")  # the value form serves the groups too
    _, d1, k1 = path_call(hd, 1, field=False)
    assert np.array_equal(kv, k1) and np.array_equal(dv, d1)
    hd.close()


def test_guide_and_path_have_no_side_effects(goldens):
    """Twin envs on the same seeds and keys, one with guide="stairs+gold" and a path(field=True) call every step: the same observations, rewards and dones at
    every step, the same mirrors, flag words, status and state records at the end."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    n, steps = 128, 60
    cfgs = [dict(goldens["configs"]["mini"], seed=800 + i) for i in range(n)]
    setting = ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, True)
    table = torch.as_tensor(mu.key_table(7, steps, n))
    trace = []
    for guided in (False, True):
        env = HipVecRogueEnv(cfgs, max_steps=40, image_setting=setting, guide="stairs+gold" if guided else None)
        per_step = [env.obs.cpu().clone()]
        for t in range(steps):
            if guided:
                keys, dist, field = env.path("stairs+gold", field=True)
                assert torch.equal(keys, env.guide_keys) and torch.equal(dist, env.guide_dist)
                assert tuple(field.shape) == (n, 16, 32) and field.dtype == torch.uint16
            obs, reward, done = env.step_keys(table[t].to(env.device).contiguous())
            per_step.append((obs.cpu().clone(), reward.cpu().clone(), done.cpu().clone()))
        end = (env.screen.cpu().clone(), env.flags.cpu().clone(), env.status.cpu().clone(), env.save_state().cpu())
        env.check_errors()
        env.close()
        trace.append((per_step, end))
    (a_steps, a_end), (b_steps, b_end) = trace
    assert torch.equal(a_steps[0], b_steps[0])
    for t in range(1, steps + 1):
        for x, y, what in zip(a_steps[t], b_steps[t], ("obs", "reward", "done")):
            assert torch.equal(x, y), "t=%d %s differs" % (t, what)
    for x, y, what in zip(a_end, b_end, ("screen", "flags", "status", "state records")):
        assert torch.equal(x, y), what + " differs at the end"


def test_teacher_is_judged_by_what_the_step_does(goldens):
    """Without the oracle: 4 096 mini envs without enemies, 60 steps of step_keys(env.guide_keys), torch ops only.  On steps that neither end the episode
    nor change the level, guide_dist falls by exactly 1 from every finite positive value; '>' is issued iff guide_dist == 0, and then the level rises; an
    unreachable env gets 's'.  (On the CPU oracle: 48 833 such moves of 1 024 envs, no exception.)"""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    n, steps = 4096, 60
    cfg = dict(goldens["configs"]["mini"], enemies={"enemies": []})
    env = HipVecRogueEnv([dict(cfg, seed=100 + i) for i in range(n)], max_steps=1000, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), guide="stairs")
    assert env.guide_keys.dtype == torch.uint8 and tuple(env.guide_keys.shape) == (n,) and env.guide_dist.dtype == torch.int32 and tuple(env.guide_dist.shape) == (n,)
    moves = descents = searches = 0
    for t in range(steps):
        keys, dist, level = env.guide_keys.clone(), env.guide_dist.clone(), env.status[:, 0].clone()
        assert bool(((keys == ord(">")) == (dist == 0)).all()), "t=%d: '>' is issued iff the distance is 0" % t
        assert bool((keys[dist < 0] == ord("s")).all()), "t=%d: an unreachable env gets 's'" % t
        assert bool((dist >= -1).all())
        _, _, done = env.step_keys(keys)
        now = env.status[:, 0]
        down = (dist == 0) & ~done
        assert bool((now[down] == level[down] + 1).all()), "t=%d: '>' at distance 0 did not raise the level" % t
        stay = ~done & (now == level) & (dist > 0)
        assert bool((env.guide_dist[stay] == dist[stay] - 1).all()), "t=%d: a teacher move did not bring its env one move closer" % t
        moves, descents, searches = moves + int(stay.sum()), descents + int(down.sum()), searches + int((dist < 0).sum())
    env.check_errors()
    print("teacher moves %d, descents %d, searches %d of %d" % (moves, descents, searches, n * steps))
    assert moves >= n * steps // 2 and descents >= n and searches >= n  # (the CPU oracle: 79 % moves, 6 % descents, 12 % searches)
    env.close()


class Counting:
    """A library whose calls of rg_path are counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        if name == "rg_path":
            self.calls += 1
        return getattr(self._lib, name)


def test_python_surface(goldens):
    torch = torch_mod()
    from rogue_gym.envs import ParallelRogueEnv, RogueEnv
    from rogue_gym.envs.device import HipVecRogueEnv

    n = 72
    cfg = dict(goldens["configs"]["mini"], enemies={"enemies": []})
    cfgs = [dict(cfg, seed=9100 + i) for i in range(n)]
    env = HipVecRogueEnv(cfgs, max_steps=1000, guide="stairs+gold")

    def fresh(where):
        keys, dist, field = env.path("stairs+gold")
        assert field is None
        assert torch.equal(env.guide_keys, keys) and torch.equal(env.guide_dist, dist), where
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
    env.load_state(records)
    assert torch.equal(fresh("after load_state"), saved)
    env.clone_state([0] * n, list(range(n)))
    assert bool((fresh("after clone_state") == saved[0]).all())
    env.reset()
    assert torch.equal(fresh("after reset"), at_reset)
    # the other goal names, a caller's cells, the field; goal=None needs cells
    ks, ds, _ = env.path("stairs")
    kg, dg, fg = env.path("gold", field=True)
    assert fg.dtype == torch.uint16 and tuple(fg.shape) == (n, 16, 32)
    both = torch.where((ds >= 0) & ((dg < 0) | (ds <= dg)), ds, dg)
    assert torch.equal(env.guide_dist, both)  # the nearer of the two goal kinds
    cells = torch.tensor([[3, 5]] * n, dtype=torch.int32, device=env.device)
    kc, dc, fc = env.path(None, cells=cells, field=True)
    fc = fc.view(torch.int16)  # (uint16 tensors carry few operators; 0 is 0 either way)
    assert bool((fc[:, 3, 5] == 0).all()) and bool(((fc == 0).sum(dim=(1, 2)) == 1).all())
    for bad in (dict(goal="amulet"), dict(goal=None), dict(goal=3), dict(cells=cells.long()), dict(cells=cells[:5]), dict(cells=cells.cpu())):
        with pytest.raises(ValueError):
            env.path(**bad)
    env.check_errors()
    # the value forms agree with the tensor form
    penv = ParallelRogueEnv(cfgs[:8], max_steps=1000)
    for goal in ("stairs", "gold", "stairs+gold"):
        keys, dist = penv.path_keys(goal)
        tk, td, _ = env.path(goal)
        assert keys.dtype == np.uint8 and dist.dtype == np.int32 and np.array_equal(keys, tk[:8].cpu().numpy()) and np.array_equal(dist, td[:8].cpu().numpy()), goal
    with pytest.raises(ValueError):
        penv.path_keys("amulet")
    penv.close()
    one = RogueEnv(config_dict=cfg, max_steps=1000, seed=9100)
    key, dist = one.path_key("stairs+gold")
    assert key == chr(int(env.guide_keys[0])) and dist == (None if int(env.guide_dist[0]) < 0 else int(env.guide_dist[0]))
    assert key in RogueEnv.ACTIONS
    for _ in range(200):  # the single env follows its teacher down the first stairs
        key, dist = one.path_key("stairs")
        one.step(key)
        if key == ">":
            break
    assert key == ">" and dist == 0
    env.close()
    # guide=None: no attribute, no launch anywhere; the argument's refusals
    plain = HipVecRogueEnv(cfgs, max_steps=1000)
    assert plain.guide is None and plain.guide_keys is None and plain.guide_dist is None
    plain._h.L = counted = Counting(plain._h.L)
    plain.reset()
    plain.step(torch.zeros(n, dtype=torch.int64, device=plain.device))
    plain.reset_envs(env_ids=[0, 5])
    plain.load_state(plain.save_state())
    assert counted.calls == 0
    plain.path("stairs")
    assert counted.calls == 1
    plain._h.L = counted._lib
    plain.close()
    for bad in ("amulet", "", "stairs,gold", 3, True, b"stairs"):
        with pytest.raises(ValueError, match="guide"):
            HipVecRogueEnv(cfgs[:2], guide=bad)


def test_refusals_launch_nothing(goldens):
    torch = torch_mod()
    hip = HipBatch(goldens["configs"]["mini"], [1 + i for i in range(70)], max_steps=60, auto_reset=True)
    hd, L = hip.h, hip.h.L
    dev = "cuda:%d" % hd.device
    f = torch.full((70 * 512 + 16,), 0x2AAA, dtype=torch.int16, device=dev)
    d = torch.full((70,), -7, dtype=torch.int32, device=dev)
    k = torch.full((70,), 0xAA, dtype=torch.uint8, device=dev)
    c = torch.zeros((70, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fp, dp, kp, cp = f.data_ptr(), d.data_ptr(), k.data_ptr(), c.data_ptr()
    assert fp % 16 == 0
    cases = [((0, None, fp, dp, kp), ("goals", "got 0")), ((8, cp, fp, dp, kp), ("goals", "got 8")), ((0x10001, cp, fp, dp, kp), ("goals",)),
             ((4, None, fp, dp, kp), ("cells_dev", "RG_GOAL_CELL")), ((5, None, None, dp, None), ("cells_dev",)),
             ((1, None, None, None, None), ("field_dev", "dist_dev", "key_dev")), ((1, None, fp + 2, dp, kp), ("field_dev", "16-byte")),
             ((3, None, fp + 8, None, None), ("field_dev", "16-byte"))]
    for (goals, cc, ff, dd, kk), words in cases:
        rc = L.rg_path(hd.h, goals, *(None if p is None else C.c_void_p(p) for p in (cc, ff, dd, kk)))
        msg = L.rg_last_error(hd.h).decode()
        assert rc != 0 and "rg_path" in msg and all(w in msg for w in words), (goals, msg)
        hip.sync()
        assert bool((f == 0x2AAA).all()) and bool((d == -7).all()) and bool((k == 0xAA).all()), "a refused call wrote: " + msg
    # and the same buffers are written by a call that is not refused: exactly the envs' entries, nothing behind them
    assert L.rg_path(hd.h, 1, None, C.c_void_p(fp), C.c_void_p(dp), C.c_void_p(kp)) == 0
    hip.sync()
    assert bool((f[:70 * 512] != 0x2AAA).all()) and bool((f[70 * 512:] == 0x2AAA).all()) and bool((d >= -1).all()) and bool((k != 0xAA).all())
