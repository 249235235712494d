"""rg_action_mask on the GPU (rogue-gym_amd/csrc/rg_action_mask.hip k_action_mask): the mask against the CPU oracle in lock-step -- one group, dead envs,
config groups and mixed sizes --, its meaning checked by what the step then does, custom key lists and the sampled key, no side effects, the refresh
after every state change, the refusals, and the value API.  Shapes: partial waves, more than one wave, the ext scatter, grid edges."""
import ctypes as C

import numpy as np
import pytest

import mask_util as mu
from mask_util import KEYS, RUN_A, RUN_B, RUN_C
from parity_util import HipBatch

pytestmark = pytest.mark.gpu

# (dx, dy) of ACTIONS[1..8] = h j k l n b u y
MOVES = np.array([mu.DIRS[chr(k)] for k in KEYS[1:9]], np.int64)


def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def read(hd, t):
    """Host copy of device tensor `t` through the handle (rg_dev_read waits for the handle's stream)."""
    out = np.empty(tuple(t.shape), np.uint8)
    hd.check(hd.L.rg_dev_read(hd.h, ptr(t), out.ctypes.data, out.nbytes))
    return out


def mask_call(hd, keys=None, mask=True, sample=False, seed=0, draw=0):
    """rg_action_mask on a raw handle into buffers pre-filled with 0xAA -> (rows u8 [n][n_keys] or None, sampled keys u8 [n] or None)."""
    torch = torch_mod()
    nk = len(KEYS) if keys is None else len(keys)
    dev = "cuda:%d" % hd.device
    m = torch.full((hd.n, nk), 0xAA, dtype=torch.uint8, device=dev) if mask else None
    s = torch.full((hd.n,), 0xAA, dtype=torch.uint8, device=dev) if sample else None
    torch.cuda.synchronize()
    hd.check(hd.L.rg_action_mask(hd.h, keys, nk, ptr(m), ptr(s), seed, draw))
    return (None if m is None else read(hd, m)), (None if s is None else read(hd, s))


def assert_rows(got, exp, where):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero((got != exp).any(axis=1))
        raise AssertionError("%s: %d rows differ, first env %d: %s vs %s" % (where, len(bad), bad[0], got[bad[0]], exp[bad[0]]))


@pytest.mark.parametrize("name", ["a", "b"])
def test_mask_equals_the_oracle_in_lockstep(goldens, name):
    """Runs a (136 mini envs: two full waves and 8 lanes) and b (72 of 80 x 24: one wave and 8), default keys, before every step and after the last.
    Floors as in tests/test_action_mask_host.py (the oracle gave 225 / 6 857 / 987 / 317 for a, 29 / 1 834 for b)."""
    torch_mod()
    run = RUN_A if name == "a" else RUN_B
    rows, _, st, table = mu.oracle_run(goldens, run)
    cfg, seeds, _ = mu.run_config(goldens, run)
    hip = HipBatch(cfg, seeds, max_steps=run["max_steps"], auto_reset=True)
    for t in range(run["T"] + 1):
        got, _ = mask_call(hip.h)
        assert_rows(got, rows[t], "run %s t=%d" % (name, t))
        if t < run["T"]:
            hip.step(table[t])
    hip.sync()
    print(st)
    assert st.rows == run["n"] * (run["T"] + 1)
    if name == "a":
        assert st.stairs >= 100 and st.why.get("corner", 0) >= 3000 and st.why.get("out", 0) >= 400 and st.deep >= 100, str(st)
    else:
        assert st.why.get("hidden", 0) >= 10 and st.why.get("corner", 0) >= 800, str(st)


def test_dead_envs_have_no_legal_key(goldens):
    """Run c on a handle without auto-reset: RG_FLAG_DEAD and the all-zero rows agree with the oracle step by step (61 envs die there).  An env once
    dead is fed '.', which raises RG_FLAG_ERR_DEAD: the error is expected at the end."""
    torch_mod()
    rows, dead, st, table = mu.oracle_run(goldens, RUN_C)
    cfg, seeds, _ = mu.run_config(goldens, RUN_C)
    hip = HipBatch(cfg, seeds, max_steps=RUN_C["max_steps"], auto_reset=False)
    flags = np.empty(hip.n, np.uint32)
    for t in range(RUN_C["T"] + 1):
        got, _ = mask_call(hip.h)
        hip.h.check(hip.h.L.rg_fetch_states(hip.h.h, None, None, None, flags.ctypes.data))
        assert np.array_equal((flags & 2) != 0, dead[t]), "t=%d dead flags" % t
        assert_rows(got, rows[t], "run c t=%d" % t)
        assert not got[dead[t]].any()
        if t < RUN_C["T"]:
            hip.step(np.where(dead[t], np.uint8(ord(".")), table[t]))
    n_dead = int(dead[-1].sum())
    print(st, "dead envs", n_dead)
    assert n_dead >= 30
    assert hip.h.L.rg_sync(hip.h.h) != 0 and "Ignored input" in hip.h.L.rg_last_error(hip.h.h).decode()


def test_groups_and_mixed_sizes(goldens):
    """96 envs cycling mini / 80 x 24 / 48 x 20, as test_gpu_crop.py's mixed case: three config groups of different sizes, every group's rows scattered
    into the caller's env order (ext).  Through _Handle.action_mask.  The per-env oracles gave 3 936 rows, corner 1 139, '>' legal 15."""
    torch_mod()
    import json
    from oracle.pyoracle import OracleEnv
    from rogue_gym_python import _rogue_gym as inner

    mini = goldens["configs"]["mini"]
    enemies = {"enemies": list(range(10))}
    shapes = [dict(mini, enemies=enemies), {"width": 80, "height": 24, "enemies": enemies},
              {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": enemies}]
    n, steps = 96, 40
    cfgs = [dict(shapes[i % 3], seed=6000 + i) for i in range(n)]
    hd = inner._Handle([json.dumps(c) for c in cfgs], 60, auto_reset=True)
    assert hd.mixed_sizes
    oracles = [OracleEnv(c, max_steps=60, seed=c["seed"]) for c in cfgs]
    table = mu.key_table(1, steps, n)
    st = mu.Stats()
    for t in range(steps + 1):
        exp = np.stack([mu.oracle_row(o, why=st.why) for o in oracles])
        for o, row in zip(oracles, exp):
            st.add(o, row)
        got = hd.action_mask()
        assert got.dtype == np.bool_ and got.shape == (n, 11)
        assert_rows(got.view(np.uint8), exp, "mixed t=%d" % t)
        if t < steps:
            keys = np.ascontiguousarray(table[t])
            hd.check(hd.L.rg_step(hd.h, keys.ctypes.data, 0))
            mu.step_oracles(oracles, keys, True)
    hd.check(hd.L.rg_sync(hd.h))
    print(st)
    assert st.rows == n * (steps + 1) and st.why.get("corner", 0) >= 500 and st.stairs >= 5, str(st)
    # a custom list on the same handle: the run keys' columns are the lower-case ones
    both = hd.action_mask(b"hjklyubnHJKLYUBN")
    assert both.shape == (n, 16) and np.array_equal(both[:, :8], both[:, 8:])
    hd.close()


def test_mask_predicts_what_the_step_does(goldens):
    """Without the oracle: 4 096 mini envs with enemies, 60 random steps, the mask of before a step against the player's cell and the level after it."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    n, steps = 4096, 60
    cfg = dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)
    env = HipVecRogueEnv([dict(cfg, seed=100 + i) for i in range(n)], max_steps=60, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), action_mask=True)
    view = env.add_crop(0)  # its centre is the player's cell (y, x)
    assert env.action_mask.dtype == torch.bool and tuple(env.action_mask.shape) == (n, 11)
    gen = torch.Generator(device=env.device).manual_seed(4)
    moves = torch.as_tensor(MOVES, device=env.device)
    moved = legal_moves = left_out = stairs_legal = 0
    for t in range(steps):
        act = torch.randint(0, 11, (n,), generator=gen, device=env.device)
        mask = env.action_mask.gather(1, act[:, None])[:, 0].clone()
        cell, level = view.center.clone().long(), env.status[:, 0].clone()
        _, _, done = env.step(act)
        alive = ~done
        left_out += int(done.sum())
        now = view.center.long()
        same = (now == cell).all(dim=1)
        is_move = (act >= 1) & (act <= 8) & alive
        d = moves[(act - 1).clamp(0, 7)]
        at_target = (now[:, 0] == cell[:, 0] + d[:, 1]) & (now[:, 1] == cell[:, 1] + d[:, 0])
        assert bool(same[is_move & ~mask].all()), "t=%d: a move the mask calls illegal moved the player" % t
        assert bool((same | at_target)[is_move & mask].all()), "t=%d: a legal move ended somewhere else" % t
        legal_moves += int((is_move & mask).sum())
        moved += int((is_move & mask & at_target).sum())
        is_down = (act == 9) & alive
        rose = env.status[:, 0] > level
        assert bool((rose == mask)[is_down].all()), "t=%d: '>' descended against the mask" % t
        stairs_legal += int((is_down & mask).sum())
    env.check_errors()
    print("legal moves %d, moved %d (%.1f %%), '>' legal %d, left out for done %d of %d" % (legal_moves, moved, 100.0 * moved / legal_moves, stairs_legal, left_out, n * steps))
    assert moved >= 0.75 * legal_moves  # (the rest attacked a monster; the oracle run gave 90 %)
    assert left_out <= 0.05 * n * steps   # (2.3 % there)
    env.close()


def test_custom_keys_and_sampling(goldens):
    torch_mod()
    cfg = dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)
    n = 200
    hip = HipBatch(cfg, [300 + i for i in range(n)], max_steps=60, auto_reset=True)
    for keys in mu.key_table(5, 25, n):
        hip.step(keys)
    keys = b"HJKLYUBN>.sh"
    default, _ = mask_call(hip.h)
    rows, _ = mask_call(hip.h, keys)
    assert set(np.unique(rows)) <= {0, 1}
    assert np.array_equal(rows, default[:, [KEYS.index(bytes([k]).lower()) for k in keys]])  # the run-key columns equal the lower-case columns
    karr = np.frombuffer(keys, np.uint8)
    for seed, draw in ((0, 0), (12345, 7), ((1 << 64) - 1, (1 << 63) + 5)):
        r2, s = mask_call(hip.h, keys, sample=True, seed=seed, draw=draw)
        assert np.array_equal(r2, rows)
        assert np.array_equal(s, mu.sample_of_rows(rows, karr, seed, draw)), (seed, draw)
        assert all(rows[e, keys.index(bytes([s[e]]))] for e in range(n))  # every sampled key is legal in its row ('.' always is, so no row is empty)
        _, again = mask_call(hip.h, keys, sample=True, seed=seed, draw=draw)
        assert np.array_equal(s, again)
        _, nxt = mask_call(hip.h, keys, sample=True, seed=seed, draw=(draw + 1) & ((1 << 64) - 1))
        assert (s != nxt).sum() >= n // 4, (s != nxt).sum()
        _, alone = mask_call(hip.h, keys, mask=False, sample=True, seed=seed, draw=draw)  # mask_dev = NULL
        assert np.array_equal(s, alone)
    # the default list through NULL, and 32 keys with duplicates: every column is its key's
    _, s = mask_call(hip.h, None, sample=True, seed=3, draw=4)
    assert np.array_equal(s, mu.sample_of_rows(default, np.frombuffer(KEYS, np.uint8), 3, 4))
    long = (KEYS * 3)[:32]
    r32, s32 = mask_call(hip.h, long, sample=True, seed=9, draw=1)
    assert np.array_equal(r32, default[:, [KEYS.index(bytes([k])) for k in long]])
    assert np.array_equal(s32, mu.sample_of_rows(r32, np.frombuffer(long, np.uint8), 9, 1))
    hip.sync()


@pytest.mark.parametrize("persistent", [False, True])
def test_mask_and_sampling_have_no_side_effects(goldens, persistent):
    """Twin envs on the same seeds and keys, one with action_mask=True and a sample_keys() call every step: the same observations, rewards and dones at
    every step, the same mirrors, flag words, status and state records at the end."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    n, steps = 512, 50
    cfgs = [dict(goldens["configs"]["mini"], seed=800 + i) for i in range(n)]
    setting = ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, not persistent)  # gray + history (the bound tensor takes no history plane)
    table = torch.as_tensor(mu.key_table(7, steps, n))
    trace = []
    for masked in (False, True):
        env = HipVecRogueEnv(cfgs, max_steps=40, image_setting=setting, persistent_obs=persistent, action_mask=masked)
        assert (env.action_mask is None) == (not masked)
        per_step = [env.obs.cpu().clone()]
        for t in range(steps):
            if masked:
                env.sample_keys(seed=t)
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


def test_mask_follows_every_state_change(goldens):
    """72 envs of 80 x 24: the mask after three debug descents, after steps, after reset_envs of the odd envs and after load_state of records saved ten
    steps earlier, against the oracle or the rows saved with the records."""
    torch = torch_mod()
    from parity_util import make_oracles
    from rogue_gym.envs.device import HipVecRogueEnv

    n = 72
    seeds = [9100 + i for i in range(n)]
    env = HipVecRogueEnv([dict(mu.DEFAULT_SIZE, seed=s) for s in seeds], max_steps=1000, action_mask=True)
    oracles = make_oracles(mu.DEFAULT_SIZE, seeds, max_steps=1000)

    def expect():
        return np.stack([mu.oracle_row(o) for o in oracles])

    def steps(table):
        for keys in table:
            env.step_keys(torch.as_tensor(keys).to(env.device))
            mu.step_oracles(oracles, keys, True)

    assert_rows(env.action_mask.cpu().numpy().view(np.uint8), expect(), "constructor")
    first = expect()
    for _ in range(3):
        env._h.check(env._h.L.rg_debug_descend(env._h.h))
        for o in oracles:
            o.debug_descend()
    assert_rows(env.legal_mask().cpu().numpy().view(np.uint8), expect(), "after three descents")
    assert (expect() != first).any()
    out = torch.zeros((n, 11), dtype=torch.uint8, device=env.device)
    assert env.legal_mask(out=out).data_ptr() == out.data_ptr()
    assert_rows(out.cpu().numpy(), expect(), "legal_mask(out=)")
    steps(mu.key_table(3, 10, n))
    assert_rows(env.action_mask.cpu().numpy().view(np.uint8), expect(), "after steps on level 4")
    odd = list(range(1, n, 2))
    env.reset_envs(env_ids=odd)
    for i in odd:
        oracles[i].reset()
    assert_rows(env.action_mask.cpu().numpy().view(np.uint8), expect(), "after reset_envs")
    records, saved = env.save_state(), env.action_mask.clone()
    steps(mu.key_table(4, 10, n))
    assert_rows(env.action_mask.cpu().numpy().view(np.uint8), expect(), "ten steps later")
    assert not torch.equal(env.action_mask, saved)
    env.load_state(records)
    assert torch.equal(env.action_mask, saved), "after load_state"
    env.clone_state([0] * n, list(range(n)))
    assert bool((env.action_mask == saved[0]).all()), "after clone_state"
    env.reset()
    for o in oracles:
        o.reset()
    assert_rows(env.action_mask.cpu().numpy().view(np.uint8), expect(), "after reset")
    # sample_keys: a key of ACTIONS that is legal, the counter advances
    k0, k1 = env.sample_keys(), env.sample_keys()
    rows = env.action_mask.cpu().numpy()
    for ks in (k0.cpu().numpy(), k1.cpu().numpy()):
        assert all(rows[e, KEYS.index(bytes([ks[e]]))] for e in range(n))
    assert np.array_equal(k0.cpu().numpy(), mu.sample_of_rows(rows, np.frombuffer(KEYS, np.uint8), 0, 0))
    assert np.array_equal(k1.cpu().numpy(), mu.sample_of_rows(rows, np.frombuffer(KEYS, np.uint8), 0, 1))
    assert torch.equal(env.sample_keys(seed=5, draw=9), env.sample_keys(seed=5, draw=9))
    env.step_keys(env.sample_keys())
    env.check_errors()
    env.close()


def test_refusals_launch_nothing(goldens):
    torch = torch_mod()
    hip = HipBatch(goldens["configs"]["mini"], [1 + i for i in range(70)], max_steps=60, auto_reset=True)
    hd, L = hip.h, hip.h.L
    dev = "cuda:%d" % hd.device
    buf = torch.full((70 * 33 + 16,), 0xAA, dtype=torch.uint8, device=dev)
    smp = torch.full((70,), 0xAA, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    base = buf.data_ptr()
    assert base % 16 == 0
    cases = [((b"h", 0, base, smp.data_ptr()), ("n_keys", "got 0")), ((b"h" * 33, 33, base, smp.data_ptr()), ("n_keys", "33")),
             ((b"hjxk", 4, base, smp.data_ptr()), ("keys[2]", "0x78")), ((b"hj", 2, None, None), ("mask_dev", "sample_dev")),
             ((b"hj", 2, base + 1, smp.data_ptr()), ("mask_dev", "16-byte")), ((None, 0, base + 8, None), ("mask_dev", "16-byte"))]
    for (keys, nk, m, s), words in cases:
        rc = L.rg_action_mask(hd.h, keys, nk, None if m is None else C.c_void_p(m), None if s is None else C.c_void_p(s), 1, 2)
        msg = L.rg_last_error(hd.h).decode()
        assert rc != 0 and "rg_action_mask" in msg and all(w in msg for w in words), (keys, nk, msg)
        hip.sync()
        assert bool((buf == 0xAA).all()) and bool((smp == 0xAA).all()), "a refused call wrote: " + msg
    # and the same buffers are written by a call that is not refused: exactly the rows, nothing behind them
    assert L.rg_action_mask(hd.h, None, 0, C.c_void_p(base), C.c_void_p(smp.data_ptr()), 1, 2) == 0
    hip.sync()
    assert bool((buf[:70 * 11] <= 1).all()) and bool((buf[70 * 11:] == 0xAA).all()) and bool((smp != 0xAA).all())


def test_value_api(goldens):
    """RogueEnv.action_mask() and ParallelRogueEnv.action_masks() (8 envs) against the oracle over 40 steps of the mini config with enemies."""
    torch_mod()
    from parity_util import make_oracles
    from rogue_gym.envs import ParallelRogueEnv, RogueEnv

    cfg = dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)
    table = np.random.RandomState(8).randint(0, 11, size=(40, 8))
    env = RogueEnv(config_dict=cfg, max_steps=1000, seed=21)
    o = make_oracles(cfg, [21], max_steps=1000)[0]
    for t in range(41):
        got = env.action_mask()
        assert got.dtype == np.bool_ and got.shape == (11,)
        assert np.array_equal(got.view(np.uint8), mu.oracle_row(o)), "RogueEnv t=%d" % t
        if o.flags()["dead"]:
            assert not got.any()
            break
        if t < 40:
            env.step(int(table[t, 0]))
            o.react(int(KEYS[table[t, 0]]))
    penv = ParallelRogueEnv([dict(cfg, seed=40 + i) for i in range(8)], max_steps=30)
    oracles = make_oracles(cfg, [40 + i for i in range(8)], max_steps=30)
    for t in range(41):
        got = penv.action_masks()
        assert got.dtype == np.bool_ and got.shape == (8, 11)
        assert_rows(got.view(np.uint8), np.stack([mu.oracle_row(x) for x in oracles]), "ParallelRogueEnv t=%d" % t)
        if t < 40:
            penv.step([int(a) for a in table[t]])
            mu.step_oracles(oracles, np.frombuffer(KEYS, np.uint8)[table[t]], True)
    penv.close()
