"""The step-wave shapes bench.py times, against the CPU oracle on every lane.  rgk_step_epw gives a step wave 64 envs only from 65 473 envs up and the
wide stepper 33 envs at 32 768 envs of 80x24; the lock-step suites run n <= 512 (16 envs per wave).  Here HipVecRogueEnv.step_keys, the call bench.py
times, plays the benchmark's own batch sizes with max_steps = 1000 and a fresh uniform key of the 11-action table per env and step, past the mass
timeouts at steps 1 000 and 2 000, and an OracleBatch plays the compared envs: contiguous runs of env indices at the start of the batch, at its very
end (the partial or tail wave) and at offsets that are multiples of neither 64 nor 33 in between, so whole waves are compared on every lane
whatever rgk_step_epw returns.  Every step: reward, done, the ten status words and the terminal / dead / message bits, read from the device tensors
with nothing that flushes the mirrors between the step and its observation; the gray observation bit for bit at every 4th step and at every step
around the mass timeouts; at the checkpoints the screen and history mirrors of every compared env and the internals (scalars, RNG words, tiles, gold
and monster tables) of every 61st.  No compared env is ever skipped and no check depends on what the library returned."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.pyoracle import OracleBatch
from parity_util import ACTION_KEYS, compare_internal

pytestmark = pytest.mark.gpu

MAX_STEPS = 1000
MSG_SHIFT, MSG_MASK = 8, 0x7F
STATUS = ["dungeon_level", "gold", "hp_current", "hp_max", "str_current", "str_max", "defense", "player_level", "exp", "hunger"]


def torch_mod():
    import torch

    return torch


def threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def text(screen):
    return "\n".join(bytes(r).decode("latin-1") for r in screen)


def vec_env(cfgs, **kw):
    from rogue_gym.envs.device import HipVecRogueEnv

    return HipVecRogueEnv(cfgs, max_steps=MAX_STEPS, **kw)  # (the default image setting: f32 gray, no status planes, no history)


def device_keys(env, keys):
    return torch_mod().as_tensor(np.ascontiguousarray(keys, np.uint8), device=env.device)


def compared_runs(n, run, count):
    """`count` disjoint runs of `run` env indices: [0, run), [n - run, n) and count - 2 evenly spread between at starts that are multiples of neither
    64 nor 33 (nor 16: no wave size in use puts lane 0 there)."""
    starts = [0]
    for k in range(1, count - 1):
        s = (n - run) * k // (count - 1)
        while s % 64 == 0 or s % 33 == 0 or s % 16 == 0:
            s += 1
        starts.append(s)
    starts.append(n - run)
    for a, b in zip(starts, starts[1:]):
        assert a + run <= b, "compared runs overlap"
    assert all(s % 64 and s % 33 for s in starts[1:-1])
    return np.concatenate([np.arange(s, s + run) for s in starts]), starts


class Handle:
    """One HipVecRogueEnv under test and the debug view compare_internal reads (by env index)."""

    def __init__(self, name, env, cmp):
        self.name, self.env, self.cmp = name, env, cmp
        self.idx = torch_mod().as_tensor(cmp, device=env.device)

    def debug(self, e):
        return self.env._h.debug_state(int(e))


class OracleView:
    """oracles[e] for compare_internal: the oracle of env index e (position pos[e] of the batch)."""

    def __init__(self, ob, cmp):
        self.ob, self.pos = ob, {int(e): k for k, e in enumerate(cmp)}

    def __getitem__(self, e):
        return self.ob.env(self.pos[int(e)])


def where(case, hd, t, k, epw, starts, run):
    e = int(hd.cmp[k])
    return "%s [%s] step %d env %d (e %% %d = %d, %d of the run at %d)" % (case, hd.name, t, e, epw, e % epw, e - starts[k // run], starts[k // run])


def raise_diff(msg, hd, k, ob):
    """Both screens as text (read only after a comparison failed: the fetch flushes pending Redraws)."""
    try:
        mine = text(hd.env._h.fetch()[0][int(hd.cmp[k])])
    except Exception as ex:  # noqa: BLE001
        mine = "(unavailable: %s)" % ex
    raise AssertionError("%s\nHIP:\n%s\nORACLE:\n%s" % (msg, mine, text(ob.env(int(k)).screen())))


def first_bad(ok):
    return int(np.flatnonzero(~ok)[0])


def play(case, cfg, n, run, count, steps, epw, slots, handles, windows, checkpoints, need):
    """epw, slots: the envs per step wave this batch must get, and its kernel's slot class (rgk_step_epw).  handles: {name: vec_env keywords}.  windows: [(lo, hi)] of steps whose observation is compared at every step (else every 4th).  need: the
    oracle-side floors (mean resets per env, descents per env, share of envs with >= 4 resets or None)."""
    from rogue_gym_python import _rogue_gym as inner

    f = inner.load_library().rgk_step_epw
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int]
    assert f(n, slots) == epw, "%s: the library gives this batch %d envs per step wave, not the %d this test is written for" % (case, f(n, slots), epw)
    cmp, starts = compared_runs(n, run, count)
    hds = []
    try:
        for name, kw in handles.items():
            hds.append(Handle(name, vec_env([dict(cfg, seed=i) for i in range(n)], **kw), cmp))
        _play(case, cfg, run, steps, epw, hds, cmp, starts, windows, checkpoints, need)
    finally:
        for hd in hds:
            hd.env.close()


def _play(case, cfg, run, steps, epw, hds, cmp, starts, windows, checkpoints, need):
    torch = torch_mod()
    n, m = hds[0].env.num_envs, len(cmp)
    ob = OracleBatch([dict(cfg, seed=int(e)) for e in cmp], max_steps=MAX_STEPS, n_threads=threads())
    H, W = ob.h, ob.w
    exp_obs = np.empty((m, 1, H, W), np.float32)
    rng = np.random.RandomState(0)
    resets = np.zeros(m, np.int64)
    descents = 0
    _, _, st_prev, _ = ob.fetch(screen=False, hist=False)
    views = OracleView(ob, cmp)

    def loc(hd, t, k):
        return where(case, hd, t, k, epw, starts, run)

    for t in range(1, steps + 1):
        keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)]
        with_obs = t % 4 == 0 or any(lo <= t <= hi for lo, hi in windows)
        dev_keys = device_keys(hds[0].env, keys)
        outs = [hd.env.step_keys(dev_keys) for hd in hds]
        ob.step(keys[cmp], exp_obs if with_obs else None)
        _, _, st, fl = ob.fetch(screen=False, hist=False)
        term = fl[:, 0] != 0
        exp_reward = np.maximum(0, st[:, 1].astype(np.int64) - st_prev[:, 1].astype(np.int64)).astype(np.float32)
        resets += term
        descents += int(((st[:, 0] > st_prev[:, 0]) & ~term).sum())
        exp_dev = torch.as_tensor(exp_obs, device=hds[0].env.device) if with_obs else None
        for hd, (obs, _, _) in zip(hds, outs):
            env = hd.env
            reward = env.reward[hd.idx].cpu().numpy()
            done = env.done[hd.idx].cpu().numpy()
            status = env.status[hd.idx].cpu().numpy().astype(np.uint32)
            flags = env.flags[hd.idx].cpu().numpy().astype(np.uint32)
            if not np.array_equal(status, st):
                k = first_bad((status == st).all(1))
                c = first_bad(status[k] == st[k])
                raise_diff("%s: status %s %d, oracle %d (all ten: %s vs %s)" % (loc(hd, t, k), STATUS[c], status[k, c], st[k, c], status[k], st[k]), hd, k, ob)
            if not np.array_equal(reward, exp_reward):
                k = first_bad(reward == exp_reward)
                raise_diff("%s: reward %r, oracle gold %d -> %d" % (loc(hd, t, k), float(reward[k]), st_prev[k, 1], st[k, 1]), hd, k, ob)
            for field, got, exp in (("done", done.astype(bool), term), ("terminal bit", (flags & 1) != 0, term), ("dead bit", (flags & 2) != 0, fl[:, 3] != 0),
                                    ("message bits", (flags >> MSG_SHIFT) & MSG_MASK, fl[:, 1])):
                if not np.array_equal(got, exp):
                    k = first_bad(got == exp)
                    raise_diff("%s: %s %d, oracle %d" % (loc(hd, t, k), field, got[k], exp[k]), hd, k, ob)
            if with_obs:
                got_dev = obs[hd.idx]
                if not torch.equal(got_dev, exp_dev):
                    got = got_dev.cpu().numpy()
                    k = first_bad((got == exp_obs).reshape(m, -1).all(1))
                    _, y, x = (int(v) for v in np.argwhere(got[k] != exp_obs[k])[0])
                    raise_diff("%s: gray observation first differs at (y %d, x %d): %r, oracle %r" % (loc(hd, t, k), y, x, float(got[k, 0, y, x]), float(exp_obs[k, 0, y, x])),
                               hd, k, ob)
        st_prev = st
        if t in checkpoints:
            o_scr, o_hist, _, _ = ob.fetch(status=False, flags=False)
            for hd in hds:
                scr, hist, _, _ = hd.env._h.fetch()
                scr, hist = scr[cmp], hist[cmp]
                for field, got, exp in (("screen mirror", scr, o_scr), ("history mirror", hist, o_hist)):
                    if not np.array_equal(got, exp):
                        k = first_bad((got == exp).reshape(m, -1).all(1))
                        y, x = (int(v) for v in np.argwhere(got[k] != exp[k])[0])
                        raise_diff("%s: %s first differs at (y %d, x %d): %d, oracle %d" % (loc(hd, t, k), field, y, x, got[k, y, x], exp[k, y, x]), hd, k, ob)
                for k in range(0, m, 61):
                    compare_internal(hd, views, [int(cmp[k])], loc(hd, t, k) + ": internals,")
    for hd in hds:
        hd.env.check_errors()
        c = hd.env.counters()
        assert c["spares_taken"] >= 0.9 * c["resets"], "%s [%s]: %d spares taken for %d auto-resets" % (case, hd.name, c["spares_taken"], c["resets"])
        assert c["descents"] > 0 and c["next_level_structures_used"] > 0, "%s [%s]: counters %s" % (case, hd.name, c)
    # what keeps the run from going hollow, from the oracle's side alone
    mean_resets, per_env_descents, share4 = resets.mean(), descents / m, (resets >= 4).mean()
    print("%s: %d compared envs, %.2f resets per env (min %d), %.3f descents per env, %.1f %% of envs with >= 4 resets"
          % (case, m, mean_resets, resets.min(), per_env_descents, 100 * share4))
    assert mean_resets >= need[0], "%s: %.2f resets per compared env, %g required" % (case, mean_resets, need[0])
    assert per_env_descents >= need[1], "%s: %.3f descents per compared env, %g required" % (case, per_env_descents, need[1])
    if need[2] is not None:
        assert share4 >= need[2], "%s: %.1f %% of the compared envs were reset 4 times or more, %g %% required" % (case, 100 * share4, 100 * need[2])


@pytest.mark.timeout(900)
def test_bench_workload_every_lane_mini(goldens):
    """bench.py's headline shape: 65 536 mini envs (k_step_w32, 64 envs per wave), 2 100 steps -- the mass timeouts at 1 000 and 2 000, the rotation
    through all four spare slots, and the timed window after bench.py's 1 500-step pre-roll.  The default f32 gray handle and a persistent_obs=True
    handle (the bound tensor, whose turn writes pixels itself) on the same keys against one OracleBatch of 8 192 envs in 16 runs of 512."""
    play("mini 65536", goldens["configs"]["mini"], 65536, 512, 16, 2100, 64, 2, {"gray": {}, "bound": {"persistent_obs": True}},
         [(995, 1010), (1995, 2010)], (500, 1001, 1500, 2100), (5, 0.3, 0.4))


@pytest.mark.timeout(900)
def test_bench_workload_every_lane_default(goldens):
    """32 768 envs of the default 80x24 config: k_step<2> at 33 envs per wave (993 waves, the last of 32), whose lanes 16..32 play no env in any
    n <= 512 lock-step run.  1 100 steps, 2 178 compared envs in 11 runs of 198 (six waves each)."""
    play("default 32768", goldens["configs"]["default"], 32768, 198, 11, 1100, 33, 1, {"gray": {}}, [(995, 1010)], (500, 1001, 1100), (3, 0.04, None))
