"""Count-based novelty on the GPU (rogue-gym_amd/csrc/rg_novelty.hip): hashes and episodic counts against dicts at every step, global counts under
contention, overflow counted and not hidden, the seams (resets, loads, a stepped prefix, a handle without novelty, no side effect on the stepper) and the
refusals.  The count oracle -- a dict per env and one global dict, keyed by a numpy restatement of the hash -- is tests/novelty_util.py's; it is fed with the
screens, status words and player cells fetched from the device after every step and knows nothing of slots or probing."""
import ctypes as C

import numpy as np
import pytest

import grid_util as gu
import mask_util as mu
import novelty_util as nu

pytestmark = pytest.mark.gpu

SLACK = 64
FILL = {"hash": -0x0123456789ABCDEF, "count": -77, "gcount": -99}


def config(goldens, shape):
    if shape == "mini":
        return dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)
    if shape == "80x24":
        return dict(mu.DEFAULT_SIZE)
    return dict(gu.shape_config(shape), enemies=mu.ENEMIES)


def make_env(cfg, seeds, max_steps, **kw):
    from rogue_gym.envs import HipVecRogueEnv
    return HipVecRogueEnv([dict(cfg, seed=int(s)) for s in seeds], max_steps=max_steps, **kw)


def raw_arrays(env):
    """The handle's arrays as torch views WITH their 64 envs of slack."""
    import torch
    from rogue_gym.envs.device import _DevArray
    from rogue_gym_python._rogue_gym import RgNoveltyArrays
    a = RgNoveltyArrays()
    env._h.check(env._h.L.rg_novelty_arrays(env._h.h, C.byref(a)))
    m = env.num_envs + SLACK
    return {k: torch.as_tensor(_DevArray(p, (m,), t), device=env.device) for k, p, t in (("hash", a.hash, "<i8"), ("count", a.count, "<i4"), ("gcount", a.gcount, "<i4")) if p}


def fill_slack(env):
    raw = raw_arrays(env)
    for k, t in raw.items():
        t[env.num_envs:] = FILL[k]
    return raw


def fetch(env, raw, view):
    """One wait for the stream: what the device reports (with the slack) and what the rule is fed with."""
    env.torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in raw.items()}
    n = env.num_envs
    for k, a in got.items():
        assert (a[n:] == FILL[k]).all(), "the slack of %s was written" % k
    return {k: a[:n] for k, a in got.items()}, env.screen.cpu().numpy(), env.status[:, 0].cpu().numpy(), view.center.cpu().numpy()


def hashes_of(env, what, screens, levels, centers, crop):
    return nu.batch_hashes(nu.WHATS[what], screens, levels, centers, *(crop or (0, 0)))


CASES = [("mini", 1), ("mini", 67), ("mini", 256), ("80x24", 33), ("33x17", 5)]


@pytest.mark.parametrize("what", ["pos", "screen", "crop"])
@pytest.mark.parametrize("shape,n", CASES)
def test_episodic_counts_against_the_dict(goldens, shape, n, what):
    """300 steps of the masked random policy with max_steps = 40: novelty_hash and visit_count of every env after the enable and after every step, and the
    slack behind env N-1.  mini and 80x24 take the 16-byte loads (32 and 64 lanes per env), 33x17 (495 key bytes) and every window the byte path; 1, 67 and
    256 envs leave blocks partly empty, fill one, and need several."""
    crop = (2, 3) if what == "crop" else None
    env = make_env(config(goldens, shape), range(700, 700 + n), 40, novelty=what, novelty_scope="episode", novelty_crop=crop, novelty_slots=64)
    assert env.visit_count_global is None and env.novelty_hash.dtype == env.torch.int64 and env.visit_count.dtype == env.torch.int32
    view = env.add_crop(0)   # its centre is the player's cell (y, x)
    raw = fill_slack(env)
    ora = nu.CountOracle(n)
    got, screens, levels, centers = fetch(env, raw, view)
    hs = hashes_of(env, what, screens, levels, centers, crop)
    ora.visit(range(n), hs, True)
    assert np.array_equal(got["hash"].view(np.uint64), hs) and np.array_equal(got["count"], ora.count), "after the enable"
    ora.ends[:] = 0
    top = 0
    for t in range(300):
        _, _, done = env.step_keys(env.sample_keys(seed=5))
        got, screens, levels, centers = fetch(env, raw, view)
        hs = hashes_of(env, what, screens, levels, centers, crop)
        ora.visit(range(n), hs, done.cpu().numpy())
        bad = np.flatnonzero(got["hash"].view(np.uint64) != hs)
        assert bad.size == 0, "%s %s t=%d: novelty_hash differs in envs %s" % (shape, what, t, bad[:8])
        bad = np.flatnonzero(got["count"] != ora.count)
        assert bad.size == 0, "%s %s t=%d: visit_count differs in envs %s: device %s, dict %s" % (shape, what, t, bad[:8], got["count"][bad[:4]], ora.count[bad[:4]])
        top = max(top, int(ora.count.max()))
    print(shape, n, what, "highest count", top, "episode ends per env", ora.ends.min(), "..", ora.ends.max())
    assert top >= 3 and ora.ends.min() >= 1   # else the run shows nothing
    assert env.novelty_stats() == dict(occupied_global=0, dropped_global=0, dropped_episode=0, calls=300)
    env.check_errors()
    env.close()


def test_global_counts_under_contention(goldens):
    """256 mini envs on 4 seeds, 64 identical games each, the same keys: every wave of the insert launch offers ONE hash 64 times.  visit_count_global is the
    dict's count after all envs of the step (a multiple of 64: identical games stay identical), the table equals the dict, nothing is dropped."""
    import torch
    n, steps = 256, 120
    env = make_env(config(goldens, "mini"), [900 + e // 64 for e in range(n)], 40, novelty="screen", novelty_scope="both", novelty_slots=64, novelty_global_slots=1 << 14)
    view = env.add_crop(0)
    raw = fill_slack(env)
    ora = nu.CountOracle(n)
    table = np.repeat(mu.key_table(7, steps, 4), 64, axis=1)
    keys = torch.as_tensor(np.ascontiguousarray(table), device=env.device)
    got, screens, levels, centers = fetch(env, raw, view)
    hs = hashes_of(env, "screen", screens, levels, centers, None)
    ora.visit(range(n), hs, True)
    assert np.array_equal(got["gcount"], ora.gcount) and (got["gcount"] % 64 == 0).all()
    for t in range(steps):
        _, _, done = env.step_keys(keys[t])
        got, screens, levels, centers = fetch(env, raw, view)
        hs = hashes_of(env, "screen", screens, levels, centers, None)
        ora.visit(range(n), hs, done.cpu().numpy())
        assert np.array_equal(got["hash"].view(np.uint64), hs), t
        bad = np.flatnonzero(got["gcount"] != ora.gcount)
        assert bad.size == 0, "t=%d: visit_count_global differs in envs %s: device %s, dict %s" % (t, bad[:8], got["gcount"][bad[:4]], ora.gcount[bad[:4]])
        assert np.array_equal(got["count"], ora.count), t
        assert (got["gcount"] % 64 == 0).all(), t
    hashes, counts = env.novelty_table()
    wh, wc = ora.table()
    assert hashes.dtype == np.uint64 and counts.dtype == np.uint32
    assert np.array_equal(hashes, wh) and np.array_equal(counts, wc)
    assert int(counts.sum()) == ora.offered == n * (steps + 1) and ora.gcount.max() >= 3 * 64
    assert env.novelty_stats() == dict(occupied_global=len(ora.glob), dropped_global=0, dropped_episode=0, calls=steps)
    # clear: the global table and the counters start again, the episodic tables stay
    env.novelty_clear()
    assert env.novelty_stats() == dict(occupied_global=0, dropped_global=0, dropped_episode=0, calls=0) and len(env.novelty_table()[0]) == 0
    _, _, done = env.step_keys(torch.full((n,), ord("s"), dtype=torch.uint8, device=env.device))
    got, screens, levels, centers = fetch(env, raw, view)
    hs = hashes_of(env, "screen", screens, levels, centers, None)
    ora.visit(range(n), hs, done.cpu().numpy())
    fresh = nu.CountOracle(n)
    fresh.visit(range(n), hs, True)
    assert np.array_equal(got["gcount"], fresh.gcount) and np.array_equal(got["count"], ora.count)
    env.close()


def test_episodic_overflow_is_counted(goldens):
    """64 slots per env, the explorer guide and long episodes: the restatement of the probing (tests/novelty_util.py ProbeTable) drops visits, and the device
    reports the same counts -- 0 for a dropped visit -- and the same number of drops."""
    n, steps = 8, 220
    env = make_env(dict(goldens["configs"]["mini"], enemies={"enemies": []}), range(40, 40 + n), 2000, novelty="screen", novelty_scope="episode", novelty_slots=64, guide="explore")
    view = env.add_crop(0)
    raw = fill_slack(env)
    tabs = [nu.ProbeTable(64) for _ in range(n)]
    got, screens, levels, centers = fetch(env, raw, view)
    hs = hashes_of(env, "screen", screens, levels, centers, None)
    want = np.array([tabs[e].insert(int(hs[e])) for e in range(n)])
    assert np.array_equal(got["count"], want)
    drops = 0
    for t in range(steps):
        _, _, done = env.step_keys(env.guide_keys.clone())
        got, screens, levels, centers = fetch(env, raw, view)
        hs = hashes_of(env, "screen", screens, levels, centers, None)
        d = done.cpu().numpy()
        for e in range(n):
            if d[e]:
                tabs[e].new_episode()
            want[e] = tabs[e].insert(int(hs[e]))
        drops += int((want == 0).sum())
        assert np.array_equal(got["hash"].view(np.uint64), hs), t
        assert np.array_equal(got["count"], want), "t=%d: device %s, restated probing %s" % (t, got["count"], want)
    print("dropped by the restatement:", drops)
    assert drops >= 1   # else the run shows nothing
    assert env.novelty_stats()["dropped_episode"] == drops
    env.close()


def test_global_overflow_is_counted(goldens):
    """1 024 global slots, 64 envs, played until the table is full: the call that fills it returns, keys that were in the table before it keep exact counts, and
    every visit offered is either in the table's counts or in dropped_global."""
    n = 64
    env = make_env(config(goldens, "mini"), range(300, 300 + n), 60, novelty="screen", novelty_scope="global", novelty_global_slots=1024)
    assert env.visit_count is None
    view = env.add_crop(0)
    raw = fill_slack(env)
    ora = nu.CountOracle(n)
    got, screens, levels, centers = fetch(env, raw, view)
    ora.visit(range(n), hashes_of(env, "screen", screens, levels, centers, None), True)
    full_at, after = None, 0
    for t in range(600):
        known = dict(zip(*(a.tolist() for a in env.novelty_table()))) if full_at is None else known
        _, _, done = env.step_keys(env.sample_keys(seed=11))
        got, screens, levels, centers = fetch(env, raw, view)
        hs = hashes_of(env, "screen", screens, levels, centers, None)
        ora.visit(range(n), hs, done.cpu().numpy())
        st = env.novelty_stats()
        hashes, counts = env.novelty_table()
        assert int(counts.sum()) + st["dropped_global"] == ora.offered, (t, st)            # the conservation law
        assert st["occupied_global"] == len(hashes) <= 1024
        have = dict(zip(hashes.tolist(), counts.tolist()))
        for k in known:                                                                      # in the table before the table filled: exact ever after
            assert have[k] == ora.glob[k], (t, hex(k))
        for e in range(n):                                                                   # a reported count is the table's, 0 for a dropped visit
            assert got["gcount"][e] == have.get(int(hs[e]), 0), (t, e)
        if st["dropped_global"] == 0:
            assert have == ora.glob
        elif full_at is None:
            full_at = t
            assert st["occupied_global"] == 1024
        if full_at is not None:
            after += 1
            if after >= 5:
                break
    print("the table filled at step", full_at, "dropped", st["dropped_global"])
    assert full_at is not None and st["dropped_global"] > 0
    env.close()


def test_resets_and_loads_start_a_new_episode_of_counts(goldens):
    import torch
    n = 70
    env = make_env(dict(goldens["configs"]["mini"], enemies={"enemies": []}), range(500, 500 + n), 1000, novelty="pos", novelty_scope="both", novelty_slots=64, novelty_global_slots=4096)
    raw = raw_arrays(env)

    def play(k):
        for _ in range(k):
            env.step_keys(torch.full((n,), ord("s"), dtype=torch.uint8, device=env.device))   # searching: the same cell again and again
        return env.visit_count.cpu().numpy().copy(), env.novelty_hash.cpu().numpy().copy()

    cnt, hs = play(4)
    assert (cnt == 5).all()
    env.reset()
    assert (env.visit_count.cpu().numpy() == 1).all()
    cnt, hs = play(3)
    assert (cnt == 4).all()
    mask = torch.zeros(n, dtype=torch.bool, device=env.device)
    mask[[0, 3, 64, 69]] = True
    env.reset_envs(mask=mask)
    m = mask.cpu().numpy()
    got = env.visit_count.cpu().numpy()
    assert (got[m] == 1).all() and (got[~m] == 4).all() and np.array_equal(env.novelty_hash.cpu().numpy()[~m], hs[~m])
    env.reset_envs(env_ids=[5, 6])
    got = env.visit_count.cpu().numpy()
    assert got[5] == got[6] == 1 and got[7] == 4 and got[0] == 1
    cnt, hs = play(2)
    recs = env.save_state([1, 2])
    env.load_state(recs, [10, 65])
    got, gh = env.visit_count.cpu().numpy(), env.novelty_hash.cpu().numpy()
    touched = np.zeros(n, bool)
    touched[[10, 65]] = True
    assert (got[touched] == 1).all() and np.array_equal(got[~touched], cnt[~touched]) and np.array_equal(gh[~touched], hs[~touched])
    assert gh[10] == hs[1] and gh[65] == hs[2]   # the loaded games stand where the saved ones stood
    env.clone_state([1, 1, 1], torch.tensor([20, 21, 22], device=env.device))
    got2 = env.visit_count.cpu().numpy()
    touched[:] = False
    touched[[20, 21, 22]] = True
    assert (got2[touched] == 1).all() and np.array_equal(got2[~touched], got[~touched])
    # the global count remembers across all of it: env 1's cell has been visited by env 1, by its copies and by the loads
    assert env.visit_count_global.cpu().numpy()[20] >= got[1] + 4
    # a stepped prefix: the tail keeps its counts
    L, h = env._h.L, env._h.h
    keys = torch.full((n,), ord("s"), dtype=torch.uint8, device=env.device)
    before = {k: t.cpu().numpy().copy() for k, t in raw.items()}
    env._h.check(L.rg_step_prefix(h, C.c_void_p(keys.data_ptr()), 33, 1))
    env._h.check(L.rg_novelty_update(h))
    torch.cuda.synchronize()
    for k, t in raw.items():
        a = t.cpu().numpy()
        assert np.array_equal(a[33:], before[k][33:]), k
    assert np.array_equal(raw["count"].cpu().numpy()[:33], before["count"][:33] + 1)
    env.check_errors()
    env.close()


def test_a_handle_without_novelty_pays_nothing(goldens):
    import torch
    n = 64
    env = make_env(config(goldens, "mini"), range(n), 40)
    assert env.novelty is None and env.novelty_hash is None and env.visit_count is None and env.visit_count_global is None
    L, h = env._h.L, env._h.h
    for call in (lambda: L.rg_novelty_update(h), lambda: L.rg_novelty_cut(h, None, 0, 0, None), lambda: L.rg_novelty_clear(h)):
        assert call() != 0 and "not enabled" in L.rg_last_error(h).decode()
    for f in (env.novelty_stats, env.novelty_table, env.novelty_clear):
        with pytest.raises(ValueError):
            f()
    env.step_keys(env.sample_keys(seed=1))
    torch.cuda.synchronize()
    same = False
    for _ in range(3):   # (the device's free memory is everybody's: an allocation per step shows every time, a neighbour's does not)
        free0 = torch.cuda.mem_get_info(env.device)[0]
        for _ in range(20):
            env.step_keys(env.sample_keys(seed=1))
        env.reset()
        torch.cuda.synchronize()
        same = same or torch.cuda.mem_get_info(env.device)[0] == free0
    assert same
    env.close()


def test_no_side_effect_on_the_stepper(goldens):
    """obs, reward, done and the state records of a handle with novelty on against a twin without it, 200 steps."""
    n = 96
    cfg = config(goldens, "mini")
    a = make_env(cfg, range(n), 30, novelty="crop", novelty_crop=3, novelty_scope="both", novelty_slots=64, novelty_global_slots=1 << 16)
    b = make_env(cfg, range(n), 30)
    import torch
    assert torch.equal(a.obs, b.obs)
    for t in range(200):
        keys = b.sample_keys(seed=3)
        oa, ra, da = a.step_keys(keys)
        ob, rb, db = b.step_keys(keys)
        assert torch.equal(oa, ob) and torch.equal(ra.view(torch.int32), rb.view(torch.int32)) and torch.equal(da, db), t
        if t % 40 == 39:
            assert torch.equal(a.save_state(), b.save_state()), t
            assert torch.equal(a.screen, b.screen) and torch.equal(a.status, b.status)
    a.check_errors()
    b.check_errors()
    a.close()
    b.close()


@pytest.mark.parametrize("what,crop", [("screen", None), ("pos", None), ("crop", (2, 3))])
def test_the_value_forms_count_what_the_device_counts(goldens, what, crop):
    """ParallelRogueEnv.visit_counts (the host twin of the hash and a dict per env) against HipVecRogueEnv.visit_count on the same games and keys, every step
    across several episode ends; RogueEnv.visit_count on one game with its reset and load_state."""
    import torch
    from rogue_gym.envs import ParallelRogueEnv, RogueEnv
    n, steps = 6, 70
    cfg = config(goldens, "mini")
    cfgs = [dict(cfg, seed=int(s)) for s in range(800, 800 + n)]
    dev = make_env(cfg, range(800, 800 + n), 20, novelty=what, novelty_crop=crop, novelty_slots=64)
    par = ParallelRogueEnv(cfgs, max_steps=20)
    assert np.array_equal(par.visit_counts(what, crop), dev.visit_count.cpu().numpy())
    table = mu.key_table(3, steps, n)
    ends, top = 0, 0
    for t in range(steps):
        dev.step_keys(torch.as_tensor(table[t], device=dev.device))
        _, _, done, _ = par.step(bytes(table[t]).decode("latin-1"))
        got = par.visit_counts(what, crop)
        assert got.dtype == np.int32 and np.array_equal(got, dev.visit_count.cpu().numpy()), t
        assert np.array_equal(par._visits.hashes, dev.novelty_hash.cpu().numpy().view(np.uint64)), t
        ends, top = ends + sum(done), max(top, int(got.max()))
    assert ends >= n and top >= 3
    par.reset()
    assert (par.visit_counts(what, crop) == 1).all()
    par.close()
    dev.close()
    one = RogueEnv(config_dict=dict(cfg, enemies={"enemies": []}), seed=3, max_steps=100)
    assert one.visit_count(what, crop) == 1 == one.visit_count(what, crop)   # asking twice is one visit
    one.step("s")
    one.step("s")
    assert one.visit_count(what, crop) == 3
    rec = one.save_state()
    one.reset()
    assert one.visit_count(what, crop) == 1
    one.load_state(rec)
    assert one.visit_count(what, crop) == 1
    one.step("s")
    assert one.visit_count(what, crop) == 2
    one.close() if hasattr(one, "close") else None


def test_refusals_allocate_nothing(goldens):
    import torch
    from rogue_gym_python import _rogue_gym as inner
    cfg = config(goldens, "mini")
    cfgs = [dict(cfg, seed=i) for i in range(8)]
    import json
    hd = inner._Handle([json.dumps(c) for c in cfgs], 40, auto_reset=True)
    plain = inner._Handle([json.dumps(c) for c in cfgs], 40, auto_reset=False)
    groups = inner._Handle([json.dumps(cfgs[0]), json.dumps(dict(cfgs[1], enemies={"enemies": []}))], 40, auto_reset=True)
    L = hd.L
    torch.cuda.synchronize()
    dev = torch.device("cuda", hd.device)

    def refused(handle, frag, *args):
        same = False
        for _ in range(3):   # (the device's free memory is everybody's: a refused call that allocates shows every time, a neighbour's allocation does not)
            free = torch.cuda.mem_get_info(dev)[0]
            assert L.rg_novelty_enable(handle.h, *args) != 0
            msg = L.rg_last_error(handle.h).decode()
            assert msg.startswith("rg_novelty_enable: ") and frag in msg, msg
            same = same or torch.cuda.mem_get_info(dev)[0] == free
        assert same, "a refused enable allocated"
        assert L.rg_novelty_update(handle.h) != 0 and "not enabled" in L.rg_last_error(handle.h).decode()

    ok = (nu.SCREEN, 3, 0, 0, 64, 1024)
    refused(plain, "auto-reset", *ok)
    refused(groups, "config groups", *ok)
    refused(hd, "what", 0, 3, 0, 0, 64, 1024)
    refused(hd, "what", 4, 3, 0, 0, 64, 1024)
    refused(hd, "scope", nu.SCREEN, 0, 0, 0, 64, 1024)
    refused(hd, "scope", nu.SCREEN, 4, 0, 0, 64, 1024)
    refused(hd, "radius", nu.SCREEN, 3, 1, 0, 64, 1024)
    refused(hd, "radius", nu.POS, 3, 0, 2, 64, 1024)
    refused(hd, "radius", nu.CROP, 3, 48, 2, 64, 1024)
    refused(hd, "radius", nu.CROP, 3, 2, 160, 64, 1024)
    refused(hd, "radius", nu.CROP, 3, -1, 2, 64, 1024)
    for cap in (0, 32, 63, 96, 1 << 17, -64):
        refused(hd, "cap", nu.SCREEN, 1, 0, 0, cap, 1024)
    for gcap in (0, 512, 1000, 3 << 10, 1 << 29, -1024):
        refused(hd, "gcap", nu.SCREEN, 2, 0, 0, 64, gcap)
    hd.check(L.rg_novelty_enable(hd.h, nu.CROP, 3, 47, 159, 64, 1024))   # the widest window there is
    assert L.rg_novelty_enable(hd.h, *ok) != 0 and "already" in L.rg_last_error(hd.h).decode()
    # the cut's list rules are rg_episode_cut's
    ids = (C.c_int32 * 3)(1, 2, 2)
    assert L.rg_novelty_cut(hd.h, ids, 3, 0, None) != 0 and "twice" in L.rg_last_error(hd.h).decode()
    ids = (C.c_int32 * 2)(1, 8)
    assert L.rg_novelty_cut(hd.h, ids, 2, 0, None) != 0 and "out of range" in L.rg_last_error(hd.h).decode()
    assert L.rg_novelty_cut(hd.h, ids, 9, 0, None) != 0
    mask = torch.zeros(8, dtype=torch.uint8, device=dev)
    assert L.rg_novelty_cut(hd.h, ids, 1, 0, C.c_void_p(mask.data_ptr())) != 0 and "not both" in L.rg_last_error(hd.h).decode()
    hd.check(L.rg_novelty_update(hd.h))
    hd.check(L.rg_sync(hd.h))
    st = (C.c_uint64 * 4)()
    hd.check(L.rg_novelty_stats(hd.h, st))
    assert 1 <= st[0] <= 8 and list(st)[1:] == [0, 0, 1]
    for x in (hd, plain, groups):
        x.close()
