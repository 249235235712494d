"""The cell archive on the GPU (rogue-gym_amd/csrc/rg_archive.hip): the table and every stored record against a dict at the end of seeded runs and `stored` /
`slot` after every step, ties under contention, caller-given keys and scores, overflow counted and not hidden, the way back (restore), the seams (a handle
without the archive, no side effect on the stepper) and the refusals.  The oracle -- tests/archive_util.py's DictArchive -- is fed with novelty_hash,
score_in, steps_in and save_state() of all envs fetched after every step and knows nothing of slots."""
import ctypes as C
import json

import numpy as np
import pytest

import archive_util as au
import grid_util as gu
import mask_util as mu

pytestmark = pytest.mark.gpu

SLACK = 64
FILL = {"slot": -77, "stored": 0x5A, "score_in": -99, "steps_in": -55}


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
    """The per-env arrays as torch views WITH their 64 envs of slack."""
    import torch
    from rogue_gym.envs.device import _DevArray
    from rogue_gym_python._rogue_gym import RgArchiveArrays
    a = RgArchiveArrays()
    env._h.check(env._h.L.rg_archive_arrays(env._h.h, C.byref(a)))
    m = env.num_envs + SLACK
    return {k: torch.as_tensor(_DevArray(getattr(a, k), (m,), t), device=env.device) for k, t in (("slot", "<i4"), ("stored", "|u1"), ("score_in", "<i4"), ("steps_in", "<i4"))}


def fill_slack(env):
    raw = raw_arrays(env)
    for k, t in raw.items():
        t[env.num_envs:] = FILL[k]
    return raw


def fetch(env, raw):
    """One wait for the stream: the per-env arrays (the slack checked) and the slots' keys."""
    env.torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in raw.items()}
    n = env.num_envs
    for k, a in got.items():
        assert (a[n:] == FILL[k]).all(), "the slack of %s was written" % k
    got = {k: a[:n] for k, a in got.items()}
    got["steps_in"] = got["steps_in"].view(np.uint32)
    got["key"] = env.archive.key.cpu().numpy().view(np.uint64)
    return got


def check_call(env, got, ora, keys, records, t, envs=None, admit=None):
    """One update against the dict: stored[], and slot[] names the key's slot."""
    stored, dropped = ora.update(keys, got["score_in"], got["steps_in"], records, envs, admit)
    offering = np.zeros(env.num_envs, bool)
    offering[list(range(env.num_envs) if envs is None else envs)] = True
    assert np.array_equal(got["slot"] < 0, dropped | ~offering), "t=%d: slot == -1 in envs %s, the dict drops %s" % (t, np.flatnonzero(got["slot"] < 0)[:8], np.flatnonzero(dropped)[:8])
    at = got["slot"][got["slot"] >= 0]
    want = np.array([int(k) or 1 for k in keys], np.uint64)[got["slot"] >= 0]
    assert np.array_equal(got["key"][at], want), "t=%d: key[slot[e]] is not the env's key" % t
    bad = np.flatnonzero(got["stored"].astype(bool) != stored)
    assert bad.size == 0, "t=%d: stored differs in envs %s: device %s, dict %s" % (t, bad[:8], got["stored"][bad[:4]], stored[bad[:4]])
    return dropped


def check_table(env, ora, what=""):
    """The table sorted by key equals the dict, and so does every cell's record, byte for byte."""
    at, keys, score, steps, seen, when = au.device_table(env.archive)
    wk, ws, wt, wn, ww = ora.rows()
    assert np.array_equal(keys, wk), "%s: %d keys on the device, %d in the dict" % (what, keys.size, wk.size)
    assert np.array_equal(score, ws) and np.array_equal(steps & 0xFFFFFFFF, wt) and np.array_equal(seen, wn) and np.array_equal(when, ww), what
    recs = env.archive.records[env.torch.as_tensor(at, device=env.device)].cpu().numpy()
    for i, k in enumerate(wk):
        want = ora.cells[int(k)][4]
        if not np.array_equal(recs[i], want):
            bad = np.flatnonzero(recs[i] != want)
            raise AssertionError("%s: the record of cell %016x (slot %d) differs in %d bytes from offset %d" % (what, int(k), at[i], bad.size, bad[0]))
    return at


CASES = [("mini", 1), ("mini", 67), ("mini", 256), ("80x24", 33), ("33x17", 5)]


@pytest.mark.parametrize("shape,n", CASES)
def test_records_against_the_dict(goldens, shape, n):
    """150 steps of the masked random policy with max_steps = 40 and the player's cell as the key: stored, slot and the slack after every step, the whole table
    and every record at the end.  33x17 has record sections on no 16-byte boundary; 67 envs leave the word writer's block partly empty; 256 need several."""
    env = make_env(config(goldens, shape), range(700, 700 + n), 40, novelty="pos", archive=4096)
    A = env.archive
    assert A.records.shape == (4096, env.state_bytes) and A.key.dtype == env.torch.int64 and A.stored.dtype == env.torch.bool and A.slot.dtype == env.torch.int32
    raw = fill_slack(env)
    ora = au.DictArchive()
    ends = np.zeros(n, np.int64)
    for t in range(150):
        _, _, done = env.step_keys(env.sample_keys(seed=5))
        recs = env.save_state().cpu().numpy()
        got = fetch(env, raw)
        ends += done.cpu().numpy()
        check_call(env, got, ora, env.novelty_hash.cpu().numpy().view(np.uint64), recs, t)
    check_table(env, ora, "%s %d" % (shape, n))
    st = env.archive_stats()
    print(shape, n, "cells", len(ora.cells), "replacements", ora.replaced, "episode ends per env", ends.min(), "..", ends.max(), st)
    assert ora.replaced >= 1 and ends.min() >= 1   # else the run shows nothing
    assert st == dict(occupied=len(ora.cells), dropped=0, written=len(ora.cells) + ora.replaced, calls=150)
    env.check_errors()
    env.close()


def test_ties_under_contention(goldens):
    """256 mini envs on 4 seeds, 64 identical games each, the same keys: every wave offers ONE cell 64 times with equal (score, steps).  The lowest env of each
    game takes it, and an update without a step in between stores nothing."""
    import torch
    n, steps = 256, 60
    env = make_env(config(goldens, "mini"), [900 + e // 64 for e in range(n)], 40, novelty="screen", archive=4096)
    raw = fill_slack(env)
    ora = au.DictArchive()
    keys = torch.as_tensor(np.ascontiguousarray(np.repeat(mu.key_table(7, steps, 4), 64, axis=1)), device=env.device)
    for t in range(steps):
        env.step_keys(keys[t])
        recs = env.save_state().cpu().numpy()
        got = fetch(env, raw)
        check_call(env, got, ora, env.novelty_hash.cpu().numpy().view(np.uint64), recs, t)
        assert not got["stored"][np.arange(n) % 64 != 0].any(), t
        if t % 20 == 19:
            assert (env.archive.seen[env.archive.key != 0] % 64 == 0).all(), t
    assert len(ora.cells) >= 8
    before = env.archive.records.clone()
    hs = env.novelty_hash.cpu().numpy().view(np.uint64)
    env.archive_update()
    got = fetch(env, raw)
    check_call(env, got, ora, hs, None, steps)
    assert not got["stored"].any() and torch.equal(env.archive.records, before)
    assert (env.archive.seen[env.archive.key != 0] % 64 == 0).all()
    env.close()


def test_caller_given_keys_and_scores(goldens):
    """archive_update(keys, score, mask) without novelty: seeded scores with negative values and both i32 extremes; a worse later offer replaces nothing, equal
    score with fewer steps replaces, an equal (score, steps) from a later call does not, a mask keeps masked envs out of seen; key 0 is offered as 1."""
    import torch
    n = 96
    env = make_env(config(goldens, "mini"), range(300, 300 + n), 1000, archive=1024, archive_auto=False)
    raw = fill_slack(env)
    ora = au.DictArchive()
    rng = np.random.RandomState(4)
    keys_np = (np.arange(n) % 12).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15 // 12)   # twelve cells, the first one under key 0
    keys_np[5] = 1                                                                            # ... which key 1 shares
    keys = torch.as_tensor(keys_np.view(np.int64), device=env.device)
    s0 = rng.randint(-5, 6, n).astype(np.int64)
    s0[[3, 40]], s0[[7, 50]] = au.I32_MIN, au.I32_MAX
    s0[13], s0[25] = au.I32_MIN, au.I32_MAX   # cell 1 holds both extremes
    dev = lambda a: torch.as_tensor(np.asarray(a, np.int64).astype(np.int32), device=env.device)

    def call(score, mask=None, tag=""):
        env.archive_update(keys, dev(score), None if mask is None else torch.as_tensor(mask, device=env.device))
        recs = env.save_state().cpu().numpy()
        got = fetch(env, raw)
        envs = None if mask is None else np.flatnonzero(mask)
        assert np.array_equal(got["score_in"][envs if envs is not None else slice(None)], np.asarray(score)[envs if envs is not None else slice(None)]), tag
        check_call(env, got, ora, keys_np, recs, ora.calls, envs)
        return got["stored"].astype(bool)

    for _ in range(3):
        env.step_keys(env.sample_keys(seed=2))
    first = call(s0, tag="first")
    assert first.sum() == 12 and first[25] and first[7]                    # twelve cells: the best score of each, i32 max where it was offered
    assert not call(s0, tag="equal, later").any()                          # equal (score, steps) from a later call
    assert not call(np.maximum(s0 - 1, au.I32_MIN), tag="worse").any()     # worse scores
    env.step_keys(env.sample_keys(seed=2))
    assert not call(s0, tag="more steps").any()                            # equal scores, more steps
    better = call(np.minimum(s0 + 1, au.I32_MAX), tag="better")            # better scores replace, except where the score cannot grow
    assert better.sum() == 9 and not better[25] and not better[7] and not better[50]   # (i32 max stands in three cells)
    env.reset()                                                            # steps back to 0
    s1 = np.minimum(s0 + 1, au.I32_MAX)
    again = call(s1, tag="fewer steps")
    assert again.sum() == 12 and again[25] and again[7]                    # equal score, fewer steps: every cell's record is replaced
    seen0 = {k: c[2] for k, c in ora.cells.items()}
    mask = (np.arange(n) % 3 == 0)
    m = call(np.minimum(s1 + 1, au.I32_MAX), mask, tag="masked")
    assert not m[~mask].any() and m.any()
    assert sum(c[2] - seen0[k] for k, c in ora.cells.items()) == mask.sum()  # only the offering envs were counted
    check_table(env, ora, "caller-given")
    assert 1 in ora.cells and 0 not in ora.cells
    st = env.archive_stats()
    assert st["occupied"] == 12 and st["dropped"] == 0 and st["calls"] == ora.calls == 7
    # the refusals of the explicit call
    with pytest.raises(ValueError):
        env.archive_update()                                               # no novelty: no hash to take
    assert env._h.L.rg_archive_update(env._h.h, None, None, None) != 0 and "novelty" in env._h.L.rg_last_error(env._h.h).decode()
    with pytest.raises(ValueError):
        env.archive_update(keys[:5])
    with pytest.raises(ValueError):
        env.archive_update(keys.to(torch.int32))
    env.archive_clear()
    assert env.archive_stats() == dict(occupied=0, dropped=0, written=0, calls=0)
    assert not env.archive.key.any() and not env.archive.records.any() and not env.archive.seen.any() and (env.archive.slot == -1).all()
    env.check_errors()
    env.close()


def test_overflow_is_counted_not_hidden(goldens):
    """1 024 cells, 512 envs, whole-screen keys: the table fills within a few steps.  slot == -1 exactly for the keys that are not in the table afterwards
    (which of the new keys got the last empty slots is the one thing scheduling decides: the dict is told the device's occupancy), a dropped key found no
    empty slot, sum(seen) + dropped == offers, and every stored record is still exact."""
    n, cells = 512, 1024
    env = make_env(config(goldens, "mini"), range(100, 100 + n), 40, novelty="screen", archive=cells)
    raw = fill_slack(env)
    ora = au.DictArchive()
    dropped = 0
    for t in range(8):
        env.step_keys(env.sample_keys(seed=5))
        recs = env.save_state().cpu().numpy()
        got = fetch(env, raw)
        hs = env.novelty_hash.cpu().numpy().view(np.uint64)
        d = check_call(env, got, ora, hs, recs, t, admit=au.admitted_by(got["key"]))
        for e in np.flatnonzero(d):
            assert au.window_full(got["key"], int(hs[e]), cells), (t, e)
        dropped += int(d.sum())
    st = env.archive_stats()
    print("overflow:", st, "offers", 8 * n)
    assert dropped > 0 and st["dropped"] == dropped and st["occupied"] == cells == len(ora.cells)
    assert int(env.archive.seen.sum()) + dropped == 8 * n == ora.offers + dropped
    check_table(env, ora, "overflow")
    env.check_errors()
    env.close()


def test_restore(goldens):
    """The way back: restore slots into chosen envs, save_state(env_ids) equals records[slots], chosen is raised, restored and untouched lanes that hold the
    same state stay equal for 40 more steps under equal keys, an empty slot leaves its env alone and raises the state error, and the restored envs' visit
    counts start a new episode."""
    import torch
    n = 64
    env = make_env(config(goldens, "mini"), [41] * n, 40, novelty="pos", archive=4096, episodes=True)   # one dungeon, 64 ways through it
    A = env.archive
    for t in range(60):
        env.step_keys(env.sample_keys(seed=9))
    for t in range(40):   # until a step stores the states of a few lanes: those lanes then hold exactly what their cells hold
        env.step_keys(env.sample_keys(seed=9))
        if int(A.stored.sum()) >= 2:
            break
    src = torch.nonzero(A.stored).flatten()[:8]
    assert src.numel() >= 2
    slots = A.slot[src].clone()
    dst = torch.as_tensor([e for e in range(n) if e not in set(src.tolist())][:src.numel()], dtype=torch.int32, device=env.device)
    assert torch.equal(env.save_state(src), A.records[slots.long()])
    chosen0 = A.chosen.clone()
    env.archive_restore(slots, dst)
    assert torch.equal(env.save_state(dst), A.records[slots.long()]) and torch.equal(env.save_state(dst), env.save_state(src))
    assert torch.equal(A.chosen - chosen0, torch.bincount(slots.long(), minlength=A.cells).to(torch.int32))
    assert (env.visit_count[dst.long()] == 1).all()
    env.check_errors()
    for t in range(40):   # equal keys for the pairs; both lanes restart from the same seed when the episode ends
        keys = env.sample_keys(seed=11)
        keys[dst.long()] = keys[src]
        obs, rew, done = env.step_keys(keys)
        assert torch.equal(obs[dst.long()], obs[src]) and torch.equal(rew[dst.long()], rew[src]) and torch.equal(done[dst.long()], done[src]), t
    assert torch.equal(env.save_state(dst), env.save_state(src))
    # sampled slots, host lists, the same slot into several envs
    for weights in ("seen", "uniform", torch.ones(A.cells, device=env.device)):
        g = torch.Generator(device=env.device)
        g.manual_seed(3)
        s = env.archive_sample(24, weights, generator=g)
        assert s.dtype == torch.int32 and s.shape == (24,) and (A.key[s.long()] != 0).all()
        g.manual_seed(3)
        assert torch.equal(s, env.archive_sample(24, weights, generator=g))
    recs = A.records[s.long()].clone()   # (the restore below steps nothing: the table stays as it is)
    chosen0 = A.chosen.clone()
    ids = list(range(40, 64))
    env.archive_restore(s.tolist(), ids)
    assert torch.equal(env.save_state(ids), recs)
    assert torch.equal(A.chosen - chosen0, torch.bincount(s.long(), minlength=A.cells).to(torch.int32))
    env.check_errors()
    # an empty slot: the env keeps its state, the error is raised, chosen stays
    empty = int(torch.nonzero(A.key == 0).flatten()[0])
    keep, chosen0 = env.save_state([5, 6]), A.chosen.clone()
    env.archive_restore([empty, int(s[0])], [5, 6])
    now = env.save_state([5, 6])
    assert torch.equal(now[0], keep[0]) and torch.equal(now[1], A.records[int(s[0])])
    assert int(A.chosen[empty]) == 0 and int(A.chosen[int(s[0])]) == int(chosen0[int(s[0])]) + 1
    with pytest.raises(RuntimeError):
        env.check_errors()
    # refusals of the restore
    L, h = env._h.L, env._h.h
    for sl, ids_, frag in (([A.cells], [1], "out of range"), ([-1], [1], "out of range"), ([0, 1], [2, 2], "twice"), ([0], [n], "out of range")):
        a, b = (C.c_int32 * len(sl))(*sl), (C.c_int32 * len(ids_))(*ids_)
        assert L.rg_archive_restore(h, a, b, len(sl), 0) != 0 and frag in L.rg_last_error(h).decode(), (sl, ids_, L.rg_last_error(h))
    assert L.rg_archive_restore(h, None, None, 0, 0) != 0 and "slot_ids" in L.rg_last_error(h).decode()
    with pytest.raises(ValueError):
        env.archive_restore([0, 1], [3])
    env.close()


def test_a_handle_without_the_archive_pays_nothing(goldens):
    import torch
    n = 64
    cfg = config(goldens, "mini")
    env = make_env(cfg, range(n), 40, novelty="pos")
    twin = make_env(cfg, range(n), 40, novelty="pos", archive=1024)
    assert env.archive is None and twin.archive is not None
    L, h = env._h.L, env._h.h
    arr = (C.c_uint64 * 4)()
    for call in (lambda: L.rg_archive_update(h, None, None, None), lambda: L.rg_archive_clear(h), lambda: L.rg_archive_stats(h, arr),
                 lambda: L.rg_archive_restore(h, arr, None, 0, 0)):
        assert call() != 0 and "not enabled" in L.rg_last_error(h).decode()
    for f in (env.archive_update, env.archive_stats, env.archive_clear, lambda: env.archive_sample(1), lambda: env.archive_restore([0], [0])):
        with pytest.raises(ValueError):
            f()
    for t in range(60):   # the same outputs and the same workload counters as the handle that has one
        keys = env.sample_keys(seed=1)
        oa, ra, da = env.step_keys(keys)
        ob, rb, db = twin.step_keys(keys)
        assert torch.equal(oa, ob) and torch.equal(ra.view(torch.int32), rb.view(torch.int32)) and torch.equal(da, db), t
    assert env.counters() == twin.counters()
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
    twin.close()


def test_no_side_effect_on_the_stepper(goldens):
    """obs, reward, done, the visit counts and the state records of a handle with the archive against a twin without it, 160 steps."""
    import torch
    n = 96
    cfg = config(goldens, "mini")
    a = make_env(cfg, range(n), 30, novelty="screen", archive=1 << 14)
    b = make_env(cfg, range(n), 30, novelty="screen")
    assert torch.equal(a.obs, b.obs)
    for t in range(160):
        keys = b.sample_keys(seed=3)
        oa, ra, da = a.step_keys(keys)
        ob, rb, db = b.step_keys(keys)
        assert torch.equal(oa, ob) and torch.equal(ra.view(torch.int32), rb.view(torch.int32)) and torch.equal(da, db), t
        assert torch.equal(a.visit_count, b.visit_count) and torch.equal(a.novelty_hash, b.novelty_hash), t
        if t % 40 == 39:
            assert torch.equal(a.save_state(), b.save_state()), t
            assert torch.equal(a.screen, b.screen) and torch.equal(a.status, b.status)
    assert a.archive_stats()["dropped"] == 0
    a.check_errors()
    b.check_errors()
    a.close()
    b.close()


def test_refusals_allocate_nothing(goldens):
    import torch
    from rogue_gym_python import _rogue_gym as inner
    cfg = config(goldens, "mini")
    cfgs = [dict(cfg, seed=i) for i in range(8)]
    hd = inner._Handle([json.dumps(c) for c in cfgs], 40, auto_reset=True)
    groups = inner._Handle([json.dumps(cfgs[0]), json.dumps(dict(cfgs[1], enemies={"enemies": []}))], 40, auto_reset=True)
    big = inner._Handle([json.dumps(dict(config(goldens, "80x24"), seed=1))], 40, auto_reset=True)
    L = hd.L
    torch.cuda.synchronize()
    dev = torch.device("cuda", hd.device)

    def refused(handle, frag, cells):
        same = False
        for _ in range(3):   # (the device's free memory is everybody's: a refused call that allocates shows every time, a neighbour's allocation does not)
            free = torch.cuda.mem_get_info(dev)[0]
            assert L.rg_archive_enable(handle.h, cells) != 0
            msg = L.rg_last_error(handle.h).decode()
            assert msg.startswith("rg_archive_enable: ") and frag in msg, msg
            same = same or torch.cuda.mem_get_info(dev)[0] == free
        assert same, "a refused enable allocated"
        assert L.rg_archive_update(handle.h, None, None, None) != 0 and "not enabled" in L.rg_last_error(handle.h).decode()

    refused(groups, "config groups", 1024)
    for cells in (0, 512, 1000, 3 << 10, 1 << 25, -1024):
        refused(hd, "cells", cells)
    # an allocation that fails: 2^24 records of an 80x24 env are some 760 GB
    assert L.rg_state_record_bytes(big.h) * (1 << 24) > torch.cuda.mem_get_info(dev)[1]
    refused(big, "cells = 16777216", 1 << 24)
    hd.check(L.rg_archive_enable(hd.h, 1024))
    assert L.rg_archive_enable(hd.h, 1024) != 0 and "already" in L.rg_last_error(hd.h).decode()
    assert L.rg_archive_update(hd.h, None, None, None) != 0 and "novelty" in L.rg_last_error(hd.h).decode()   # no keys given and no hash to take
    assert L.rg_archive_arrays(hd.h, None) != 0 and L.rg_archive_stats(hd.h, None) != 0
    st = (C.c_uint64 * 4)()
    hd.check(L.rg_archive_stats(hd.h, st))
    assert list(st) == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        make_env(cfg, range(4), 40, archive=1024)   # archive_auto needs novelty
    for x in (hd, groups, big):
        x.close()
