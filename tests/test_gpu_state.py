"""Batched save / restore of env game states (rg_state_save / rg_state_load; HipVecRogueEnv.save_state / load_state / clone_state, RogueEnv.save_state /
load_state): round trips, continuation against the CPU oracle after restoring into other envs, the full 65 536-env wave shape, records across handle
kinds, the bound observation tensor, the stair set and the next-level structures around a restore, and the refusals."""
import ctypes as C
import json

import numpy as np
import pytest

from grid_util import record_offsets
from oracle.pyoracle import OracleEnv
from parity_util import ALL_KEYS, HipBatch, compare_internal, custom_enemy_config

pytestmark = pytest.mark.gpu

RG_FLAG_SCR_CHANGED = 0x40
RG_FLAG_ERR_STATE = 0x00100000


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


def on_stairs(rec):
    o_cell, o_words, H, W = record_offsets(rec)
    rec = np.asarray(rec)
    pos = int(rec[o_words:o_words + 4].view("<u4")[0])
    x, y = pos >> 8, pos & 0xFF
    cell = rec[o_cell:o_cell + 2 * H * W].view("<u2")
    return (int(cell[y * W + x]) & 7) == 4


def mirrors_equal(hip, oracles, envs, where):
    """compare_mirrors of parity_util over a subset of envs (oracles: dict env -> OracleEnv)."""
    screen, hist, status, flags = hip.fetch()
    for i in envs:
        o = oracles[i]
        assert np.array_equal(screen[i], o.screen()), "%s env %d screen\nHIP:\n%s\nORACLE:\n%s" % (
            where, i, "\n".join(bytes(r).decode() for r in screen[i]), "\n".join(bytes(r).decode() for r in o.screen()))
        assert np.array_equal(hist[i], o.hist()), "%s env %d hist" % (where, i)
        assert [int(v) & 0xFFFFFFFF for v in status[i]] == [int(v) for v in o.status_arr()], "%s env %d status" % (where, i)
        f = o.flags()
        assert bool(flags[i] & 1) == f["is_terminal"] and bool(flags[i] & 2) == f["dead"], "%s env %d terminal / dead" % (where, i)
        assert ((int(flags[i]) >> 8) & 0x7F) == f["message"], "%s env %d message" % (where, i)


def save_batch(hip, ids=None):
    """rg_state_save of a HipBatch into a torch tensor (u8 [k, R])."""
    torch = torch_mod()
    L, h = hip.h.L, hip.h.h
    R = L.rg_state_record_bytes(h)
    k = hip.n if ids is None else len(ids)
    out = torch.empty((k, R), dtype=torch.uint8, device="cuda:%d" % hip.h.device)
    if ids is None:
        hip.h.check(L.rg_state_save(h, None, k, 0, C.c_void_p(out.data_ptr())))
    else:
        a = np.ascontiguousarray(ids, np.int32)
        hip.h.check(L.rg_state_save(h, a.ctypes.data, k, 0, C.c_void_p(out.data_ptr())))
    hip.sync()
    return out


def load_batch(hip, recs, ids):
    a = np.ascontiguousarray(ids, np.int32)
    hip.h.check(hip.h.L.rg_state_load(hip.h.h, C.c_void_p(recs.data_ptr()), int(recs.shape[1]), a.ctypes.data, len(a), 0))
    hip.sync()


# ---------------------------------------------------------------------------------------------
# 1. round trip
# ---------------------------------------------------------------------------------------------
def test_round_trip_and_replay(goldens):
    torch = torch_mod()
    from rogue_gym.envs.rogue_env import DungeonType, ImageSetting, StatusFlag

    cfg = goldens["configs"]["mini"]
    n = 512
    env = vec_env(cfg, range(n), max_steps=200)
    rng = np.random.RandomState(1)
    dev = env.device
    for _ in range(40):
        env.step_keys(torch.as_tensor(ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)], device=dev))
    first = env.save_state().clone()
    keys = [torch.as_tensor(ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)], device=dev) for _ in range(30)]
    sym = ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False)

    def continuation():
        for k in keys:
            env.step_keys(k)
        out = dict(screen=env.screen.clone(), status=env.status.clone(), reward=env.reward.clone(), done=env.done.clone(),
                   flags=(env.flags & ~RG_FLAG_SCR_CHANGED).clone(), gray=env.obs.clone(), symbol=env.expand_records(env.packed_records(), sym).clone(),
                   hist=env.all_gather_compact(with_hist=True)[2].clone(), records=env.save_state().clone())
        torch.cuda.synchronize()
        return out

    a = continuation()
    env.load_state(first)
    again = env.save_state()
    torch.cuda.synchronize()
    assert torch.equal(again, first), "save -> load -> save is not byte-identical"
    b = continuation()
    env.check_errors()
    for name in a:
        assert torch.equal(a[name], b[name]), "replay after load differs in %s" % name
    env.close()


# ---------------------------------------------------------------------------------------------
# 2. oracle continuation: sources restored into other envs, played on against the uninterrupted oracle of the source
# ---------------------------------------------------------------------------------------------
def _continuation_case(cfg, n, steps, seed):
    rng = np.random.RandomState(seed)
    src_seeds = [1000 + i for i in range(n)]
    dst_seeds = [5000 + i for i in range(n)]
    A = HipBatch(cfg, src_seeds, max_steps=400)
    B = HipBatch(cfg, dst_seeds, max_steps=400)
    src_or = [OracleEnv(cfg, max_steps=400, seed=s) for s in src_seeds]
    # sources of varying progress: env i plays 40 - 40 i / n keys (a key prefix per step: rg_step_prefix keys the first nk envs only)
    plan = [40 - (40 * i) // n for i in range(n)]
    for t in range(40):
        keys = ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)].copy()
        nk = sum(1 for p in plan if p > t)
        A.h.check(A.h.L.rg_step_prefix(A.h.h, keys.ctypes.data, nk, 0))
        for i in range(nk):
            src_or[i].step_autoreset(int(keys[i]))
    for _ in range(7):
        B.step(ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)])
    recs = save_batch(A)
    perm = rng.permutation(n)  # source i -> destination perm[i]: every lane of the full waves, other seeds, other progress
    load_batch(B, recs, perm)
    oracles = {int(perm[i]): src_or[i] for i in range(n)}
    check = sorted(oracles)[:: max(1, n // 24)]
    mirrors_equal(B, oracles, range(n), "after load")
    compare_internal(B, oracles, check, "after load")
    reset_seen = 0
    for t in range(steps):
        keys = ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)].copy()
        B.step(keys)
        skip = set()
        for j in range(n):
            o = oracles[j]
            o.step_autoreset(int(keys[j]))
            if o.flags()["is_terminal"]:
                # the destination resets from ITS seed: from here on it is the fresh oracle of the destination's seed (this step's reported state
                # carries the forced terminal flag, which a fresh oracle does not: compared from the next step on)
                oracles[j] = OracleEnv(cfg, max_steps=400, seed=dst_seeds[j])
                skip.add(j)
                reset_seen += 1
        mirrors_equal(B, oracles, [j for j in range(n) if j not in skip], "t=%d" % t)
        if t % 10 == 9:
            compare_internal(B, oracles, [j for j in check if j not in skip], "t=%d" % t)
    B.sync()
    return reset_seen


@pytest.mark.parametrize("name", ["mini", "default", "enemies"])
def test_oracle_continuation_after_load(goldens, name):
    if name == "enemies":
        cfg = custom_enemy_config(goldens["configs"]["mini"])
    else:
        cfg = goldens["configs"][name]
    n = 128 if name != "default" else 64
    resets = _continuation_case(cfg, n, 300, seed={"mini": 3, "default": 4, "enemies": 5}[name])
    assert resets > 0  # (some destinations played past the restored episode into one of their own)


# ---------------------------------------------------------------------------------------------
# 3. full wave shape: 65 536 envs, restored permuted into a second handle
# ---------------------------------------------------------------------------------------------
def test_full_batch_permuted_into_second_handle(goldens):
    torch = torch_mod()
    cfg = goldens["configs"]["mini"]
    n = 65536
    A = vec_env(cfg, [7] * n, max_steps=150)
    B = vec_env(cfg, [7] * n, max_steps=150)
    dev = A.device
    g = torch.Generator(device="cpu").manual_seed(0)
    keyset = torch.as_tensor(ALL_KEYS.copy(), device=dev)
    for _ in range(200):
        A.step_keys(keyset[torch.randint(0, len(ALL_KEYS), (n,), generator=g).to(dev)])
    perm = torch.randperm(n, generator=g).to(dev)  # A's env i -> B's env perm[i]
    B.load_state(A.save_state(), perm)
    for t in range(200):
        ka = keyset[torch.randint(0, len(ALL_KEYS), (n,), generator=g).to(dev)]
        kb = torch.empty_like(ka)
        kb[perm] = ka
        A.step_keys(ka)
        B.step_keys(kb)
        if t % 25 == 24:
            ra, rb = A.save_state(), B.save_state()
            assert torch.equal(ra, rb[perm]), "t=%d: the permuted records differ" % t
            assert torch.equal(A.obs, B.obs[perm]), "t=%d: observations differ" % t
    A.check_errors()
    B.check_errors()
    A.close()
    B.close()


# ---------------------------------------------------------------------------------------------
# 4. records across handle kinds: HipVecRogueEnv (auto-reset, n = 256, logging on / off) <-> RogueEnv (n = 1, no auto-reset, logging on)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logging", [True, False])
def test_records_between_vec_env_and_rogue_env(goldens, logging):
    torch = torch_mod()
    from rogue_gym.envs.rogue_env import RogueEnv

    cfg = goldens["configs"]["mini"]
    n = 256
    vec = vec_env(cfg, range(300, 300 + n), max_steps=500)
    if logging:
        vec.enable_history(4096)
    rng = np.random.RandomState(9)
    for _ in range(25):
        vec.step_keys(torch.as_tensor(ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)], device=vec.device))
    live = np.nonzero((vec.flags.cpu().numpy() & 3) == 0)[0]  # (lanes neither dead nor just reset: a RogueEnv refuses keys on a terminal game)
    src = int(live[len(live) // 3])
    rec = vec.save_state([src])
    torch.cuda.synchronize()
    d = dict(cfg)
    d["seed"] = 12345
    env = RogueEnv(config_dict=d, max_steps=500)
    env.step("hjkl")
    before = env.result
    before_dungeon = list(before.dungeon)
    state = env.load_state(bytes(rec[0].cpu().numpy()))
    assert state is env.result and list(before.dungeon) == before_dungeon  # earlier values keep what they were
    if logging:
        assert env.game.dump_history() == vec.dump_history(src)
    else:
        with pytest.raises(RuntimeError, match="incomplete"):
            env.game.dump_history()
    # both go on with the same keys: RogueEnv's game == the vec env's lane
    for t in range(40):
        k = ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)].copy()
        vec.step_keys(torch.as_tensor(k, device=vec.device))
        _, _, done, _ = env.step(chr(k[src]))
        if done:
            break
        scr, _, status, _ = env.game._h.fetch()
        assert np.array_equal(scr[0], vec.screen[src].cpu().numpy()), "t=%d screen" % t
        assert np.array_equal(status[0], vec.status[src].cpu().numpy()), "t=%d status" % t
    steps_there = t
    if env.result.is_terminal:  # (the game ended: go on from another live lane of the vec env)
        live = np.nonzero((vec.flags.cpu().numpy() & 3) == 0)[0]
        env.load_state(bytes(vec.save_state([int(live[0])])[0].cpu().numpy()))
    # and back: RogueEnv's record into another lane of the vec env
    dst = 200
    r2 = env.save_state()
    vec.load_state(torch.frombuffer(bytearray(r2), dtype=torch.uint8).to(vec.device)[None], [dst])
    assert not int(vec.flags[dst]) & RG_FLAG_ERR_STATE  # (check_errors would also report the random keys its dead players got)
    if logging:
        assert vec.history_keys(dst) == env.game._h.history_keys(0)
    for t in range(30):
        k = ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)].copy()
        vec.step_keys(torch.as_tensor(k, device=vec.device))
        _, _, done, _ = env.step(chr(k[dst]))
        if done:
            break
        scr, _, status, _ = env.game._h.fetch()
        assert np.array_equal(scr[0], vec.screen[dst].cpu().numpy()), "back t=%d screen" % t
        assert np.array_equal(status[0], vec.status[dst].cpu().numpy()), "back t=%d status" % t
    assert steps_there > 0 and t > 0  # (both directions were compared)
    vec.close()


# ---------------------------------------------------------------------------------------------
# 5. the bound observation tensor
# ---------------------------------------------------------------------------------------------
def test_bound_tensor_after_load(goldens):
    torch = torch_mod()
    cfg = goldens["configs"]["mini"]
    n = 256
    a = vec_env(cfg, range(n), max_steps=300, persistent_obs=True)
    b = vec_env(cfg, range(n), max_steps=300)
    src = vec_env(cfg, range(900, 900 + n), max_steps=300)
    rng = np.random.RandomState(2)
    dev = a.device

    def keys():
        return torch.as_tensor(ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)], device=dev)

    for _ in range(12):
        k = keys()
        a.step_keys(k)
        b.step_keys(k)
        src.step_keys(keys())
    ids = list(range(1, n, 3))
    recs = src.save_state(ids)
    oa, ob = a.load_state(recs, ids), b.load_state(recs, ids)
    assert torch.equal(oa, ob)
    for t in range(20):
        k = keys()
        oa, _, _ = a.step_keys(k)
        ob, _, _ = b.step_keys(k)
        assert torch.equal(oa, ob), "t=%d" % t
    # rg_step -> rg_state_load -> bound observation, no observation call in between
    k = keys()
    for e in (a, b):
        e._h.check(e._h.L.rg_step(e._h.h, C.c_void_p(k.data_ptr()), 1))
    recs = src.save_state(list(range(0, n, 5)))
    oa, ob = a.load_state(recs, list(range(0, n, 5))), b.load_state(recs, list(range(0, n, 5)))
    assert torch.equal(oa, ob)
    for t in range(5):
        k = keys()
        oa, _, _ = a.step_keys(k)
        ob, _, _ = b.step_keys(k)
        assert torch.equal(oa, ob), "after step-load t=%d" % t
    for e in (a, b, src):
        e.check_errors()
        e.close()


# ---------------------------------------------------------------------------------------------
# 6. stairs and descents around a restore
# ---------------------------------------------------------------------------------------------
def test_stairs_and_next_level_structures_after_load(goldens):
    cfg = goldens["configs"]["mini"]
    n = 4096
    seeds = [100 + i for i in range(n)]
    A = HipBatch(cfg, seeds, max_steps=500)
    recs = save_batch(A)
    host = recs.cpu().numpy()
    on = [i for i in range(n) if on_stairs(host[i])]
    off = [i for i in range(n) if not on_stairs(host[i])]
    m = min(16, len(on) // 2)
    assert m >= 2, len(on)
    B = HipBatch(cfg, seeds, max_steps=500)
    # destinations ON[m:2m] stand on the stairs and ask for their next level: two steps later their structure is READY
    for _ in range(3):
        B.step(np.frombuffer(b"." * n, np.uint8))
    B.sync()
    pairs = [(on[j], off[j]) for j in range(m)]                       # on the stairs -> into an env that is not
    pairs += [(off[m + j], on[j]) for j in range(m)]                  # not on the stairs -> into one that is
    pairs += [(on[m + (j + 1) % m], on[m + j]) for j in range(m)]     # on the stairs -> into one on the stairs holding a READY structure
    src_ids = [s for s, _ in pairs]
    dst_ids = [d for _, d in pairs]
    load_batch(B, recs[src_ids], dst_ids)
    oracles = {d: OracleEnv(cfg, max_steps=500, seed=seeds[s]) for s, d in pairs}
    mirrors_equal(B, oracles, dst_ids, "after load")
    keys = np.frombuffer(b"." * n, np.uint8).copy()
    keys[dst_ids] = ord(">")
    rng = np.random.RandomState(6)
    descended = 0
    for t in range(25):
        B.step(keys)
        skip = set()
        for d in dst_ids:
            oracles[d].step_autoreset(int(keys[d]))
            if oracles[d].flags()["is_terminal"]:  # the episode is over: the destination goes on from its own seed
                oracles[d] = OracleEnv(cfg, max_steps=500, seed=seeds[d])
                skip.add(d)
        if t == 0:
            descended = sum(1 for d in dst_ids[:m] if oracles[d].status_arr()[0] == 2)
        live = [d for d in dst_ids if d not in skip]
        mirrors_equal(B, oracles, live, "t=%d" % t)
        if t in (0, 24):
            compare_internal(B, oracles, live, "t=%d" % t)
        keys = ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)].copy()
    assert descended == m  # (every restored on-stairs player went down)
    B.sync()


# ---------------------------------------------------------------------------------------------
# 7. host-side env-id lists share one staging buffer
# ---------------------------------------------------------------------------------------------
def test_host_id_lists_back_to_back_equal_device_lists(goldens):
    """rg_episode_cut, rg_novelty_cut and rg_state_save upload their host-side env ids into ONE buffer of the handle.  Three calls with three lists and no
    sync in between must serve the envs each was given: a second handle, same seeds and keys, is given the same lists as device tensors, which are not staged,
    and the episode arrays, the novelty arrays and the saved records of the two are byte-equal."""
    torch = torch_mod()
    from episode_util import CUT
    from novelty_util import SCREEN
    from rogue_gym_python._rogue_gym import RgEpisodeArrays, RgNoveltyArrays

    n, steps = 8, 8
    lists = ([1, 5], [2, 6, 7], [0, 3, 3])   # the cut of the episodes, the cut of the novelty tables, the save (which takes a duplicate)
    rng = np.random.RandomState(77)
    keys = [ALL_KEYS[rng.randint(0, len(ALL_KEYS), n)] for _ in range(steps)]

    def run(on_device):
        hip = HipBatch(goldens["configs"]["mini"], [900 + i for i in range(n)], max_steps=5, auto_reset=True)   # (5 < steps: every env has auto-reset once)
        hd, L = hip.h, hip.h.L
        dev = "cuda:%d" % hd.device
        hd.check(L.rg_episode_enable(hd.h, 3, 0))
        hd.check(L.rg_novelty_enable(hd.h, SCREEN, 3, 0, 0, 64, 1024))
        for k in keys:
            hip.step(k)
            hd.check(L.rg_episode_update(hd.h))
            hd.check(L.rg_novelty_update(hd.h))
        recs = torch.zeros((len(lists[2]), L.rg_state_record_bytes(hd.h)), dtype=torch.uint8, device=dev)
        if on_device:
            held = [torch.tensor(l, dtype=torch.int32, device=dev) for l in lists]
            ptr = [C.c_void_p(t.data_ptr()) for t in held]
        else:
            held = [np.array(l, np.int32) for l in lists]
            ptr = [a.ctypes.data for a in held]
        torch.cuda.synchronize()
        hd.check(L.rg_episode_cut(hd.h, ptr[0], len(lists[0]), int(on_device), None, 1))
        hd.check(L.rg_novelty_cut(hd.h, ptr[1], len(lists[1]), int(on_device), None))
        hd.check(L.rg_state_save(hd.h, ptr[2], len(lists[2]), int(on_device), C.c_void_p(recs.data_ptr())))
        hip.sync()

        def read(p, count, dtype):
            out = np.empty(count, dtype)
            hd.check(L.rg_dev_read(hd.h, C.c_void_p(p), out.ctypes.data, out.nbytes))
            return out

        e, v = RgEpisodeArrays(), RgNoveltyArrays()
        hd.check(L.rg_episode_arrays(hd.h, C.byref(e)))
        hd.check(L.rg_novelty_arrays(hd.h, C.byref(v)))
        got = {k: read(getattr(e, k), n, t) for k, t in (("ret", "<f4"), ("len", "<i4"), ("depth", "<i4"), ("died", "|u1"), ("time_limit", "|u1"), ("last_return", "<f4"),
                                                         ("last_length", "<i4"), ("last_depth", "<i4"), ("last_cause", "|u1"), ("scout", "<f4"))}
        got["seen"] = read(e.seen, n * e.seen_bytes, "|u1")
        got.update({"nov_" + k: read(getattr(v, k), n, t) for k, t in (("hash", "<u8"), ("count", "<i4"), ("gcount", "<i4"))})
        got["records"] = recs.cpu().numpy()
        hd.close()
        return got

    host, device = run(False), run(True)
    assert sorted(host) == sorted(device)
    for k in host:
        assert host[k].tobytes() == device[k].tobytes(), k
    assert np.array_equal(host["records"][1], host["records"][2]) and not np.array_equal(host["records"][0], host["records"][1])   # env 3 twice, env 0 once
    cut = np.isin(np.arange(n), lists[0])
    assert ((host["last_cause"] == CUT) == cut).all(), host["last_cause"]   # the recorded cut ended the episodes of its envs and of no other


# ---------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals(goldens):
    torch = torch_mod()
    mini = goldens["configs"]["mini"]
    n = 64
    env = vec_env(mini, range(n), max_steps=100)
    dev = env.device
    for _ in range(5):
        env.step_keys(torch.as_tensor(ALL_KEYS[np.arange(n) % len(ALL_KEYS)], device=dev))
    other_cfg = json.loads(json.dumps(mini))
    other_cfg["dungeon"]["min_room_size"] = {"x": 3, "y": 3}       # another config, same geometry
    wider = dict(mini, width=40)                                     # another geometry
    grid = json.loads(json.dumps(mini))
    grid["dungeon"]["room_num_x"] = 3                                # another room grid
    foreign = []
    for c in (other_cfg, wider, grid):
        o = vec_env(c, [1], max_steps=100)
        foreign.append(o.save_state())
        o.close()
    bad = env.save_state([1]).clone()
    bad[0, 0] ^= 1                                                   # corrupted magic
    foreign.append(bad)
    for rec in foreign:
        before = env.save_state([0]).clone()
        env.load_state(rec, [0])
        assert int(env.flags[0]) & RG_FLAG_ERR_STATE
        with pytest.raises(RuntimeError, match="state record"):
            env.check_errors()
        assert torch.equal(env.save_state([0]), before)
    env.check_errors()  # (the error was reported once)
    recs = env.save_state([2, 3])
    with pytest.raises(ValueError, match="duplicate"):
        env.load_state(recs, [5, 5])
    with pytest.raises(ValueError, match="duplicate"):
        env.load_state(recs, torch.tensor([5, 5], device=dev))
    a = np.array([5, 5], np.int32)
    assert env._h.L.rg_state_load(env._h.h, C.c_void_p(recs.data_ptr()), int(recs.shape[1]), a.ctypes.data, 2, 0) != 0
    assert b"twice" in env._h.L.rg_last_error(env._h.h)
    with pytest.raises(RuntimeError, match="out of range"):
        env.save_state([n])
    with pytest.raises(RuntimeError, match="out of range"):
        env.load_state(recs, [0, n])
    env.close()
    # a handle with config groups refuses both calls with a message
    from rogue_gym.envs.device import HipVecRogueEnv

    grp = HipVecRogueEnv([dict(mini, seed=1), dict(other_cfg, seed=2)], max_steps=100)
    with pytest.raises(RuntimeError, match="config groups"):
        grp.save_state()
    with pytest.raises(RuntimeError, match="config groups"):
        grp.load_state(torch.zeros((2, 64), dtype=torch.uint8, device=grp.device))
    grp.close()
