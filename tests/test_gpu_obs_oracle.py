"""Every observation path against the CPU oracle at the step where it draws.  The library and the oracle play in lock step; after every step the
observation the call under test returns is compared bit for bit with the oracle's image of the same env (OracleEnv.gray_image / symbol_image).
Nothing that reads the mirrors (rg_fetch_states, rg_screen, rg_flags, HipBatch.fetch) runs between the step and the observation call, so the pass
under test draws the pending Redraws itself: k_obs_stream and its second runs, k_obs's one-, two- and three-wave and staged blocks past their first
pass, the config-group kernels, the unfused fallbacks, the bound tensor under every call cadence, the crop, and the host and compact paths.
The oracle plays only the envs that are compared: every env is independent given its seed."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.pyoracle import OracleBatch, OracleEnv
from parity_util import ALL_KEYS, crop_window

pytestmark = pytest.mark.gpu

FULL = 0x1FF
RG_FLAG_ERR_TILE = 0x00040000
STEP_KEYS = np.frombuffer(b"hjklyubnHJKLYUBN>>s.", np.uint8)  # run keys and '>'
DIRS = {(0, -1): "k", (0, 1): "j", (-1, 0): "h", (1, 0): "l", (-1, -1): "y", (1, -1): "u", (-1, 1): "b", (1, 1): "n"}
ZED = {"attack": [], "attr": 0, "defense": 1, "exp": 1, "gold": 0, "level": 1, "name": "zed", "tile": 90, "rarelity": 0}  # shown as 'Z': no symbol


def torch_mod():
    import torch

    return torch


def threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def grid_cfg(w, h, rx, ry, mr=4, **kw):
    return dict({"width": w, "height": h, "dungeon": {"style": "rogue", "room_num_x": rx, "room_num_y": ry, "min_room_size": {"x": mr, "y": mr}}}, **kw)


def text(screen):
    return "\n".join(bytes(r).decode("latin-1") for r in screen)


def hip_screen(h, e):
    """The library's screen mirror of env e as text (read only after a comparison failed: it flushes pending Redraws)."""
    try:
        return text(h.fetch()[0][e])
    except Exception as ex:  # noqa: BLE001  (a mixed-size batch has no common screen tensor)
        return "(unavailable: %s)" % ex


def fail(case, t, e, got, exp, h, oracle_screen):
    p, y, x = (int(v) for v in np.argwhere(~((got == exp) | (np.isnan(got) & np.isnan(exp))))[0]) if got.shape == exp.shape else (-1, -1, -1)
    msg = "%s step %d env %d: observation differs from the oracle's" % (case, t, e)
    if p >= 0:
        msg += " first at (plane %d, y %d, x %d): %r vs %r" % (p, y, x, float(got[p, y, x]), float(exp[p, y, x]))
    else:
        msg += " shape %s vs %s" % (got.shape, exp.shape)
    raise AssertionError("%s\nHIP:\n%s\nORACLE:\n%s" % (msg, hip_screen(h, e), text(oracle_screen)))


def check_batch(case, t, envs, got, exp, h, oracle_screen):
    """got / exp: [m, C, H, W] of envs (in that order); raises on the first env that differs."""
    if got.shape == exp.shape and np.array_equal(got, exp):
        return
    for k, e in enumerate(envs):
        if got.shape[1:] != exp.shape[1:] or not np.array_equal(got[k], exp[k]):
            fail(case, t, e, got[k], exp[k], h, oracle_screen(k))


def expected(oracles, kind, flag, with_hist):
    """The oracle's images of `oracles` and the set of their positions whose one-hot image raises (a 'Z' on screen: not a symbol)."""
    exp, bad = [], set()
    for k, o in enumerate(oracles):
        try:
            exp.append(image(o, kind, flag, with_hist))
        except RuntimeError:
            if not kind:
                raise
            bad.add(k)
            exp.append(None)
    return exp, bad


def check_list(case, t, envs, got, exp, bad, h, oracle_screen, flags=None):
    """Every env whose oracle image exists matches bit for bit; with flags (the flag words of envs), the envs flagged RG_FLAG_ERR_TILE are
    exactly those whose oracle image raises."""
    for k, e in enumerate(envs):
        if k not in bad and not np.array_equal(got[k], exp[k]):
            fail(case, t, e, got[k], exp[k], h, oracle_screen(k))
    if flags is not None:
        flagged = {k for k in range(len(envs)) if int(flags[k]) & RG_FLAG_ERR_TILE}
        assert flagged == bad, "%s step %d: envs flagged ERR_TILE %s, envs whose oracle image raises %s" % (
            case, t, sorted(int(envs[k]) for k in flagged), sorted(int(envs[k]) for k in bad))


def drain(h, bad):
    """rg_sync after a one-hot call: fails iff some env showed a 'Z' (and clears the error word)."""
    rc = h.L.rg_sync(h.h)
    assert (rc != 0) == bool(bad), "rg_sync rc %d with %d envs showing 'Z'" % (rc, len(bad))


def image(o, kind, flag, with_hist):
    return o.symbol_image(flag, with_hist) if kind else o.gray_image(flag, with_hist)


def seeker_keys(oracles, rng):
    """One key per oracle: '>' on the stairs, else mostly a greedy step towards them, else a random key (short episodes then see descents)."""
    out = np.empty(len(oracles), np.uint8)
    for k, o in enumerate(oracles):
        surf = o.grid()[0]
        sc = o.scalars()
        px, py = sc["px"], sc["py"]
        ys, xs = np.nonzero(surf == 4)
        if len(xs) and (xs[0], ys[0]) == (px, py):
            out[k] = ord(">")
        elif len(xs) and rng.rand() < 0.7:
            out[k] = ord(DIRS[(int(np.sign(xs[0] - px)), int(np.sign(ys[0] - py)))])
        else:
            out[k] = ALL_KEYS[rng.randint(0, len(ALL_KEYS))]
    return out


def vec_env(cfgs, kind, flag=0, with_hist=False, no_mirror=False, **kw):
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    st = ImageSetting(DungeonType.SYMBOL if kind else DungeonType.GRAY, StatusFlag(flag), with_hist)
    if no_mirror:  # every Redraw drawn from the tiles by the observation pass (read when the handle is created)
        os.environ["ROGUE_GYM_HIP_NO_MIRROR_UPDATE"] = "1"
    try:
        return HipVecRogueEnv(cfgs, image_setting=st, **kw)
    finally:
        os.environ.pop("ROGUE_GYM_HIP_NO_MIRROR_UPDATE", None)


def device_keys(env, keys):
    return torch_mod().as_tensor(np.ascontiguousarray(keys, np.uint8), device=env.device)


# ---------------------------------------------------------------------------------------------
# 1. the headline stream path: k_obs_stream, second runs of its persistent waves
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(240)
@pytest.mark.parametrize("no_mirror", [False, True], ids=["mirror_update", "no_mirror_update"])
def test_stream_path_every_step(goldens, no_mirror):
    """65 536 + 4 093 mini envs: 16 384 waves of 4-env runs, the first 1 024 of which run a second (the last one partial).  Envs [0, 4096) and
    [65536, n) against an OracleBatch at every step of 100, 40-step episodes, run keys and '>'."""
    torch = torch_mod()
    mini = goldens["configs"]["mini"]
    n, steps = 65536 + 4093, 100
    cmp = np.r_[0:4096, 65536:n]
    env = vec_env([dict(mini, seed=i) for i in range(n)], 0, no_mirror=no_mirror, max_steps=40)
    ob = OracleBatch([dict(mini, seed=int(i)) for i in cmp], max_steps=40, n_threads=threads())
    idx = torch.as_tensor(cmp, device=env.device)
    exp = np.empty((len(cmp), 1, 16, 32), np.float32)
    rng = np.random.RandomState(11)
    case = "stream%s" % (" no-mirror" if no_mirror else "")
    for t in range(1, steps + 1):
        keys = STEP_KEYS[rng.randint(0, len(STEP_KEYS), n)]
        obs, _, _ = env.step_keys(device_keys(env, keys))
        ob.step(keys[cmp], exp)
        got = obs[idx].cpu().numpy()
        check_batch(case, t, cmp, got, exp, env._h, lambda k: ob.env(k).screen())
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------
# 2. general k_obs with status and history planes, descents and auto-resets at the step they happen
# ---------------------------------------------------------------------------------------------
def play_planes(case, cfg, n, cmp, steps, max_steps, kind, flag, with_hist, seed, need_descent=True, zed=False):
    """HipVecRogueEnv of n envs (seed = env index) against one OracleEnv per compared env: the compared envs follow the stair seeker, the others
    random keys; every step the observation of every compared env is checked.  One-hot (every env compared): the oracle image of an env with a 'Z'
    on screen raises; those envs must be the envs whose flag word carries RG_FLAG_ERR_TILE, and rg_sync must fail iff there is one.  zed: some
    env must have shown a 'Z'."""
    torch = torch_mod()
    env = vec_env([dict(cfg, seed=i) for i in range(n)], kind, flag, with_hist, max_steps=max_steps)
    cmp = np.asarray(cmp)
    assert not kind or len(cmp) == n
    oracles = [OracleEnv(cfg, max_steps=max_steps, seed=int(i)) for i in cmp]
    idx = torch.as_tensor(cmp, device=env.device)
    rng = np.random.RandomState(seed)
    descents = errs = 0
    for t in range(0, steps + 1):
        if t:
            keys = STEP_KEYS[rng.randint(0, len(STEP_KEYS), n)]
            keys[cmp] = seeker_keys(oracles, rng)
            lv = [int(o.status_arr()[0]) for o in oracles]
            obs, _, _ = env.step_keys(device_keys(env, keys))
            for k, o in enumerate(oracles):
                o.step_autoreset(int(keys[cmp[k]]))
                descents += int(o.status_arr()[0]) > lv[k]
        else:
            obs = env.obs
        got = obs[idx].cpu().numpy()
        fl = env.flags[idx].cpu().numpy() if kind else None
        exp, bad = expected(oracles, kind, flag, with_hist)
        check_list(case, t, cmp, got, exp, bad, env._h, lambda k: oracles[k].screen(), fl)
        if kind:
            drain(env._h, bad)
            errs += bool(bad)
    if need_descent:
        assert descents > 0, "%s: no compared env descended" % case
    if zed:
        assert errs > 0, "%s: no compared env ever showed a 'Z'" % case
    env.close()
    return descents


@pytest.mark.timeout(150)
@pytest.mark.parametrize("geom", ["mini", "default", "48x20", "32x48", "160x48"])
def test_kobs_status_and_history_planes(goldens, geom):
    """Gray + StatusFlag.FULL + history (the general k_obs), compared at every step while descents and auto-resets happen: the HIST_STALE /
    HIST_LAG rule at the step it applies.  mini past its 16 384 looping one-wave blocks, 80x24 past its 8 192 blocks, two-wave (48x20),
    three-wave (32x48) and staged (160x48) blocks."""
    if geom == "mini":
        cfg, n = goldens["configs"]["mini"], 16384 + 2000
        cmp = np.r_[0:48, 16384:n]
        steps, max_steps = 40, 25
    elif geom == "default":
        cfg, n = goldens["configs"]["default"], 8192 + 1000
        cmp = np.r_[0:24, 8192:n:2]
        steps, max_steps = 30, 25
    else:
        w, h = (int(v) for v in geom.split("x"))
        rx, ry = {"48x20": (2, 2), "32x48": (1, 3), "160x48": (4, 4)}[geom]
        cfg, n = grid_cfg(w, h, rx, ry), 300 if w < 160 else 160
        cmp = np.arange(n)
        steps, max_steps = (40, 30) if w < 160 else (25, 25)
    play_planes("k_obs %s FULL+hist" % geom, cfg, n, cmp, steps, max_steps, 0, FULL, True, seed=len(geom))


# ---------------------------------------------------------------------------------------------
# 3. one-hot, and the 'Z' rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(150)
@pytest.mark.parametrize("name,planes", [("nohide", False), ("nohide", True), ("mini", False), ("mini", True), ("zed", True)])
def test_symbol_image_every_step(goldens, name, planes):
    """One-hot images of nohide 80x24 and mini, with and without FULL + history, every step; and a mini config whose common monster is a custom
    'Z': the envs whose oracle image raises are exactly the envs flagged RG_FLAG_ERR_TILE, every other env matches."""
    if name == "zed":
        cfg = dict(goldens["configs"]["mini"], enemies={"enemies": [ZED], "appear_rate_gold": 100, "appear_rate_nogold": 100}, hide_dungeon=False)
    else:
        cfg = goldens["configs"][name]
    n = 160 if name == "nohide" else 256
    steps = 16 if name == "nohide" and planes else 24
    flag, with_hist = (FULL, True) if planes else (0, False)
    play_planes("one-hot %s%s" % (name, " FULL+hist" if planes else ""), cfg, n, range(n), steps, 20, 1, flag, with_hist, seed=7 + planes,
                need_descent=False, zed=name == "zed")


# ---------------------------------------------------------------------------------------------
# 4. the bound tensor under every call cadence
# ---------------------------------------------------------------------------------------------
class Lockstep:
    """One OracleEnv per env of a handle, with the keys each has taken since its seed (a restored env's oracle is rebuilt by replay)."""

    def __init__(self, cfg, seeds, max_steps):
        self.cfg, self.max_steps = cfg, max_steps
        self.seeds = list(seeds)
        self.oracles = [OracleEnv(cfg, max_steps=max_steps, seed=s) for s in self.seeds]
        self.log = [[] for _ in self.seeds]

    def step(self, keys, n_keys=None):
        for i in range(len(self.oracles) if n_keys is None else n_keys):
            self.oracles[i].step_autoreset(int(keys[i]))
            self.log[i].append(int(keys[i]))

    def reset(self):
        for i, o in enumerate(self.oracles):
            o.reset()
            self.log[i] = ["reset"]

    def replay(self, dst, seed, log):
        o = OracleEnv(self.cfg, max_steps=self.max_steps, seed=seed)
        for k in log:
            if k == "reset":
                o.reset()
            else:
                o.step_autoreset(k)
        self.oracles[dst], self.log[dst] = o, list(log)


@pytest.mark.timeout(200)
@pytest.mark.parametrize("name,kind", [("mini", 0), ("default", 0), ("nohide", 1)])
def test_bound_tensor_every_cadence(goldens, name, kind):
    """persistent_obs=True against the oracle after every observation call: an observation every step; two rg_steps then one; rg_step_prefix
    with a short key vector; rg_step -> rg_reset -> observation; rg_step -> rg_seed + rg_reset -> observation; save / load / clone of states
    (envs 2k and 2k+1 share a seed, so a state cloned between them continues as its source's oracle)."""
    torch = torch_mod()
    cfg = goldens["configs"][name]
    n = 128 if name == "mini" else 64
    seeds = [i // 2 for i in range(n)]
    env = vec_env([dict(cfg, seed=s) for s in seeds], kind, persistent_obs=True, max_steps=30)
    lk = Lockstep(cfg, seeds, 30)
    L, h = env._h.L, env._h.h
    rng = np.random.RandomState(3 + kind)
    t = [0]

    def keys():
        return STEP_KEYS[rng.randint(0, len(STEP_KEYS), n)]

    def raw_step(k, n_keys=None):
        kd = device_keys(env, k)
        if n_keys is None:
            env._h.check(L.rg_step(h, C.c_void_p(kd.data_ptr()), 1))
        else:
            env._h.check(L.rg_step_prefix(h, C.c_void_p(kd.data_ptr()), n_keys, 1))
        lk.step(k, n_keys)

    def check(case, obs=None):
        t[0] += 1
        obs = env._encode() if obs is None else obs
        got = obs.cpu().numpy()
        exp, bad = expected(lk.oracles, kind, 0, False)
        check_list("bound %s %s: %s" % (name, "one-hot" if kind else "gray", case), t[0], np.arange(n), got, exp, bad, env._h, lambda e: lk.oracles[e].screen(),
                   env.flags.cpu().numpy())
        drain(env._h, bad)

    check("t=0", env.obs)
    for _ in range(6):
        k = keys()
        obs, _, _ = env.step_keys(device_keys(env, k))
        lk.step(k)
        check("observation every step", obs)
    for _ in range(3):
        raw_step(keys())
        raw_step(keys())
        check("two rg_steps, then one observation")
    for nk in (5, 1, n - 3):
        raw_step(keys()[:nk].copy(), nk)
        check("rg_step_prefix of %d keys" % nk)
        raw_step(keys())
        check("rg_step after a prefix step")
    for _ in range(2):
        raw_step(keys())
        env._h.check(L.rg_reset(h))
        lk.reset()
        check("rg_step -> rg_reset -> observation")
        raw_step(keys())
        check("rg_step after rg_step -> rg_reset")
    raw_step(keys())
    new = [100 + s for s in seeds]
    lo = (C.c_uint64 * n)(*new)
    env._h.check(L.rg_seed(h, lo, None, n))
    env._h.check(L.rg_reset(h))
    for i, o in enumerate(lk.oracles):
        o.set_seed(new[i])
    lk.reset()
    lk.seeds = new
    check("rg_step -> rg_seed + rg_reset -> observation")
    raw_step(keys())
    check("rg_step after rg_seed + rg_reset")
    # a state saved now, played on, and loaded back (no observation call between the step and the load)
    ids = list(range(0, n, 3))
    recs = env.save_state(ids)
    saved = {i: list(lk.log[i]) for i in ids}
    for _ in range(3):
        raw_step(keys())
    env.load_state(recs, ids)  # (returns the re-encoded observation; checked through a fresh observation call below)
    for i in ids:
        lk.replay(i, lk.seeds[i], saved[i])
    check("rg_step -> load_state -> observation")
    raw_step(keys())
    check("rg_step after load_state")
    # clone: env 2k -> env 2k+1 (the same seed)
    raw_step(keys())
    src = list(range(0, n, 2))
    dst = [i + 1 for i in src]
    obs = env.clone_state(src, dst)
    for s, d in zip(src, dst):
        lk.replay(d, lk.seeds[d], lk.log[s])
    check("rg_step -> clone_state", obs)
    for _ in range(4):
        k = keys()
        obs, _, _ = env.step_keys(device_keys(env, k))
        lk.step(k)
        check("observation every step after clone_state", obs)
    raw_step(keys())
    check("rg_step after clone_state")
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------
# 5. the crop, against the oracle's image gathered at the oracle's player cell
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(150)
@pytest.mark.parametrize("kind", [0, 1], ids=["gray", "one-hot"])
@pytest.mark.parametrize("radii", [(0, 0), (3, 5), (8, 8), (16, 40)])
def test_crop_every_step(goldens, kind, radii):
    """HipVecRogueEnv(crop=...) with FULL + history: the window equals the oracle's image padded with the encoding of ' ' and gathered at the
    oracle's player cell, and crop_center is that cell, for every env at every step (mini and nohide 80x24 in one batch: mixed sizes)."""
    ry, rx = radii
    mini, nohide = goldens["configs"]["mini"], goldens["configs"]["nohide"]
    n = 96
    cfgs = [dict(nohide if i % 3 == 2 else mini, seed=i) for i in range(n)]
    env = vec_env(cfgs, kind, FULL, True, crop=radii, max_steps=25)
    oracles = [OracleEnv(c, max_steps=25) for c in cfgs]
    rng = np.random.RandomState(ry * 100 + rx)
    planes = env.symbols if kind else 1
    case = "crop %s %dx%d" % ("one-hot" if kind else "gray", ry, rx)
    for t in range(0, 21):
        if t:
            keys = seeker_keys(oracles, rng)
            obs, _, _ = env.step_keys(device_keys(env, keys))
            for i, o in enumerate(oracles):
                o.step_autoreset(int(keys[i]))
        else:
            obs = env.obs
        got, cen = obs.cpu().numpy(), env.crop_center.cpu().numpy()
        for i, o in enumerate(oracles):
            sc = o.scalars()
            assert (int(cen[i, 0]), int(cen[i, 1])) == (sc["py"], sc["px"]), "%s step %d env %d: centre %s, oracle player (%d, %d)" % (case, t, i, cen[i], sc["py"], sc["px"])
            try:
                img = image(o, kind, FULL, True)
            except RuntimeError:  # (a 'Z' on the screen: the library raises only if it lies inside the window -- tests/test_gpu_crop.py)
                continue
            exp = crop_window(img, sc["py"], sc["px"], ry, rx, kind, planes, True)
            if not np.array_equal(got[i], exp):
                fail(case, t, i, got[i], exp, env._h, o.screen())
        env._h.L.rg_sync(env._h.h)  # (drains a possible tile error of such a window)
    env.close()


# ---------------------------------------------------------------------------------------------
# 6. config groups and the unfused fallbacks
# ---------------------------------------------------------------------------------------------
def mixed_configs(goldens, n):
    mini = goldens["configs"]["mini"]
    variants = [dict(mini), dict(mini, enemies={"enemies": []}),
                dict(mini, dungeon={"style": "rogue", "room_num_x": 1, "room_num_y": 2, "dark_level": 2, "maze_rate_inv": 3, "max_extra_edges": 2}),
                dict(mini, enemies={"enemies": [1, 18, 10], "appear_rate_gold": 95, "appear_rate_nogold": 70}, hide_dungeon=False)]
    order = np.random.RandomState(3).randint(0, len(variants), n)
    return [dict(variants[k], seed=4000 + i) for i, k in enumerate(order)]


@pytest.mark.timeout(150)
@pytest.mark.parametrize("case", ["groups", "50x21", "34x18", "160x48 66 rooms"])
def test_groups_and_fallbacks_every_step(goldens, case):
    """A handle over several configs (k_obs<.., GROUPS>), a 50x21 grid (k_render + k_encode_scalar), H*W % 8 == 4 (34x18: k_render + k_gray /
    k_symbol) and more than 64 rooms (160x48, 11x6 rooms: unfused), gray with FULL + history and one-hot, every step."""
    if case == "groups":
        all_cfgs = mixed_configs(goldens, 192)
    else:
        cfg = {"50x21": grid_cfg(50, 21, 3, 2), "34x18": grid_cfg(34, 18, 2, 2), "160x48 66 rooms": grid_cfg(160, 48, 11, 6)}[case]
        all_cfgs = [dict(cfg, seed=i) for i in range(48 if case.startswith("160") else 128)]
    steps = 12 if case.startswith("160") else 24
    for kind, flag, with_hist in ((0, FULL, True), (1, 0, False)):
        cfgs = all_cfgs
        if kind:  # (one-hot: only the configs with env 0's symbol count, which sets the handle's channel count; a config without monsters has fewer)
            sym = OracleEnv(all_cfgs[0]).symbols
            cfgs = [c for c in all_cfgs if OracleEnv(c).symbols == sym]
        env = vec_env(cfgs, kind, flag, with_hist, max_steps=20)
        oracles = [OracleEnv(c, max_steps=20) for c in cfgs]
        rng = np.random.RandomState(kind + 5)
        name = "%s %s" % (case, "gray FULL+hist" if not kind else "one-hot")
        for t in range(0, steps + 1):
            if t:
                keys = seeker_keys(oracles, rng)
                obs, _, _ = env.step_keys(device_keys(env, keys))
                for i, o in enumerate(oracles):
                    o.step_autoreset(int(keys[i]))
            else:
                obs = env.obs
            got = obs.cpu().numpy()
            exp, bad = expected(oracles, kind, flag, with_hist)
            check_list(name, t, np.arange(len(cfgs)), got, exp, bad, env._h, lambda e: oracles[e].screen())
            drain(env._h, bad)
        env.close()


# ---------------------------------------------------------------------------------------------
# 7. host and compact paths straight after rg_step
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(150)
@pytest.mark.parametrize("name", ["mini", "default"])
def test_host_and_compact_paths_after_step(goldens, name):
    """rg_obs_host, rg_pack_compact + rg_expand_compact (kinds 0 and 1, with and without history) and rg_status_vec(FULL), each straight after
    an rg_step of pending Redraws, against the oracle."""
    torch = torch_mod()
    from parity_util import HipBatch

    cfg = goldens["configs"][name]
    n = 64
    hip = HipBatch(cfg, range(n), max_steps=20)
    h, L = hip.h, hip.h.L
    oracles = [OracleEnv(cfg, max_steps=20, seed=i) for i in range(n)]
    rng = np.random.RandomState(9)
    rec = L.rg_compact_record_bytes(h.h, 1)
    packed = torch.empty((n, rec), dtype=torch.uint8, device="cuda:%d" % h.device)
    settings = [(0, FULL, True), (1, FULL, True), (0, 0, False), (1, 0, False), (1, 0x5, True)]
    for t in range(1, 25):
        keys = seeker_keys(oracles, rng)
        hip.step(keys)
        for i, o in enumerate(oracles):
            o.step_autoreset(int(keys[i]))
        kind, flag, with_hist = settings[t % len(settings)]
        exp = np.stack([image(o, kind, flag, with_hist) for o in oracles])
        if t % 3 == 0:
            st = np.empty(n * 9, np.int32)
            h.check(L.rg_status_vec(h.h, FULL, st.ctypes.data))
            for i, o in enumerate(oracles):
                assert [int(v) for v in st[9 * i:9 * i + 9]] == o.status_vec(FULL), "%s step %d env %d status_vec" % (name, t, i)
        if t % 2:
            out = np.empty(exp.shape, np.float32)
            h.check(L.rg_obs_host(h.h, kind, flag, int(with_hist), out.ctypes.data))
            check_batch("%s rg_obs_host %s" % (name, settings[t % len(settings)]), t, range(n), out, exp, h, lambda e: oracles[e].screen())
        else:
            ph = int(with_hist) if t % 4 else 1
            h.check(L.rg_pack_compact(h.h, ph, C.c_void_p(packed.data_ptr())))
            out = torch.empty(exp.shape, dtype=torch.float32, device=packed.device)
            h.check(L.rg_expand_compact(h.h, C.c_void_p(packed.data_ptr()), n, ph, kind, flag, int(with_hist), C.c_void_p(out.data_ptr())))
            check_batch("%s compact %s packed_hist=%d" % (name, settings[t % len(settings)], ph), t, range(n), out.cpu().numpy(), exp, h,
                        lambda e: oracles[e].screen())
    hip.sync()
    h.close()


@pytest.mark.timeout(120)
def test_encode_host_batch_of_oracle_screens(goldens):
    """rg_encode_host_batch fed the oracle's own screens, history and status (mini, 80x24 and 50x21, gray and one-hot, every plane) equals the
    oracle's images; a screen with a 'Z' is refused."""
    from rogue_gym_python import _rogue_gym as inner

    L = inner.load_library()
    dev = inner._default_device()
    rng = np.random.RandomState(4)
    for cfg in (goldens["configs"]["mini"], goldens["configs"]["default"], grid_cfg(50, 21, 3, 2)):
        oracles = [OracleEnv(cfg, max_steps=30, seed=i) for i in range(24)]
        for _ in range(rng.randint(5, 40)):
            keys = seeker_keys(oracles, rng)
            for i, o in enumerate(oracles):
                o.step_autoreset(int(keys[i]))
        scr = np.ascontiguousarray(np.stack([o.screen() for o in oracles]))
        hist = np.ascontiguousarray(np.stack([o.hist() for o in oracles]))
        st = np.ascontiguousarray(np.stack([o.status_arr() for o in oracles]).astype(np.int32))
        hh, ww, sym = scr.shape[1], scr.shape[2], oracles[0].symbols
        for kind, flag, with_hist in ((0, FULL, True), (1, FULL, True), (1, 0x22, False), (0, 0, False)):
            exp = np.stack([image(o, kind, flag, with_hist) for o in oracles])
            out = np.empty(exp.shape, np.float32)
            rc = L.rg_encode_host_batch(dev, len(oracles), scr.ctypes.data, hist.ctypes.data, st.ctypes.data, hh, ww, sym, flag, int(with_hist), kind, out.ctypes.data)
            assert rc == 0, L.rg_last_error(None)
            for i, o in enumerate(oracles):
                if not np.array_equal(out[i], exp[i]):
                    p, y, x = (int(v) for v in np.argwhere(out[i] != exp[i])[0])
                    raise AssertionError("encode_host_batch %dx%d %s env %d first at (plane %d, y %d, x %d)\n%s" % (ww, hh, (kind, flag, with_hist), i, p, y, x, text(o.screen())))
    zscr = scr.copy()
    zscr[3, 1, 1] = ord("Z")
    out = np.empty((len(oracles), sym, hh, ww), np.float32)
    assert L.rg_encode_host_batch(dev, len(oracles), zscr.ctypes.data, hist.ctypes.data, st.ctypes.data, hh, ww, sym, 0, 0, 1, out.ctypes.data) != 0
    assert b"Invalid tile" in L.rg_last_error(None)
