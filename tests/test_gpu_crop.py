"""Player-centred cropped observations (rg_obs_crop; HipVecRogueEnv(crop=...)).  The expected crop is always built in torch from the library's own full
encode (which tests/test_gpu_obs_oracle.py pins to the oracle at every step; that module also checks the crop itself against the oracle): the full image padded with the encoding of a blank cell ' ', then gathered at the window centres.  Benchmark shape,
the 80x24 dungeon with descents, edges, pending Redraws, the bound observation tensor, config groups and mixed sizes, refusals and the 'Z' rule, and
batches and config groups that end in a short run of envs, between guard bytes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL = 0x1FF


def torch_mod():
    import torch

    return torch


def seeded(cfg, seeds):
    return [dict(cfg, seed=int(s)) for s in seeds]


def full_image(h, kind, flag, with_hist):
    """The library's full image f32 [n, C, H, W] of every env, now (rg_obs_gray / rg_obs_symbol)."""
    torch = torch_mod()
    c = h.L.rg_obs_channels(h.h, kind, flag, int(with_hist))
    out = torch.empty((h.n, c, h.height, h.width), dtype=torch.float32, device="cuda:%d" % h.device)
    fn = h.L.rg_obs_symbol if kind else h.L.rg_obs_gray
    h.check(fn(h.h, flag, int(with_hist), C.c_void_p(out.data_ptr())))
    return out


def crop_call(h, kind, ry, rx, flag, with_hist):
    """rg_obs_crop into fresh tensors: (crop f32 [n, C, 2ry+1, 2rx+1], centres i32 [n, 2])."""
    torch = torch_mod()
    c = h.L.rg_obs_channels(h.h, kind, flag, int(with_hist))
    dev = "cuda:%d" % h.device
    out = torch.full((h.n, c, 2 * ry + 1, 2 * rx + 1), float("nan"), dtype=torch.float32, device=dev)
    cen = torch.full((h.n, 2), -1, dtype=torch.int32, device=dev)
    h.check(h.L.rg_obs_crop(h.h, kind, ry, rx, flag, int(with_hist), C.c_void_p(out.data_ptr()), C.c_void_p(cen.data_ptr())))
    return out, cen


def expect(full, centers, ry, rx, kind, planes, with_hist):
    """Pad `full` [N, C, H, W] with the encoding of ' ' (gray 0; one-hot channel 0 = 1, the rest 0; status planes their constant; history 0) and
    gather the [2ry+1, 2rx+1] window at centres (y, x)."""
    torch = torch_mod()
    n, c, hh, ww = full.shape
    pad = torch.zeros((n, c, hh + 2 * ry, ww + 2 * rx), dtype=full.dtype, device=full.device)
    if kind:
        pad[:, 0] = 1.0
    nst = c - planes - (1 if with_hist else 0)
    if nst > 0:
        pad[:, planes:planes + nst] = full[:, planes:planes + nst, :1, :1]
    pad[:, :, ry:ry + hh, rx:rx + ww] = full
    cen = centers.to(device=full.device, dtype=torch.int64)
    rows = cen[:, 0, None] + torch.arange(2 * ry + 1, device=full.device)
    cols = cen[:, 1, None] + torch.arange(2 * rx + 1, device=full.device)
    t = pad.gather(2, rows[:, None, :, None].expand(n, c, 2 * ry + 1, ww + 2 * rx))
    return t.gather(3, cols[:, None, None, :].expand(n, c, 2 * ry + 1, 2 * rx + 1))


def check_crop(h, kind, ry, rx, flag, with_hist, got=None, centers=None, where=""):
    """Crop (given, or by a fresh rg_obs_crop call) == the padded full image gathered at the centres; returns the centres."""
    torch = torch_mod()
    if got is None:
        got, centers = crop_call(h, kind, ry, rx, flag, with_hist)
    full = full_image(h, kind, flag, with_hist)
    planes = h.symbols if kind else 1
    exp = expect(full, centers, ry, rx, kind, planes, with_hist)
    assert got.shape == exp.shape, (where, got.shape, exp.shape)
    if not torch.equal(got, exp):
        bad = (got != exp).reshape(got.shape[0], -1).any(1).nonzero().flatten()
        raise AssertionError("%s: crop differs from the padded full image in %d envs, first %s" % (where, bad.numel(), bad[:8].tolist()))
    return centers


def centres_match_player_glyph(screen, centers):
    """Wherever '@' is drawn on the screen mirror, it is at the window centre."""
    torch = torch_mod()
    n, hh, ww = screen.shape
    at = screen == ord("@")
    has = at.reshape(n, -1).any(1)
    idx = at.reshape(n, -1).to(torch.int32).argmax(1)
    y, x = idx // ww, idx % ww
    cen = centers.to(device=screen.device, dtype=torch.int64)
    ok = (y == cen[:, 0]) & (x == cen[:, 1])
    assert bool(ok[has].all()), "centre != '@' cell in %d envs" % int((~ok & has).sum())
    return float(has.float().mean())


def random_keys(env, gen):
    torch = torch_mod()
    return env._action_keys[torch.randint(0, len(env.ACTIONS), (env.num_envs,), generator=gen, device="cpu").to(env.device)]


def stair_seeker_keys(env, gen):
    """'>' where the stairs are not in sight (the player may stand on them), a greedy step towards a '%' in sight, one key in four at random:
    deep enough to produce descents and stale-history levels on the 80x24 dungeon."""
    torch = torch_mod()
    scr = env.screen
    n, hh, ww = scr.shape
    st = scr == ord("%")
    has = st.reshape(n, -1).any(1)
    idx = st.reshape(n, -1).to(torch.int32).argmax(1)
    sy, sx = idx // ww, idx % ww
    cy, cx = env.crop_center[:, 0].long(), env.crop_center[:, 1].long()
    dy, dx = torch.sign(sy - cy), torch.sign(sx - cx)
    table = torch.tensor([ord(k) for k in "yku" "h>l" "bjn"], dtype=torch.uint8, device=env.device)
    keys = torch.where(has, table[(dy + 1) * 3 + (dx + 1)], torch.full_like(table[:1].expand(n), ord(">")))
    rnd = random_keys(env, gen)
    pick = torch.rand(n, generator=gen).to(env.device) < 0.25
    return torch.where(pick, rnd, keys).contiguous()


def test_crop_benchmark_shape(goldens):
    """65 536 mini envs (full 64-env step waves), random policy with auto-resets, gray crop 4x4 every 10 steps; the centres against the player's
    position (rg_debug_fetch, envs on a stride coprime to 64) and against the '@' cell of the screen."""
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv

    n = 65536
    env = HipVecRogueEnv(seeded(goldens["configs"]["mini"], range(n)), max_steps=60, crop=4)
    assert tuple(env.obs.shape) == (n, 1, 9, 9) and tuple(env.crop_center.shape) == (n, 2) and env.crop_center.dtype == torch.int32
    gen = torch.Generator().manual_seed(1)
    check_crop(env._h, 0, 4, 4, 0, False, env.obs, env.crop_center, "t=0")
    shown = []
    for t in range(1, 301):
        env.step(torch.randint(0, len(env.ACTIONS), (n,), generator=gen).to(env.device))
        if t % 10 == 0:
            check_crop(env._h, 0, 4, 4, 0, False, env.obs, env.crop_center, "t=%d" % t)
            shown.append(centres_match_player_glyph(env.screen, env.crop_center))
        if t in (150, 300):
            cen = env.crop_center.cpu().numpy()
            for i in range(0, n, 61):
                d, _ = env._h.debug_state(i)
                assert (int(cen[i, 0]), int(cen[i, 1])) == (d.py, d.px), (t, i)
    assert min(shown) > 0.5, shown
    env.check_errors()
    env.close()


def test_crop_default_dungeon_descents(goldens):
    """80x24: one-hot with every status plane and the history plane, crop 5x5, every step for 300 steps under a stair-seeking policy (descents and
    stale-history levels); gray with the history plane alongside."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    n = 2048
    env = HipVecRogueEnv(seeded(goldens["configs"]["default"], range(100, 100 + n)), max_steps=500,
                         image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.FULL, True), crop=5)
    h = env._h
    assert tuple(env.obs.shape) == (n, h.symbols + 9 + 1, 11, 11)
    gen = torch.Generator().manual_seed(2)
    deepest = torch.ones(n, dtype=torch.int32, device=env.device)
    for t in range(300):
        env.step_keys(stair_seeker_keys(env, gen))
        check_crop(h, 1, 5, 5, FULL, True, env.obs, env.crop_center, "symbol t=%d" % t)
        _, cen = crop_call(h, 0, 5, 5, 0, True)
        assert torch.equal(cen, env.crop_center)
        check_crop(h, 0, 5, 5, 0, True, where="gray t=%d" % t)
        deepest = torch.maximum(deepest, env.status[:, 0])
    assert int(deepest.max()) >= 3 and int((deepest >= 2).sum()) >= 20, (int(deepest.max()), int((deepest >= 2).sum()))
    h.L.rg_sync(h.h)  # (drain a possible tile error: a 'Z' is a legal monster of this config, and not a symbol)
    env.close()


def test_crop_edges(goldens):
    """A window larger than the screen (mini, ry = 20, rx = 40): every screen cell appears exactly once, the rest is blank; radius 0 is the
    player's cell; a window of the largest radii."""
    torch = torch_mod()
    from parity_util import HipBatch

    n = 256
    hip = HipBatch(goldens["configs"]["mini"], range(n), max_steps=80)
    h = hip.h
    rng = np.random.RandomState(3)
    for _ in range(40):
        hip.step(np.frombuffer(b".hjklnbuy>s", np.uint8)[rng.randint(0, 11, n)])
    for kind, flag, with_hist in ((0, 0, True), (1, FULL, True), (0, 0b101, False)):
        got, cen = crop_call(h, kind, 20, 40, flag, with_hist)
        check_crop(h, kind, 20, 40, flag, with_hist, got, cen, "big kind=%d" % kind)
        full = full_image(h, kind, flag, with_hist)
        if kind:  # the non-blank symbol channels hold every screen cell exactly once
            planes = h.symbols
            assert torch.equal(got[:, 1:planes].sum((1, 2, 3)), full[:, 1:planes].sum((1, 2, 3)))
        # the screen block sits at (ry - cy, rx - cx) of the window; outside it every glyph plane is blank
        c0 = cen.long()
        blank = torch.ones((n, 41, 81), dtype=torch.bool, device=got.device)
        ys = (20 - c0[:, 0, None] + torch.arange(16, device=got.device))
        xs = (40 - c0[:, 1, None] + torch.arange(32, device=got.device))
        blank[torch.arange(n, device=got.device)[:, None, None], ys[:, :, None], xs[:, None, :]] = False
        assert int((~blank).sum()) == n * 16 * 32
        out_plane = got[:, 0][blank]
        assert bool((out_plane == (1.0 if kind else 0.0)).all())
        if with_hist:
            assert bool((got[:, -1][blank] == 0).all())
    for kind, flag, with_hist in ((0, FULL, True), (1, 0, False)):
        got, cen = crop_call(h, kind, 0, 0, flag, with_hist)
        assert got.shape[2:] == (1, 1)
        check_crop(h, kind, 0, 0, flag, with_hist, got, cen, "r0 kind=%d" % kind)
        full = full_image(h, kind, flag, with_hist)
        idx = torch.arange(n, device=got.device)
        assert torch.equal(got[:, :, 0, 0], full[idx, :, cen[:, 0].long(), cen[:, 1].long()])
    got, cen = crop_call(h, 1, 47, 159, FULL, True)
    check_crop(h, 1, 47, 159, FULL, True, got, cen, "max radii")
    hip.sync()
    h.close()


def test_crop_draws_pending_redraws(goldens):
    """A crop straight after rg_step with no encode in between, after rg_reset, after rg_debug_descend and after load_state of another env's
    record: the pending Redraws are drawn first."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    n = 512
    cfg = dict(goldens["configs"]["mini"], enemies={"enemies": list(range(12))})
    env = HipVecRogueEnv(seeded(cfg, range(n)), max_steps=100, image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.FULL, True), crop=(3, 4))
    h, L = env._h, env._h.L
    gen = torch.Generator().manual_seed(4)
    for t in range(30):  # HipVecRogueEnv: rg_step, then the crop
        env.step_keys(random_keys(env, gen))
        check_crop(h, 1, 3, 4, FULL, True, env.obs, env.crop_center, "step t=%d" % t)
    for t in range(5):  # the raw calls: rg_step, rg_obs_crop
        h.check(L.rg_step(h.h, C.c_void_p(random_keys(env, gen).data_ptr()), 1))
        check_crop(h, 0, 6, 2, 0b11, True, where="raw step t=%d" % t)
    env.reset()
    check_crop(h, 1, 3, 4, FULL, True, env.obs, env.crop_center, "reset")
    lvl = env.status[:, 0].clone()
    h.check(L.rg_debug_descend(h.h))
    env._encode()
    check_crop(h, 1, 3, 4, FULL, True, env.obs, env.crop_center, "descend")
    assert bool((env.status[:, 0] == lvl + 1).all())
    for _ in range(10):
        env.step_keys(random_keys(env, gen))
    recs = env.save_state([7] * 64 + [300] * 64)
    ids = list(range(100, 228))
    obs = env.load_state(recs, ids)
    check_crop(h, 1, 3, 4, FULL, True, obs, env.crop_center, "load_state")
    cen = env.crop_center.cpu().numpy()
    assert (cen[100:164] == cen[7]).all() and (cen[164:228] == cen[300]).all()
    assert torch.equal(env.obs[100:164], env.obs[7:8].expand(64, -1, -1, -1))
    L.rg_sync(h.h)
    env.close()


def test_crop_leaves_bound_tensor(goldens):
    """A persistent_obs handle with crop calls between its steps (after the observation, and between rg_step and the observation): its bound
    `obs` stays equal to an unbound twin's at every step."""
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv

    n = 4096
    cfgs = seeded(goldens["configs"]["mini"], range(n))
    bound = HipVecRogueEnv(cfgs, max_steps=50, persistent_obs=True)
    twin = HipVecRogueEnv(cfgs, max_steps=50)
    h, L = bound._h, bound._h.L
    gen = torch.Generator().manual_seed(5)
    assert torch.equal(bound.obs, twin.obs)
    for t in range(120):
        keys = random_keys(bound, gen)
        if t % 2 == 0:
            bound.step_keys(keys)
            got, cen = crop_call(h, 0, 3, 3, 0, False)
        else:
            h.check(L.rg_step(h.h, C.c_void_p(keys.data_ptr()), 1))
            got, cen = crop_call(h, 1, 2, 5, 0, True)
            bound._encode()
        twin.step_keys(keys)
        assert torch.equal(bound.obs, twin.obs), "bound tensor differs at t=%d" % t
        if t % 2 == 0:
            assert torch.equal(got, expect(twin.obs, cen, 3, 3, 0, 1, False)), t
    bound.close()
    twin.close()


def _ragged_expected(env, setting, ry, rx, kind, planes, with_hist):
    """The crop of every env's own full image, from rg_fetch_states' ragged host copies through ImageSetting.expand (grouped by screen size)."""
    torch = torch_mod()
    states = env._h.snapshot()
    imgs = [np.asarray(setting.expand(states[i]), np.float32) for i in range(env.num_envs)]
    cen = env.crop_center.cpu()
    exp = torch.empty(tuple(env.obs.shape), dtype=torch.float32)
    screens = []
    for shape in sorted({im.shape for im in imgs}):
        idx = [i for i, im in enumerate(imgs) if im.shape == shape]
        full = torch.from_numpy(np.stack([imgs[i] for i in idx]))
        exp[idx] = expect(full, cen[idx], ry, rx, kind, planes, with_hist)
        screens.append((idx, torch.from_numpy(np.stack([np.asarray(states.screen[i], np.uint8) for i in idx]))))
    return exp, screens


def test_crop_groups_and_mixed_sizes(goldens):
    """A handle with config groups and a mixed-size handle (mini + 80x24 + 48x20): HipVecRogueEnv(crop=...) builds on the mixed one, and each env's
    crop equals the crop of its own full image.  A config group with more symbols than env 0's is refused for the one-hot kind."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    mini = goldens["configs"]["mini"]
    gen = torch.Generator().manual_seed(6)
    # config groups of one size: on the device, against the library's own full encode
    variants = [dict(mini), dict(mini, enemies={"enemies": []}), dict(mini, enemies={"enemies": [1, 18, 10], "appear_rate_gold": 95, "appear_rate_nogold": 70},
                                                                      hide_dungeon=False)]
    order = np.random.RandomState(6).randint(0, 3, 300)
    order[0] = 0
    env = HipVecRogueEnv([dict(variants[k], seed=5000 + i) for i, k in enumerate(order)], max_steps=60,
                         image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.FULL, True), crop=(3, 5))
    for t in range(40):
        env.step_keys(random_keys(env, gen))
        if t % 8 == 7:
            check_crop(env._h, 1, 3, 5, FULL, True, env.obs, env.crop_center, "groups t=%d" % t)
            check_crop(env._h, 0, 4, 2, 0b1, True, where="groups gray t=%d" % t)
    centres_match_player_glyph(env.screen, env.crop_center)
    env._h.L.rg_sync(env._h.h)
    env.close()
    # mixed sizes: no [N, H, W] tensor, but one crop tensor
    enemies = {"enemies": list(range(10))}
    shapes = [dict(mini, enemies=enemies), {"width": 80, "height": 24, "enemies": enemies},
              {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": enemies}]
    n = 96
    cfgs = [dict(shapes[i % 3], seed=6000 + i) for i in range(n)]
    for setting, kind, crop in ((ImageSetting(DungeonType.GRAY, StatusFlag.FULL, True), 0, (4, 6)),
                                (ImageSetting(DungeonType.SYMBOL, StatusFlag.DUNGEON_LEVEL, True), 1, (2, 3))):
        env = HipVecRogueEnv(cfgs, max_steps=80, image_setting=setting, crop=crop)
        assert env._h.mixed_sizes and tuple(env.obs.shape) == (n, env.channels, 2 * crop[0] + 1, 2 * crop[1] + 1)
        with pytest.raises(RuntimeError, match="differ in width / height"):
            env.screen
        planes = env._h.symbols if kind else 1
        for t in range(30):
            env.step_keys(random_keys(env, gen))
            if t % 10 == 9:
                exp, screens = _ragged_expected(env, setting, crop[0], crop[1], kind, planes, True)
                assert torch.equal(env.obs.cpu(), exp), "mixed kind=%d t=%d" % (kind, t)
                for idx, scr in screens:
                    centres_match_player_glyph(scr, env.crop_center.cpu()[idx])
        env.check_errors()
        env.close()
    # the one-hot depth is env 0's: a group with more symbols is refused, as by rg_obs_symbol
    env = HipVecRogueEnv([dict(mini, seed=1, enemies={"enemies": []}), dict(mini, seed=2)], crop=2)
    h = env._h
    with pytest.raises(RuntimeError, match="more symbols"):
        crop_call(h, 1, 2, 2, 0, False)
    with pytest.raises(RuntimeError, match="more symbols"):
        full_image(h, 1, 0, False)
    check_crop(h, 0, 2, 2, 0, False, where="gray with more symbols")
    env.close()


def test_crop_refusals_and_invalid_tiles(goldens):
    """Bad radii, a bad kind, a null output and crop + persistent_obs are refused; a 'Z' glyph (a custom monster shown as 'Z': not a symbol)
    raises as rg_obs_symbol does when it lies inside the window, and not when it lies outside."""
    torch = torch_mod()
    from parity_util import HipBatch
    from rogue_gym.envs.device import HipVecRogueEnv

    mini = goldens["configs"]["mini"]
    hip = HipBatch(mini, range(64))
    h, L = hip.h, hip.h.L
    out = torch.empty((64, 1, 95, 319), dtype=torch.float32, device="cuda:%d" % h.device)
    for kind, ry, rx in ((0, -1, 0), (0, 0, -1), (0, 48, 0), (1, 0, 160), (2, 1, 1), (-1, 1, 1)):
        assert L.rg_obs_crop(h.h, kind, ry, rx, 0, 0, C.c_void_p(out.data_ptr()), None) != 0, (kind, ry, rx)
        assert b"rg_obs_crop" in L.rg_last_error(h.h), (kind, ry, rx)
    assert L.rg_obs_crop(h.h, 0, 1, 1, 0, 0, None, None) != 0
    assert L.rg_obs_crop(h.h, 0, 47, 159, 0, 0, C.c_void_p(out.data_ptr()), None) == 0  # the largest radii; centres are optional
    h.close()
    with pytest.raises(ValueError, match="persistent_obs"):
        HipVecRogueEnv(seeded(mini, range(4)), persistent_obs=True, crop=2)
    for bad in (-1, (2, -3), "x", (1.5, 2)):
        with pytest.raises(ValueError, match="crop"):
            HipVecRogueEnv(seeded(mini, range(4)), crop=bad)
    # a common monster shown as 'Z' (symbol 42 of 43: no channel) -> InvalidTileError
    zed = {"attack": [], "attr": 0, "defense": 1, "exp": 1, "gold": 0, "level": 1, "name": "zed", "tile": 90, "rarelity": 0}
    cfg = dict(mini, enemies={"enemies": [zed], "appear_rate_gold": 100, "appear_rate_nogold": 100}, hide_dungeon=False)
    n = 256
    hip = HipBatch(cfg, range(n))
    h, L = hip.h, hip.h.L
    screen, _, _, _ = hip.fetch()
    has_z = (screen == ord("Z")).reshape(n, -1).any(1)
    assert has_z.sum() > 0, "no 'Z' on any screen"
    with pytest.raises(RuntimeError, match="Invalid tile"):
        full_image(h, 1, 0, False)
        hip.sync()
    _, cen = crop_call(h, 1, 0, 0, 0, False)  # the player's cell only: never a 'Z'
    hip.sync()
    # a window that holds the whole screen: raises ...
    crop_call(h, 1, 16, 32, 0, False)
    with pytest.raises(RuntimeError, match="Invalid tile"):
        hip.sync()
    # ... and so does the smallest window that holds a 'Z' of one env
    cen = cen.cpu().numpy()
    e = int(np.argmax(has_z))
    zy, zx = np.nonzero(screen[e] == ord("Z"))
    r_in = int(np.maximum(np.abs(zy - cen[e, 0]), np.abs(zx - cen[e, 1])).min())
    assert r_in >= 1
    crop_call(h, 1, r_in, r_in, 0, False)
    with pytest.raises(RuntimeError, match="Invalid tile"):
        hip.sync()
    h.close()


GUARD = 64  # bytes of a known pattern on either side of a crop tensor


def guarded_crop_call(h, kind, ry, rx, flag, with_hist):
    """rg_obs_crop into a tensor that lies between two guards of GUARD bytes of 0xA5 inside one allocation (the tensor itself starts as NaNs):
    (crop f32 [n, C, 2ry+1, 2rx+1], centres i32 [n, 2]); the guards are checked to be untouched."""
    torch = torch_mod()
    c = h.L.rg_obs_channels(h.h, kind, flag, int(with_hist))
    dev = "cuda:%d" % h.device
    shape = (h.n, c, 2 * ry + 1, 2 * rx + 1)
    nbytes = 4 * int(np.prod(shape))
    raw = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    raw[GUARD:GUARD + nbytes] = 0xFF
    out = raw[GUARD:GUARD + nbytes].view(torch.float32).view(shape)
    assert out.data_ptr() % 16 == 0
    cen = torch.full((h.n, 2), -1, dtype=torch.int32, device=dev)
    h.check(h.L.rg_obs_crop(h.h, kind, ry, rx, flag, int(with_hist), C.c_void_p(out.data_ptr()), C.c_void_p(cen.data_ptr())))
    assert bool((raw[:GUARD] == 0xA5).all()), "the crop wrote in front of its tensor"
    assert bool((raw[GUARD + nbytes:] == 0xA5).all()), "the crop wrote past its tensor"
    return out, cen


# radius_y, radius_x, status flag, history plane
SHORT_RUN_WINDOWS = ((0, 0, 0, False), (1, 1, 0, False), (5, 5, 0, False), (3, 4, FULL, True))


@pytest.mark.parametrize("n", [1, 7, 67])
def test_crop_short_last_run(goldens, n):
    """Env counts that are no multiple of the run length (a wave serves 4 or more envs), so the batch ends in a short run whose last 16-byte piece is
    written element by element: both kinds, four windows, after each of a dozen random steps, against the padded full image; nothing is written
    outside the tensor."""
    from parity_util import ACTION_KEYS, HipBatch

    hip = HipBatch(goldens["configs"]["mini"], range(700, 700 + n), max_steps=80)
    rng = np.random.RandomState(n)
    for t in range(12):
        hip.step(ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)])
        for kind in (0, 1):
            for ry, rx, flag, with_hist in SHORT_RUN_WINDOWS:
                got, cen = guarded_crop_call(hip.h, kind, ry, rx, flag, with_hist)
                check_crop(hip.h, kind, ry, rx, flag, with_hist, got, cen, "n=%d t=%d kind=%d window=(%d, %d)" % (n, t, kind, ry, rx))
    hip.sync()
    hip.h.close()


def test_crop_short_runs_of_config_groups(goldens):
    """Ten envs of three screen sizes on one handle, in groups of 3, 5 and 2 envs: every group's only run is short and every element is stored by itself
    at the handle's env index.  Each env's crop equals the crop of its own full image; nothing is written outside the tensor."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    enemies = {"enemies": list(range(10))}
    shapes = [dict(goldens["configs"]["mini"], enemies=enemies), {"width": 80, "height": 24, "enemies": enemies},
              {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": enemies}]
    order = [0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    cfgs = [dict(shapes[k], seed=6100 + i) for i, k in enumerate(order)]
    gen = torch.Generator().manual_seed(7)
    for setting, kind, flag, crop in ((ImageSetting(DungeonType.GRAY, StatusFlag.FULL, True), 0, FULL, (3, 4)),
                                      (ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False), 1, 0, (5, 5))):
        env = HipVecRogueEnv(cfgs, max_steps=80, image_setting=setting, crop=crop)
        assert env._h.mixed_sizes
        planes = env._h.symbols if kind else 1
        with_hist = bool(setting.includes_hist)
        for t in range(12):
            env.step_keys(random_keys(env, gen))
            exp, _ = _ragged_expected(env, setting, crop[0], crop[1], kind, planes, with_hist)
            got, cen = guarded_crop_call(env._h, kind, crop[0], crop[1], flag, with_hist)
            assert torch.equal(cen, env.crop_center), (kind, t)
            assert torch.equal(got.cpu(), exp), "groups kind=%d t=%d" % (kind, t)
            assert torch.equal(env.obs.cpu(), exp), "groups kind=%d t=%d (the env's own crop)" % (kind, t)
        env.check_errors()
        env.close()
