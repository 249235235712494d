"""rg_obs_pixels / rg_obs_pixels_crop on the device against the numpy rule (tests/pixel_util.py) on the screen mirror read back after every step, and the
entry points' contract: sentinels, corners and edges, crop = slice of the padded full image, config groups and mixed sizes, twin handles, the step forms,
the tileset, and the Python surface."""
import ctypes as C

import numpy as np
import pytest

import grid_util as gu
import pixel_util as pu
from parity_util import ACTION_KEYS, HipBatch

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5


def torch_mod():
    import torch
    return torch


def grid_cfg(w, h, rx, ry):
    return {"width": w, "height": h, "dungeon": {"style": "rogue", "room_num_x": rx, "room_num_y": ry, "min_room_size": {"x": 4, "y": 4}}}


def use_torch_stream(h):
    h.check(h.L.rg_set_stream(h.h, C.c_void_p(torch_mod().cuda.current_stream().cuda_stream)))


def set_tileset(h, font, pal):
    h.check(h.L.rg_tileset_set(h.h, font.shape[1], np.ascontiguousarray(font).ctypes.data, np.ascontiguousarray(pal).ctypes.data))


def pixel_call(h, th, channels, window=None, keys=None, hw=None):
    """The pass into a fresh buffer with GUARD sentinel bytes before the first env and behind the last: (u8 [n, C, hp, wp] on the host, centres or None).
    keys (a device tensor): the step form."""
    torch = torch_mod()
    dev = "cuda:%d" % h.device
    H, W = (h.height, h.width) if hw is None else hw
    hc, wc = (H, W) if window is None else (2 * window[0] + 1, 2 * window[1] + 1)
    shape = (h.n, channels, hc * th, wc * 8)
    nbytes = int(np.prod(shape))
    raw = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    out = raw[GUARD:GUARD + nbytes]
    assert out.data_ptr() % 16 == 0
    cen = None if window is None else torch.full((h.n, 2), -1, dtype=torch.int32, device=dev)
    L, p = h.L, C.c_void_p(out.data_ptr())
    if window is None:
        h.check(L.rg_obs_pixels(h.h, channels, p) if keys is None else L.rg_step_obs_pixels(h.h, C.c_void_p(keys.data_ptr()), 1, channels, p))
    else:
        pc = C.c_void_p(cen.data_ptr())
        h.check(L.rg_obs_pixels_crop(h.h, channels, window[0], window[1], p, pc) if keys is None else
                L.rg_step_obs_pixels_crop(h.h, C.c_void_p(keys.data_ptr()), 1, channels, window[0], window[1], p, pc))
    host = raw.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all(), "sentinel bytes before the first env were written"
    assert (host[GUARD + nbytes:] == SENTINEL).all(), "sentinel bytes behind the last env were written"
    return host[GUARD:GUARD + nbytes].reshape(shape), (None if cen is None else cen.cpu().numpy())


def crop_centers(h):
    """crop_center of an rg_obs_crop call (gray, the smallest window)."""
    torch = torch_mod()
    dev = "cuda:%d" % h.device
    out = torch.empty((h.n, 1, 1, 1), dtype=torch.float32, device=dev)
    cen = torch.full((h.n, 2), -1, dtype=torch.int32, device=dev)
    h.check(h.L.rg_obs_crop(h.h, 0, 0, 0, 0, 0, C.c_void_p(out.data_ptr()), C.c_void_p(cen.data_ptr())))
    return cen.cpu().numpy()


def assert_same(got, want, where):
    assert got.shape == want.shape, (where, got.shape, want.shape)
    if not np.array_equal(got, want):
        e, c, y, x = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError("%s: %d bytes differ from the numpy rule, first env %d channel %d row %d column %d: %d vs %d" % (
            where, int((got != want).sum()), e, c, y, x, got[e, c, y, x], want[e, c, y, x]))


def records(h):
    torch = torch_mod()
    R = h.L.rg_state_record_bytes(h.h)
    recs = torch.empty((h.n, R), dtype=torch.uint8, device="cuda:%d" % h.device)
    h.check(h.L.rg_state_save(h.h, None, h.n, 0, C.c_void_p(recs.data_ptr())))
    return recs.cpu().numpy()


def dev_keys(h, keys):
    return torch_mod().as_tensor(np.ascontiguousarray(keys), device="cuda:%d" % h.device)


# ---------------------------------------------------------------------------------------------
# 1. device against the numpy rule, every step
# ---------------------------------------------------------------------------------------------
CASES = {"mini": (None, 135, 60), "33x17": ((33, 17, 2, 2), 71, 40), "80x24": ((80, 24, 3, 3), 71, 40), "97x33": ((97, 33, 3, 3), 71, 40),
         "mini n=1": (None, 1, 12), "mini n=65": (None, 65, 12)}
WINDOWS = [(0, 0), (5, 5), (1, 7)]


@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_numpy_rule_every_step(goldens, case):
    """Random policy with enemies.  Every step: one window (rotating through the radii) and, every fourth step, the whole screen -- the tile height, the
    channel count and the tileset itself rotate too, so every (th, channels, form) pair is compared many times on changing screens."""
    shape, n, steps = CASES[case]
    cfg = goldens["configs"]["mini"] if shape is None else grid_cfg(*shape)
    hip = HipBatch(cfg, range(300, 300 + n), max_steps=25)
    h = hip.h
    use_torch_stream(h)
    rng = np.random.RandomState(11)
    tiles = {th: pu.random_tileset(np.random.RandomState(th), th) for th in pu.TILE_HEIGHTS}
    seen = set()
    for t in range(steps + 1):
        if t:
            hip.step(ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)])
        th = pu.TILE_HEIGHTS[t % 3]
        font, pal = tiles[th]
        set_tileset(h, font, pal)
        channels = (1, 3)[(t // 3) % 2]
        window = WINDOWS[(t // 6) % 3]
        got, cen = pixel_call(h, th, channels, window)
        screen = h.fetch()[0]
        assert_same(cen, crop_centers(h), "%s step %d: centres" % (case, t))
        assert_same(got, pu.crop_images(font, pal, screen, channels, cen, *window), "%s step %d window %s th %d C %d" % (case, t, window, th, channels))
        seen.add((th, channels, window))
        if t % 4 == 0:
            ch2 = (3, 1)[(t // 4) % 2]
            got, _ = pixel_call(h, th, ch2)
            assert_same(got, pu.full_images(font, pal, screen, ch2), "%s step %d whole screen th %d C %d" % (case, t, th, ch2))
            seen.add((th, ch2, None))
    hip.sync()
    if steps >= 40:
        assert len(seen) >= 18 + 6, sorted(seen, key=str)


@pytest.mark.parametrize("th", pu.TILE_HEIGHTS)
def test_largest_window_on_two_envs(goldens, th):
    """(47, 159) on 2 mini envs, gray and RGB: the window that holds any screen from any cell, almost all of it padding drawn as ' ' through the tileset."""
    hip = HipBatch(goldens["configs"]["mini"], [5, 6], max_steps=25)
    h = hip.h
    use_torch_stream(h)
    font, pal = pu.random_tileset(np.random.RandomState(40 + th), th)
    set_tileset(h, font, pal)
    hip.step(ACTION_KEYS[[1, 4]])
    for channels in (1, 3):
        got, cen = pixel_call(h, th, channels, (47, 159))
        assert_same(got, pu.crop_images(font, pal, h.fetch()[0], channels, cen, 47, 159), "th %d C %d" % (th, channels))


# ---------------------------------------------------------------------------------------------
# 2. corners and edges: the player moved there through the state records
# ---------------------------------------------------------------------------------------------
def test_corners_and_edges(goldens):
    """The player on the four corners and the four edge midpoints (each env keeps its own level: only the position word of its record changes), windows
    that hang over one, two and all sides; the centres are rg_obs_crop's; crop = slice of the padded full image, device against device."""
    cfg = dict(goldens["configs"]["mini"], enemies={"enemies": []})
    n = 9
    hip = HipBatch(cfg, range(40, 40 + n), max_steps=100)
    h = hip.h
    use_torch_stream(h)
    H, W = h.height, h.width
    grids = np.stack([h.debug_state(i)[1] for i in range(n)])
    players = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2), (W // 2, H // 2)]
    gu.inject(hip, grids, players, np.zeros(n, np.uint32))
    font, pal = pu.random_tileset(np.random.RandomState(8), 13)
    set_tileset(h, font, pal)
    want_cen = np.array([(py, px) for px, py in players], np.int32)
    full, _ = pixel_call(h, 13, 3)
    screen = h.fetch()[0]
    assert_same(full, pu.full_images(font, pal, screen, 3), "whole screen")
    for ry, rx in [(1, 1), (5, 5), (1, 7), (7, 15), (8, 16), (20, 40)]:   # (7, 15): one or two sides; (8, 16) and up: every side from some cells
        got, cen = pixel_call(h, 13, 3, (ry, rx))
        assert_same(cen, want_cen, "centres")
        assert_same(cen, crop_centers(h), "centres against rg_obs_crop")
        assert_same(got, pu.crop_images(font, pal, screen, 3, cen, ry, rx), "window (%d, %d)" % (ry, rx))
        # device against device: the slice of the device's own full image, padded with the ' ' tile
        blank = pu.full_image(font, pal, np.array([[0x20]], np.uint8), 3)                       # [3, th, 8]
        padded = np.tile(blank, (1, H + 2 * ry, W + 2 * rx))[None].repeat(n, 0)
        padded[:, :, ry * 13:(ry + H) * 13, rx * 8:(rx + W) * 8] = full
        for e, (cy, cx) in enumerate(cen):
            assert np.array_equal(got[e], padded[e, :, cy * 13:(cy + 2 * ry + 1) * 13, cx * 8:(cx + 2 * rx + 1) * 8]), (ry, rx, e)


# ---------------------------------------------------------------------------------------------
# 3. config groups and mixed sizes
# ---------------------------------------------------------------------------------------------
def _handle(cfgs, max_steps=30):
    import json
    from rogue_gym_python import _rogue_gym as inner
    return inner._Handle([json.dumps(c) for c in cfgs], max_steps, auto_reset=True)


@pytest.mark.parametrize("kind", ["three sizes", "groups of one size"])
def test_groups_and_mixed_sizes(goldens, kind):
    mini = goldens["configs"]["mini"]
    if kind == "three sizes":
        shapes = [dict(mini), grid_cfg(80, 24, 3, 3), dict(grid_cfg(48, 20, 3, 2), dungeon={"style": "rogue", "room_num_x": 3, "room_num_y": 2})]
    else:
        shapes = [dict(mini), dict(mini, enemies={"enemies": []}), dict(mini, hide_dungeon=False)]
    n = 26
    h = _handle([dict(shapes[i % 3], seed=700 + i) for i in range(n)])
    use_torch_stream(h)
    font, pal = pu.random_tileset(np.random.RandomState(5), 13)
    set_tileset(h, font, pal)
    rng = np.random.RandomState(2)
    for t in range(8):
        keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)]
        h.check(h.L.rg_step(h.h, np.ascontiguousarray(keys).ctypes.data, 0))
        screens = h.snapshot().screen
        for channels, window in ((1, (5, 5)), (3, (1, 7))):
            got, cen = pixel_call(h, 13, channels, window)
            assert_same(cen, crop_centers(h), "centres")
            assert_same(got, pu.crop_images(font, pal, list(screens), channels, cen, *window), "%s step %d C %d window %s" % (kind, t, channels, window))
    torch = torch_mod()
    out = torch.full((n * 3 * 48 * 13 * 160 * 8 // 64,), SENTINEL, dtype=torch.uint8, device="cuda:%d" % h.device)
    assert h.L.rg_obs_pixels(h.h, 1, C.c_void_p(out.data_ptr())) != 0
    msg = h.L.rg_last_error(h.h).decode()
    assert msg.startswith("rg_obs_pixels: ") and "config groups" in msg, msg
    assert bool((out == SENTINEL).all())
    h.check(h.L.rg_sync(h.h))


# ---------------------------------------------------------------------------------------------
# 4. side effects: twin handles, the bound tensor, the step forms, refusals, the tileset
# ---------------------------------------------------------------------------------------------
def test_twin_handles_pixels_only_against_crop_only(goldens):
    """a makes only pixel calls, b only rg_obs_crop calls: screen and history mirrors, status, flag words and whole state records (RNG words included) are equal
    after every step."""
    torch = torch_mod()
    cfg, n = goldens["configs"]["mini"], 135
    a, b = HipBatch(cfg, range(n), max_steps=12), HipBatch(cfg, range(n), max_steps=12)
    for hb in (a, b):
        use_torch_stream(hb.h)
    rng = np.random.RandomState(9)
    out_b = torch.empty((n, 1, 11, 11), dtype=torch.float32, device="cuda:%d" % b.h.device)
    for t in range(40):
        keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)]
        a.step(keys)
        b.step(keys)
        if t % 5 == 4:
            pixel_call(a.h, 8, 3)
        else:
            pixel_call(a.h, 8, (1, 3)[t % 2], (5, 5))
        b.h.check(b.h.L.rg_obs_crop(b.h.h, 0, 5, 5, 0, 0, C.c_void_p(out_b.data_ptr()), None))
        ra, rb = records(a.h), records(b.h)
        assert np.array_equal(ra, rb), "step %d: state records differ in %d envs" % (t, int((ra != rb).any(1).sum()))
        for x, y, name in zip(a.fetch(), b.fetch(), ("screen", "hist", "status", "flags")):
            assert np.array_equal(x, y), "step %d: %s mirrors differ" % (t, name)


def test_bound_gray_tensor_survives_pixel_calls(goldens):
    """A handle with a bound gray tensor that makes a pixel call between every step and the tensor's own call: the tensor equals the unbound call's."""
    torch = torch_mod()
    cfg, n = goldens["configs"]["mini"], 67
    a, c = HipBatch(cfg, range(n), max_steps=12), HipBatch(cfg, range(n), max_steps=12)
    for hb in (a, c):
        use_torch_stream(hb.h)
    dev = "cuda:%d" % a.h.device
    bound = torch.zeros((n, 1, a.h.height, a.h.width), dtype=torch.float32, device=dev)
    plain = torch.zeros_like(bound)
    a.h.check(a.h.L.rg_obs_bind(a.h.h, 0, 0, 0, C.c_void_p(bound.data_ptr())))
    a.h.check(a.h.L.rg_obs_gray(a.h.h, 0, 0, C.c_void_p(bound.data_ptr())))
    rng = np.random.RandomState(10)
    for t in range(30):
        keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)]
        a.step(keys)
        c.step(keys)
        pixel_call(a.h, 8, 1, (5, 5))
        a.h.check(a.h.L.rg_obs_gray(a.h.h, 0, 0, C.c_void_p(bound.data_ptr())))
        c.h.check(c.h.L.rg_obs_gray(c.h.h, 0, 0, C.c_void_p(plain.data_ptr())))
        assert torch.equal(bound, plain), "step %d" % t
    a.h.check(a.h.L.rg_obs_bind(a.h.h, 0, 0, 0, None))


def test_step_forms_and_refusals(goldens):
    """rg_step_obs_pixels[_crop] = step then pass; a refused call does not step and writes nothing (the state records say so)."""
    torch = torch_mod()
    cfg, n = goldens["configs"]["mini"], 65
    a, b = HipBatch(cfg, range(n), max_steps=12), HipBatch(cfg, range(n), max_steps=12)
    for hb in (a, b):
        use_torch_stream(hb.h)
    rng = np.random.RandomState(12)
    for t in range(12):
        keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)]
        window = None if t % 3 == 2 else (5, 5)
        got_a, cen_a = pixel_call(a.h, 8, 3, window, keys=dev_keys(a.h, keys))
        b.step(keys)
        got_b, cen_b = pixel_call(b.h, 8, 3, window)
        assert np.array_equal(got_a, got_b) and (window is None or np.array_equal(cen_a, cen_b)), t
        assert np.array_equal(records(a.h), records(b.h)), t
    h, L = a.h, a.h.L
    before = records(h)
    dev = "cuda:%d" % h.device
    out = torch.full((n * 3 * 128 * 256 + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    k = dev_keys(h, ACTION_KEYS[rng.randint(1, 9, n)])
    kp, op = C.c_void_p(k.data_ptr()), C.c_void_p(out.data_ptr())
    refusals = [
        (lambda: L.rg_step_obs_pixels(h.h, kp, 1, 2, op), "rg_step_obs_pixels: ", "channels"),
        (lambda: L.rg_step_obs_pixels_crop(h.h, kp, 1, 4, 5, 5, op, None), "rg_step_obs_pixels_crop: ", "channels"),
        (lambda: L.rg_step_obs_pixels_crop(h.h, kp, 1, 1, 48, 5, op, None), "rg_step_obs_pixels_crop: ", "radius_y"),
        (lambda: L.rg_step_obs_pixels_crop(h.h, kp, 1, 1, 5, 160, op, None), "rg_step_obs_pixels_crop: ", "radius_x"),
        (lambda: L.rg_step_obs_pixels_crop(h.h, kp, 1, 1, -1, 5, op, None), "rg_step_obs_pixels_crop: ", "radius_y"),
        (lambda: L.rg_step_obs_pixels(h.h, kp, 1, 1, None), "rg_step_obs_pixels: ", "out_dev"),
        (lambda: L.rg_step_obs_pixels(h.h, kp, 1, 1, C.c_void_p(out.data_ptr() + 8)), "rg_step_obs_pixels: ", "out_dev"),
        (lambda: L.rg_obs_pixels(h.h, 0, op), "rg_obs_pixels: ", "channels"),
        (lambda: L.rg_obs_pixels_crop(h.h, 3, 5, 5, C.c_void_p(out.data_ptr() + 4), None), "rg_obs_pixels_crop: ", "out_dev"),
        (lambda: L.rg_tileset_set(h.h, 7, op, op), "rg_tileset_set: ", "th"),
        (lambda: L.rg_tileset_set(h.h, 17, op, op), "rg_tileset_set: ", "th"),
    ]
    for call, prefix, frag in refusals:
        assert call() != 0
        msg = L.rg_last_error(h.h).decode()
        assert msg.startswith(prefix) and frag in msg, msg
    assert bool((out == SENTINEL).all())
    assert np.array_equal(records(h), before), "a refused call stepped"
    a.sync()


def test_changing_the_tileset_changes_the_next_image_and_nothing_else(goldens):
    cfg, n = goldens["configs"]["mini"], 33
    hip = HipBatch(cfg, range(n), max_steps=30)
    h = hip.h
    use_torch_stream(h)
    hip.step(ACTION_KEYS[np.arange(n) % len(ACTION_KEYS)])
    font, pal = pu.default_tileset(h.L)
    first, _ = pixel_call(h, 8, 3, (5, 5))          # no rg_tileset_set so far: the built-in
    screen, before = h.fetch()[0], records(h)
    cen = crop_centers(h)
    assert_same(first, pu.crop_images(font, pal, screen, 3, cen, 5, 5), "built-in")
    font2, pal2 = pu.random_tileset(np.random.RandomState(1), 16)
    set_tileset(h, font2, pal2)
    second, _ = pixel_call(h, 16, 3, (5, 5))
    assert_same(second, pu.crop_images(font2, pal2, screen, 3, cen, 5, 5), "after rg_tileset_set")
    h.check(h.L.rg_tileset_set(h.h, 0, None, None))   # NULL tables: the built-in again
    third, _ = pixel_call(h, 8, 3, (5, 5))
    assert np.array_equal(third, first)
    assert np.array_equal(records(h), before) and np.array_equal(h.fetch()[0], screen)


# ---------------------------------------------------------------------------------------------
# 5. the Python surface
# ---------------------------------------------------------------------------------------------
def _seeded(cfg, seeds):
    return [dict(cfg, seed=int(s)) for s in seeds]


def _check_env(env, font, pal, where):
    torch = env.torch
    torch.cuda.synchronize()
    screen = env.screen.cpu().numpy()
    ch = env.pixels.shape[1]
    if env.pixel_center is None:
        want = pu.full_images(font, pal, screen, ch)
    else:
        want = pu.crop_images(font, pal, screen, ch, env.pixel_center.cpu().numpy(), (env.pixels.shape[2] // env.tileset.th - 1) // 2, (env.pixels.shape[3] // 8 - 1) // 2)
    assert_same(env.pixels.cpu().numpy(), want, where)


@pytest.mark.parametrize("form", ["gray crop", "rgb whole"])
def test_env_pixels_current_on_every_refresh_path(goldens, form):
    from rogue_gym.envs import HipVecFirstFloor, HipVecRogueEnv, Tileset
    torch = torch_mod()
    cfg, n = goldens["configs"]["mini"], 40
    font, pal = pu.random_tileset(np.random.RandomState(21), 13)
    kw = dict(pixels="gray", pixel_crop=5) if form == "gray crop" else dict(pixels="rgb")
    env = HipVecRogueEnv(_seeded(cfg, range(n)), max_steps=20, tileset=Tileset(font, pal), **kw)
    assert env.pixels.dtype == torch.uint8 and tuple(env.pixels.shape) == ((n, 1, 11 * 13, 88) if form == "gray crop" else (n, 3, 16 * 13, 256))
    assert (env.pixel_center is None) == (form != "gray crop")
    _check_env(env, font, pal, "constructor")
    rng = np.random.RandomState(4)
    for t in range(6):
        env.step(torch.as_tensor(rng.randint(0, 11, n), device=env.device))
        _check_env(env, font, pal, "step %d" % t)
    env.step_keys(torch.as_tensor(ACTION_KEYS[rng.randint(0, 11, n)].copy(), device=env.device))
    _check_env(env, font, pal, "step_keys")
    saved = env.save_state()
    env.reset_envs(env_ids=[0, 7, 39])
    _check_env(env, font, pal, "reset_envs")
    env.load_state(saved)
    _check_env(env, font, pal, "load_state")
    env.clone_state([3] * 5, range(10, 15))
    _check_env(env, font, pal, "clone_state")
    env.reset()
    _check_env(env, font, pal, "reset")
    # render_pixels: fresh and into `out`
    img = env.render_pixels(rgb=True, crop=(1, 7))
    out = torch.zeros_like(img)
    assert env.render_pixels(rgb=True, crop=(1, 7), out=out) is out and torch.equal(out, img)
    with pytest.raises(ValueError):
        env.render_pixels(rgb=False, crop=(1, 7), out=out)
    env.close()
    ff = HipVecFirstFloor(_seeded(cfg, range(n)), max_steps=20, tileset=Tileset(font, pal), **kw)
    for t in range(4):
        ff.step_keys(torch.as_tensor(ACTION_KEYS[rng.randint(0, 11, n)].copy(), device=ff.device))
        _check_env(ff, font, pal, "first floor step %d" % t)
    ff.close()


def test_frame_and_value_forms(goldens):
    from rogue_gym.envs import HipVecRogueEnv, ParallelRogueEnv, RogueEnv
    torch = torch_mod()
    cfg = goldens["configs"]["mini"]
    env = HipVecRogueEnv(_seeded(cfg, range(8)), max_steps=20)
    assert env.pixels is None and env.pixel_center is None
    font, pal = pu.default_tileset(env._h.L)
    ids = [5, 0, 3, 1, 7, 2]
    fr = env.frame(ids, cols=3)
    torch.cuda.synchronize()
    screen = env.screen.cpu().numpy()
    full = pu.full_images(font, pal, screen, 3)
    assert fr.dtype == torch.uint8 and tuple(fr.shape) == (2 * 128, 3 * 256, 3)
    fr = fr.cpu().numpy()
    for k, e in enumerate(ids):
        r, c = divmod(k, 3)
        assert np.array_equal(fr[r * 128:(r + 1) * 128, c * 256:(c + 1) * 256], full[e].transpose(1, 2, 0)), (k, e)
    assert tuple(env.frame([1, 2, 3]).shape) == (2 * 128, 2 * 256, 3)
    env.close()
    one = RogueEnv(config_dict=cfg, seed=3)
    one.step("l")
    frame = one.render("rgb_array")
    assert frame.dtype == np.uint8 and frame.shape == (128, 256, 3)
    assert np.array_equal(frame, pu.full_image(font, pal, one.result._map, 3).transpose(1, 2, 0))
    par = ParallelRogueEnv(_seeded(cfg, range(5)), max_steps=20)
    par.step("hjkl.")
    frames = par.render_frames()
    assert frames.dtype == np.uint8 and frames.shape == (5, 128, 256, 3)
    assert np.array_equal(frames, pu.full_images(font, pal, np.asarray(par.states.screen), 3).transpose(0, 2, 3, 1))
    par.close()
