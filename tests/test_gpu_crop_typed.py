"""Typed player-centred crops (rg_obs_crop_typed / rg_step_obs_crop_typed) and crop views (HipVecRogueEnv.add_crop).  The expected window is always
built from the library's own f32 full image (rg_obs_gray / rg_obs_symbol, which tests/test_gpu_obs_oracle.py pins to the oracle) and the `centers`
output: padded and gathered (test_gpu_crop.expect), then rounded by torch's own conversion; a few envs of every call also through the numpy
reference of tests/test_crop_typed_abi.py.  Output buffers are pre-filled with 0xFF bytes and end in guard bytes; comparisons are on bit patterns."""
import ctypes as C

import numpy as np
import pytest

from parity_util import ACTION_KEYS, HipBatch
from test_crop_typed_abi import typed_crop_reference
from test_gpu_crop import crop_call, expect, seeded
from test_gpu_obs_typed import drain_tile_errors, tdtype, use_torch_stream
from typed_util import RG_OBS_BF16, RG_OBS_F16, RG_OBS_F32, RG_OBS_U8

pytestmark = pytest.mark.gpu

FULL = 0x1FF
RG_FLAG_ERR_TILE = 0x00040000
GUARD = 64
PAIRS = [(0, RG_OBS_F16), (0, RG_OBS_BF16), (1, RG_OBS_F16), (1, RG_OBS_BF16), (2, RG_OBS_U8)]
ZED = {"attack": [], "attr": 0, "defense": 1, "exp": 1, "gold": 0, "level": 1, "name": "zed", "tile": 90, "rarelity": 0}  # shown as 'Z': no symbol


def torch_mod():
    import torch

    return torch


def channels(h, kind, flag, with_hist):
    return 1 + int(bool(with_hist)) if kind == 2 else h.L.rg_obs_channels(h.h, kind, flag, int(bool(with_hist)))


def buffers(h, kind, dt, ry, rx, flag, with_hist):
    """(raw u8 buffer of 0xFF bytes: the output and GUARD bytes behind it, bytes of the output, its shape, centres of -1)."""
    torch = torch_mod()
    dev = "cuda:%d" % h.device
    shape = (h.n, channels(h, kind, flag, with_hist), 2 * ry + 1, 2 * rx + 1)
    nbytes = int(np.prod(shape)) * (4 if dt == RG_OBS_F32 else 1 if dt == RG_OBS_U8 else 2)
    raw = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    return raw, nbytes, shape, torch.full((h.n, 2), -1, dtype=torch.int32, device=dev)


def as_bits(raw, nbytes, shape, dt):
    """The output part of a raw buffer as bit patterns: int16 (16-bit types), int32 (f32) or uint8, in the output's shape."""
    torch = torch_mod()
    assert bool((raw[nbytes:] == 0xFF).all()), "guard bytes behind the output were written"
    return raw[:nbytes].view(torch.uint8 if dt == RG_OBS_U8 else torch.int32 if dt == RG_OBS_F32 else torch.int16).view(shape)


def typed_crop_call(h, kind, dt, ry, rx, flag, with_hist, keys=None):
    """rg_obs_crop_typed (keys: rg_step_obs_crop_typed with those device keys) into fresh 0xFF buffers: (bit patterns [n, C, 2ry+1, 2rx+1], centres)."""
    raw, nbytes, shape, cen = buffers(h, kind, dt, ry, rx, flag, with_hist)
    if keys is None:
        h.check(h.L.rg_obs_crop_typed(h.h, kind, dt, ry, rx, flag, int(with_hist), C.c_void_p(raw.data_ptr()), C.c_void_p(cen.data_ptr())))
    else:
        h.check(h.L.rg_step_obs_crop_typed(h.h, C.c_void_p(keys.data_ptr()), 1, kind, dt, ry, rx, flag, int(with_hist), C.c_void_p(raw.data_ptr()),
                                           C.c_void_p(cen.data_ptr())))
    return as_bits(raw, nbytes, shape, dt), cen


class Fulls:
    """The library's f32 full images of one handle in its present state, each encoded once and shared by every window compared against it."""

    def __init__(self, h, env_symbols=None):
        self.h, self.cache = h, {}
        torch = torch_mod()
        sy = h.env_symbols if env_symbols is None else env_symbols
        self.symbols = torch.as_tensor(np.asarray(sy, np.float32), device="cuda:%d" % h.device).reshape(-1, 1, 1, 1)

    def get(self, kind, flag, with_hist):
        torch = torch_mod()
        key = (kind, flag, bool(with_hist))
        if key not in self.cache:
            h = self.h
            out = torch.full((h.n, h.L.rg_obs_channels(h.h, kind, flag, int(bool(with_hist))), h.height, h.width), float("nan"), dtype=torch.float32, device="cuda:%d" % h.device)
            h.check((h.L.rg_obs_symbol if kind else h.L.rg_obs_gray)(h.h, flag, int(bool(with_hist)), C.c_void_p(out.data_ptr())))
            self.cache[key] = out
        return self.cache[key]

    def ids(self, with_hist):
        """f32 [n, 1 + hist, H, W]: every cell's symbol id (gray value x the env's symbol count: the gray image is id / symbols by one division) and the
        0 / 1 history plane."""
        torch = torch_mod()
        g = self.get(0, 0, with_hist)
        return torch.cat([torch.round(g[:, :1] * self.symbols), g[:, 1:]], 1)


def expected_bits(fulls, kind, dt, ry, rx, flag, with_hist, cen, planes=None):
    """(bit patterns of the expected windows, the f32 image they were cut from and its (kind, planes) for the numpy reference)."""
    torch = torch_mod()
    if kind == 2:
        img = fulls.ids(with_hist)
        return expect(img, cen, ry, rx, 0, 1, with_hist).to(torch.uint8), img, (2, 1)
    img = fulls.get(kind, flag, with_hist)
    planes = (fulls.h.symbols if kind else 1) if planes is None else planes
    win = expect(img, cen, ry, rx, kind, planes, with_hist)
    return (win.view(torch.int32) if dt == RG_OBS_F32 else win.to(tdtype(dt)).view(torch.int16)), img, (kind, planes)


def check_window(fulls, kind, dt, ry, rx, flag, with_hist, got, cen, where, sample=(0, -1)):
    torch = torch_mod()
    exp, img, (rk, planes) = expected_bits(fulls, kind, dt, ry, rx, flag, with_hist, cen)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (where, got.shape, exp.shape, got.dtype, exp.dtype)
    if not torch.equal(got, exp):
        bad = (got != exp).reshape(got.shape[0], -1).any(1).nonzero().flatten()
        e = int(bad[0])
        p, y, x = (int(v) for v in (got[e] != exp[e]).nonzero()[0])
        raise AssertionError("%s: %d envs differ from the rounded window of the full image, first env %d (plane %d, row %d, column %d): %#x vs %#x, centre %s" % (
            where, bad.numel(), e, p, y, x, int(got[e, p, y, x]) & 0xFFFFFFFF, int(exp[e, p, y, x]) & 0xFFFFFFFF, cen[e].tolist()))
    if dt != RG_OBS_F32:  # the numpy reference, on a few envs
        c = cen.cpu().numpy()
        for e in sorted({s % got.shape[0] for s in sample}):
            ref = typed_crop_reference(img[e].cpu().numpy(), int(c[e, 0]), int(c[e, 1]), ry, rx, rk, planes, with_hist, dt)
            g = got[e].cpu().numpy()
            assert np.array_equal(g if rk == 2 else g.view(np.uint16), ref), "%s env %d: differs from the numpy reference" % (where, e)


def edges_seen(seen, cen, ry, rx, hh, ww):
    """Which screen edges the windows of these centres cross, and whether one lies wholly inside (radii that say something: not (0, 0), which
    never crosses, for the crossings' counterpart, and not a window that always crosses)."""
    c = np.asarray(cen)
    top, bottom, left, right = c[:, 0] - ry < 0, c[:, 0] + ry >= hh, c[:, 1] - rx < 0, c[:, 1] + rx >= ww
    if 2 * ry + 1 <= hh and 2 * rx + 1 <= ww:
        for name, m in (("top", top), ("bottom", bottom), ("left", left), ("right", right)):
            seen[name] = seen.get(name, False) or bool(m.any())
        if ry or rx:
            seen["inside"] = seen.get("inside", False) or bool((~(top | bottom | left | right)).any())


# ---------------------------------------------------------------------------------------------
# 1. shapes where the store path can go wrong
# ---------------------------------------------------------------------------------------------
STORE_RADII = [(0, 0), (1, 1), (2, 3), (5, 5), (8, 8), (15, 31)]
STORE_STEPS, STORE_MAX_STEPS = 40, 10
# First seed per batch size, chosen on the CPU oracle (same keys) so that the windows (of the radii whose window fits the screen) cross every screen
# edge and one lies wholly inside.  A single env replays its own seed's level every episode and does not get from border to border of it in 40 random
# keys (no seed of the first 1 500 does, with run keys and longer episodes either): seed 152 crosses the top, bottom and left edges and lies inside.
STORE_SEED0 = {1: 152, 3: 10, 21: 0, 67: 0}
STORE_EDGES = {1: ("top", "bottom", "left", "inside"), 3: ("top", "bottom", "left", "right", "inside"), 21: ("top", "bottom", "left", "right", "inside"),
               67: ("top", "bottom", "left", "right", "inside")}


def store_keys(n):
    rng = np.random.RandomState(100 + n)
    return [ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)] for _ in range(STORE_STEPS)]


@pytest.mark.parametrize("n", [1, 3, 21, 67])
def test_store_path_shapes(goldens, n):
    """Mini, batch sizes and radii at which C x area x sizeof(T) is odd, env starts are unaligned and the batch's last 16-byte piece is partial; every
    kind / type pair with FULL + history (ids: history), after reset and after each of 40 random-key steps with 10-step episodes."""
    torch = torch_mod()
    cfg = goldens["configs"]["mini"]
    hip = HipBatch(cfg, range(STORE_SEED0[n], STORE_SEED0[n] + n), max_steps=STORE_MAX_STEPS)
    h = hip.h
    use_torch_stream(h)
    seen = {}
    sizes = set()
    for t, keys in enumerate([None] + store_keys(n)):
        if keys is not None:
            torch.cuda.synchronize()
            hip.step(keys)
        fulls = Fulls(h)
        for ry, rx in STORE_RADII:
            for kind, dt in PAIRS:
                flag = 0 if kind == 2 else FULL
                got, cen = typed_crop_call(h, kind, dt, ry, rx, flag, True)
                check_window(fulls, kind, dt, ry, rx, flag, True, got, cen, "n=%d t=%d r=(%d,%d) kind %d dt %d" % (n, t, ry, rx, kind, dt))
                sizes.add(int(np.prod(got.shape[1:])) * got.element_size())
            got, cen = typed_crop_call(h, 2, RG_OBS_U8, ry, rx, 0, False)  # the ids alone: an env's image is (2ry+1)(2rx+1) bytes, odd
            check_window(fulls, 2, RG_OBS_U8, ry, rx, 0, False, got, cen, "n=%d t=%d r=(%d,%d) ids alone" % (n, t, ry, rx))
            sizes.add(int(np.prod(got.shape[1:])))
            edges_seen(seen, cen.cpu().numpy(), ry, rx, h.height, h.width)
        drain_tile_errors(h)
    assert any(s % 2 for s in sizes) and any(s % 16 for s in sizes), sizes  # (odd env images, env starts off the 16-byte pieces)
    assert all(seen.get(k) for k in STORE_EDGES[n]), seen
    h.close()


# ---------------------------------------------------------------------------------------------
# 2. the LDS ceiling, and a grid with an odd cell count
# ---------------------------------------------------------------------------------------------
def grid_cfg(w, h, rx, ry):
    return {"width": w, "height": h, "dungeon": {"style": "rogue", "room_num_x": rx, "room_num_y": ry, "min_room_size": {"x": 4, "y": 4}}}


@pytest.mark.parametrize("radii", [(47, 159), (23, 80)])
def test_largest_windows_on_the_largest_screen(radii):
    """160x48, 5 envs: the window that holds the whole screen from any cell (with the history plane: the whole screen staged twice per env, 61 440 bytes
    of LDS for the run of 4) and one of half that size; ids with history and the bf16 one-hot image with history."""
    ry, rx = radii
    hip = HipBatch(grid_cfg(160, 48, 4, 4), range(5), max_steps=30)
    h = hip.h
    use_torch_stream(h)
    rng = np.random.RandomState(7)
    for _ in range(6):
        hip.step(ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), 5)])
    fulls = Fulls(h)
    for kind, dt in ((2, RG_OBS_U8), (1, RG_OBS_BF16)):
        got, cen = typed_crop_call(h, kind, dt, ry, rx, 0, True)
        check_window(fulls, kind, dt, ry, rx, 0, True, got, cen, "160x48 r=(%d,%d) kind %d" % (ry, rx, kind), sample=(0,))
    drain_tile_errors(h)
    h.close()


def test_odd_cell_count_grid_is_served():
    """33x17 (561 cells: no multiple of 8, which rg_obs_typed refuses): the crop stages cells, so every pair is served."""
    hip = HipBatch(grid_cfg(33, 17, 2, 2), range(8), max_steps=30)
    h = hip.h
    use_torch_stream(h)
    rng = np.random.RandomState(8)
    for t in range(4):
        hip.step(ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), 8)])
        fulls = Fulls(h)
        for kind, dt in PAIRS:
            flag = 0 if kind == 2 else FULL
            got, cen = typed_crop_call(h, kind, dt, 4, 4, flag, True)
            check_window(fulls, kind, dt, 4, 4, flag, True, got, cen, "33x17 t=%d kind %d dt %d" % (t, kind, dt))
    drain_tile_errors(h)
    h.close()


# ---------------------------------------------------------------------------------------------
# 3. pending Redraws: drawn first, as by rg_obs_crop
# ---------------------------------------------------------------------------------------------
def same_mirrors(ha, hb, where):
    torch_mod().cuda.synchronize()
    for what, x, y in zip(("screen", "hist", "status", "flags"), ha.fetch(), hb.fetch()):
        if not np.array_equal(x, y):
            bad = np.nonzero((x != y).reshape(ha.n, -1).any(1))[0]
            raise AssertionError("%s: %s of %d envs differ between the typed-crop handle and the f32-crop handle, first %s" % (where, what, len(bad), bad[:8].tolist()))


@pytest.mark.parametrize("kind,dt", PAIRS)
def test_pending_redraws_and_the_f32_crop_twin(goldens, kind, dt):
    """Twin handles of 64 envs: one makes only rg_obs_crop_typed calls, the other only rg_obs_crop calls, right after rg_reset, rg_debug_descend,
    rg_state_load and every one of 30 steps -- the typed window equals the reference, and screen, history and flag words of the twins are equal."""
    torch = torch_mod()
    n, ry, rx = 64, 3, 4
    cfg = dict(goldens["configs"]["mini"], enemies={"enemies": list(range(12))})
    a, b, c = (HipBatch(cfg, range(n), max_steps=12) for _ in range(3))  # (c: the same game, for the reference's full images -- the twins make no other call)
    ha, hb, hc, L = a.h, b.h, c.h, a.h.L
    for h in (ha, hb, hc):
        use_torch_stream(h)
    flag = 0 if kind == 2 else FULL
    fk = 1 if kind else 0  # (the f32 twin of the ids: the one-hot window, which raises the same tile errors)
    rng = np.random.RandomState(11)

    def both(where):
        got, cen = typed_crop_call(ha, kind, dt, ry, rx, flag, True)   # Redraws pending: nothing else has looked at `ha` since the event
        _, cen_b = crop_call(hb, fk, ry, rx, flag, True)
        assert torch.equal(cen, cen_b), where
        check_window(Fulls(hc), kind, dt, ry, rx, flag, True, got, cen, where)
        same_mirrors(ha, hb, where)
        for h in (ha, hb, hc):
            drain_tile_errors(h)

    both("create")
    for t in range(30):
        keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)]
        torch.cuda.synchronize()
        for x in (a, b, c):
            x.step(keys)
        both("t=%d" % t)
        if t == 9:
            for h in (ha, hb, hc):
                h.check(L.rg_reset(h.h))
            both("reset")
        if t == 14:
            for h in (ha, hb, hc):
                h.check(L.rg_debug_descend(h.h))
            both("descend")
        if t == 20:
            ids = np.arange(8, 40, dtype=np.int32)
            src = np.asarray([3] * 16 + [50] * 16, np.int32)
            for h in (ha, hb, hc):
                rec = torch.empty((len(src), h.state_bytes()), dtype=torch.uint8, device="cuda:%d" % h.device)
                h.check(L.rg_state_save(h.h, src.ctypes.data, len(src), 0, C.c_void_p(rec.data_ptr())))
                h.check(L.rg_state_load(h.h, C.c_void_p(rec.data_ptr()), int(rec.shape[1]), ids.ctypes.data, len(ids), 0))
            both("state_load")
    for h in (ha, hb, hc):
        h.close()


# ---------------------------------------------------------------------------------------------
# 4. config groups and mixed sizes
# ---------------------------------------------------------------------------------------------
def host_images(h, setting):
    """Every env's own f32 full image through the host encode (ImageSetting.expand of rg_fetch_states' ragged copies), as test_gpu_crop does for
    mixed-size batches: the rg_obs_* device calls refuse those."""
    states = h.snapshot()
    return [np.asarray(setting.expand(states[i]), np.float32) for i in range(h.n)]


def check_host(h, kind, dt, ry, rx, setting, got, cen, where):
    """A typed window of a batch with mixed sizes against the numpy reference, env by env."""
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag

    hist = bool(setting.includes_hist)
    imgs = host_images(h, ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, hist) if kind == 2 else setting)
    g, c = got.cpu().numpy(), cen.cpu().numpy()
    for e in range(h.n):
        img = imgs[e]
        if kind == 2:
            img = np.concatenate([np.round(img[:1] * np.float32(h.env_symbols[e])), img[1:]])
        ref = typed_crop_reference(img, int(c[e, 0]), int(c[e, 1]), ry, rx, kind, h.symbols if kind == 1 else 1, hist, dt)
        assert np.array_equal(g[e] if kind == 2 else g[e].view(np.uint16), ref), "%s env %d (%d x %d): differs from the numpy reference" % (
            where, e, h.env_heights[e], h.env_widths[e])


def test_groups_and_mixed_sizes(goldens):
    """One batch of mini, 80x24 and 48x20 configs (as test_gpu_crop.test_crop_groups_and_mixed_sizes builds it), 11 envs, radius (3, 5), every pair; then
    a batch with a group of more symbols than env 0's: the one-hot kind is refused, the ids are served with each env judged by its own symbols."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym_python import _rogue_gym as inner
    import json

    mini = goldens["configs"]["mini"]
    enemies = {"enemies": list(range(10))}
    shapes = [dict(mini, enemies=enemies), {"width": 80, "height": 24, "enemies": enemies},
              {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": enemies}]
    n, ry, rx = 11, 3, 5
    h = inner._Handle([json.dumps(dict(shapes[i % 3], seed=6000 + i)) for i in range(n)], 40, auto_reset=True)
    assert h.mixed_sizes
    use_torch_stream(h)
    rng = np.random.RandomState(12)
    settings = {0: ImageSetting(DungeonType.GRAY, StatusFlag.FULL, True), 1: ImageSetting(DungeonType.SYMBOL, StatusFlag.FULL, True),
                2: ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, True)}
    for t in range(12):
        keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)]
        torch.cuda.synchronize()
        h.check(h.L.rg_step(h.h, keys.ctypes.data, 0))
        if t % 4 == 3:
            for kind, dt in PAIRS:
                flag = 0 if kind == 2 else FULL
                got, cen = typed_crop_call(h, kind, dt, ry, rx, flag, True)
                check_host(h, kind, dt, ry, rx, settings[kind], got, cen, "mixed t=%d kind %d dt %d" % (t, kind, dt))
            h.check(h.L.rg_sync(h.h))
    h.close()
    # env 0 without monsters (17 symbols), env 1 with the stock ones (43): a larger-symbols group
    hip = inner._Handle([json.dumps(dict(mini, seed=1, enemies={"enemies": []})), json.dumps(dict(mini, seed=2)), json.dumps(dict(mini, seed=3, enemies={"enemies": []}))],
                        40, auto_reset=True)
    use_torch_stream(hip)
    assert hip.env_symbols[1] > hip.symbols
    raw, nbytes, shape, cen = buffers(hip, 1, RG_OBS_BF16, 2, 2, 0, False)
    for step in (False, True):
        keys = torch.full((3,), ord("."), dtype=torch.uint8, device=raw.device)
        before = hip.fetch()[2].copy()
        if step:
            rc = hip.L.rg_step_obs_crop_typed(hip.h, C.c_void_p(keys.data_ptr()), 1, 1, RG_OBS_BF16, 2, 2, 0, 0, C.c_void_p(raw.data_ptr()), C.c_void_p(cen.data_ptr()))
        else:
            rc = hip.L.rg_obs_crop_typed(hip.h, 1, RG_OBS_BF16, 2, 2, 0, 0, C.c_void_p(raw.data_ptr()), C.c_void_p(cen.data_ptr()))
        assert rc != 0 and b"more symbols" in hip.L.rg_last_error(hip.h) and b"rg_obs_crop_typed" in hip.L.rg_last_error(hip.h).replace(b"step_obs", b"obs")
        torch.cuda.synchronize()
        assert bool((raw == 0xFF).all()) and np.array_equal(hip.fetch()[2], before)
    got, cen = typed_crop_call(hip, 2, RG_OBS_U8, 2, 2, 0, True)
    check_window(Fulls(hip), 2, RG_OBS_U8, 2, 2, 0, True, got, cen, "ids with a larger-symbols group", sample=(0, 1, 2))
    got, cen = typed_crop_call(hip, 0, RG_OBS_F16, 2, 2, FULL, True)
    check_window(Fulls(hip), 0, RG_OBS_F16, 2, 2, FULL, True, got, cen, "gray with a larger-symbols group", sample=(0, 1, 2))
    hip.check(hip.L.rg_sync(hip.h))
    hip.close()


# ---------------------------------------------------------------------------------------------
# 5. invalid tiles: only inside the window
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dt", [(2, RG_OBS_U8), (1, RG_OBS_BF16), (1, RG_OBS_F16)])
def test_invalid_tile_rule(goldens, kind, dt):
    """A config whose common monster is a custom 'Z' (symbol 42 of 43: no channel), windows of growing radii on one state.  After each call the envs
    flagged RG_FLAG_ERR_TILE are exactly those with a 'Z' inside a window so far, and rg_sync is non-zero exactly when this window holds one in some
    env -- a small window that holds none leaves no flag and a clean rg_sync; the byte written (ids) is still the id, 42."""
    torch = torch_mod()
    cfg = dict(goldens["configs"]["mini"], enemies={"enemies": [ZED], "appear_rate_gold": 100, "appear_rate_nogold": 100}, hide_dungeon=False)
    n = 64
    hip = HipBatch(cfg, range(n))
    h, L = hip.h, hip.h.L
    use_torch_stream(h)
    screen, _, _, flags0 = hip.fetch()
    assert not (flags0 & RG_FLAG_ERR_TILE).any()
    has_z = (screen == ord("Z")).reshape(n, -1).any(1)
    assert has_z.sum() > 0 and not has_z.all(), "the premise: some screens show a 'Z', some do not"
    fulls = Fulls(h)  # (the gray image and the ids cut from it: neither call raises)
    clean = raised = 0
    for ry, rx in [(r, r) for r in range(0, 16)] + [(16, 32)]:
        got, cen = typed_crop_call(h, kind, dt, ry, rx, 0, False)
        c = cen.cpu().numpy()
        inside = np.zeros(n, bool)
        for e in np.nonzero(has_z)[0]:
            zy, zx = np.nonzero(screen[e] == ord("Z"))
            m = (np.abs(zy - c[e, 0]) <= ry) & (np.abs(zx - c[e, 1]) <= rx)
            inside[e] = m.any()
            if kind == 2:
                assert int((got[e, 0] == 42).sum()) == int(m.sum()), (ry, rx, e)
        torch.cuda.synchronize()
        flagged = (hip.fetch()[3] & RG_FLAG_ERR_TILE) != 0
        assert np.array_equal(flagged, inside), "r=(%d,%d): flagged %s, a 'Z' inside the window %s" % (ry, rx, np.nonzero(flagged)[0].tolist(), np.nonzero(inside)[0].tolist())
        rc = L.rg_sync(h.h)
        assert (rc != 0) == bool(inside.any()), (ry, rx, rc)
        if rc:
            assert b"Invalid tile" in L.rg_last_error(h.h)
            raised += 1
        else:
            clean += 1
        if kind == 2:
            check_window(fulls, kind, dt, ry, rx, 0, False, got, cen, "zed r=(%d,%d)" % (ry, rx))
    assert clean >= 1 and raised >= 1 and np.array_equal(flagged, has_z), (clean, raised)
    h.close()


# ---------------------------------------------------------------------------------------------
# 6. refusals, the f32 pass-through, the fused step call
# ---------------------------------------------------------------------------------------------
def test_refusals(goldens):
    torch = torch_mod()
    hip = HipBatch(goldens["configs"]["mini"], range(16))
    h, L = hip.h, hip.h.L
    use_torch_stream(h)
    raw = torch.full((16 * 64 * 25 * 4 + GUARD,), 0xFF, dtype=torch.uint8, device="cuda:%d" % h.device)
    keys = torch.full((16,), ord("j"), dtype=torch.uint8, device=raw.device)
    out, odd = C.c_void_p(raw.data_ptr()), C.c_void_p(raw.data_ptr() + 8)
    _, cen0 = typed_crop_call(h, 2, RG_OBS_U8, 1, 1, 0, False)
    status0 = hip.fetch()[2].copy()
    # (kind, dtype, ry, rx, status_flag, out, what the message names)
    cases = [(3, RG_OBS_BF16, 2, 2, 0, out, b"kind"), (-1, RG_OBS_F16, 2, 2, 0, out, b"kind"), (0, 4, 2, 2, 0, out, b"dtype"), (1, -1, 2, 2, 0, out, b"dtype"),
             (2, RG_OBS_BF16, 2, 2, 0, out, b"dtype"), (2, RG_OBS_F16, 2, 2, 0, out, b"dtype"), (2, RG_OBS_F32, 2, 2, 0, out, b"dtype"),
             (0, RG_OBS_U8, 2, 2, 0, out, b"RG_OBS_U8"), (1, RG_OBS_U8, 2, 2, 0, out, b"RG_OBS_U8"), (2, RG_OBS_U8, 2, 2, 1, out, b"status_flag"),
             (2, RG_OBS_U8, 2, 2, FULL, out, b"status_flag"), (0, RG_OBS_F16, -1, 2, 0, out, b"radius_y"), (0, RG_OBS_BF16, 2, -1, 0, out, b"radius_x"),
             (1, RG_OBS_BF16, 48, 2, 0, out, b"radius_y"), (2, RG_OBS_U8, 2, 160, 0, out, b"radius_x"), (0, RG_OBS_F32, 48, 0, 0, out, b"radius_y"),
             (0, RG_OBS_F16, 2, 2, 0, None, b"out_dev"), (2, RG_OBS_U8, 2, 2, 0, odd, b"out_dev"), (1, RG_OBS_F32, 2, 2, 0, odd, b"out_dev")]
    for kind, dt, ry, rx, flag, o, word in cases:
        for name in ("rg_obs_crop_typed", "rg_step_obs_crop_typed"):
            if name == "rg_obs_crop_typed":
                rc = L.rg_obs_crop_typed(h.h, kind, dt, ry, rx, flag, 0, o, None)
            else:
                rc = L.rg_step_obs_crop_typed(h.h, C.c_void_p(keys.data_ptr()), 1, kind, dt, ry, rx, flag, 0, o, None)
            msg = L.rg_last_error(h.h)
            assert rc != 0 and msg.startswith(name.encode() + b":") and word in msg, (name, kind, dt, ry, rx, flag, msg)
    torch.cuda.synchronize()
    assert bool((raw == 0xFF).all()), "a refused call wrote to the buffer"
    assert np.array_equal(hip.fetch()[2], status0), "a refused rg_step_obs_crop_typed stepped"
    assert torch.equal(typed_crop_call(h, 2, RG_OBS_U8, 1, 1, 0, False)[1], cen0), "a refused rg_step_obs_crop_typed moved a player"
    big, nbytes, shape, _ = buffers(h, 2, RG_OBS_U8, 47, 159, 0, True)
    assert L.rg_obs_crop_typed(h.h, 2, RG_OBS_U8, 47, 159, 0, 1, C.c_void_p(big.data_ptr()), None) == 0  # the largest radii; centres are optional
    as_bits(big, nbytes, shape, RG_OBS_U8)
    hip.sync()
    h.close()


def test_f32_is_the_f32_crop_and_the_step_call_is_step_then_crop(goldens):
    """RG_OBS_F32 with kinds 0 / 1 equals rg_obs_crop bit for bit; rg_step_obs_crop_typed equals rg_step + rg_obs_crop_typed on a twin over 20 steps."""
    torch = torch_mod()
    n, ry, rx = 21, 2, 3
    cfg = goldens["configs"]["mini"]
    a, b = HipBatch(cfg, range(n), max_steps=12), HipBatch(cfg, range(n), max_steps=12)
    ha, hb = a.h, b.h
    use_torch_stream(ha)
    use_torch_stream(hb)
    rng = np.random.RandomState(13)
    for t in range(20):
        keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)]
        dkeys = torch.as_tensor(keys, device="cuda:%d" % ha.device)
        kind, dt = PAIRS[t % len(PAIRS)]
        flag = 0 if kind == 2 else FULL
        got_a, cen_a = typed_crop_call(ha, kind, dt, ry, rx, flag, True, keys=dkeys)
        torch.cuda.synchronize()
        b.step(keys)
        got_b, cen_b = typed_crop_call(hb, kind, dt, ry, rx, flag, True)
        assert torch.equal(got_a, got_b) and torch.equal(cen_a, cen_b), t
        same_mirrors(ha, hb, "step call t=%d" % t)
        check_window(Fulls(ha), kind, dt, ry, rx, flag, True, got_a, cen_a, "step call t=%d" % t)
        for fk in (0, 1):
            got, cen = typed_crop_call(ha, fk, RG_OBS_F32, ry, rx, FULL, True)
            ref, cen_r = crop_call(ha, fk, ry, rx, FULL, True)
            assert torch.equal(got, ref.view(torch.int32)) and torch.equal(cen, cen_r), (t, fk)
        for h in (ha, hb):
            drain_tile_errors(h)
    ha.close()
    hb.close()


# ---------------------------------------------------------------------------------------------
# 7. crop views beside the main observation
# ---------------------------------------------------------------------------------------------
def view_env(goldens, mode, with_views):
    """(env, twin kwargs-free description) of one of the env kinds the class builds."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    mini = goldens["configs"]["mini"]
    n = 24
    cfgs = seeded(mini, range(40, 40 + n))
    kw = {}
    if mode == "persistent":
        kw = {"persistent_obs": True}
    elif mode == "bf16":
        kw = {"obs_dtype": torch.bfloat16}
    elif mode == "ids":
        kw = {"symbol_ids": True, "image_setting": ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, True)}
    elif mode == "crop0":
        kw = {"crop": 0}
    elif mode == "mixed":
        enemies = {"enemies": list(range(10))}
        shapes = [dict(mini, enemies=enemies), {"width": 80, "height": 24, "enemies": enemies},
                  {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": enemies}]
        cfgs = [dict(shapes[i % 3], seed=6100 + i) for i in range(12)]
        kw = {"crop": (2, 3)}
    env = HipVecRogueEnv(cfgs, max_steps=12, **kw)
    views = []
    if with_views:
        views = [env.add_crop(4, image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False), symbol_ids=True),
                 env.add_crop((2, 6), image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, True), obs_dtype=torch.bfloat16)]
        assert env.crops == tuple(views)
        assert views[0].obs.dtype == torch.uint8 and tuple(views[0].obs.shape) == (env.num_envs, 1, 9, 9)
        assert views[1].obs.dtype == torch.bfloat16 and tuple(views[1].obs.shape) == (env.num_envs, env._h.symbols + 1, 5, 13)
        assert all(v.center.dtype == torch.int32 and tuple(v.center.shape) == (env.num_envs, 2) for v in views)
    return env, views


def check_views(env, twin, views, where):
    """env.obs equals the twin's (an identical env without views); the views equal the reference built from the twin's full f32 images."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag

    assert env.obs.dtype == twin.obs.dtype and torch.equal(env.obs.view(torch.uint8), twin.obs.view(torch.uint8)), "%s: obs differs from the env without views" % where
    if env.crop_center is not None:
        assert torch.equal(env.crop_center, twin.crop_center), where
    ids, oh = views
    assert torch.equal(ids.center, oh.center), where
    if twin._h.mixed_sizes:
        check_host(twin._h, 2, RG_OBS_U8, 4, 4, ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False), ids.obs, ids.center, where + " id view")
        check_host(twin._h, 1, RG_OBS_BF16, 2, 6, oh.image_setting, oh.obs.view(torch.int16), oh.center, where + " one-hot view")
    else:
        fulls = Fulls(twin._h)
        check_window(fulls, 2, RG_OBS_U8, 4, 4, 0, False, ids.obs, ids.center, where + " id view")
        check_window(fulls, 1, RG_OBS_BF16, 2, 6, 0, True, oh.obs.view(torch.int16), oh.center, where + " one-hot view")
    drain_tile_errors(env._h)
    drain_tile_errors(twin._h)


@pytest.mark.parametrize("mode", ["default", "persistent", "bf16", "ids", "crop0", "mixed"])
def test_views_follow_every_refresh(goldens, mode):
    """Two views (ids of radius 4, bf16 one-hot with history of radius (2, 6)) on each kind of env, 30 steps with a reset_envs(mask=...), a clone_state
    and a reset(): after every call the views equal the reference and `obs` equals that of an identical env without views."""
    torch = torch_mod()
    env, views = view_env(goldens, mode, True)
    twin, _ = view_env(goldens, mode, False)
    n = env.num_envs
    check_views(env, twin, views, "%s added" % mode)
    gen = torch.Generator().manual_seed(21)
    kept = 0
    for t in range(30):
        keys = env._action_keys[torch.randint(0, len(env.ACTIONS), (n,), generator=gen).to(env.device)]
        if mode == "persistent":  # a mark in a cell that never changes (row 0 is blank): an env that is not re-encoded keeps it
            mark = env.obs[:, 0, 0, 0].clone()
            env.obs[:, 0, 0, 0] = 7.0
        obs, _, _ = env.step_keys(keys)
        twin.step_keys(keys)
        assert obs.data_ptr() == env.obs.data_ptr()
        if mode == "persistent":
            if t > 0:
                kept += int((env.obs[:, 0, 0, 0] == 7.0).sum())
            env.obs[:, 0, 0, 0] = mark
        check_views(env, twin, views, "%s t=%d" % (mode, t))
        if t == 8 and not env._h.mixed_sizes:  # (rg_reset_mask and the state records are not for handles with config groups)
            mask = torch.arange(n, device=env.device) % 3 == 1
            env.reset_envs(mask=mask)
            twin.reset_envs(mask=mask)
            check_views(env, twin, views, "%s reset_envs" % mode)
        if t == 15 and not env._h.mixed_sizes:
            env.clone_state([2] * 5, range(5, 10))
            twin.clone_state([2] * 5, range(5, 10))
            check_views(env, twin, views, "%s clone_state" % mode)
            assert torch.equal(views[0].obs[5:10], views[0].obs[2:3].expand(5, -1, -1, -1))
        if t == 22:
            env.reset()
            twin.reset()
            check_views(env, twin, views, "%s reset" % mode)
    if mode == "persistent":  # the views did not force the bound tensor into full re-encodes: envs whose screen did not change were not rewritten
        assert kept > 0, "every env of the bound tensor was rewritten at every step"
        assert env.counters()["keys"] == twin.counters()["keys"]
    env.close()
    twin.close()


def test_first_floor_view_shows_the_rebuilt_envs(goldens):
    """HipVecFirstFloor with a view: after a step that rebuilds envs (level 2 reached), the view shows the rebuilt envs' windows, like `obs`."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecFirstFloor

    n = 48
    env = HipVecFirstFloor(seeded(goldens["configs"]["mini"], range(n)), max_steps=200)
    view = env.add_crop(4, image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False), symbol_ids=True)
    gen = torch.Generator().manual_seed(22)
    rebuilt = 0
    for t in range(12):
        if t % 4 == 3:  # every env at level 2 before the step's end, whatever the key: the wrapper rebuilds them all
            env._h.check(env._h.L.rg_debug_descend(env._h.h))
        keys = env._action_keys[torch.randint(0, len(env.ACTIONS), (n,), generator=gen).to(env.device)]
        _, _, done = env.step_keys(keys)
        rebuilt += int(done.sum())
        assert bool((env.status[:, 0] == 1).all())
        check_window(Fulls(env._h), 2, RG_OBS_U8, 4, 4, 0, False, view.obs, view.center, "first floor t=%d" % t)
        drain_tile_errors(env._h)
    assert rebuilt >= n, rebuilt
    env.close()


def test_add_crop_argument_errors(goldens):
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    mini = goldens["configs"]["mini"]
    env = HipVecRogueEnv(seeded(mini, range(4)))
    sym = ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False)
    for bad in (None, -1, (2, -3), "x", (1.5, 2)):
        with pytest.raises(ValueError, match="crop"):
            env.add_crop(bad)
    with pytest.raises(ValueError, match="obs_dtype"):
        env.add_crop(2, obs_dtype=torch.float64)
    with pytest.raises(ValueError, match="symbol_ids"):
        env.add_crop(2, symbol_ids=True)  # the env's setting is gray
    with pytest.raises(ValueError, match="symbol_ids"):
        env.add_crop(2, image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.FULL, False), symbol_ids=True)
    with pytest.raises(ValueError, match="symbol_ids"):
        env.add_crop(2, image_setting=sym, obs_dtype=torch.bfloat16, symbol_ids=True)
    with pytest.raises(ValueError, match="image_setting"):
        env.add_crop(2, image_setting="gray")
    assert env.crops == ()
    v = env.add_crop(2)  # defaults: the env's own setting, f32
    assert v.obs.dtype == torch.float32 and tuple(v.obs.shape) == (4, 1, 5, 5) and env.crops == (v,)
    ref, cen = crop_call(env._h, 0, 2, 2, 0, False)
    assert torch.equal(v.obs, ref) and torch.equal(v.center, cen)
    env.close()
    # the constructor keeps its restrictions
    with pytest.raises(ValueError):
        HipVecRogueEnv(seeded(mini, range(4)), image_setting=sym, symbol_ids=True, crop=2)
    with pytest.raises(ValueError):
        HipVecRogueEnv(seeded(mini, range(4)), obs_dtype=torch.bfloat16, crop=2)
