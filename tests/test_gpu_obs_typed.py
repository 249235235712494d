"""Typed observations (rg_obs_typed / rg_step_obs_typed; HipVecRogueEnv(obs_dtype=..., symbol_ids=...)): f16 / bf16 images and the u8 symbol-id plane.

1. against the library's own f32 images (bit-identical to f32.to(T)) on the benchmark shapes; 2. a handle that only makes typed calls keeps the mirrors
and flag words of one that only makes f32 calls; 3. against the CPU oracle at the step it draws (tests/test_gpu_obs_oracle.py's scheme and helpers),
with the 'Z' rule; 4. interplay with the bound tensor, load_state and rg_set_stream; 5. refusals; 6. the Python surface."""
import ctypes as C

import numpy as np
import pytest

import typed_util as tu
from typed_util import RG_OBS_BF16, RG_OBS_F16, RG_OBS_F32, RG_OBS_U8

pytestmark = pytest.mark.gpu

FULL = 0x1FF
RG_FLAG_ERR_TILE = 0x00040000


def torch_mod():
    import torch

    return torch


def tdtype(dt):
    torch = torch_mod()
    return {RG_OBS_F16: torch.float16, RG_OBS_BF16: torch.bfloat16, RG_OBS_U8: torch.uint8, RG_OBS_F32: torch.float32}[dt]


def seeded(cfg, seeds):
    return [dict(cfg, seed=int(s)) for s in seeds]


def grid_cfg(w, h, rx, ry):
    return {"width": w, "height": h, "dungeon": {"style": "rogue", "room_num_x": rx, "room_num_y": ry, "min_room_size": {"x": 4, "y": 4}}}


def use_torch_stream(h):
    """A raw handle works on torch's current stream (what HipVecRogueEnv does for its own), so that torch's kernels and the handle's are ordered."""
    h.check(h.L.rg_set_stream(h.h, C.c_void_p(torch_mod().cuda.current_stream().cuda_stream)))


def prefilled(h, kind, dt, flag, with_hist):
    """The output tensor of a typed call, every element a NaN (16-bit types: 0xFFFF) or 0xFF, so that an element the pass does not write shows."""
    torch = torch_mod()
    dev = "cuda:%d" % h.device
    if kind == 2:
        return torch.full((h.n, 1 + int(with_hist), h.height, h.width), 0xFF, dtype=torch.uint8, device=dev)
    c = h.L.rg_obs_channels(h.h, kind, flag, int(with_hist))
    return torch.full((h.n, c, h.height, h.width), -1, dtype=torch.int16, device=dev).view(tdtype(dt))


def typed_call(h, kind, dt, flag, with_hist):
    out = prefilled(h, kind, dt, flag, with_hist)
    h.check(h.L.rg_obs_typed(h.h, kind, dt, flag, int(with_hist), C.c_void_p(out.data_ptr())))
    return out


def full_image(h, kind, flag, with_hist):
    """The library's f32 image of every env, now (rg_obs_gray / rg_obs_symbol), into a fresh tensor."""
    torch = torch_mod()
    c = h.L.rg_obs_channels(h.h, kind, flag, int(with_hist))
    out = torch.full((h.n, c, h.height, h.width), float("nan"), dtype=torch.float32, device="cuda:%d" % h.device)
    fn = h.L.rg_obs_symbol if kind else h.L.rg_obs_gray
    h.check(fn(h.h, flag, int(with_hist), C.c_void_p(out.data_ptr())))
    return out


def bits(t):
    return t.view(torch_mod().int16)


def assert_rounded(typed, f32, where):
    torch = torch_mod()
    exp = f32.to(typed.dtype)
    if not torch.equal(bits(typed), bits(exp)):
        bad = (bits(typed) != bits(exp)).reshape(typed.shape[0], -1).any(1).nonzero().flatten()
        e = int(bad[0])
        p, y, x = (int(v) for v in (bits(typed[e]) != bits(exp[e])).nonzero()[0])
        raise AssertionError("%s: %d envs differ from f32.to(%s), first env %d (plane %d, y %d, x %d): bits %#06x vs %#06x (f32 %r)" % (
            where, bad.numel(), typed.dtype, e, p, y, x, int(bits(typed)[e, p, y, x]) & 0xFFFF, int(bits(exp)[e, p, y, x]) & 0xFFFF, float(f32[e, p, y, x])))


def random_keys(env, gen):
    torch = torch_mod()
    return env._action_keys[torch.randint(0, len(env.ACTIONS), (env.num_envs,), generator=gen, device="cpu").to(env.device)]


def drain_tile_errors(h):
    """rg_sync after one-hot / id calls: a 'Z' is a legal monster of the stock configs and not a symbol; nothing else may be reported."""
    if h.L.rg_sync(h.h):
        assert b"Invalid tile" in h.L.rg_last_error(h.h), h.L.rg_last_error(h.h)


def compare_every_setting(h, where, typed_first):
    """Every kind x type x status_flag x with_hist of the typed call against the f32 call on the same handle and state; the ids against argmax of the
    one-hot image (envs whose image is valid) and against round(gray * symbols) (every env)."""
    torch = torch_mod()
    gray = onehot = hist_plane = None
    for kind in (0, 1):
        for flag in (0, FULL):
            for with_hist in (0, 1):
                if typed_first:
                    ty = [typed_call(h, kind, dt, flag, with_hist) for dt in (RG_OBS_F16, RG_OBS_BF16)]
                    f = full_image(h, kind, flag, with_hist)
                else:
                    f = full_image(h, kind, flag, with_hist)
                    ty = [typed_call(h, kind, dt, flag, with_hist) for dt in (RG_OBS_F16, RG_OBS_BF16)]
                for t in ty:
                    assert_rounded(t, f, "%s kind %d flag %#x hist %d" % (where, kind, flag, with_hist))
                if flag == 0 and kind == 0 and with_hist:
                    gray, hist_plane = f[:, 0].clone(), f[:, 1].clone()
                if flag == 0 and kind == 1 and not with_hist:
                    onehot = f
                del ty, f
    valid = (onehot.sum(1) == 1).reshape(h.n, -1).all(1)  # (a 'Z' on screen: no channel set at that cell)
    arg = onehot.argmax(1).to(torch.uint8)
    del onehot
    by_gray = torch.round(gray * h.symbols).to(torch.uint8)
    for with_hist in (0, 1):
        ids = typed_call(h, 2, RG_OBS_U8, 0, with_hist)
        assert torch.equal(ids[:, 0], by_gray), "%s ids hist %d: differ from round(gray * symbols)" % (where, with_hist)
        assert torch.equal(ids[valid, 0], arg[valid]), "%s ids hist %d: differ from onehot.argmax(1)" % (where, with_hist)
        if with_hist:
            assert torch.equal(ids[:, 1], hist_plane.to(torch.uint8)), "%s ids: history plane" % where
    return int(valid.sum())


# ---------------------------------------------------------------------------------------------
# 1. against the f32 path, benchmark shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,n", [("mini", 65536), ("default", 32768), ("nohide", 32768)])
def test_typed_is_the_rounded_f32_image(goldens, name, n):
    """Random policy with auto-resets, 300 steps, every setting compared at steps 1-3 and every 10th; on odd comparisons the typed call comes first
    after the step (it draws the pending Redraws), on even ones the f32 call."""
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv

    env = HipVecRogueEnv(seeded(goldens["configs"][name], range(n)), max_steps=60)
    gen = torch.Generator().manual_seed(5)
    compare_every_setting(env._h, "%s t=0" % name, True)
    k = 0
    for t in range(1, 301):
        keys = random_keys(env, gen)
        if not (t <= 3 or t % 10 == 0):
            env.step_keys(keys)
        else:  # (the step alone: the first observation call of the comparison draws its Redraws)
            env._h.check(env._h.L.rg_step(env._h.h, C.c_void_p(keys.data_ptr()), 1))
            k += 1
            valid = compare_every_setting(env._h, "%s t=%d" % (name, t), bool(k & 1))
            assert valid > n // 2, valid
    drain_tile_errors(env._h)
    env.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("geom", ["36x18", "48x20", "32x48", "160x48", "160x48-66rooms"])
def test_typed_on_other_grids(geom):
    """Grids whose items do not fill whole waves (36x18: 81 pieces of 8 cells, and no 16-cell pieces: ids refused), two- and three-wave envs and the largest
    grid (four items per thread, one env per block); with 66 rooms the Redraw sweep does not apply and k_render draws."""
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv

    w, hh = (int(v) for v in geom.split("-")[0].split("x"))
    rx, ry = {"36x18": (2, 2), "48x20": (2, 2), "32x48": (1, 3), "160x48": (4, 4), "160x48-66rooms": (11, 6)}[geom]
    n = 1031 if w < 160 else 259
    env = HipVecRogueEnv(seeded(grid_cfg(w, hh, rx, ry), range(n)), max_steps=40)
    h = env._h
    gen = torch.Generator().manual_seed(8)
    for t in range(1, 41):
        keys = random_keys(env, gen)
        if t % 5:
            env.step_keys(keys)
        else:  # (the step alone: the first observation call below draws its Redraws)
            h.check(h.L.rg_step(h.h, C.c_void_p(keys.data_ptr()), 1))
            if (w * hh) % 16 == 0:
                compare_every_setting(h, "%s t=%d" % (geom, t), bool(t & 1))
            else:
                for kind, flag, with_hist in ((0, 0, 0), (1, FULL, 1), (0, FULL, 1), (1, 0, 0)):
                    t16 = typed_call(h, kind, RG_OBS_BF16, flag, with_hist)
                    assert_rounded(t16, full_image(h, kind, flag, with_hist), "%s t=%d kind %d" % (geom, t, kind))
                out = prefilled(h, 2, RG_OBS_U8, 0, 0)
                assert h.L.rg_obs_typed(h.h, 2, RG_OBS_U8, 0, 0, C.c_void_p(out.data_ptr())) != 0
                assert b"multiple of 16" in h.L.rg_last_error(h.h)
    drain_tile_errors(h)
    env.close()


# ---------------------------------------------------------------------------------------------
# 2. Redraws drawn by the typed call itself: twin handles
# ---------------------------------------------------------------------------------------------
def stair_seeker_keys(drv, gen):
    from test_gpu_crop import stair_seeker_keys as seeker

    return seeker(drv, gen)


def descents_of(h):
    out = (C.c_uint64 * 9)()
    h.check(h.L.rg_counters_ex(h.h, out, 9, 0))
    return int(out[1])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind,dt,flag,with_hist", [(0, RG_OBS_BF16, 0, 0), (0, RG_OBS_F16, FULL, 1), (1, RG_OBS_BF16, 0, 1), (1, RG_OBS_F16, FULL, 0), (2, RG_OBS_U8, 0, 1)],
                         ids=["gray-bf16", "gray-f16-planes", "onehot-bf16-hist", "onehot-f16-status", "ids-hist"])
def test_typed_only_handle_has_the_mirrors_of_an_f32_only_handle(goldens, kind, dt, flag, with_hist):
    """Twin handles on the 80x24 dungeon, same seeds and keys: one makes only typed calls (rg_step_obs_typed, or rg_step + rg_obs_typed on every third
    step), the other only f32 calls; neither's mirrors are read inside a 20-step block.  At the end of every block of 200 steps: screen, history, status
    and the whole flag words (public and bookkeeping bits) of all envs are equal.  The keys come from a stair seeker that looks at a THIRD env batch
    of the same seeds (a crop env: it reads its own mirrors), so descents with stale history planes happen."""
    torch = torch_mod()
    from parity_util import HipBatch
    from rogue_gym.envs.device import HipVecRogueEnv

    cfg, n = goldens["configs"]["nohide"], 2048
    seeds = range(300, 300 + n)
    drv = HipVecRogueEnv(seeded(cfg, seeds), max_steps=500, crop=0)
    a, b = HipBatch(cfg, seeds, max_steps=500), HipBatch(cfg, seeds, max_steps=500)
    ha, hb, L = a.h, b.h, a.h.L
    use_torch_stream(ha)
    use_torch_stream(hb)
    out_a = prefilled(ha, kind, dt, flag, with_hist)
    fk = 1 if kind else 0  # the f32 twin: the gray image, or the one-hot image (for the ids too: it raises the same tile errors)
    out_b = full_image(hb, fk, flag, with_hist)
    ha.check(L.rg_obs_typed(ha.h, kind, dt, flag, with_hist, C.c_void_p(out_a.data_ptr())))
    f32_call = L.rg_obs_symbol if fk else L.rg_obs_gray
    gen = torch.Generator().manual_seed(4)
    for t in range(1, 201):
        keys = stair_seeker_keys(drv, gen)
        kp = C.c_void_p(keys.data_ptr())
        drv.step_keys(keys)
        if t % 3:
            ha.check(L.rg_step_obs_typed(ha.h, kp, 1, kind, dt, flag, with_hist, C.c_void_p(out_a.data_ptr())))
        else:
            ha.check(L.rg_step(ha.h, kp, 1))
            ha.check(L.rg_obs_typed(ha.h, kind, dt, flag, with_hist, C.c_void_p(out_a.data_ptr())))
        hb.check(L.rg_step(hb.h, kp, 1))
        hb.check(f32_call(hb.h, flag, with_hist, C.c_void_p(out_b.data_ptr())))
        if kind == 2:
            pass  # (compared in section 1)
        elif t % 20 == 0:
            assert_rounded(out_a, out_b, "twins t=%d" % t)
        if t % 20 == 0:
            torch.cuda.synchronize()
            fa, fb = ha.fetch(), hb.fetch()
            for what, x, y in zip(("screen", "hist", "status", "flags"), fa, fb):
                if not np.array_equal(x, y):
                    bad = np.nonzero((x != y).reshape(n, -1).any(1))[0]
                    raise AssertionError("t=%d: %s of %d envs differ between the typed-only and the f32-only handle, first %s: %s vs %s" % (
                        t, what, len(bad), bad[:8].tolist(), x[bad[0]].reshape(-1)[:16], y[bad[0]].reshape(-1)[:16]))
            assert np.array_equal(fa[0], drv.screen.cpu().numpy()), "t=%d: the policy's env batch left the twins" % t
    d = descents_of(hb)
    print("descents of the f32 twin: %d of %d envs x 200 steps" % (d, n))
    assert d >= n // 100 and descents_of(ha) == d, (d, descents_of(ha))
    for h in (ha, hb):
        drain_tile_errors(h)
        h.close()
    drv.close()


# ---------------------------------------------------------------------------------------------
# 3. against the oracle at the step it draws
# ---------------------------------------------------------------------------------------------
def play_typed(case, cfg, n, steps, max_steps, kind, dt, flag, with_hist, seed, zed=False, no_mirror=False):
    """HipVecRogueEnv(obs_dtype / symbol_ids) of n envs against one OracleEnv per env under the stair seeker of test_gpu_obs_oracle.py; after every step
    (nothing reads the mirrors in between) every env's typed observation equals the oracle's image rounded by typed_util -- ids: Symbol::from_tile of
    the oracle's screen (typed_util.SYMBOL_OF_TILE) and its history plane.  One-hot and ids: the envs flagged RG_FLAG_ERR_TILE are exactly the envs whose
    oracle image raises, and rg_sync fails iff there is one."""
    import test_gpu_obs_oracle as oo
    from oracle.pyoracle import OracleEnv

    torch = torch_mod()
    ids = kind == 2
    kw = {"symbol_ids": True} if ids else {"obs_dtype": tdtype(dt)}
    env = oo.vec_env(seeded(cfg, range(n)), 1 if ids else kind, flag, bool(with_hist), no_mirror=no_mirror, max_steps=max_steps, **kw)
    assert env.obs.dtype == tdtype(dt) and tuple(env.obs.shape) == (n, env.channels, env.height, env.width)
    oracles = [OracleEnv(cfg, max_steps=max_steps, seed=i) for i in range(n)]
    rng = np.random.RandomState(seed)
    envs = np.arange(n)
    descents = errs = 0
    for t in range(0, steps + 1):
        if t:
            keys = oo.seeker_keys(oracles, rng)
            lv = [int(o.status_arr()[0]) for o in oracles]
            obs, _, _ = env.step_keys(oo.device_keys(env, keys))
            for k, o in enumerate(oracles):
                o.step_autoreset(int(keys[k]))
                descents += int(o.status_arr()[0]) > lv[k]
        else:
            obs = env.obs
        fl = env.flags.cpu().numpy() if kind else None
        if ids:
            got = obs.cpu().numpy()
            _, bad = oo.expected(oracles, 1, 0, False)
            exp = [np.stack([tu.symbol_ids(o.screen())] + ([np.asarray(o.hist(), np.uint8)] if with_hist else [])) for o in oracles]
            oo.check_list(case, t, envs, got, exp, set(), env._h, lambda k: oracles[k].screen())
            flagged = {k for k in range(n) if int(fl[k]) & RG_FLAG_ERR_TILE}
            assert flagged == bad, "%s step %d: envs flagged ERR_TILE %s, envs whose oracle image raises %s" % (case, t, sorted(flagged), sorted(bad))
            for k in bad:
                assert (got[k][0] >= env.symbols - 1).any(), "%s step %d env %d: no id without a channel" % (case, t, k)
                if zed:
                    assert np.array_equal(got[k][0] == 42, oracles[k].screen() == ord("Z")), "%s step %d env %d: 'Z' is id 42" % (case, t, k)
        else:
            got = obs.view(torch.int16).cpu().numpy().view(np.uint16)
            exp, bad = oo.expected(oracles, kind, flag, bool(with_hist))
            exp = [None if e is None else tu.bits16(e, dt) for e in exp]
            oo.check_list(case, t, envs, got, exp, bad, env._h, lambda k: oracles[k].screen(), fl)
        if kind:
            errs += bool(bad)
            if bad and t % 2:  # (the Python surface of the same report)
                with pytest.raises(RuntimeError, match="Invalid tile"):
                    env.check_errors()
            else:
                oo.drain(env._h, bad)
    if not zed:
        assert descents > 0, "%s: no env descended" % case
    else:
        assert errs > 1, "%s: no env showed a 'Z'" % case
    env.close()


@pytest.mark.timeout(400)
@pytest.mark.parametrize("name,kind,dt,planes", [
    ("mini", 0, RG_OBS_BF16, False), ("mini", 0, RG_OBS_F16, True), ("mini", 1, RG_OBS_F16, False), ("mini", 1, RG_OBS_BF16, True), ("mini", 2, RG_OBS_U8, True),
    ("default", 0, RG_OBS_F16, False), ("default", 0, RG_OBS_BF16, True), ("nohide", 1, RG_OBS_BF16, False), ("nohide", 1, RG_OBS_F16, True), ("nohide", 2, RG_OBS_U8, True),
    ("nohide", 2, RG_OBS_U8, False)])
def test_typed_against_the_oracle_every_step(goldens, name, kind, dt, planes):
    """64 envs x 150 steps of mini and 80x24, lock step with the oracle."""
    flag, with_hist = (0 if kind == 2 else FULL, 1) if planes else (0, 0)
    play_typed("typed %s kind %d dtype %d%s" % (name, kind, dt, " planes" if planes else ""), goldens["configs"][name], 64, 150, 40, kind, dt, flag, with_hist,
               seed=3 + kind + dt)


@pytest.mark.timeout(400)
@pytest.mark.parametrize("name,kind,dt", [("mini", 0, RG_OBS_BF16), ("default", 0, RG_OBS_F16), ("nohide", 2, RG_OBS_U8)])
def test_typed_against_the_oracle_every_redraw_from_the_tiles(goldens, name, kind, dt):
    """The same with ROGUE_GYM_HIP_NO_MIRROR_UPDATE: the step kernel leaves every Redraw to the observation call, which draws all of them from the tiles."""
    play_typed("typed no-mirror-update %s kind %d" % (name, kind), goldens["configs"][name], 64, 100, 40, kind, dt, 0 if kind == 2 else FULL, 1, seed=17 + kind,
               no_mirror=True)


@pytest.mark.timeout(400)
@pytest.mark.parametrize("kind,dt", [(2, RG_OBS_U8), (1, RG_OBS_BF16)])
def test_typed_invalid_tile_rule(goldens, kind, dt):
    """A mini config whose common monster is a custom 'Z' (symbol 42 of 43: no channel): the ids hold 42 at its cell, RG_FLAG_ERR_TILE is set on exactly
    the envs whose oracle image raises, check_errors() raises."""
    import test_gpu_obs_oracle as oo

    cfg = dict(goldens["configs"]["mini"], enemies={"enemies": [oo.ZED], "appear_rate_gold": 100, "appear_rate_nogold": 100}, hide_dungeon=False)
    play_typed("typed zed kind %d" % kind, cfg, 64, 150, 40, kind, dt, 0, 1, seed=9, zed=True)


# ---------------------------------------------------------------------------------------------
# 4. interplay: the bound tensor, load_state, rg_set_stream
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,kind", [("mini", 0), ("nohide", 1)])
def test_typed_call_between_bound_tensor_calls(goldens, name, kind):
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    n = 4096 if name == "mini" else 1024
    env = HipVecRogueEnv(seeded(goldens["configs"][name], range(n)), max_steps=50, persistent_obs=True,
                         image_setting=ImageSetting(DungeonType.SYMBOL if kind else DungeonType.GRAY, StatusFlag.EMPTY, False))
    h, L = env._h, env._h.L
    gen = torch.Generator().manual_seed(12)
    for t in range(1, 61):
        keys = random_keys(env, gen)
        cmp_typed = False
        if t % 3 == 0:    # bound call, typed call (nothing pending: the bound tensor stays current), bound call in place
            env.step_keys(keys)
            ty = typed_call(h, kind, RG_OBS_BF16, 0, 0)
            env.step_keys(random_keys(env, gen))
        elif t % 3 == 1:  # step, typed call (draws the pending Redraws), bound call
            h.check(L.rg_step(h.h, C.c_void_p(keys.data_ptr()), 1))
            ty = typed_call(h, 2 if kind and t % 2 else kind, RG_OBS_U8 if kind and t % 2 else RG_OBS_F16, 0, 0)
            env._encode()
            cmp_typed = ty.dtype != torch.uint8
        else:             # two steps with a typed call after the first, then the bound call
            h.check(L.rg_step(h.h, C.c_void_p(keys.data_ptr()), 1))
            ty = typed_call(h, kind, RG_OBS_BF16, FULL, 1)
            env.step_keys(random_keys(env, gen))
        fresh = full_image(h, kind, 0, False)  # (another tensor: the unbound encode of every env)
        assert torch.equal(env.obs, fresh), "t=%d: the bound tensor differs from an unbound encode in %d envs" % (
            t, int((env.obs != fresh).reshape(n, -1).any(1).sum()))
        if cmp_typed:
            assert_rounded(ty, fresh, "t=%d typed beside the bound tensor" % t)
        env._encode()  # (the bound tensor's own call again: in place from here)
    drain_tile_errors(h)
    env.close()


@pytest.mark.timeout(300)
def test_typed_after_load_state_and_on_a_side_stream(goldens):
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv

    cfg, n = goldens["configs"]["default"], 1024
    ref = HipVecRogueEnv(seeded(cfg, range(n)), max_steps=80)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # (the env takes torch's current stream: rg_set_stream)
        env = HipVecRogueEnv(seeded(cfg, range(n)), max_steps=80, obs_dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(13)

    def both(fn):
        torch.cuda.synchronize()  # (the keys were made on the default stream)
        with torch.cuda.stream(side):
            got = fn(env)
        side.synchronize()
        exp = fn(ref)
        torch.cuda.synchronize()
        return got, exp

    def same(where):
        side.synchronize()
        torch.cuda.synchronize()
        assert env.obs.dtype == torch.bfloat16
        assert_rounded(env.obs, ref.obs, where)

    same("t=0")
    for t in range(25):
        keys = random_keys(ref, gen)
        both(lambda e: e.step_keys(keys))
        same("side stream t=%d" % t)
    recs, recs_ref = both(lambda e: e.save_state())
    for t in range(10):
        keys = random_keys(ref, gen)
        both(lambda e: e.step_keys(keys))
    both(lambda e: e.load_state(recs_ref if e is ref else recs))
    same("after load_state")
    half = list(range(0, n, 2))
    both(lambda e: e.load_state((recs_ref if e is ref else recs)[1::2], half))
    same("after load_state of every other env")
    for t in range(10):
        keys = random_keys(ref, gen)
        both(lambda e: e.step_keys(keys))
        same("after load_state t=%d" % t)
    env.check_errors()
    ref.check_errors()
    env.close()
    ref.close()


# ---------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_typed_refusals(goldens):
    torch = torch_mod()
    from parity_util import HipBatch
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    mini = goldens["configs"]["mini"]
    hip = HipBatch(mini, range(64))
    h, L = hip.h, hip.h.L
    use_torch_stream(h)
    buf = torch.full((64 * 64 * 16 * 32 + 64,), 0xFF, dtype=torch.uint8, device="cuda:%d" % h.device)  # room for every image of this handle
    p = buf.data_ptr()
    assert p % 16 == 0

    def refused(fn, args, match):
        assert fn(h.h, *args) != 0, args
        msg = L.rg_last_error(h.h).decode()
        assert match in msg and ("rg_step_obs_typed" if fn is L.rg_step_obs_typed else "rg_obs_typed") in msg, (args, msg)

    status0 = hip.fetch()[2].copy()
    keys = torch.full((64,), ord("h"), dtype=torch.uint8, device=buf.device)
    for fn, pre in ((L.rg_obs_typed, ()), (L.rg_step_obs_typed, (C.c_void_p(keys.data_ptr()), 1))):
        refused(fn, pre + (0, RG_OBS_BF16, 0, 0, None), "out_dev")
        refused(fn, pre + (0, RG_OBS_BF16, 0, 0, C.c_void_p(p + 2)), "out_dev")
        refused(fn, pre + (0, RG_OBS_F32, 0, 0, C.c_void_p(p + 4)), "out_dev")
        refused(fn, pre + (2, RG_OBS_U8, 0, 0, C.c_void_p(p + 8)), "out_dev")
        refused(fn, pre + (0, RG_OBS_U8, 0, 0, C.c_void_p(p)), "RG_OBS_U8")
        refused(fn, pre + (1, RG_OBS_U8, 0, 1, C.c_void_p(p)), "RG_OBS_U8")
        refused(fn, pre + (2, RG_OBS_BF16, 0, 0, C.c_void_p(p)), "kind 2")
        refused(fn, pre + (2, RG_OBS_F32, 0, 0, C.c_void_p(p)), "kind 2")
        refused(fn, pre + (2, RG_OBS_U8, 0x1, 0, C.c_void_p(p)), "status_flag")
        refused(fn, pre + (3, RG_OBS_BF16, 0, 0, C.c_void_p(p)), "kind")
        refused(fn, pre + (-1, RG_OBS_F16, 0, 0, C.c_void_p(p)), "kind")
        refused(fn, pre + (0, 4, 0, 0, C.c_void_p(p)), "dtype")
        refused(fn, pre + (1, -1, 0, 0, C.c_void_p(p)), "dtype")
    torch.cuda.synchronize()
    assert bool((buf == 0xFF).all()), "a refused call wrote to its tensor"
    assert np.array_equal(hip.fetch()[2], status0), "a refused rg_step_obs_typed stepped"
    # dtype F32 with kinds 0 / 1 is the existing call
    for kind in (0, 1):
        f = full_image(h, kind, FULL, True)
        g = torch.full_like(f, float("nan"))
        h.check(L.rg_obs_typed(h.h, kind, RG_OBS_F32, FULL, 1, C.c_void_p(g.data_ptr())))
        assert torch.equal(f, g)
    hip.sync()
    h.close()

    def refused_on(env, match):
        hh = env._h
        out = torch.full((hh.n * 64 * 48 * 160,), 0xFF, dtype=torch.uint8, device=env.device)
        for kind, dt in ((0, RG_OBS_BF16), (1, RG_OBS_F16), (2, RG_OBS_U8)):
            assert L.rg_obs_typed(hh.h, kind, dt, 0, 0, C.c_void_p(out.data_ptr())) != 0
            msg = L.rg_last_error(hh.h).decode()
            assert "rg_obs_typed" in msg and match in msg, msg
        torch.cuda.synchronize()
        assert bool((out == 0xFF).all())
        env.close()

    # config groups, mixed sizes (handles that a crop env can be built on)
    refused_on(HipVecRogueEnv([dict(mini, seed=1), dict(mini, seed=2, enemies={"enemies": []}), dict(mini, seed=3)], crop=2), "config groups")
    refused_on(HipVecRogueEnv([dict(mini, seed=1), {"width": 80, "height": 24, "seed": 2}], crop=2), "config groups or mixed sizes")
    # H*W not a multiple of 8: the smallest screen is 32x16, so 30x15 is no config at all; 33x17 is the nearest grid with an odd cell count
    with pytest.raises(RuntimeError, match="too narrow"):
        HipBatch(grid_cfg(30, 15, 2, 2), range(2))
    env = HipVecRogueEnv(seeded(grid_cfg(33, 17, 2, 2), range(8)))
    assert (env.height * env.width) % 8 != 0
    refused_on(env, "multiple of")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        HipVecRogueEnv(seeded(grid_cfg(33, 17, 2, 2), range(8)), obs_dtype=torch.bfloat16)

    # the Python surface
    sym = ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False)
    cfgs = seeded(mini, range(4))
    with pytest.raises(ValueError, match="obs_dtype"):
        HipVecRogueEnv(cfgs, obs_dtype=torch.float64)
    with pytest.raises(ValueError, match="obs_dtype"):
        HipVecRogueEnv(cfgs, obs_dtype=torch.uint8)
    with pytest.raises(ValueError, match="symbol_ids"):
        HipVecRogueEnv(cfgs, symbol_ids=True)  # (gray)
    with pytest.raises(ValueError, match="symbol_ids"):
        HipVecRogueEnv(cfgs, image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.FULL, False), symbol_ids=True)
    with pytest.raises(ValueError, match="symbol_ids"):
        HipVecRogueEnv(cfgs, image_setting=sym, symbol_ids=True, obs_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="symbol_ids=True cannot be combined with crop"):
        HipVecRogueEnv(cfgs, image_setting=sym, symbol_ids=True, crop=2)
    with pytest.raises(ValueError, match="symbol_ids=True cannot be combined with persistent_obs"):
        HipVecRogueEnv(cfgs, image_setting=sym, symbol_ids=True, persistent_obs=True)
    with pytest.raises(ValueError, match="bfloat16 cannot be combined with crop"):
        HipVecRogueEnv(cfgs, obs_dtype=torch.bfloat16, crop=(1, 2))
    with pytest.raises(ValueError, match="float16 cannot be combined with persistent_obs"):
        HipVecRogueEnv(cfgs, obs_dtype=torch.float16, persistent_obs=True)
    HipVecRogueEnv(cfgs, obs_dtype=torch.float32, crop=2).close()  # (f32 by name: today's paths)
    HipVecRogueEnv(cfgs, obs_dtype=torch.float32, persistent_obs=True).close()


# ---------------------------------------------------------------------------------------------
# 6. HipVecRogueEnv(obs_dtype=...), (symbol_ids=True)
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", ["bf16-gray", "f16-gray-planes", "bf16-onehot", "ids", "ids-hist"])
def test_vec_env_typed_follows_the_default_env(goldens, mode):
    """100 steps of step(): obs equal to a default env's obs.to(...) / argmax(1), reward and done equal; then seed() + reset(), and 20 steps more."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    n = 2048
    cfg = goldens["configs"]["mini" if "gray" in mode else "nohide"]
    ids = mode.startswith("ids")
    st = {"bf16-gray": ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), "f16-gray-planes": ImageSetting(DungeonType.GRAY, StatusFlag.FULL, True),
          "bf16-onehot": ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False), "ids": ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False),
          "ids-hist": ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, True)}[mode]
    kw = {"symbol_ids": True} if ids else {"obs_dtype": torch.float16 if mode.startswith("f16") else torch.bfloat16}
    env = HipVecRogueEnv(seeded(cfg, range(n)), max_steps=30, image_setting=st, **kw)
    ref = HipVecRogueEnv(seeded(cfg, range(n)), max_steps=30, image_setting=st)
    assert env.obs.dtype == (torch.uint8 if ids else kw["obs_dtype"]) and ref.obs.dtype == torch.float32
    assert env.channels == (1 + int(st.includes_hist) if ids else ref.channels) and tuple(env.obs.shape) == (n, env.channels, env.height, env.width)

    def same(where, obs, robs):
        if ids:
            valid = (robs[:, :ref.symbols].sum(1) == 1).reshape(n, -1).all(1)
            assert torch.equal(obs[valid, 0], robs[valid, :ref.symbols].argmax(1).to(torch.uint8)), where
            assert int(valid.sum()) > n // 2
            if st.includes_hist:
                assert torch.equal(obs[:, 1], robs[:, -1].to(torch.uint8)), where
        else:
            assert_rounded(obs, robs, where)

    same("t=0", env.obs, ref.obs)
    gen = torch.Generator().manual_seed(21)
    for t in range(120):
        if t == 100:
            env.seed(range(7000, 7000 + n))
            ref.seed(range(7000, 7000 + n))
            same("reset", env.reset(), ref.reset())
        act = torch.randint(0, len(env.ACTIONS), (n,), generator=gen).to(env.device)
        obs, rew, done = env.step(act)
        robs, rrew, rdone = ref.step(act)
        assert obs is env.obs
        same("t=%d" % t, obs, robs)
        assert torch.equal(rew, rrew) and torch.equal(done, rdone), t
    table = torch.arange(env.symbols, device=env.device, dtype=torch.float32)[:, None].expand(env.symbols, 4).contiguous()
    if ids:  # nn.Embedding-style indexing
        emb = table[env.obs[:, 0].long().clamp(max=env.symbols - 1)]
        assert tuple(emb.shape) == (n, env.height, env.width, 4)
    for e in (env, ref):
        drain_tile_errors(e._h)
        e.close()
