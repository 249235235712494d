"""The C calls the Python bindings make, by name and in order (rogue_gym/envs/device.py, rogue_gym_python/_rogue_gym.py): a recording proxy stands in for the
loaded library while an env is built, so every entry point the env or its handle looks up is logged and forwarded.  The expected sequences are literals: an env
without optional features makes one call per step, every optional feature adds its own calls at its own place, and the handle's host readers share one
grow-only device scratch buffer.  (A binding that looked its functions up once and kept them would log nothing and fail here.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4
CROPS = ["rg_obs_crop_typed", "rg_obs_crop_typed"]
# what follows every refresh of `obs` in an env with every optional feature: the crop views in add_crop order, pixels, action mask, guide, monsters, objects
REFRESH = CROPS + ["rg_obs_pixels_crop", "rg_action_mask", "rg_path", "rg_monsters", "rg_objects"]
REFRESH_ROUTE = [c if c != "rg_path" else "rg_route" for c in REFRESH]
AFTER_STEP = ["rg_episode_update", "rg_novelty_update", "rg_archive_update"]


class Recorder:
    """Stands in for the ctypes library: every attribute is a wrapper that logs the entry point's name and forwards the call."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.log.append(name)
            return fn(*args)
        return call

    def take(self):
        out, self.log[:] = list(self.log), []
        return out


@pytest.fixture
def rec(monkeypatch):
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    r = Recorder(inner.load_library())
    monkeypatch.setattr(inner, "_lib", r)
    return r


def make_env(goldens, **kw):
    from rogue_gym.envs import HipVecRogueEnv
    return HipVecRogueEnv([dict(goldens["configs"]["mini"], seed=11 + i) for i in range(N)], max_steps=50, **kw)


def full_env(goldens, **kw):
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    opts = dict(pixels="gray", pixel_crop=2, action_mask=True, guide="stairs", monsters="shown", objects="known", episodes=True, scout=True, novelty="screen",
                archive=1024, archive_auto=True)
    opts.update(kw)
    env = make_env(goldens, **opts)
    env.add_crop(2)
    env.add_crop((1, 3), ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False), symbol_ids=True)
    return env


def keys_of(env, ch="h"):
    return env.torch.full((N,), ord(ch), dtype=env.torch.uint8, device=env.device)


def test_plain_gray_env_makes_one_call_per_step(rec, goldens):
    env = make_env(goldens)
    keys = keys_of(env)
    rec.take()
    for _ in range(3):
        env.step_keys(keys)
        assert rec.take() == ["rg_step_obs_gray"]
    env.reset()
    assert rec.take() == ["rg_reset", "rg_obs_gray"]
    env.step(env.torch.ones((N,), dtype=env.torch.int64, device=env.device))
    assert rec.take() == ["rg_step_obs_gray"]
    env.check_errors()
    env.close()


def check_full(env, rec, refresh):
    torch = env.torch
    keys = keys_of(env)
    rec.take()
    for _ in range(2):
        env.step_keys(keys)
        assert rec.take() == ["rg_step_obs_gray"] + AFTER_STEP + refresh
    env.reset()
    assert rec.take() == ["rg_reset", "rg_episode_cut", "rg_obs_gray"] + refresh + ["rg_novelty_cut"]
    env.reset_envs(env_ids=[1])
    assert rec.take() == ["rg_reset_envs", "rg_episode_cut", "rg_obs_gray"] + refresh + ["rg_novelty_cut"]
    mask = torch.tensor([True, False, False, True], device=env.device)
    rec.take()
    env.reset_envs(mask=mask)
    assert rec.take() == ["rg_reset_mask", "rg_episode_cut", "rg_obs_gray"] + refresh + ["rg_novelty_cut"]
    env.load_state(env.save_state())
    assert rec.take() == ["rg_state_record_bytes", "rg_state_save", "rg_state_load", "rg_obs_gray"] + refresh + ["rg_novelty_cut"]
    env.check_errors()
    env.close()


def test_every_feature_adds_its_calls_in_order(rec, goldens):
    check_full(full_env(goldens), rec, REFRESH)


@pytest.mark.parametrize("guide", [dict(guide="explore"), dict(guide="stairs", guide_secrets=True)], ids=["explore", "secrets"])
def test_route_guides_call_rg_route_not_rg_path(rec, goldens, guide):
    assert "rg_route" in REFRESH_ROUTE and "rg_path" not in REFRESH_ROUTE
    check_full(full_env(goldens, **guide), rec, REFRESH_ROUTE)


def test_handle_readers_share_one_grow_only_scratch(rec, goldens):
    """action_mask (44 bytes for 4 envs), path_keys (20), route_keys (24), monster_tables (320), object_tables (576) in a row: the first call allocates, the
    two that fit allocate nothing, each of the two that outgrow the buffer replaces it (the outgrown one is released right before the one allocation of that
    growth -- the only rg_dev_free before close()), a second round allocates and frees nothing, and close() frees the buffer once."""
    env = make_env(goldens)
    h = env._h
    rec.take()
    mask = h.action_mask()
    assert rec.take() == ["rg_dev_alloc", "rg_action_mask", "rg_dev_read"]
    keys, dist = h.path_keys("stairs")
    assert rec.take() == ["rg_path", "rg_dev_read"]
    rkeys, rdist, rtier = h.route_keys("stairs", "frontier", False, True)
    assert rec.take() == ["rg_route", "rg_dev_read"]
    mon, threat = h.monster_tables("all", 4)
    assert rec.take() == ["rg_dev_free", "rg_dev_alloc", "rg_monsters", "rg_dev_read"]
    obj, count = h.object_tables("stairs+gold+door", False, False, 8)
    assert rec.take() == ["rg_dev_free", "rg_dev_alloc", "rg_objects", "rg_dev_read"]
    again = (h.action_mask(), h.path_keys("stairs"), h.route_keys("stairs", "frontier", False, True), h.monster_tables("all", 4),
             h.object_tables("stairs+gold+door", False, False, 8))
    assert rec.take() == ["rg_action_mask", "rg_dev_read", "rg_path", "rg_dev_read", "rg_route", "rg_dev_read", "rg_monsters", "rg_dev_read", "rg_objects", "rg_dev_read"]
    first = (mask, (keys, dist), (rkeys, rdist, rtier), (mon, threat), (obj, count))
    for a, b in zip(first, again):
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert x.dtype == y.dtype and np.array_equal(x, y)

    def host(t):
        return t.cpu().numpy()
    assert mask.dtype == np.bool_ and mask.shape == (N, 11) and np.array_equal(mask, host(env.legal_mask()))
    k2, d2, _ = env.path("stairs")
    assert keys.dtype == np.uint8 and dist.dtype == np.int32 and np.array_equal(keys, host(k2)) and np.array_equal(dist, host(d2))
    k3, d3, t3 = env.route("stairs", "frontier", False, True)
    assert rtier.dtype == np.uint8 and np.array_equal(rkeys, host(k3)) and np.array_equal(rdist, host(d3)) and np.array_equal(rtier, host(t3))
    m2, th2 = env.monster_table("all", 4)
    assert mon.dtype == np.int16 and mon.shape == (N, 4, 8) and threat.shape == (N, 4) and np.array_equal(mon, host(m2)) and np.array_equal(threat, host(th2))
    o2, c2 = env.object_table("stairs+gold+door", False, False, 8)
    assert obj.dtype == np.int16 and obj.shape == (N, 8, 8) and count.shape == (N, 4) and np.array_equal(obj, host(o2)) and np.array_equal(count, host(c2))
    rec.take()
    env.close()
    log = rec.take()
    assert log.count("rg_dev_free") == 1 and log.count("rg_dev_alloc") == 0 and log.index("rg_dev_free") < log.index("rg_destroy")
