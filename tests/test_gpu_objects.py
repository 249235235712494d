"""Object tables on the GPU (rogue-gym_amd/csrc/rg_objects.hip k_objects): the device against the host entry fed from rg_debug_fetch and against the numpy
rule on the CPU oracle's own state after every step of a lock-step run, constructed grids loaded as records, three screen sizes on one handle, no side
effects on the stepper, the Python surface on every path that refreshes `obs`, the value forms and the refusals.  The rule's numpy restatement is
tests/object_util.py's."""
import ctypes as C
import json

import numpy as np
import pytest

import grid_util as gu
import mask_util as mu
import object_util as ou
from grid_util import C_DRAWN, C_GOLD, FLOOR, STAIR
from object_util import DOOR, FRONTIER, GOLD, STAIRS
from parity_util import HipBatch, make_oracles
from route_util import KNOWN, SECRETS

pytestmark = pytest.mark.gpu

CAPS = (1, 5, 8, 32)
SGD = STAIRS | GOLD | DOOR


@pytest.fixture(scope="module")
def lib():
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def fetch(hd, dims=None):
    """(grids, players, dead) of every env from rg_debug_fetch and the flag words."""
    from rogue_gym_python._rogue_gym import RgDebugState
    flags = np.empty(hd.n, np.uint32)
    hd.check(hd.L.rg_fetch_states(hd.h, None, None, None, flags.ctypes.data))
    grids, players = [], []
    for i in range(hd.n):
        h, w = (hd.height, hd.width) if dims is None else dims[i]
        st, cells = RgDebugState(), np.empty((h, w), np.uint16)
        hd.check(hd.L.rg_debug_fetch(hd.h, i, C.byref(st), cells.ctypes.data))
        grids.append(cells)
        players.append((int(st.px), int(st.py)))
    return grids, players, ((flags & 2) != 0).astype(np.int32)


def check_against_host(lib, hd, state, combos, where, stats=None):
    """Device == host entry for every env and every (kinds, mode, cap) of combos; both outputs, the sentinel slack untouched (objects_call)."""
    grids, players, dead = state
    for kinds, mode, cap in combos:
        tb, cnt = ou.objects_call(hd, kinds, mode, cap)
        hb, hc = ou.host_tables(lib, grids, players, dead, kinds, mode, cap)
        if not (np.array_equal(cnt, hc) and np.array_equal(tb, hb)):
            i = int(np.flatnonzero((cnt != hc).any(1) | (tb != hb).any((1, 2)))[0])
            raise AssertionError("%s kinds %d mode %d cap %d env %d player %s: device counts %s table\n%s\nhost entry counts %s table\n%s"
                                 % (where, kinds, mode, cap, i, players[i], cnt[i], tb[i], hc[i], hb[i]))
        if stats is not None:
            listed = (tb[:, :, 0] != 0).sum(1)
            stats["listed"] = stats.get("listed", 0) + int(listed.sum())
            stats["full"] = stats.get("full", 0) + (int((tb[:, -1, 0] != 0).sum()) if cap > 1 else 0)
            stats["max_walk"] = max(stats.get("max_walk", 0), int(tb[:, :, 3].max()))
            stats["unlisted"] = stats.get("unlisted", 0) + (int(((hc.sum(1) > listed) & (tb[:, -1, 0] == 0)).sum()) if cap == 32 else 0)


def step_combos(t):
    """The (kinds, mode, cap) asked after step t: every mode in every step, each walking through its (kind set, cap) pairs -- 16 of them, 24 under KNOWN --
    one a step, so every pair comes up several times in a run."""
    out = []
    for j, mode in enumerate(ou.MODES):
        pairs = [(kinds, cap) for kinds in ou.kind_sets(mode) for cap in CAPS]
        out.append(pairs[(5 * t + 7 * j) % len(pairs)][:1] + (mode,) + pairs[(5 * t + 7 * j) % len(pairs)][1:])
    return out


RUNS = {   # name -> (config builder, envs, first seed, steps); enemies 0..11, auto-reset, max_steps 60
    "mini": (lambda g: dict(g["configs"]["mini"], enemies=mu.ENEMIES), 135, 9000, 80),      # WN 1, GS 16: four envs a wave, a partial last wave
    "80x24": (lambda g: dict(mu.DEFAULT_SIZE), 71, 9100, 60),                                # WN 3, GS 32
    "97x33": (lambda g: dict(gu.shape_config("97x33"), enemies=mu.ENEMIES), 71, 9200, 60),   # WN 5, GS 64, cell-by-cell loads
}
# Half of what the CPU oracle gives with exactly these runs -- rows listed over all calls, tables filled to the last row, the longest walk listed, cap-32 tables
# that list less than the counts say exists: mini 101 902 / 3 821 / 70 / 630, 80x24 62 466 / 2 866 / 192 / 494, 97x33 63 463 / 3 137 / 284 / 545
FLOORS = {"mini": dict(listed=50951, full=1910, max_walk=35, unlisted=315), "80x24": dict(listed=31233, full=1433, max_walk=96, unlisted=247),
          "97x33": dict(listed=31731, full=1568, max_walk=142, unlisted=272)}


@pytest.mark.parametrize("name", list(RUNS))
def test_lock_step_with_the_oracle(goldens, lib, name):
    """After every step: device == host entry on rg_debug_fetch's grid for every env (every mode, the caps 1, 5, 8, 32 and the kind sets in turn), and
    == the numpy rule on the CPU oracle's own state for an eighth of the envs, another one every step."""
    build, n, seed0, T = RUNS[name]
    cfg = build(goldens)
    seeds = [seed0 + i for i in range(n)]
    table = mu.key_table(1, T, n)
    hip, oracles = HipBatch(cfg, seeds, max_steps=60), make_oracles(cfg, seeds, max_steps=60)
    stats = {}
    for t in range(T + 1):
        check_against_host(lib, hip.h, fetch(hip.h), step_combos(t), "%s t=%d" % (name, t), stats)
        mode = ou.MODES[t % 4]
        kinds = ou.kind_sets(mode)[-1]
        tb, cnt = ou.objects_call(hip.h, kinds, mode, 32)
        for i in range(t % 8, n, 8):
            o = oracles[i]
            sc = o.scalars()
            ob = ou.Objects(mu.cell_words(*o.grid()), sc["px"], sc["py"], int(o.flags()["dead"]), mode)
            assert np.array_equal(tb[i], ou.capped(ob.rows(kinds), 32)) and np.array_equal(cnt[i], ob.count(kinds)), (name, t, i, mode, tb[i], ob.rows(kinds))
        if t < T:
            hip.step(table[t])
            mu.step_oracles(oracles, table[t], True)
    hip.sync()
    print(name, stats)
    assert all(stats[k] >= v for k, v in FLOORS[name].items()), (stats, FLOORS[name])
    hip.h.close()


# ---------------------------------------------------------------------------------------------
# constructed grids, loaded as records
# ---------------------------------------------------------------------------------------------
SHAPES = ("32x16", "33x17", "64x32", "96x32", "104x20", "128x16", "160x48")
KNOWN_FLOOR = FLOOR | C_DRAWN


def shape_envs(name):
    """(grids, players, dead, names) of one shape.  The env order puts a grid without any object beside one with many in one wave (H <= 32), in both orders."""
    w, h = gu.SHAPES[name][:2]
    rng = np.random.RandomState(4000 + 3 * w + h)
    envs = []
    snake = gu.serpentine(w, h) | C_DRAWN                                  # one walk through every corridor: the far end is thousands of moves away
    last = h - 1 - (h - 1) % 2
    far = (w - 1 if (last // 2) % 2 == 0 else 0, last)
    snake[far[1], far[0]] = STAIR | C_DRAWN
    snake[0, w // 2] |= C_GOLD
    envs.append(("snake far stairs", snake, (0, 0)))                       # fewer objects than cap 5: the search runs to the far end
    bare = np.full((h, w), KNOWN_FLOOR, np.uint16)
    envs.append(("bare", bare, (w // 2, h // 2)))                          # no object at all beside ...
    golden = bare | C_GOLD
    envs.append(("all gold", golden, (w // 2, h // 2)))                    # ... far more than cap in every level, spread over many rows
    envs.append(("bare again", bare, (0, h - 1)))
    seams = np.full((h, w), KNOWN_FLOOR, np.uint16)                        # objects at bits 0, 31, 32, 63, 64, 95, 96 and W - 1, in rows 0, H - 1 and a middle one
    for y in (0, h // 2, h - 1):
        for k, x in enumerate(sorted({x for x in (0, 31, 32, 63, 64, 95, 96, w - 1) if x < w})):
            seams[y, x] = ((FLOOR | C_GOLD), STAIR, gu.DOOR)[(k + y) % 3] | C_DRAWN
    envs.append(("seams", seams, (w // 3, h // 3)))
    envs.append(("seams from a corner", seams, (w - 1, h - 1)))
    packed = bare.copy()                                                   # more than cap reached in one level, packed into one row: 2 (h // 2) + 1 cells of row 0 at once
    packed[0, :] |= C_GOLD
    envs.append(("packed row", packed, (w // 2, h // 2)))
    snake_gold = snake.copy()                                              # cap reached early on the long walk: an early exit beside a wave that runs on
    snake_gold[0, 1:w:2] |= C_GOLD
    envs.append(("snake early exit", snake_gold, (0, 0)))
    for cap in CAPS:                                                       # the cap-th object is the one in the last row of the group, a farther one behind it
        if h - 1 - cap >= 0:
            col = bare.copy()
            col[h - cap:, w // 2] |= C_GOLD
            col[0, 0] = STAIR | C_DRAWN
            envs.append(("column cap %d" % cap, col, (w // 2, h - 1 - cap)))
    half = gu.serpentine(w, h) | C_DRAWN                                   # the far half not on the map, objects in both halves
    half[h // 2:, :] &= ~np.uint16(C_DRAWN)
    half[last, w // 2] = STAIR
    half[0, w - 1] = gu.DOOR | C_DRAWN
    envs.append(("half known", half, (0, 0)))
    from test_gpu_route_grids import holes_at_seams, snake_with_doors
    holes = holes_at_seams(w, h)
    holes[h - 1, 0] = STAIR | C_DRAWN
    envs.append(("holes", holes, (0, 0)))
    doors, far_d = snake_with_doors(w, h, False)
    doors[0, w // 2 + 1] |= C_GOLD
    envs.append(("snake with secrets", doors, far_d))
    envs.append(("all gold from a corner", golden, (w - 1, 0)))
    envs.append(("bare at the end", bare, (w - 1, h - 1)))
    unseen = np.full((h, w), gu.WALLX | C_DRAWN, np.uint16)                # tests/test_objects_host.py's hand-answered grid in the top left corner: a drawn
    unseen[1, :7] = gu.PASSAGE | C_DRAWN                                   # passage with gold on it, a door and the stairs beyond that are not on the map
    unseen[1, 2] |= C_GOLD
    unseen[1, 4], unseen[1, 6] = gu.DOOR, STAIR
    envs.append(("unseen objects", unseen, (0, 1)))
    for p in (0.55, 0.75, 0.9):
        envs.append(("random %.2f" % p, gu.random_words(w, h, rng, p), None))
        envs.append(("random %.2f again" % p, gu.random_words(w, h, rng, p), None))
    grids, players, names = [], [], []
    for nm, g, p in envs:
        if p is None:
            ys, xs = np.nonzero(~np.isin(g & 7, (gu.WALLX, gu.WALLY, gu.NONE)))
            i = rng.randint(0, len(ys))
            p = (int(xs[i]), int(ys[i]))
        grids.append(g)
        players.append(p)
        names.append(nm)
    dead = np.zeros(len(grids), np.uint32)
    dead[[5, len(grids) - 2]] = 1
    return np.stack(grids), players, dead, names


@pytest.mark.parametrize("name", SHAPES)
def test_constructed_grids(lib, name):
    w, h = gu.SHAPES[name][:2]
    grids, players, dead, names = shape_envs(name)
    n = len(grids)
    hip = HipBatch(gu.shape_config(name), [3000 + i for i in range(n)], max_steps=1000, auto_reset=True)
    gu.inject(hip, grids, players, dead, check_every=4)
    hd = hip.h
    env = {nm: i for i, nm in enumerate(names)}
    state = (grids, players, dead)
    combos = [(kinds, mode, cap) for mode in ou.MODES for kinds in (ou.kind_sets(mode)[-1], GOLD) for cap in CAPS]
    check_against_host(lib, hd, state, combos, name)
    check_against_host(lib, hd, state, [(STAIRS, 0, 8), (DOOR, KNOWN, 5), (FRONTIER, KNOWN | SECRETS, 32)], name)
    # ... and what the grids were built for, by name, with the numpy rule beside the device
    tb, cnt = ou.objects_call(hd, SGD, 0, 5)
    for i in range(n):
        ob = ou.Objects(grids[i], players[i][0], players[i][1], int(dead[i]), 0)
        assert np.array_equal(tb[i], ou.capped(ob.rows(SGD), 5)) and np.array_equal(cnt[i], ob.count(SGD)), (name, names[i])
    i = env["snake far stairs"]
    assert tb[i][:2, 0].tolist() == [GOLD, STAIRS] and tb[i][1, 3] >= (w - 1) * ((h + 1) // 2) and not tb[i][2:].any(), (name, tb[i])   # the whole walk
    assert not tb[env["bare"]].any() and not cnt[env["bare"]].any() and not tb[env["bare again"]].any()
    assert (tb[env["all gold"]][:, 0] == GOLD).all() and (tb[env["all gold"]][:, 3] == 1).all() and cnt[env["all gold"]].tolist() == [0, w * h - 1, 0, 0]
    i = env["packed row"]
    assert (tb[i][:, 3] == h // 2).all() and (tb[i][:, 5] == 0).all() and tb[i][0, 4] == w // 2 - h // 2 and (np.diff(tb[i][:, 4]) == 1).all(), (name, tb[i])
    assert tb[env["snake early exit"]][:, 3].tolist() == [1, 3, 5, 7, 9]
    assert not tb[5].any() and not cnt[5].any() and dead[5] == 1
    for cap in CAPS:
        if "column cap %d" % cap in env:
            i = env["column cap %d" % cap]
            t2, c2 = ou.objects_call(hd, SGD, 0, cap)
            assert t2[i][-1].tolist() == [GOLD, 0, cap, cap, w // 2, h - 1, cap, 0] and c2[i].tolist() == [1, cap, 0, 0], (name, cap, t2[i])
    seam_cells = {(int(r[4]), int(r[5])) for r in ou.objects_call(hd, SGD, KNOWN, 32)[0][env["seams"]] if r[0]}
    assert {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)} <= seam_cells and all((x, y) in seam_cells for x in (31, 32, 63, 64, 95, 96) if x < w for y in (0, h - 1))
    half_known, half_all = ou.objects_call(hd, SGD | FRONTIER, KNOWN, 32)[0][env["half known"]], ou.objects_call(hd, SGD, 0, 32)[0][env["half known"]]
    assert STAIRS in half_all[:, 0] and STAIRS not in half_known[:, 0] and FRONTIER in half_known[:, 0] and (half_known[:, 0] & DOOR).any()
    i = env["unseen objects"]                                              # by hand: on the player's map only the gold counts; without KNOWN all three do
    t2, c2 = ou.objects_call(hd, SGD, KNOWN, 5)
    assert c2[i].tolist() == [0, 1, 0, 0] and t2[i][0].tolist() == [GOLD, 2, 0, 2, 2, 1, 2, 0] and not t2[i][1:].any(), (name, t2[i], c2[i])
    assert cnt[i].tolist() == [1, 1, 1, 0] and [r[[0, 3, 4]].tolist() for r in tb[i][:3]] == [[GOLD, 2, 2], [DOOR, 4, 4], [STAIRS, 6, 6]], (name, tb[i])
    i = env["snake with secrets"]                                          # only with SECRETS does the walk pass the first door
    plain, through = ou.objects_call(hd, SGD, 0, 8)[0][i], ou.objects_call(hd, SGD, SECRETS, 8)[0][i]
    assert not (plain[:, 0] & STAIRS).any() and (through[:, 0] & STAIRS).any() and through[:, 3].max() >= (w // 2) * (h // 2), (name, plain, through)
    hd.close()


# ---------------------------------------------------------------------------------------------
# mixed sizes, side effects, the Python surface
# ---------------------------------------------------------------------------------------------
def seeded(cfg, seeds):
    return [dict(cfg, seed=int(s)) for s in seeds]


def _mini(goldens):
    return dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)


def test_three_screen_sizes_on_one_handle(goldens, lib):
    """96 envs cycling mini / 80 x 24 / 48 x 20: three config groups, every group's rows written at the caller's env index (ext)."""
    from rogue_gym_python import _rogue_gym as inner
    shapes = [_mini(goldens), dict(mu.DEFAULT_SIZE), {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": mu.ENEMIES}]
    n, steps = 96, 40
    cfgs = [dict(shapes[i % 3], seed=6000 + i) for i in range(n)]
    dims = [(c["height"], c["width"]) for c in cfgs]
    hd = inner._Handle([json.dumps(c) for c in cfgs], 60, auto_reset=True)
    assert hd.mixed_sizes
    table = mu.key_table(1, steps, n)
    stats = {}
    for t in range(steps + 1):
        if t % 4 == 0:
            check_against_host(lib, hd, fetch(hd, dims), step_combos(t // 4), "mixed t=%d" % t, stats)
        if t < steps:
            hd.check(hd.L.rg_step(hd.h, np.ascontiguousarray(table[t]).ctypes.data, 0))
    hd.check(hd.L.rg_sync(hd.h))
    print(stats)
    assert stats["listed"] >= 5000, stats
    hd.close()


def test_config_groups_of_one_size(goldens, lib):
    """Two configs of one screen size (with and without enemies) in one batch: a handle with config groups whose envs interleave."""
    from rogue_gym_python import _rogue_gym as inner
    a, b = _mini(goldens), dict(goldens["configs"]["mini"], enemies={"enemies": []})
    cfgs = [dict((a, b, b)[i % 3], seed=6500 + i) for i in range(50)]
    hd = inner._Handle([json.dumps(c) for c in cfgs], 60, auto_reset=True)
    table = mu.key_table(2, 24, 50)
    for t in range(25):
        if t % 6 == 0:
            check_against_host(lib, hd, fetch(hd), step_combos(t // 6), "groups t=%d" % t)
        if t < 24:
            hd.check(hd.L.rg_step(hd.h, np.ascontiguousarray(table[t]).ctypes.data, 0))
    hd.close()


def test_twin_handles_no_side_effects(goldens):
    """One env with objects="known" and all four kinds, one without, same seeds and keys: observations, rewards, done flags, flag words, status rows, screens
    and whole state records (RNG words included) stay equal, bit for bit, over 60 steps."""
    import torch
    from rogue_gym.envs import HipVecRogueEnv
    cfg, seeds = _mini(goldens), [9000 + i for i in range(135)]
    a = HipVecRogueEnv(seeded(cfg, seeds), max_steps=60)
    b = HipVecRogueEnv(seeded(cfg, seeds), max_steps=60, objects="known", object_kinds="stairs+gold+door+frontier", object_cap=32, object_secrets=True)
    assert a.objects is None and a.object_count is None and a._refresh == [] and b.objects.shape == (135, 32, 8) and b.object_count.shape == (135, 4)
    keys = torch.as_tensor(mu.key_table(1, 60, 135), device=a.device)
    for t in range(60):
        a.step_keys(keys[t])
        b.step_keys(keys[t])
        b.object_table("stairs+gold", False, False, 5)
        for k in ("obs", "reward", "done", "flags", "status"):
            x, y = getattr(a, k), getattr(b, k)
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.float32 else x, y.view(torch.uint8) if y.dtype == torch.float32 else y), (t, k)
        if t % 10 == 9:
            assert torch.equal(a.screen, b.screen), t
            assert torch.equal(a.save_state(), b.save_state()), t
    a.check_errors()
    b.check_errors()
    assert int((b.objects[:, 0, 0] != 0).sum()) > 0
    a.close()
    b.close()


def test_python_surface_on_every_refresh_path(goldens, lib):
    """env.objects / env.object_count equal a fresh object_table() after reset, reset_envs, step, step_keys, load_state and clone_state, and on
    HipVecFirstFloor; the kept tensors are what the host entry gives on rg_debug_fetch's grids."""
    import torch
    from rogue_gym.envs import OBJECT_COLS, HipVecFirstFloor, HipVecRogueEnv
    from rogue_gym_python import _rogue_gym as inner
    cfg, seeds = _mini(goldens), [9000 + i for i in range(40)]
    table = mu.key_table(1, 30, 40)

    def current(env, where, deep=False):
        kinds, known, secrets, cap = env._asked
        tb, cnt = env.object_table(kinds, known, secrets, cap)
        assert torch.equal(env.objects, tb) and torch.equal(env.object_count, cnt), where
        if deep:
            grids, players, dead = fetch(env._h)
            kw, mode, _ = inner._object_args(kinds, known, secrets, cap)
            t, c = env.objects.cpu().numpy(), env.object_count.cpu().numpy()
            for i in range(40):
                hb, hc = ou.host(lib, grids[i], players[i][0], players[i][1], int(dead[i]), kw, mode, cap)
                assert np.array_equal(t[i], hb) and np.array_equal(c[i], hc), (where, i)

    for cls, objects, kinds, cap, secrets in ((HipVecRogueEnv, "known", "stairs+gold+door+frontier", 8, False), (HipVecRogueEnv, "all", "stairs+gold+door", 5, True),
                                              (HipVecFirstFloor, "known", "gold+frontier", 32, True)):
        env = cls(seeded(cfg, seeds), max_steps=60, objects=objects, object_kinds=kinds, object_cap=cap, object_secrets=secrets)
        env._asked = (kinds, objects == "known", secrets, cap)
        assert env.objects.dtype == torch.int16 and env.objects.shape == (40, cap, 8) and env.object_count.dtype == torch.int32 and len(OBJECT_COLS) == 8
        current(env, "constructor", deep=True)
        keys = torch.as_tensor(table, device=env.device)
        for t in range(12):
            env.step_keys(keys[t])
            current(env, "step_keys %d" % t, deep=t == 11)
        env.step(torch.zeros(40, dtype=torch.int64, device=env.device))
        current(env, "step")
        saved = env.save_state()
        for t in range(12, 20):
            env.step_keys(keys[t])
        env.reset_envs(env_ids=[1, 5, 39])
        current(env, "reset_envs ids", deep=True)
        env.reset_envs(mask=torch.arange(40, device=env.device) % 3 == 0)
        current(env, "reset_envs mask")
        env.load_state(saved)
        current(env, "load_state", deep=True)
        env.clone_state([3] * 10, list(range(10, 20)))
        current(env, "clone_state")
        assert torch.equal(env.objects[10:20], env.objects[3:4].expand(10, -1, -1)) and torch.equal(env.object_count[10], env.object_count[3])
        env.reset()
        current(env, "reset", deep=True)
        env.check_errors()
        env.close()
    plain = HipVecRogueEnv(seeded(cfg, seeds[:2]))
    assert plain.objects is None and plain.object_count is None
    assert plain.object_table("stairs", cap=1)[0].shape == (2, 1, 8)       # the explicit call works either way
    plain.close()
    for kw in (dict(objects="every"), dict(objects="all", object_cap=33), dict(objects="all", object_kinds="stairs+frontier"), dict(objects="known", object_kinds="amulet")):
        with pytest.raises(ValueError):
            HipVecRogueEnv(seeded(cfg, seeds[:2]), **kw)


def test_a_row_is_a_target_for_route(goldens):
    """The option loop of examples/quickstart.py: a listed row's (y, x) handed to route(goal=None, cells=...) is answered with the row's walk."""
    import torch
    from rogue_gym.envs import HipVecRogueEnv
    env = HipVecRogueEnv(seeded(_mini(goldens), range(9000, 9032)), max_steps=60, objects="known", object_kinds="stairs+gold+door+frontier")
    keys = torch.as_tensor(mu.key_table(1, 20, 32), device=env.device)
    for t in range(20):
        rows = env.objects[:, 0].to(torch.int32)
        key, dist, _ = env.route(goal=None, known=True, cells=rows[:, [5, 4]].contiguous())
        listed = rows[:, 0] != 0
        assert torch.equal(dist[listed], rows[listed, 3]), t
        assert bool(listed.any())
        env.step_keys(torch.where(listed, key, keys[t]))
    env.close()


def test_value_forms(goldens, lib):
    """ParallelRogueEnv.object_tables against the device tensors of a HipVecRogueEnv on the same seeds and keys; RogueEnv.objects against the host entry on
    its own game's rg_debug_fetch."""
    import torch
    from rogue_gym.envs import HipVecRogueEnv, ParallelRogueEnv, RogueEnv
    cfg, seeds = _mini(goldens), [9000 + i for i in range(12)]
    table = mu.key_table(1, 40, 12)
    dev = HipVecRogueEnv(seeded(cfg, seeds), max_steps=60)
    par = ParallelRogueEnv(config_dicts=seeded(cfg, seeds), max_steps=60)
    one = RogueEnv(config_dict=dict(cfg, seed=seeds[0]), max_steps=10 ** 6)
    keys = torch.as_tensor(table, device=dev.device)
    seen = 0
    for t in range(40):
        dev.step_keys(keys[t])
        par.step("".join(chr(k) for k in table[t]))
        for args in (("stairs+gold+door", False, False, 8), ("gold+frontier", True, True, 32), ("door", True, False, 1)):
            tb, cnt = dev.object_table(*args)
            ptb, pc = par.object_tables(*args)
            assert ptb.dtype == np.int16 and ptb.shape == (12, args[3], 8) and pc.dtype == np.int32 and pc.shape == (12, 4)
            assert np.array_equal(tb.cpu().numpy(), ptb) and np.array_equal(cnt.cpu().numpy(), pc), (t, args)
            seen += int((ptb[:, 0, 0] != 0).sum())
    assert seen > 50
    listed = 0
    for t in range(25):
        one.step(chr(table[t][0]))
        grids, players, dead = fetch(one.game._h)
        for kinds, kw, known, mode in (("stairs+gold+door", SGD, False, 0), ("stairs+frontier", STAIRS | FRONTIER, True, KNOWN)):
            tb, cnt = one.objects(kinds, known, False, 8)
            hb, hc = ou.host(lib, grids[0], players[0][0], players[0][1], int(dead[0]), kw, mode, 8)
            assert tb.shape == (8, 8) and cnt.shape == (4,) and np.array_equal(tb, hb) and np.array_equal(cnt, hc), (t, kinds)
            listed += int(tb[0, 0] != 0)
    assert listed > 0
    tb, cnt = one.objects()
    assert tb.shape == (8, 8) and tb.dtype == np.int16 and cnt.dtype == np.int32
    with pytest.raises(ValueError):
        one.objects("gold", cap=0)
    dev.close()
    par.close()


def test_refusals_leave_the_buffers_untouched(goldens):
    import torch
    hip = HipBatch(_mini(goldens), [1, 2, 3], max_steps=60)
    hd, dev = hip.h, "cuda:%d" % hip.h.device
    tb = torch.full((3 + 8, 32, 8), int(ou.SENT16), dtype=torch.int16, device=dev)
    cn = torch.full((3 + 8, 4), int(ou.SENT32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    pt, pc = C.c_void_p(tb.data_ptr()), C.c_void_p(cn.data_ptr())
    for args, frag in (((0, 0, 8, pt, pc), "kinds"), ((16, 0, 8, pt, pc), "kinds"), ((1, 4, 8, pt, pc), "mode"), ((8, 0, 8, pt, pc), "RG_ROUTE_KNOWN"), ((9, 1, 8, pt, pc), "RG_ROUTE_KNOWN"),
                       ((1, 0, 0, pt, pc), "cap"), ((1, 0, 33, pt, pc), "cap"), ((1, 0, -1, pt, None), "cap"), ((1, 0, 8, None, None), "both NULL"),
                       ((1, 0, 8, C.c_void_p(tb.data_ptr() + 2), pc), "16-byte"), ((1, 0, 8, pt, C.c_void_p(cn.data_ptr() + 4)), "16-byte")):
        assert hd.L.rg_objects(hd.h, *args) != 0, args
        msg = hd.L.rg_last_error(hd.h).decode()
        assert msg.startswith("rg_objects:") and frag in msg, msg
    hd.check(hd.L.rg_sync(hd.h))
    torch.cuda.synchronize()
    assert bool((tb == int(ou.SENT16)).all()) and bool((cn == int(ou.SENT32)).all())
    hd.check(hd.L.rg_objects(hd.h, 7, 0, 99, None, pc))   # cap is only read with a table
    torch.cuda.synchronize()
    assert bool((cn[:3] >= 0).all()) and bool((cn[3:] == int(ou.SENT32)).all()) and bool((tb == int(ou.SENT16)).all())
    hd.close()
