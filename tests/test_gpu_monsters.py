"""Monster tables and threat words on the GPU (rogue-gym_amd/csrc/rg_monsters.hip k_monsters): the device against the host entry fed from rg_debug_fetch
after every step of a lock-step run with the CPU oracle, three screen sizes on one handle, constructed monster tables loaded as records, no side effects
on the stepper, the Python surface on every path that refreshes `obs`, the value forms and the refusals.  The rule's numpy restatement is
tests/monster_util.py's."""
import ctypes as C
import json

import numpy as np
import pytest

import grid_util as gu
import mask_util as mu
import monster_util as mo
from parity_util import HipBatch, make_oracles

pytestmark = pytest.mark.gpu

CAPS = (1, 4, 5, 8, 16)   # one cap inside each kernel instance (4, 8, 16) and the edges
SLACK = 8                 # envs of sentinel behind the last env of every output buffer


@pytest.fixture(scope="module")
def lib():
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def dev_call(hd, mode, cap, table=True, threat=True):
    """rg_monsters into sentinel-filled buffers with SLACK envs behind the last -> (table i16 [n][cap][8], threat i32 [n][4]); the slack must be untouched."""
    import torch
    dev, n = "cuda:%d" % hd.device, hd.n
    tb = torch.full((n + SLACK, max(cap, 1), mo.COLS), mo.SENTINEL16, dtype=torch.int16, device=dev) if table else None
    th = torch.full((n + SLACK, 4), mo.SENTINEL32, dtype=torch.int32, device=dev) if threat else None
    torch.cuda.synchronize()
    hd.check(hd.L.rg_monsters(hd.h, mode, cap, None if tb is None else C.c_void_p(tb.data_ptr()), None if th is None else C.c_void_p(th.data_ptr())))
    torch.cuda.synchronize()
    out = []
    for t, s in ((tb, mo.SENTINEL16), (th, mo.SENTINEL32)):
        if t is None:
            out.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[n:] == s).all(), "the slack behind the last env was written"
        out.append(a[:n])
    return out


def feeds_of(hd, rooms, dims=None):
    """[Feed] of every env from rg_debug_fetch and the flag words; rooms = (rnx, rny) or one pair per env."""
    from rogue_gym_python._rogue_gym import RgDebugState
    flags = np.empty(hd.n, np.uint32)
    hd.check(hd.L.rg_fetch_states(hd.h, None, None, None, flags.ctypes.data))
    out = []
    for i in range(hd.n):
        h, w = (hd.height, hd.width) if dims is None else dims[i]
        st, cells = RgDebugState(), np.empty((h, w), np.uint16)
        hd.check(hd.L.rg_debug_fetch(hd.h, i, C.byref(st), cells.ctypes.data))
        rnx, rny = rooms if dims is None else rooms[i]
        out.append(mo.feed_of_debug(st, cells, int((flags[i] & 2) != 0), rnx, rny))
    return out


def check_against_host(lib, hd, feeds, where, caps=CAPS, stats=None):
    """Device == host entry for every env, mode and cap.  The slot column is the device's own table slot (the host entry answers the index in the arrays it
    was given): compared apart -- distinct, inside the room count, 0 on empty rows."""
    for name, mode in mo.MODES:
        for cap in caps:
            tb, th = dev_call(hd, mode, cap)
            for i, f in enumerate(feeds):
                hb, ht = mo.host_call(lib, f, mode, cap)
                tag = "%s %s cap %d env %d player (%d, %d)" % (where, name, cap, i, f.px, f.py)
                assert np.array_equal(th[i], ht), "%s: threat device %s, host entry %s" % (tag, th[i], ht)
                assert np.array_equal(tb[i][:, :7], hb[:, :7]), "%s: device\n%s\nhost entry\n%s" % (tag, tb[i], hb)
                used = tb[i][tb[i][:, 0] != 0, 7]
                assert ((used >= 0) & (used < f.rnx * f.rny)).all() and not tb[i][tb[i][:, 0] == 0].any(), (tag, tb[i])
                if mode == mo.SHOWN:
                    assert not tb[i][:, 5:].any(), tag
                else:
                    assert len(set(used.tolist())) == len(used), (tag, tb[i])
                if stats is not None and cap == 16:
                    stats[name + "_rows"] = stats.get(name + "_rows", 0) + int((tb[i][:, 0] != 0).any())
                    stats[name + "_max"] = max(stats.get(name + "_max", 0), int((tb[i][:, 0] != 0).sum()))
                    stats["adjacent"] = stats.get("adjacent", 0) + int(mode == mo.SHOWN and th[i][0] > 0)


def check_slots(hip, where):
    """ALL mode, cap 16: column 7 names the slot whose monster word holds the row's position, active flag and hit points (the words read from state records)."""
    pos, w0, hp = mo.record_monster_words(hip)
    tb, _ = dev_call(hip.h, mo.ALL, 16)
    seen = 0
    for i in range(hip.n):
        px, py = int(pos[i]) >> 8, int(pos[i]) & 0xFF
        for r in tb[i]:
            if r[0]:
                w = int(w0[i, r[7]])
                assert (w >> 24) & mo.MF_ALIVE and ((w >> 8) & 0xFF, w & 0xFF) == (px + int(r[1]), py + int(r[2])), (where, i, r, hex(w))
                assert int(r[5]) == int(bool((w >> 24) & mo.MF_ACTIVE)) and int(r[6]) == min(int(hp[i, r[7]]), 32767), (where, i, r, hex(w), hp[i, r[7]])
                seen += 1
    return seen


RUNS = {   # name -> (config builder, envs, first seed, steps); enemies 0..11, auto-reset, max_steps 60
    "mini": (lambda g: dict(g["configs"]["mini"], enemies=mu.ENEMIES), 135, 9000, 80),
    "80x24": (lambda g: dict(mu.DEFAULT_SIZE), 71, 9100, 60),
    "97x33": (lambda g: dict(gu.shape_config("97x33"), enemies=mu.ENEMIES), 71, 9200, 60),
}
# Half of what the CPU oracle gives with exactly these runs (rows of cap-16 tables that list a monster, per mode; rows with an adjacent shown monster),
# measured on the CPU: mini 5 311 / 10 830 / 3 927, 80x24 1 810 / 4 331 / 1 037, 97x33 2 435 / 4 331 / 1 010; up to 4, 9 and 9 monsters alive.
FLOORS = {"mini": dict(shown_rows=2655, all_rows=5415, adjacent=1963, all_max=4), "80x24": dict(shown_rows=905, all_rows=2165, adjacent=518, all_max=5),
          "97x33": dict(shown_rows=1217, all_rows=2165, adjacent=505, all_max=5)}


@pytest.mark.parametrize("name", list(RUNS))
def test_lock_step_with_the_oracle(goldens, lib, name):
    """After every step, every env: device == host entry on rg_debug_fetch's arrays (both modes, caps 1, 4, 5, 8, 16, sentinel slack untouched), and the
    SHOWN table == the numpy rule on the CPU oracle's own state -- the lock step.  135 and 71 envs leave the last wave partly empty."""
    build, n, seed0, T = RUNS[name]
    cfg = build(goldens)
    seeds = [seed0 + i for i in range(n)]
    table = mu.key_table(1, T, n)
    hip, oracles = HipBatch(cfg, seeds, max_steps=60), make_oracles(cfg, seeds, max_steps=60)
    rooms = mo.room_grid(cfg)
    stats, slots = {}, 0
    for t in range(T + 1):
        feeds = feeds_of(hip.h, rooms)
        check_against_host(lib, hip.h, feeds, "%s t=%d" % (name, t), stats=stats)
        if t % 20 == 0:
            slots += check_slots(hip, "%s t=%d" % (name, t))
        shown, th = dev_call(hip.h, mo.SHOWN, 16)
        full, _ = dev_call(hip.h, mo.ALL, 16)
        for i, o in enumerate(oracles):
            f = mo.feed_of_oracle(o, cfg)
            rows, threat, _ = mo.rule_list(f, mo.SHOWN)
            assert np.array_equal(shown[i], mo.capped(rows, 16)) and np.array_equal(th[i], threat), (name, t, i, shown[i], rows)
            assert np.array_equal(full[i][:, :7], mo.capped(mo.rule_list(f, mo.ALL)[0], 16)[:, :7]), (name, t, i)
        if t < T:
            hip.step(table[t])
            mu.step_oracles(oracles, table[t], True)
    hip.sync()
    print(name, stats, "slot columns checked:", slots)
    assert slots >= n
    fl = FLOORS[name]
    assert all(stats[k] >= v for k, v in fl.items()), (stats, fl)


def test_three_screen_sizes_on_one_handle(goldens, lib):
    """96 envs cycling mini / 80 x 24 / 48 x 20: three config groups, every group's rows written at the caller's env index (ext)."""
    from rogue_gym_python import _rogue_gym as inner
    shapes = [dict(goldens["configs"]["mini"], enemies=mu.ENEMIES), dict(mu.DEFAULT_SIZE),
              {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": mu.ENEMIES}]
    n, steps = 96, 40
    cfgs = [dict(shapes[i % 3], seed=6000 + i) for i in range(n)]
    dims = [(c["height"], c["width"]) for c in cfgs]
    rooms = [mo.room_grid(c) for c in cfgs]
    hd = inner._Handle([json.dumps(c) for c in cfgs], 60, auto_reset=True)
    assert hd.mixed_sizes
    table = mu.key_table(1, steps, n)
    stats = {}
    for t in range(steps + 1):
        if t % 4 == 0:
            check_against_host(lib, hd, feeds_of(hd, rooms, dims), "mixed t=%d" % t, caps=(1, 5, 16), stats=stats)
        if t < steps:
            hd.check(hd.L.rg_step(hd.h, np.ascontiguousarray(table[t]).ctypes.data, 0))
    hd.check(hd.L.rg_sync(hd.h))
    print(stats)
    assert stats["shown_rows"] >= 100 and stats["all_rows"] >= 500, stats
    hd.close()


# ---------------------------------------------------------------------------------------------
# constructed monster tables on a 160 x 48 grid with 8 x 6 = 48 rooms: the slot loop runs far past every cap
# ---------------------------------------------------------------------------------------------
BIG = {"width": 160, "height": 48, "dungeon": {"style": "rogue", "room_num_x": 8, "room_num_y": 6, "min_room_size": {"x": 4, "y": 4}}, "enemies": mu.ENEMIES}
CORNERS = ((0, 0), (159, 0), (0, 47), (159, 47))


def _ring(px, py, w, h, want):
    """The cells at one Chebyshev distance from the player, inside the grid: the least distance that has `want` of them."""
    for r in range(1, max(w, h)):
        cells = [(x, y) for y in range(max(0, py - r), min(h, py + r + 1)) for x in range(max(0, px - r), min(w, px + r + 1)) if max(abs(x - px), abs(y - py)) == r]
        if len(cells) >= want:
            return cells[:want]
    raise AssertionError("no ring")


def _constructed(n, nr, w, h):
    """Per env: a grid, a player, dead, monster words.  Patterns in turn: every slot alive on one ring around the player (equal cheb: d2 and position decide);
    only the last four slots alive; alive slots alternating; every slot alive at random cells.  Players: the four corners in turn, then random cells."""
    rng = np.random.RandomState(48)
    grids, players, dead = np.full((n, h, w), 0x41, np.uint16), [], np.zeros(n, np.uint32)
    w0, hp = np.zeros((n, nr), np.uint32), np.zeros((n, nr), np.int32)
    for i in range(n):
        px, py = CORNERS[i % 8] if i % 8 < 4 else (int(rng.randint(0, w)), int(rng.randint(0, h)))
        players.append((px, py))
        pattern = (i // 2) % 4
        if pattern == 0:
            cells = _ring(px, py, w, h, nr)
            rng.shuffle(cells)
        else:
            flat = rng.choice(w * h, size=nr, replace=False)
            cells = [(int(c % w), int(c // w)) for c in flat]
        for s, (x, y) in enumerate(cells):
            alive = pattern in (0, 3) or (pattern == 1 and s >= nr - 4) or (pattern == 2 and s % 2 == 1)
            w0[i, s] = mo.pack_w0(x, y, int(rng.randint(0, 12)), alive, bool(rng.randint(0, 2)))
            hp[i, s] = int(rng.choice([1, 7, 300, 32767, 32768, 40000])) if alive else 0
        if i % 16 == 5:                                           # slot 0 on the player's own cell: alive, never shown ('@' is drawn there)
            w0[i, 0], hp[i, 0] = mo.pack_w0(px, py, 3, True, True), 9
        dark = rng.rand(h, w) < 0.2
        grids[i][dark] = 0x01                                     # floor the player has not seen
        grids[i][rng.rand(h, w) < 0.1] |= mo.C_GOLD
        dead[i] = int(i % 16 == 11)
    return grids, players, dead, w0, hp


def test_constructed_tables_loaded_as_records(goldens, lib):
    """70 envs (a wave and a 6-lane tail) of 48 rooms each, read only: device == host entry == numpy rule with the injected slots, all eight columns."""
    n, nr, w, h = 70, 48, 160, 48
    hip = HipBatch(BIG, [7000 + i for i in range(n)], max_steps=1000)
    grids, players, dead, w0, hp = _constructed(n, nr, w, h)
    gu.inject(hip, grids, players, dead, check_every=9)
    mo.inject_monsters(hip, w0, hp)
    feeds = feeds_of(hip.h, (8, 6))
    for i, f in enumerate(feeds):   # read back by rg_debug_fetch: exactly the alive words, in position order
        alive = sorted(((int(v) >> 8) & 0xFF, int(v) & 0xFF, s) for s, v in enumerate(w0[i]) if (int(v) >> 24) & mo.MF_ALIVE)
        assert [(int(x), int(y)) for x, y in zip(f.mx, f.my)] == [a[:2] for a in alive], i
        assert [int(v) for v in f.mhp] == [int(hp[i, a[2]]) for a in alive] and (f.px, f.py, f.dead) == (players[i][0], players[i][1], int(dead[i]))
        f.slots = np.array([a[2] for a in alive], np.int64)
    check_against_host(lib, hip.h, feeds, "constructed")
    over, ties = 0, 0
    for name, mode in mo.MODES:
        for cap in CAPS:
            tb, th = dev_call(hip.h, mode, cap)
            for i, f in enumerate(feeds):
                rows, threat, _ = mo.rule_list(f, mode)
                assert np.array_equal(tb[i], mo.capped(rows, cap)), ("constructed", name, cap, i, tb[i], rows[:cap])
                assert np.array_equal(th[i], threat), ("constructed", name, cap, i)
                over += int(len(rows) > cap)
                ties += int(cap == 16 and len(rows) >= 16 and len(set(rows[:16, 3].tolist())) == 1)
    own = [i for i, f in enumerate(feeds) if not f.dead and any((int(x), int(y)) == (f.px, f.py) for x, y in zip(f.mx, f.my))]
    assert len(own) >= 4 and all(mo.rule_list(feeds[i], mo.ALL)[0][0, 3:5].tolist() == [0, 0] for i in own)      # a monster on the player's cell: listed by ALL, not shown
    assert sum(f.py == 0 and not f.dead for f in feeds) >= 4                                                      # players in row 0: in no area
    print("rows with more qualifiers than cap:", over, "; 16-row tables of one cheb:", ties)
    assert over >= 200 and ties >= 10
    assert (dead == 1).sum() >= 4 and all(not dev_call(hip.h, mo.ALL, 16)[0][i].any() for i in np.flatnonzero(dead))
    hip.h.close()


# the rooms of tests/test_monsters_host.py's hand-built cases (32 x 16, 2 x 2 areas of 16 x 8), room 2 Empty with a rect of x 4..8, y 10..12
EMPTY_RECTS = [2 | 2 << 8 | 10 << 16 | 7 << 24, 18 | 2 << 8 | 28 << 16 | 7 << 24, 4 | 10 << 8 | 9 << 16 | 13 << 24, 18 | 9 << 8 | 28 << 16 | 14 << 24]
EMPTY_METAS = [0, 0, 2, 0]


def _empty_room_cases(n):
    """Per env of 32 x 16 lit floor: a player in area 2 (x 0..15, y 8..14) and four monsters.  Envs 0 and 1 are test_monsters_host.py's two hand-answered feeds
    (the player inside the Empty room's rect, then outside it); the others put the player on a random cell of the area, one monster inside the rect, one on
    the rect's edge row or column just outside it, one anywhere in the area and one in another area."""
    rng = np.random.RandomState(77)
    players, w0 = [], np.zeros((n, 4), np.uint32)
    for i in range(n):
        if i == 0:
            p, mons = (5, 11), [(12, 13), (6, 11), (0, 8), (16, 11)]
        elif i == 1:
            p, mons = (12, 13), [(5, 11), (14, 9), (12, 7), (20, 12)]
        else:
            while True:
                p = (int(rng.randint(0, 16)), int(rng.randint(8, 15)))
                mons = [(int(rng.randint(4, 9)), int(rng.randint(10, 13))), ((3, 9)[rng.randint(2)], int(rng.randint(10, 13))) if rng.randint(2) else (int(rng.randint(4, 9)), (9, 13)[rng.randint(2)]),
                        (int(rng.randint(0, 16)), int(rng.randint(8, 15))), (int(rng.randint(16, 32)), int(rng.randint(1, 15)))]
                if len(set(mons + [p])) == 5:
                    break
        players.append(p)
        for s, (x, y) in enumerate(mons):
            w0[i, s] = mo.pack_w0(x, y, (i + s) % 12, True, bool((i + s) % 2))
    return players, w0


def test_an_empty_room_whose_rect_has_some_area_loaded_as_records(goldens, lib):
    """Floor::in_same_room answers true for an Empty room before it looks at the rect.  Play never shows it (an Empty room's rect holds no cell), so room words
    are loaded as records: 70 mini envs whose room 2 is Empty with a rect of 5 x 3 cells, the player and the monsters on either side of its edge inside one
    area.  Device == host entry == numpy rule, the two hand-answered feeds of tests/test_monsters_host.py among them, and the clause decides most envs."""
    n = 70
    hip = HipBatch(dict(goldens["configs"]["mini"], enemies=mu.ENEMIES), [7700 + i for i in range(n)], max_steps=1000)
    players, w0 = _empty_room_cases(n)
    gu.inject(hip, np.full((n, 16, 32), 0x41, np.uint16), players, np.zeros(n, np.uint32), check_every=9)
    mo.inject_monsters(hip, w0, np.full((n, 4), 9, np.int32), rect=np.tile(np.array(EMPTY_RECTS, np.uint32), (n, 1)), meta=np.tile(np.array(EMPTY_METAS, np.uint32), (n, 1)))
    feeds = feeds_of(hip.h, (2, 2))
    for i, f in enumerate(feeds):                               # read back by rg_debug_fetch: the injected rooms, player and monsters
        assert f.rect.tolist() == EMPTY_RECTS and [int(m) & 3 for m in f.meta] == EMPTY_METAS and (f.px, f.py) == players[i] and len(f.mx) == 4, i
    check_against_host(lib, hip.h, feeds, "empty room")
    tb, th = dev_call(hip.h, mo.SHOWN, 16)
    decided = 0
    for i, f in enumerate(feeds):
        rows, threat, _ = mo.rule_list(f, mo.SHOWN)
        assert np.array_equal(tb[i], mo.capped(rows, 16)) and np.array_equal(th[i], threat), ("empty room", i, tb[i], rows)
        f.meta = np.array([0, 0, 0, 0], np.int32)               # the same feed with room 2 read as a normal room: the rect would divide the area
        decided += int(len(mo.rule_list(f, mo.SHOWN)[0]) != len(rows))
        f.meta = np.array(EMPTY_METAS, np.int32)
    shown = lambda i: sorted(mo.listed(feeds[i], [r for r in tb[i] if r[4]]))  # noqa: E731
    assert shown(0) == [(0, 8), (6, 11), (12, 13)] and shown(1) == [(5, 11), (14, 9)]      # by hand, as in tests/test_monsters_host.py
    print("envs in which the Empty-room clause decides a row:", decided, "of", n)
    assert decided >= n // 2
    hip.h.close()


def seeded(cfg, seeds):
    return [dict(cfg, seed=int(s)) for s in seeds]


def _mini(goldens):
    return dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)


def test_twin_handles_no_side_effects(goldens):
    """One env with monsters="all", one without, same seeds and keys: observations, rewards, done flags, flag words, status rows, screens and whole state
    records stay equal, bit for bit, over 60 steps."""
    import torch
    from rogue_gym.envs import HipVecRogueEnv
    cfg, seeds = _mini(goldens), [9000 + i for i in range(135)]
    a, b = HipVecRogueEnv(seeded(cfg, seeds), max_steps=60), HipVecRogueEnv(seeded(cfg, seeds), max_steps=60, monsters="all", monster_cap=16)
    assert a.monsters is None and a.threat is None and b.monsters.shape == (135, 16, 8) and b.threat.shape == (135, 4)
    keys = torch.as_tensor(mu.key_table(1, 60, 135), device=a.device)
    for t in range(60):
        a.step_keys(keys[t])
        b.step_keys(keys[t])
        for k in ("obs", "reward", "done", "flags", "status"):
            x, y = getattr(a, k), getattr(b, k)
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.float32 else x, y.view(torch.uint8) if y.dtype == torch.float32 else y), (t, k)
        if t % 10 == 9:
            assert torch.equal(a.screen, b.screen), t
            assert torch.equal(a.save_state(), b.save_state()), t
    a.check_errors()
    b.check_errors()
    assert int((b.monsters[:, 0, 0] != 0).sum()) > 0
    a.close()
    b.close()


def _fresh(env, mode, cap):
    tb, th = env.monster_table(mode, cap)
    return tb, th


def test_python_surface_on_every_refresh_path(goldens, lib):
    """env.monsters / env.threat equal a fresh monster_table() after reset, reset_envs, step, step_keys, load_state and clone_state, and on HipVecFirstFloor;
    the kept tensors are what the host entry gives on rg_debug_fetch's arrays."""
    import torch
    from rogue_gym.envs import HipVecFirstFloor, HipVecRogueEnv
    cfg, seeds = _mini(goldens), [9000 + i for i in range(40)]
    table = mu.key_table(1, 30, 40)

    def current(env, where, deep=False):
        tb, th = _fresh(env, env._mode_name, env.monsters.shape[1])
        assert torch.equal(env.monsters, tb) and torch.equal(env.threat, th), where
        if deep:
            m, t = env.monsters.cpu().numpy(), env.threat.cpu().numpy()
            for i, f in enumerate(feeds_of(env._h, mo.room_grid(cfg))):
                hb, ht = mo.host_call(lib, f, dict(mo.MODES)[env._mode_name], m.shape[1])
                assert np.array_equal(m[i][:, :7], hb[:, :7]) and np.array_equal(t[i], ht), (where, i)

    for cls, mode, cap in ((HipVecRogueEnv, "shown", 4), (HipVecRogueEnv, "all", 5), (HipVecFirstFloor, "all", 16)):
        env = cls(seeded(cfg, seeds), max_steps=60, monsters=mode, monster_cap=cap)
        env._mode_name = mode
        assert env.monsters.dtype == torch.int16 and env.monsters.shape == (40, cap, 8) and env.threat.dtype == torch.int32 and len(env.MONSTER_COLS) == 8
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
        assert torch.equal(env.monsters[10:20], env.monsters[3:4].expand(10, -1, -1)) and torch.equal(env.threat[10], env.threat[3])
        env.reset()
        current(env, "reset", deep=True)
        env.check_errors()
        env.close()
    with pytest.raises(ValueError):
        HipVecRogueEnv(seeded(cfg, seeds[:2]), monsters="every")
    with pytest.raises(ValueError):
        HipVecRogueEnv(seeded(cfg, seeds[:2]), monsters="all", monster_cap=17)


def test_value_forms(goldens, lib):
    """ParallelRogueEnv.monster_tables against the device tensors of a HipVecRogueEnv on the same seeds and keys; RogueEnv.monsters against the host entry on
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
        for mode, cap in (("shown", 4), ("all", 16), ("all", 1)):
            tb, th = dev.monster_table(mode, cap)
            ptb, pth = par.monster_tables(mode, cap)
            assert ptb.dtype == np.int16 and ptb.shape == (12, cap, 8) and pth.dtype == np.int32 and pth.shape == (12, 4)
            assert np.array_equal(tb.cpu().numpy(), ptb) and np.array_equal(th.cpu().numpy(), pth), (t, mode, cap)
            seen += int((ptb[:, 0, 0] != 0).sum())
    assert seen > 50
    listed = 0
    for t in range(25):
        one.step(chr(table[t][0]))
        f = feeds_of(one.game._h, mo.room_grid(cfg))[0]
        for mode, m in mo.MODES:
            tb, th = one.monsters(mode, 8)
            hb, ht = mo.host_call(lib, f, m, 8)
            assert tb.shape == (8, 8) and th.shape == (4,) and np.array_equal(tb[:, :7], hb[:, :7]) and np.array_equal(th, ht), (t, mode)
            listed += int(tb[0, 0] != 0)
    assert listed > 0
    tb, th = one.monsters()
    assert tb.shape == (4, 8) and tb.dtype == np.int16 and th.dtype == np.int32
    with pytest.raises(ValueError):
        one.monsters("shown", 0)
    dev.close()
    par.close()


def test_refusals_leave_the_buffers_untouched(goldens):
    import torch
    hip = HipBatch(_mini(goldens), [1, 2, 3], max_steps=60)
    hd, dev = hip.h, "cuda:%d" % hip.h.device
    tb = torch.full((3 + SLACK, 16, 8), mo.SENTINEL16, dtype=torch.int16, device=dev)
    th = torch.full((3 + SLACK, 4), mo.SENTINEL32, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    pt, ph = C.c_void_p(tb.data_ptr()), C.c_void_p(th.data_ptr())
    for args, frag in (((2, 4, pt, ph), "mode"), ((7, 4, None, ph), "mode"), ((0, 0, pt, ph), "cap"), ((1, 17, pt, ph), "cap"), ((1, -1, pt, None), "cap"),
                       ((0, 4, None, None), "both NULL"), ((0, 4, C.c_void_p(tb.data_ptr() + 2), ph), "16-byte"), ((0, 4, pt, C.c_void_p(th.data_ptr() + 4)), "16-byte")):
        assert hd.L.rg_monsters(hd.h, *args) != 0, args
        msg = hd.L.rg_last_error(hd.h).decode()
        assert msg.startswith("rg_monsters:") and frag in msg, msg
    hd.check(hd.L.rg_sync(hd.h))
    torch.cuda.synchronize()
    assert bool((tb == mo.SENTINEL16).all()) and bool((th == mo.SENTINEL32).all())
    hd.check(hd.L.rg_monsters(hd.h, 0, 99, None, ph))   # cap is only read with a table
    torch.cuda.synchronize()
    assert bool((th[:3, 1] >= -1).all()) and bool((th[3:] == mo.SENTINEL32).all()) and bool((tb == mo.SENTINEL16).all())
    hd.close()
