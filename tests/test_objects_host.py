"""rg_objects_host (the object-table rule on one env's grid, no GPU) against the numpy restatement of tests/object_util.py: on the CPU engine's state after
every step of play -- random keys on the two workloads of tests/test_monsters_host.py and a run that follows the explorer -- in all four modes, every kind
set and caps 1, 8 and 32; every listed row against rg_route_host asked for that cell; known mode against the engine's own drawing; hand-built cases clause
by clause; and the refusals."""
import os
import re

import numpy as np
import pytest

import mask_util as mu
import object_util as ou
import route_util as ru
from object_util import DOOR, FRONTIER, GOLD, STAIRS
from route_util import GOAL_CELL, GOAL_FRONTIER, GOAL_STAIRS, KNOWN, SECRETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (1, 8, 32)
SGD = STAIRS | GOLD | DOOR
PASSAGE, FLOOR, WALL, STAIR, DOORS, NONE = 0, 1, 2, 4, 5, 7   # surfaces (rg_state.h)
HIDDEN, VISIBLE, DRAWN, LOCKED, GOLDBIT = 0x20, 0x40, 0x80, 0x100, 0x800
GLYPH = {ord("%"): STAIRS, ord("*"): GOLD, ord("+"): DOOR}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


# name -> (config, first seed, envs, steps, max_steps, policy): the two workloads of tests/test_monsters_host.py under the 11-action policy from one
# RandomState(1), and 80 x 24 again with every env following the explorer's host key (rg_route_host: stairs, else the frontier, on the known map)
def _workload(goldens, name):
    if name == "mini":
        return dict(goldens["configs"]["mini"], enemies=mu.ENEMIES), 9000, 136, 120, 60, "random"
    if name == "80x24":
        return dict(mu.DEFAULT_SIZE), 9100, 48, 100, 1000, "random"
    return dict(mu.DEFAULT_SIZE), 9200, 12, 150, 1000, "explore"


_PLAYS = {}


def _check_row(lib, cells, px, py, dead, st, where):
    """One env's state: the host entry against the numpy rule for every mode, kind set and cap, and every listed row of the widest table against
    rg_route_host from the other end.  -> {mode: Objects}."""
    obs = {}
    for mode in ou.MODES:
        ob = obs[mode] = ou.Objects(cells, px, py, dead, mode)
        for kinds in ou.kind_sets(mode):
            rows, cnt = ob.rows(kinds), ob.count(kinds)
            for cap in CAPS:
                tb, c = ou.host(lib, cells, px, py, dead, kinds, mode, cap)
                assert np.array_equal(tb, ou.capped(rows, cap)), (where, mode, kinds, cap, tb, rows)
                assert np.array_equal(c, cnt), (where, mode, kinds, cap, c, cnt)
        for r in rows[:32]:   # (the last kind set is the widest one)
            d = ru.host(lib, cells, px, py, GOAL_CELL, 0, mode, 0, cell=(int(r[5]), int(r[4])), want=(False, True, False, False))[1]
            assert d == int(r[3]), (where, mode, r, d)
            st["route_checked"] += 1
    return obs


def _play(lib, goldens, name):
    """One run per workload and process; what the floors and the mirror pin need is collected for the tests that assert it."""
    if name in _PLAYS:
        return _PLAYS[name]
    from parity_util import make_oracles
    cfg, seed0, n, T, max_steps, policy = _workload(goldens, name)
    table = np.frombuffer(mu.KEYS, np.uint8)[np.random.RandomState(1).randint(0, 11, size=(n, T))].T   # [step][env]
    oracles = make_oracles(cfg, [seed0 + i for i in range(n)], max_steps=max_steps)
    st = dict(rows=0, route_checked=0, max_doors=0, max_gold=0, max_walk=0, objects_all=0, unreached_plain=0, unreached_secrets=0, max_frontier=0, known_stairs_rows=0,
              own_cell_rows=0, multi_kind=0, over_cap8=0, changed=0, glyphs=0, glyph_not_known=[], listed_known=0, listed_blank=[])
    for t in range(T):
        for e, o in enumerate(oracles):
            before = o.screen()
            if policy == "random":
                key = int(table[t][e])
            else:
                sc = o.scalars()
                key = ru.host(lib, mu.cell_words(*o.grid()), sc["px"], sc["py"], GOAL_STAIRS, GOAL_FRONTIER, KNOWN, int(o.flags()["dead"]), want=(False, False, True, False))[2]
            o.step_autoreset(key)
            after = o.screen()
            cells, sc, dead = mu.cell_words(*o.grid()), o.scalars(), int(o.flags()["dead"])
            px, py = sc["px"], sc["py"]
            obs = _check_row(lib, cells, px, py, dead, st, (name, t, e))
            st["rows"] += 1
            if dead:
                continue
            full, cnt = obs[0].rows(SGD), obs[0].count(SGD)
            st["max_doors"], st["max_gold"] = max(st["max_doors"], int(cnt[2])), max(st["max_gold"], int(cnt[1]))
            st["max_walk"] = max(st["max_walk"], int(full[:, 3].max()) if len(full) else 0)
            st["objects_all"] += int((obs[0].kind & SGD != 0).sum())
            st["unreached_plain"] += int((obs[0].kind & SGD != 0).sum()) - len(full)
            st["unreached_secrets"] += int((obs[SECRETS].kind & SGD != 0).sum()) - len(obs[SECRETS].rows(SGD))
            st["over_cap8"] += int(len(full) > 8)
            known = obs[KNOWN].rows(SGD | FRONTIER)
            st["max_frontier"] = max(st["max_frontier"], int(obs[KNOWN].count(FRONTIER)[3]))
            st["known_stairs_rows"] += int(((known[:, 0] & STAIRS) != 0).any())
            st["own_cell_rows"] += int(len(known) > 0 and known[0, 3] == 0)
            st["multi_kind"] += int(any(int(k) & (int(k) - 1) for k in known[:, 0]))
            if not np.array_equal(before, after):   # the engine drew in this step: its %, * and + against the known cells of that kind
                st["changed"] += 1
                kind = obs[KNOWN].kind
                h = after.shape[0]
                for y in range(1, h - 1):
                    for x in np.flatnonzero(np.isin(after[y], list(GLYPH))):
                        st["glyphs"] += 1
                        if not kind[y, x] & GLYPH[int(after[y, x])]:
                            st["glyph_not_known"].append((t, e, int(x), y, chr(after[y, x]), int(kind[y, x])))
                for r in obs[KNOWN].rows(SGD):
                    x, y, k = int(r[4]), int(r[5]), int(r[0])
                    if (x, y) == (px, py):
                        continue                    # the player stands on it: '@'
                    ch = int(after[y, x])
                    st["listed_known"] += 1
                    if not (ord("A") <= ch <= ord("Z") or ch == ord("*") or GLYPH.get(ch, 0) & k):
                        st["listed_blank"].append((t, e, x, y, k, chr(ch), hex(int(cells[y, x])), sc["level"]))
    _PLAYS[name] = st
    return st


def _summary(st):
    return {k: (v if not isinstance(v, list) else len(v)) for k, v in st.items()}


def test_host_entry_through_play_mini(lib, goldens):
    st = _play(lib, goldens, "mini")
    print(_summary(st))
    assert st["rows"] == 136 * 120
    # measured with exactly this run, ALL mode: up to 7 doors and 4 gold in one env, the longest walk 70; 3 379 of 161 560 objects (2.1 %) not reached without
    # RG_ROUTE_SECRETS, none with it; up to 11 frontier cells; 2 588 rows with the stairs on the player's map, 883 with the own cell listed, 10 456 with a cell of
    # two kinds; 14 437 rows with more than 8 objects; 412 005 listed rows asked of rg_route_host.  Asserted at half.
    assert st["max_doors"] >= 3 and st["max_gold"] >= 2 and st["max_walk"] >= 35 and st["max_frontier"] >= 5 and st["over_cap8"] >= 7218, _summary(st)
    assert st["route_checked"] >= 206000 and st["unreached_plain"] >= 1689 and st["unreached_secrets"] <= st["unreached_plain"] // 10, _summary(st)
    assert st["known_stairs_rows"] >= 1294 and st["own_cell_rows"] >= 441 and st["multi_kind"] >= 5228, _summary(st)


def test_host_entry_through_play_80x24(lib, goldens):
    st = _play(lib, goldens, "80x24")
    print(_summary(st))
    assert st["rows"] == 48 * 100
    # measured with exactly this run, ALL mode: up to 22 doors and 7 gold in one env, the longest walk 171; 6 300 of 116 578 objects (5.4 %) not reached without
    # RG_ROUTE_SECRETS, none with it; up to 10 frontier cells; 4 700 rows with more than 8 objects; 258 720 listed rows asked of rg_route_host; the stairs
    # never on the player's map (the explorer's run is for that).  Asserted at half.
    assert st["max_doors"] >= 11 and st["max_gold"] >= 3 and st["max_walk"] >= 85 and st["max_frontier"] >= 5 and st["over_cap8"] >= 2350, _summary(st)
    assert st["route_checked"] >= 129360 and st["unreached_plain"] >= 3150 and st["unreached_secrets"] <= st["unreached_plain"] // 10, _summary(st)


def test_host_entry_following_the_explorer(lib, goldens):
    """Random play almost never brings the stairs of 80 x 24 onto the player's own map; the explorer does."""
    st = _play(lib, goldens, "explore")
    print(_summary(st))
    assert st["rows"] == 12 * 150
    # measured: 104 rows with the stairs on the player's map, 201 with the own cell listed, up to 14 frontier cells, the longest walk 169; asserted at half
    assert st["known_stairs_rows"] >= 52 and st["own_cell_rows"] >= 100 and st["max_frontier"] >= 7 and st["max_walk"] >= 84, _summary(st)


@pytest.mark.parametrize("name", ["mini", "80x24"])
def test_known_mode_is_the_engines_drawing_where_it_drew(lib, goldens, name):
    """On every row whose step changed the engine's mirror: every %, * and + of the mirror is a known cell of that kind; and of the listed known cells at
    most 1 % are missing from the mirror (a monster's letter, or * over another kind, counts as present).  Measured: 8 of 11 150 on mini, all of them the
    stairs of a dark room the player has left -- the cell keeps C_DRAWN, leaving the room clears C_VISIBLE, and the engine draws a tile only where
    C_VISIBLE is set; 0 of 5 066 on 80 x 24."""
    st = _play(lib, goldens, name)
    print(name, "rows whose mirror changed:", st["changed"], "glyphs:", st["glyphs"], "listed known cells:", st["listed_known"], "blank on the mirror:", st["listed_blank"])
    assert st["changed"] >= (2719 if name == "mini" else 1026), st["changed"]   # measured: 5 439 and 2 053; asserted at half
    assert st["glyphs"] >= (5547 if name == "mini" else 2532) and not st["glyph_not_known"], st["glyph_not_known"][:10]   # measured: 11 095 and 5 064
    assert st["listed_known"] >= (5575 if name == "mini" else 2533) and 100 * len(st["listed_blank"]) <= st["listed_known"], (len(st["listed_blank"]), st["listed_known"])


# ---------------------------------------------------------------------------------------------
# hand-built cases
# ---------------------------------------------------------------------------------------------
def grid(w, h, base=FLOOR, **cells):
    """w x h of `base` with the named cells replaced: grid(5, 5, x2y1=WALL)."""
    g = np.full((h, w), base, np.uint16)
    for name, v in cells.items():
        x, y = name[1:].split("y")
        g[int(y), int(x)] = v
    return g


def both(lib, g, px, py, kinds, mode, cap=8, dead=0):
    """(table, count) of the host entry, checked against the numpy rule."""
    ob = ou.Objects(g, px, py, dead, mode)
    tb, c = ou.host(lib, g, px, py, dead, kinds, mode, cap)
    assert np.array_equal(tb, ou.capped(ob.rows(kinds), cap)), (tb, ob.rows(kinds))
    assert np.array_equal(c, ob.count(kinds)), (c, ob.count(kinds))
    return tb, c


def cells_of(tb):
    return [(int(r[4]), int(r[5])) for r in tb if r[0]]


def test_gold_and_stairs_under_the_player(lib):
    g = grid(5, 3, x1y1=FLOOR | GOLDBIT, x3y1=FLOOR | GOLDBIT)
    tb, c = both(lib, g, 1, 1, SGD, 0)
    assert cells_of(tb) == [(3, 1)] and c.tolist() == [0, 1, 0, 0]          # the gold under the player is neither listed nor counted
    assert tb[0].tolist() == [GOLD, 2, 0, 2, 3, 1, 2, 0]
    g = grid(5, 3, x1y1=STAIR | GOLDBIT)
    tb, c = both(lib, g, 1, 1, SGD, 0)
    assert tb[0].tolist() == [STAIRS, 0, 0, 0, 1, 1, 0, 0] and not tb[1:].any() and c.tolist() == [1, 0, 0, 0]   # the stairs under the player: walk 0
    tb, c = both(lib, g, 3, 1, SGD, 0)
    assert tb[0].tolist() == [STAIRS | GOLD, -2, 0, 2, 1, 1, 2, 0] and c.tolist() == [1, 1, 0, 0]              # one cell, one object, two kinds
    assert both(lib, g, 3, 1, GOLD, 0)[0][0, 0] == GOLD                                                        # the kind column holds asked kinds only
    g = grid(5, 3, base=FLOOR, x1y1=DOORS)                                   # a door under the player in known mode: the own cell is known whatever its word
    assert both(lib, g, 1, 1, DOOR, KNOWN)[0][0].tolist() == [DOOR, 0, 0, 0, 1, 1, 0, 0]


def test_a_door_that_is_a_frontier_cell(lib):
    g = grid(7, 3, base=WALL | DRAWN)
    g[1, :] = PASSAGE | DRAWN
    g[1, 3] = DOORS | DRAWN
    g[0, 3] = WALL                                                           # not on the map: the door has an unknown orthogonal neighbour
    tb, c = both(lib, g, 0, 1, SGD | FRONTIER, KNOWN)
    assert tb[0].tolist() == [DOOR | FRONTIER, 3, 0, 3, 3, 1, 3, 0] and not tb[1:].any() and c.tolist() == [0, 0, 1, 1]
    assert both(lib, g, 0, 1, FRONTIER, KNOWN)[0][0, 0] == FRONTIER and both(lib, g, 0, 1, DOOR, KNOWN)[0][0, 0] == DOOR
    g[1, 3] = WALL | LOCKED | DRAWN                                          # a hidden door keeps its wall surface: no door, and pass only with SECRETS
    assert both(lib, g, 0, 1, SGD | FRONTIER, KNOWN)[1].tolist() == [0, 0, 0, 0]
    tb, c = both(lib, g, 0, 1, SGD | FRONTIER, KNOWN | SECRETS)
    assert tb[0].tolist() == [FRONTIER, 3, 0, 3, 3, 1, 3, 0] and c.tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("cut", [WALL | LOCKED, NONE | HIDDEN, DOORS | LOCKED, PASSAGE | HIDDEN])
def test_an_object_behind_a_hidden_door(lib, cut):
    g = np.full((3, 7), WALL, np.uint16)
    g[1, :] = PASSAGE
    g[1, 3] = cut
    g[1, 6] = STAIR
    g[1, 1] |= GOLDBIT
    for known in (0, KNOWN):
        if known:
            g = g | DRAWN
        tb, c = both(lib, g, 0, 1, SGD, known)
        assert cells_of(tb) == [(1, 1)] and c.tolist() == [1, 1, int((cut & 7) == DOORS), 0]   # counted, not reached: not listed
        tb, c = both(lib, g, 0, 1, SGD, known | SECRETS)
        assert [r[:4].tolist() for r in tb if r[0]] == [[GOLD, 1, 0, 1]] + ([[DOOR, 3, 0, 3]] if (cut & 7) == DOORS else []) + [[STAIRS, 6, 0, 6]]


def test_an_object_that_is_known_while_the_way_is_not(lib):
    g = np.full((3, 7), WALL | DRAWN, np.uint16)
    g[1, :] = PASSAGE | DRAWN
    g[1, 6] = STAIR | VISIBLE
    g[1, 3] = PASSAGE                                                        # a hole in the player's map on the only way
    tb, c = both(lib, g, 0, 1, SGD | FRONTIER, KNOWN)
    assert c.tolist() == [1, 0, 0, 2] and [(int(r[0]), int(r[4])) for r in tb if r[0]] == [(FRONTIER, 2)]   # x = 4 is a frontier cell too, beyond the hole
    tb, c = both(lib, g, 0, 1, SGD, 0)
    assert tb[0].tolist() == [STAIRS, 6, 0, 6, 6, 1, 6, 0]


def test_an_object_the_player_has_not_seen(lib):
    """Stairs and doors count by their surface WHERE the cell is on the player's map: with RG_ROUTE_KNOWN a door and the stairs that were never drawn are neither
    listed nor counted, the gold on a drawn cell is; without it all three are."""
    g = np.full((3, 7), WALL | DRAWN, np.uint16)
    g[1, :] = PASSAGE | DRAWN
    g[1, 2] |= GOLDBIT
    g[1, 4] = DOORS                                                          # not on the map
    g[1, 6] = STAIR                                                          # not on the map
    tb, c = both(lib, g, 0, 1, SGD, KNOWN)
    assert c.tolist() == [0, 1, 0, 0] and tb[0].tolist() == [GOLD, 2, 0, 2, 2, 1, 2, 0] and not tb[1:].any()
    tb, c = both(lib, g, 0, 1, SGD, 0)
    assert c.tolist() == [1, 1, 1, 0] and [r[[0, 3, 4]].tolist() for r in tb[:3]] == [[GOLD, 2, 2], [DOOR, 4, 4], [STAIRS, 6, 6]]


def test_order_inside_one_walk(lib):
    g = grid(7, 7, x1y3=FLOOR | GOLDBIT, x5y3=FLOOR | GOLDBIT, x3y1=FLOOR | GOLDBIT, x3y5=STAIR, x5y5=DOORS, x1y1=FLOOR | GOLDBIT)
    tb, c = both(lib, g, 3, 3, SGD, 0, cap=8)
    assert [r[[0, 3, 4, 5]].tolist() for r in tb[:6]] == [[GOLD, 2, 1, 1], [GOLD, 2, 3, 1], [GOLD, 2, 1, 3], [GOLD, 2, 5, 3], [STAIRS, 2, 3, 5], [DOOR, 2, 5, 5]]   # y, then x
    assert not tb[6:].any() and c.tolist() == [1, 4, 1, 0]


def test_more_objects_than_cap_and_cap_above_the_count(lib):
    g = grid(9, 5, base=FLOOR | GOLDBIT)
    for cap in (1, 5, 8, 32):
        tb, c = both(lib, g, 4, 2, SGD, 0, cap)
        assert tb[:, 0].all() and c.tolist() == [0, 44, 0, 0] and (np.diff(tb[:, 3]) >= 0).all()
    g = grid(9, 5, x0y0=STAIR, x8y4=FLOOR | GOLDBIT)
    tb, c = both(lib, g, 4, 2, SGD, 0, 32)
    assert cells_of(tb) == [(0, 0), (8, 4)] and not tb[2:].any()
    assert not both(lib, grid(9, 5), 4, 2, SGD, 0, 32)[0].any()


def test_a_dead_player(lib):
    g = grid(5, 3, base=FLOOR | DRAWN, x3y1=STAIR | DRAWN, x0y0=FLOOR | GOLDBIT | DRAWN)
    for mode in ou.MODES:
        tb, c = both(lib, g, 1, 1, SGD, mode, dead=1)
        assert not tb.any() and not c.any()


def test_a_diagonal_that_the_corner_rule_forbids(lib):
    g = grid(4, 4, x1y0=WALL, x1y1=STAIR)
    assert both(lib, g, 0, 0, SGD, 0)[0][0].tolist() == [STAIRS, 1, 1, 2, 1, 1, 1, 0]    # (0, 0) -> (0, 1) -> (1, 1): the diagonal would cut the wall's corner
    g = grid(4, 4, x1y1=STAIR)
    assert both(lib, g, 0, 0, SGD, 0)[0][0].tolist() == [STAIRS, 1, 1, 1, 1, 1, 1, 0]
    g = grid(4, 4, base=FLOOR | DRAWN, x1y0=FLOOR, x1y1=STAIR | DRAWN)                   # under KNOWN a corner cell that is not on the map forbids it too
    assert both(lib, g, 0, 0, SGD, KNOWN)[0][0, 3] == 2 and both(lib, g, 0, 0, SGD, 0)[0][0, 3] == 1


def test_host_refusals(lib):
    g = grid(5, 3, x3y1=STAIR)
    for kw, frag in ((dict(kinds=0, mode=0, cap=8), "kinds"), (dict(kinds=16, mode=0, cap=8), "kinds"), (dict(kinds=1, mode=4, cap=8), "mode"), (dict(kinds=8, mode=0, cap=8), "RG_ROUTE_KNOWN"),
                     (dict(kinds=9, mode=SECRETS, cap=8), "RG_ROUTE_KNOWN"), (dict(kinds=1, mode=0, cap=0), "cap"), (dict(kinds=1, mode=0, cap=33), "cap"),
                     (dict(kinds=1, mode=0, cap=8, table=False, count=False), "both NULL")):
        with pytest.raises(RuntimeError, match="rg_objects_host:.*" + frag):
            ou.host(lib, g, 1, 1, 0, **kw)
    assert ou.host(lib, g, 1, 1, 0, 1, 0, 0, table=False)[1].tolist() == [1, 0, 0, 0]   # cap is only read with a table
    assert ou.host(lib, g, 1, 1, 0, 1, 0, 1, count=False)[0].tolist() == [[STAIRS, 2, 0, 2, 3, 1, 2, 0]]
    for (px, py) in ((5, 1), (1, 3), (-1, 1)):
        with pytest.raises(RuntimeError, match="player"):
            ou.host(lib, g, px, py, 0, 1, 0, 8)
    # a refusal writes nothing
    tb, c = np.full((8, 8), ou.SENT16, np.int16), np.full(4, ou.SENT32, np.int32)
    for args in ((g.ctypes.data, 3, 5, 1, 1, 0, 32, 0, 8), (g.ctypes.data, 3, 5, 1, 1, 0, 8, 1, 8), (g.ctypes.data, 3, 5, 1, 1, 0, 1, 0, 40), (None, 3, 5, 1, 1, 0, 1, 0, 8),
                 (g.ctypes.data, 0, 5, 1, 1, 0, 1, 0, 8), (g.ctypes.data, 3, 161, 1, 1, 0, 1, 0, 8), (g.ctypes.data, 3, 5, 5, 1, 0, 1, 0, 8)):
        assert lib.rg_objects_host(*args, tb.ctypes.data, c.ctypes.data) != 0, args
        assert lib.rg_last_error(None).decode().startswith("rg_objects_host: ")
        assert (tb == ou.SENT16).all() and (c == ou.SENT32).all()
    assert lib.rg_objects_host(None, 3, 5, 1, 1, 0, 1, 0, 8, tb.ctypes.data, c.ctypes.data) != 0 and "cells" in lib.rg_last_error(None).decode()


def test_header_constants_and_python_names(lib):
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for name, val in (("RG_OBJ_STAIRS", "1u"), ("RG_OBJ_GOLD", "2u"), ("RG_OBJ_DOOR", "4u"), ("RG_OBJ_FRONTIER", "8u"), ("RG_OBJ_MAX_CAP", "32"), ("RG_OBJ_COLS", "8")):
        assert re.search(r"#define %s\s+%s\b" % (name, val), hdr), name
    from rogue_gym_python import _rogue_gym as inner
    for n in ("rg_objects", "rg_objects_host"):
        assert re.search(r"^int %s\(" % n, hdr, re.M) and hasattr(lib, n) and getattr(lib, n).argtypes is not None and n in inner._INT_FUNCS, n
    assert len(lib.rg_objects.argtypes) == 6 and len(lib.rg_objects_host.argtypes) == 11
    from rogue_gym.envs import OBJECT_COLS, HipVecRogueEnv, ParallelRogueEnv, RogueEnv
    assert OBJECT_COLS == inner.OBJECT_COLS == HipVecRogueEnv.OBJECT_COLS == ("kind", "dx", "dy", "walk", "x", "y", "cheb", "zero")
    assert (inner.RG_OBJ_STAIRS, inner.RG_OBJ_GOLD, inner.RG_OBJ_DOOR, inner.RG_OBJ_FRONTIER, inner.RG_OBJ_MAX_CAP, inner.RG_OBJ_COLS) == (1, 2, 4, 8, 32, 8) == (STAIRS, GOLD, DOOR, FRONTIER, ou.MAX_CAP, ou.COLS)
    assert inner._object_args() == (7, 0, 8) and inner._object_args("stairs+frontier", True, True, 32) == (9, 3, 32) and inner._object_args("door", False, True, 1) == (4, 1, 1)
    for bad in (("frontier",), ("stairs+frontier", False), ("amulet",), ("",), (None,), (7,), ("gold", False, False, 0), ("gold", False, False, 33), ("gold", False, False, 2.5)):
        with pytest.raises(ValueError):
            inner._object_args(*bad)
    assert hasattr(RogueEnv, "objects") and hasattr(ParallelRogueEnv, "object_tables") and hasattr(HipVecRogueEnv, "object_table")
