"""rg_monsters_host (the monster-table rule on one env's host arrays, no GPU) against the numpy restatement of tests/monster_util.py: on the CPU engine's
state after every step of play, pinned both ways to the engine's own drawing where it drew, with the stale rows between two Redraws as a tested fact; on
hand-built cases clause by clause; and the refusals."""
import os
import re

import numpy as np
import pytest

import mask_util as mu
import monster_util as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (1, 4, 16)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


# name -> (config, first seed, envs, steps, max_steps): mini + enemies 0..11, seeds 9000..9135, 120 steps at max_steps 60; 80 x 24 + enemies 0..11, seeds
# 9100..9147, 100 steps at max_steps 1000.  Auto-reset, the 11-action policy from one RandomState(1) drawn env by env.
def _workload(goldens, name):
    if name == "mini":
        return dict(goldens["configs"]["mini"], enemies=mu.ENEMIES), 9000, 136, 120, 60
    return dict(mu.DEFAULT_SIZE), 9100, 48, 100, 1000


_PLAYS = {}


def _play(lib, goldens, name):
    """One run per workload and process.  After every step of every env: the host entry, both modes and caps 1, 4 and 16, against the numpy rule (asserted
    here); what the two-way pin and the stale pin need is collected for the tests that assert it."""
    if name in _PLAYS:
        return _PLAYS[name]
    from parity_util import make_oracles
    cfg, seed0, n, T, max_steps = _workload(goldens, name)
    table = np.frombuffer(mu.KEYS, np.uint8)[np.random.RandomState(1).randint(0, 11, size=(n, T))].T   # [step][env]
    oracles = make_oracles(cfg, [seed0 + i for i in range(n)], max_steps=max_steps)
    st = dict(rows=0, shown_rows=0, adjacent_rows=0, under_gold=0, two_shown=0, max_alive=0, changed=0, unchanged=0, missing_on_mirror=[], unlisted_on_mirror=[], stale=0,
              stale_checked=0, attack_rows=0)
    for t in range(T):
        for e, o in enumerate(oracles):
            before = o.screen()
            o.step_autoreset(int(table[t][e]))
            after = o.screen()
            f = mo.feed_of_oracle(o, cfg)
            assert f.assigned == mo.assigned_areas(o.w, o.h, f.rnx, f.rny), "the engine's assigned areas are the arithmetic ones"
            lists = {}
            for _, mode in mo.MODES:
                rows, th_rule, _ = mo.rule_list(f, mode)
                lists[mode] = rows
                for cap in CAPS:
                    tb, th = mo.host_call(lib, f, mode, cap)
                    assert np.array_equal(tb, mo.capped(rows, cap)), (name, t, e, mode, cap, tb, rows)
                    assert np.array_equal(th, th_rule), (name, t, e, mode, cap, th, th_rule)
            shown, threat, gold = mo.rule_list(f, mo.SHOWN)
            st["rows"] += 1
            st["shown_rows"] += int(len(shown) > 0)
            st["adjacent_rows"] += int(threat[0] > 0)
            st["attack_rows"] += int(threat[2] != 0)
            st["under_gold"] += gold
            st["two_shown"] += int(len(shown) >= 2)
            st["max_alive"] = max(st["max_alive"], len(lists[mo.ALL]))
            assert len(shown) <= 16
            want, got = mo.listed(f, shown), mo.letters_on(after)
            if not np.array_equal(before, after):   # the engine drew in this step: the table is its drawing, both ways
                st["changed"] += 1
                st["missing_on_mirror"] += [(t, e, c) for c, tile in want.items() if got.get(c) != tile]
                st["unlisted_on_mirror"] += [(t, e, c) for c, tile in got.items() if want.get(c) != tile]
            else:
                st["unchanged"] += 1
                st["stale_missing"] = st.get("stale_missing", 0) + int(any(got.get(c) != tile for c, tile in want.items()))
                if want != got:                     # ... between two Redraws it is the state's, not the image's: draw_screen's conditions, cell by cell
                    st["stale"] += 1
                    for k in range(len(f.mx)):
                        c = (int(f.mx[k]), int(f.my[k]))
                        assert mo.drawn_letter(f, k) == (c in want), (name, t, e, c)
                        st["stale_checked"] += 1
    _PLAYS[name] = st
    return st


def test_host_entry_through_play_mini(lib, goldens):
    st = _play(lib, goldens, "mini")
    print(st)
    # measured with exactly this run: 7 733 rows with a shown monster (never two), 5 783 of them adjacent, 285 monsters that only gold hides; asserted at half
    assert st["rows"] == 136 * 120
    assert st["shown_rows"] >= 3866 and st["adjacent_rows"] >= 2891 and st["under_gold"] >= 142 and st["attack_rows"] == st["adjacent_rows"], st


def test_host_entry_through_play_80x24(lib, goldens):
    st = _play(lib, goldens, "80x24")
    print(st)
    # measured with exactly this run: 1 473 rows with a shown monster, 823 adjacent, 116 monsters that only gold hides, 12 rows with two shown, up to 9
    # alive; asserted at half
    assert st["rows"] == 48 * 100
    assert st["shown_rows"] >= 736 and st["adjacent_rows"] >= 411 and st["under_gold"] >= 58 and st["two_shown"] >= 6 and st["max_alive"] >= 5, st


@pytest.mark.parametrize("name", ["mini", "80x24"])
def test_table_is_the_engines_drawing_where_it_drew(lib, goldens, name):
    """On every row whose step changed the engine's mirror: every listed shown monster's tile is on the mirror at its cell, and every monster letter on
    the mirror is listed (cap 16)."""
    st = _play(lib, goldens, name)
    print(name, "rows whose mirror changed:", st["changed"], "unchanged:", st["unchanged"])
    assert st["changed"] >= (2719 if name == "mini" else 1026), st["changed"]   # measured: 5 439 and 2 053; asserted at half
    assert not st["missing_on_mirror"], st["missing_on_mirror"][:10]
    assert not st["unlisted_on_mirror"], st["unlisted_on_mirror"][:10]


def test_between_redraws_the_table_is_more_current_than_the_mirror(lib, goldens):
    """The documented difference: rows exist whose step drew nothing and whose mirror disagrees with the table; there the table is what draw_screen's
    conditions give on the state (asserted monster by monster in _play)."""
    st = _play(lib, goldens, "mini")
    print("stale rows:", st["stale"], "of them with a listed letter missing on the mirror:", st["stale_missing"], "monsters checked on them:", st["stale_checked"])
    assert st["stale"] >= 411 and st["stale_missing"] >= 405 and st["stale_checked"] >= st["stale"], st   # measured: 823 rows differ either way, 811 of them miss a listed letter; asserted at half


# ---------------------------------------------------------------------------------------------
# hand-built cases: a 32 x 16 grid of lit floor, 2 x 2 areas of 16 x 8; room 0 = (2, 2)-(10, 7), room 1 = (18, 2)-(28, 7), room 2 Empty, room 3 = (18, 9)-(28, 14)
# ---------------------------------------------------------------------------------------------
LIT = 0x41   # floor | C_VISIBLE
RECTS = [2 | 2 << 8 | 10 << 16 | 7 << 24, 18 | 2 << 8 | 28 << 16 | 7 << 24, 5 | 10 << 8 | 5 << 16 | 10 << 24, 18 | 9 << 8 | 28 << 16 | 14 << 24]
METAS = [0, 0, 2, 0]


def _feed(px, py, mons, dead=0, cells=None, rects=None):
    """mons: [(x, y)] or [(x, y, type, active, hp)]."""
    g = np.full((16, 32), LIT, np.uint16) if cells is None else cells
    m = [(q + (k % 26, k % 2, 10 + k))[:5] if len(q) == 2 else q for k, q in enumerate(mons)]
    cols = list(zip(*m)) if m else [[], [], [], [], []]
    return mo.Feed(g, px, py, dead, cols[0], cols[1], cols[2], cols[3], cols[4], 2, 2, RECTS if rects is None else rects, METAS)


def _both(lib, f, cap=16):
    """{mode: (table, threat)} of the host entry, each checked against the numpy rule."""
    out = {}
    for _, mode in mo.MODES:
        rows, threat, _ = mo.rule_list(f, mode)
        tb, th = mo.host_call(lib, f, mode, cap)
        assert np.array_equal(tb, mo.capped(rows, cap)), (mode, tb, rows)
        assert np.array_equal(th, threat), (mode, th, threat)
        out[mode] = (tb, th)
    return out


def _shown_cells(f, tb):
    return sorted(c for c in mo.listed(f, [r for r in tb if r[4]]))


def test_rows_0_and_h_minus_1_are_never_shown(lib):
    f = _feed(5, 1, [(5, 0), (6, 0)])
    r = _both(lib, f)
    assert r[mo.SHOWN][1].tolist() == [0, -1, 0, 0] and not r[mo.SHOWN][0].any()
    assert r[mo.ALL][1].tolist() == [0, -1, 0, 2] and [int(x) for x in r[mo.ALL][0][:2, 4]] == [0, 0] and r[mo.ALL][0][0, 0] != 0
    f = _feed(5, 14, [(5, 15), (4, 15)])
    r = _both(lib, f)
    assert r[mo.SHOWN][1].tolist() == [0, -1, 0, 0] and r[mo.ALL][1].tolist() == [0, -1, 0, 2]


def test_gold_is_drawn_over_a_monster(lib):
    g = np.full((16, 32), LIT, np.uint16)
    g[4, 6] |= mo.C_GOLD
    f = _feed(5, 4, [(6, 4), (4, 4)], cells=g)
    r = _both(lib, f)
    assert _shown_cells(f, r[mo.SHOWN][0]) == [(4, 4)] and r[mo.SHOWN][1].tolist() == [1, 1, 1 << 0, 1]   # 'h' aims at (4, 4); the one under gold is not in the mask
    assert r[mo.ALL][1].tolist() == [1, 1, 1, 2]
    assert mo.rule_list(f, mo.SHOWN)[2] == 1


def test_a_cell_that_is_neither_visible_nor_drawn(lib):
    g = np.full((16, 32), LIT, np.uint16)
    g[4, 6] = 0x01            # floor, unknown
    g[4, 4] = 0x01 | 0x80     # floor, drawn only
    f = _feed(5, 4, [(6, 4), (4, 4)], cells=g)
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(4, 4)]


def test_same_room_clause_outside_the_rect(lib):
    f = _feed(12, 4, [(14, 4)])                    # two cells away in a passage of area 0, both outside room 0: d2 = 4, the same-room clause alone
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(14, 4)]
    f = _feed(12, 3, [(1, 6), (0, 1), (15, 7)])    # corridor cells of one area, far apart, all outside the rect
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(0, 1), (1, 6), (15, 7)]
    f = _feed(12, 3, [(16, 3), (12, 8)])           # ... and just across the area's borders: other areas
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == []


def test_inside_the_rect_against_outside(lib):
    f = _feed(5, 4, [(12, 4), (9, 6), (10, 4), (2, 2), (1, 2)])   # the player inside room 0
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(2, 2), (9, 6)]
    f = _feed(9, 4, [(10, 4), (10, 5), (11, 4)])                  # at the rect's edge: the near clause reaches across it, d2 = 4 does not
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(10, 4), (10, 5)]
    f = _feed(12, 4, [(5, 4), (11, 4)])                           # the player outside
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(11, 4)]


def test_empty_room_is_one_room(lib):
    f = _feed(3, 10, [(12, 13), (5, 10), (0, 8), (15, 14), (0, 15), (16, 10)])   # area 2 = x 0..15, y 8..14
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(0, 8), (5, 10), (12, 13), (15, 14)]


# The three cases below close what the mutant probe (tests/rule_mutants.py) found alive in rg_monsters.h.  They stand on this file's 32 x 16 grid of 2 x 2
# areas, not on a 5 x 5 to 9 x 9 one: each clause is about a room's assigned area and rect, which need that much room; tests/test_gpu_monsters.py loads the
# same feeds as state records (room words included) for k_monsters.
def test_an_empty_room_whose_rect_has_some_area(lib):
    """Floor::in_same_room (floor.rs:381-393) answers true for an Empty room before it looks at the rect: with the player inside a rect of some area and a monster
    outside it (and the other way round) the same area alone decides.  (test_empty_room_is_one_room's rect holds no cell, so inside == outside there.)"""
    rects = RECTS[:2] + [4 | 10 << 8 | 9 << 16 | 13 << 24] + RECTS[3:]          # the Empty room 2 with a rect of x 4..8, y 10..12
    f = _feed(5, 11, [(12, 13), (6, 11), (0, 8), (16, 11), (12, 7)], rects=rects)   # the player inside it; (16, 11) and (12, 7) stand in other areas
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(0, 8), (6, 11), (12, 13)]
    f = _feed(12, 13, [(5, 11), (14, 9)], rects=rects)                              # the player outside it
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(5, 11), (14, 9)]


def test_a_monster_on_the_players_own_cell(lib):
    """RunTime::draw_screen draws the player over whatever stands on its cell (rogue/mod.rs:398-404): a monster there is alive and not shown, and it is not the
    nearest shown monster at distance 0."""
    f = _feed(5, 4, [(5, 4), (6, 4)])
    r = _both(lib, f)
    assert _shown_cells(f, r[mo.SHOWN][0]) == [(6, 4)] and r[mo.SHOWN][1].tolist() == [1, 1, 1 << 3, 1]
    tb, th = r[mo.ALL]
    assert th.tolist() == [1, 1, 1 << 3, 2] and [int(v) for v in tb[0, 1:5]] == [0, 0, 0, 0] and tb[0, 0] != 0      # listed first (cheb 0), not shown


def test_a_player_in_row_0_stands_in_no_area(lib):
    """Room::assigned_area (rooms.rs:192-209) starts the top areas at row 1: from row 0 only the near clause is left, as from the last row."""
    f = _feed(5, 0, [(5, 1), (6, 1), (7, 1), (5, 2)])      # d2 = 1, 2, 5, 4
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(5, 1), (6, 1)]


def test_another_area_at_d2_2(lib):
    f = _feed(15, 4, [(16, 5), (17, 4), (16, 3)])
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(16, 3), (16, 5)]


def test_a_player_in_no_area(lib):
    f = _feed(5, 15, [(5, 14), (6, 14), (7, 14), (5, 13)])   # the last row belongs to no area: only the near clause is left
    assert _shown_cells(f, _both(lib, f)[mo.SHOWN][0]) == [(5, 14), (6, 14)]


def test_order_ties_on_cheb_then_d2_then_position(lib):
    f = _feed(5, 4, [(7, 5), (7, 4), (5, 6), (3, 4), (6, 4), (3, 6)])
    tb = _both(lib, f)[mo.SHOWN][0]
    assert [(f.px + int(r[1]), f.py + int(r[2])) for r in tb[:6]] == [(6, 4), (3, 4), (5, 6), (7, 4), (7, 5), (3, 6)]
    assert [int(r[3]) for r in tb[:6]] == [1, 2, 2, 2, 2, 2]
    assert not tb[6:].any()


def test_more_qualifiers_than_cap_and_cap_above_the_count(lib):
    mons = [(x, y) for y in (2, 3, 4, 5, 6) for x in range(2, 10) if (x, y) != (5, 4)]   # 39 monsters in room 0 around the player
    f = _feed(5, 4, mons)
    for cap in (1, 2, 4, 5, 8, 16):
        r = _both(lib, f, cap)
        for mode in (mo.SHOWN, mo.ALL):
            assert r[mode][1].tolist() == [8, 1, 0xFF, 39] and r[mode][0][:, 0].all()
    full = mo.rule_list(f, mo.ALL)[0]
    assert sorted(int(s) for s in full[:, 7]) == list(range(39))
    f = _feed(5, 4, [(6, 4), (8, 4)])
    tb, th = _both(lib, f, 16)[mo.ALL]
    assert th.tolist() == [1, 1, 1 << 3, 2] and tb[:2, 0].all() and not tb[2:].any()
    assert not _both(lib, _feed(5, 4, []), 16)[mo.ALL][0].any()


def test_dead_player(lib):
    f = _feed(5, 4, [(6, 4), (8, 4)], dead=1)
    for mode, (tb, th) in _both(lib, f).items():
        assert not tb.any() and th.tolist() == [0, -1, 0, 0]


def test_all_mode_columns_and_the_hp_clamp(lib):
    f = _feed(5, 4, [(6, 4, 3, 1, 40000), (8, 4, 25, 0, 32767), (9, 4, 0, 1, -5), (20, 12, 7, 0, 9)])
    r = _both(lib, f)
    assert r[mo.ALL][0][:4].tolist() == [[ord("D"), 1, 0, 1, 1, 1, 32767, 0], [ord("Z"), 3, 0, 3, 1, 0, 32767, 1], [ord("A"), 4, 0, 4, 1, 1, -5, 2],
                                        [ord("H"), 15, 8, 15, 0, 0, 9, 3]]
    assert r[mo.SHOWN][0][:3].tolist() == [[ord("D"), 1, 0, 1, 1, 0, 0, 0], [ord("Z"), 3, 0, 3, 1, 0, 0, 0], [ord("A"), 4, 0, 4, 1, 0, 0, 0]]
    assert r[mo.SHOWN][1][3] == 3 and r[mo.ALL][1][3] == 4
    alive = mo.Feed(f.cells, 5, 4, 0, f.mx, f.my, f.mtype, f.mactive, f.mhp, 2, 2, RECTS, METAS, alive=[0, 1, 0, 1])   # entries that are not alive are skipped
    assert _both(lib, alive)[mo.ALL][0][:2, 7].tolist() == [1, 3]


def test_attack_mask_bit_by_bit(lib):
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    keys = re.search(r'#define RG_ACTION_KEYS "([^"]+)"', hdr).group(1)
    assert keys[1:9] == mo.MOVE_KEYS
    for i in range(8):
        dx, dy = mu.DIRS[keys[1 + i]]
        for px, py in ((5, 4), (12, 4), (15, 7)):
            f = _feed(px, py, [(px + dx, py + dy), (px + 2 * dx, py + 2 * dy)])
            th = _both(lib, f)[mo.SHOWN][1]
            assert th[0] == 1 and th[1] == 1 and th[2] == 1 << i, (keys[1 + i], px, py, th)
    f = _feed(5, 4, [(5 + dx, 4 + dy) for dx, dy in mu.DIRS.values()])
    assert _both(lib, f)[mo.SHOWN][1].tolist() == [8, 1, 0xFF, 8]


def test_host_refusals(lib):
    f = _feed(5, 4, [(6, 4)])
    for kw, frag in ((dict(mode=2, cap=4), "mode"), (dict(mode=0, cap=0), "cap"), (dict(mode=1, cap=17), "cap"), (dict(mode=0, cap=4, table=False, threat=False), "both NULL")):
        with pytest.raises(RuntimeError, match="rg_monsters_host:.*" + frag):
            mo.host_call(lib, f, **kw)
    assert mo.host_call(lib, f, 0, 0, table=False)[1].tolist() == [1, 1, 1 << 3, 1]   # cap is only read with a table
    assert mo.host_call(lib, f, 0, 1, threat=False)[0].tolist() == [[ord("A"), 1, 0, 1, 1, 0, 0, 0]]
    for bad, frag in ((_feed(32, 4, []), "player"), (_feed(5, 16, []), "player"), (_feed(5, 4, [(32, 4)]), "outside the grid"), (_feed(5, 4, [(3, 3, 26, 0, 1)]), "mon_type")):
        with pytest.raises(RuntimeError, match=frag):
            mo.host_call(lib, bad, 0, 4)
    for rnx, rny in ((0, 2), (2, 0), (33, 1), (1, 17)):
        bad = mo.Feed(f.cells, 5, 4, 0, f.mx, f.my, f.mtype, f.mactive, f.mhp, 2, 2, RECTS, METAS)
        bad.rnx, bad.rny = rnx, rny
        with pytest.raises(RuntimeError, match="room_num"):
            mo.host_call(lib, bad, 0, 4)
    # a refusal writes nothing
    tb, th = np.full((4, 8), mo.SENT16, np.int16), np.full(4, mo.SENT32, np.int32)
    assert lib.rg_monsters_host(f.cells.ctypes.data, 16, 32, 5, 4, 0, 1, f.mx.ctypes.data, f.my.ctypes.data, f.mtype.ctypes.data, f.mactive.ctypes.data, f.mhp.ctypes.data, None, 2, 2,
                                f.rect.ctypes.data, f.meta.ctypes.data, 7, 4, tb.ctypes.data, th.ctypes.data) != 0
    assert (tb == mo.SENT16).all() and (th == mo.SENT32).all()
    assert lib.rg_monsters_host(None, 16, 32, 5, 4, 0, 0, None, None, None, None, None, None, 2, 2, f.rect.ctypes.data, f.meta.ctypes.data, 0, 4, tb.ctypes.data, th.ctypes.data) != 0
    assert "cells" in lib.rg_last_error(None).decode()


def test_header_constants_and_python_names(lib):
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for name, val in (("RG_MON_SHOWN", "0u"), ("RG_MON_ALL", "1u"), ("RG_MON_MAX_CAP", "16"), ("RG_MON_COLS", "8")):
        assert re.search(r"#define %s\s+%s\b" % (name, val), hdr), name
    for n in ("rg_monsters", "rg_monsters_host"):
        assert re.search(r"\b%s\s*\(" % n, hdr) and hasattr(lib, n), n
    from rogue_gym_python import _rogue_gym as inner
    from rogue_gym.envs import MONSTER_COLS, HipVecRogueEnv
    assert MONSTER_COLS == inner.MONSTER_COLS == HipVecRogueEnv.MONSTER_COLS == ("tile", "dx", "dy", "cheb", "shown", "active", "hp", "slot")
    assert (inner.RG_MON_SHOWN, inner.RG_MON_ALL, inner.RG_MON_MAX_CAP, inner.RG_MON_COLS) == (0, 1, 16, 8) == (mo.SHOWN, mo.ALL, mo.MAX_CAP, mo.COLS)
    assert inner._monster_args("all", 16) == (1, 16) and inner._monster_args("shown", 1) == (0, 1)
    for bad in (("seen", 4), ("all", 0), ("all", 17), (None, 4), ("shown", 2.5)):
        with pytest.raises(ValueError):
            inner._monster_args(*bad)
