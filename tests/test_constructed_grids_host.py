"""The constructed grids of tests/grid_util.py without a GPU: rg_path_host and rg_action_mask_host against the numpy rules (path_util.Graph, mask_util.rule)
on every shape, grid and player tests/test_gpu_constructed_grids.py draws from, all 13 122 stamped neighbourhoods, and the conditions that keep the GPU test
from passing on easy inputs -- asserted here on the reference alone."""
import numpy as np
import pytest

import grid_util as gu
import mask_util as mu
import path_util as pu
from path_util import GOAL_CELL, INF


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


@pytest.fixture(scope="module")
def cases():
    """name -> [(Ref, px, py, dead, cell)]: every player of every grid of every shape, built once."""
    return {name: gu.shape_cases(name) for name in gu.SHAPES}


def test_the_configs_of_the_shapes_parse(lib):
    import json
    buf = bytes(4096)
    for name in gu.SHAPES:
        assert lib.rg_config_canonical(json.dumps(gu.shape_config(name)).encode(), buf, len(buf)) == 0, (name, lib.rg_last_error(None).decode())


def test_constructors():
    g = gu.serpentine(9, 7)
    assert (g[0::2] == gu.FLOOR).all() and [int((r == gu.FLOOR).sum()) for r in g[1::2]] == [1, 1, 1] and g[1, 8] == g[3, 0] == g[5, 8] == gu.FLOOR
    assert np.array_equal(gu.serpentine(7, 9, vertical=True), g.T)
    d = gu.diagonal_bands(12, 8)
    yy, xx = np.mgrid[0:8, 0:12]
    wall = (xx - yy) % 3 == 2
    assert (d[~wall] == gu.FLOOR).all()
    opened = wall & (d == gu.FLOOR)
    for c in np.unique((xx - yy)[wall]):  # one opening per wall diagonal, at an end
        on = (xx - yy) == c
        assert opened[on].sum() == 1 and (opened[on][0] if ((c - 2) // 3) % 2 == 0 else opened[on][-1])
    assert np.array_equal(gu.diagonal_bands(12, 8, mirrored=True), d[:, ::-1])
    # no diagonal move anywhere on the bands, away from the openings: the walk goes by the four orthogonal moves
    big = gu.Ref("bands", gu.diagonal_bands(40, 20))
    assert max(big.farthest(GOAL_CELL, c)[0] for c in ((0, 0), (0, 39), (19, 0), (19, 39))) > 40 * 20 // 2  # (533 floor cells)
    assert (gu.open_floor(5, 4) == gu.FLOOR).all() and (gu.blocked(5, 4, gu.NONE, [(4, 3)]) == gu.NONE).sum() == 19
    p = gu.neighbourhoods()
    assert p.shape == (13122, 3, 3) and len({q.tobytes() for q in p}) == 13122
    assert (p[:6561, 1, 1] == gu.FLOOR).all() and (p[6561:, 1, 1] == gu.STAIR).all()
    assert ((p & gu.C_HIDDEN) != 0).sum() > 10000 and ((p & gu.C_LOCKED) != 0).sum() > 10000


def test_conditions_on_the_reference(cases):
    """What keeps the GPU test honest.  The farthest finite distances measured here, serpentine / bands from their best corner: 32x16 262 / 311,
    33x17 304 / 341, 64x32 1 038 / 1 301, 96x32 1 550 / 1 963, 80x24 970 / 1 211, 104x20 1 048 / 1 305, 128x16 1 030 / 1 271, 97x33 1 664 / 2 048,
    160x48 3 862 / 4 982."""
    bands = gu.Ref("bands", gu.diagonal_bands(160, 48))
    far = max(bands.farthest(GOAL_CELL, c)[0] for c in ((0, 0), (0, 159), (47, 0), (47, 159)))
    print("diagonal_bands(160, 48): farthest finite distance from a corner %d" % far)
    assert far >= 4096  # high plane b = 9 of the FIELD pass
    for name in gu.SHAPES:
        refs = {id(c[0]): c[0] for c in cases[name]}.values()
        best = {r.name: r.farthest()[0] for r in refs if (r.graph.surf == gu.STAIR).any()}
        print(name, best)
        assert max(best.values()) >= 256, (name, best)
        if name == "160x48":
            assert best["bands"] >= 4096 and best["bands mirrored"] >= 4096  # ... and the grids the GPU test injects reach it from their stairs
    for k, p in enumerate(gu.P_WALK):  # a family: the random grids of one p_walk over all shapes
        family = [r.grid for name in gu.SHAPES for r in {id(c[0]): c[0] for c in cases[name]}.values() if r.name == "random %s" % p]
        assert len(family) == len(gu.SHAPES)
        border = np.concatenate([np.concatenate([g[0], g[-1], g[1:-1, 0], g[1:-1, -1]]) for g in family])
        inner = np.concatenate([g[1:-1, 1:-1].ravel() for g in family])
        for where, cells in (("border", border), ("interior", inner)):
            assert set(np.unique(cells & 7)) == set(range(8)), (p, where)
            for bit_name, bit in list(gu.NAMED_BITS.items()) + list(gu.IGNORED_BITS.items()):
                assert ((cells & bit) != 0).any() and ((cells & bit) == 0).any(), (p, where, bit_name)


@pytest.mark.parametrize("name", list(gu.SHAPES))
def test_path_host_on_constructed_grids(lib, cases, name):
    """rg_path_host == path_util.Graph: field, distance and key of every grid and player of the shape, for goals 1, 2, 3, 4 + cell and 5 + cell; the cells
    lie on a wall, outside the grid, on the player's own cell and on the corners."""
    keys, far = set(), 0
    for ref, px, py, dead, cell in cases[name]:
        for goals in gu.GOAL_SETS:
            hf, hd, hk = pu.host(lib, ref.grid, px, py, goals, dead, cell)
            ef, ed, ek = ref.answer(px, py, dead, goals, cell)
            assert np.array_equal(hf, ef) and hd == ed and hk == ek, "%s %s player (%d, %d) goals %d cell %s: host entry dist %d key %r, rule dist %d key %r" % (
                name, ref.name, px, py, goals, cell, hd, chr(hk), ed, chr(ek))
            keys.add(chr(hk))
            far = max(far, hd)
    print("%s: %d cases, largest distance %d, keys %s" % (name, len(cases[name]), far, "".join(sorted(keys))))
    assert far >= 256 and len(keys & set("kjhlyubn")) >= 6 and {">", ".", "s"} <= keys, (far, keys)


@pytest.mark.parametrize("name", list(gu.SHAPES))
def test_mask_host_on_constructed_grids(lib, cases, name):
    why = {}
    for ref, px, py, dead, _ in cases[name]:
        exp = mu.rule(ref.graph.surf, ref.graph.attr, px, py, dead, why=why)
        got = mu.host_row(lib, ref.grid, px, py, dead)
        assert np.array_equal(got, exp), "%s %s player (%d, %d) dead %d: %s vs %s" % (name, ref.name, px, py, dead, got, exp)
    print(name, dict(sorted(why.items())))
    assert all(why.get(r, 0) > 0 for r in ("ok", "out", "wall", "hidden", "corner")), why


def test_mask_host_on_every_neighbourhood(lib):
    """All 13 122 patches, stamped at positions cycling through the interior, the corners and the edges: the expected row comes from the stamped grid.  Every
    direction pattern the rule admits at all occurs among the interior stamps."""
    grids, players, interior = gu.stamped()
    exp = gu.rule_rows(grids, players)
    for i, (g, (px, py)) in enumerate(zip(grids, players)):
        got = mu.host_row(lib, g, px, py, 0)
        assert np.array_equal(got, exp[i]), "patch %d at (%d, %d): %s vs %s" % (i, px, py, got, exp[i])
    assert (exp[:6561, 9] == 0).all() and (exp[6561:, 9] == 1).all()  # '>' on the stairs centres only
    # the patterns of the patches on their own, each in the middle of a 3 x 3 grid: every one of them occurs among the interior stamps, and no other
    patches = gu.neighbourhoods()[:6561]
    alone = set(gu.direction_pattern(gu.rule_rows(patches, [(1, 1)] * len(patches))).tolist())
    assert set(gu.direction_pattern(exp[interior]).tolist()) == alone and len(alone) == 256
    assert interior.sum() == 6561 and len({players[i] for i in np.flatnonzero(~interior)}) > 60
