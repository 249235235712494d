"""k_route on grids of the tests' own making, loaded as records (tests/grid_util.py): secret, unknown and frontier cells at every word seam, in the first and
last rows and columns and on either side of a group boundary in a shared wave; long serpentines through several locked doors; a tier-0 hit beside a tier-1
hit in one wave, in both orders.  Every legal (goals, fallback, mode) against the host entry, and the answers the grids were built for by name."""
import numpy as np
import pytest

import grid_util as gu
import route_util as ru
from grid_util import C_DRAWN, C_GOLD, C_HIDDEN, C_LOCKED, FLOOR, NONE, STAIR, WALLX
from parity_util import HipBatch
from route_util import GOAL_CELL, GOAL_FRONTIER, GOAL_STAIRS, KNOWN, NO_TIER, SECRETS, route_call
from test_gpu_path import torch_mod

pytestmark = pytest.mark.gpu

EXPLORE = (GOAL_STAIRS, GOAL_FRONTIER, KNOWN)
WITH_SECRETS = (GOAL_STAIRS, 0, SECRETS)
DOOR_WORD, HIDDEN_WORD = WALLX | C_LOCKED, NONE | C_HIDDEN   # secrets as the generator leaves them: a piece of wall, a bare cell


def seams(w):
    return [s for s in (32, 64, 96, 128) if s < w]


def snake_with_doors(w, h, vertical):
    """A serpentine, every cell drawn, the stairs at the walk's start; each corridor is cut by secret cells on alternating sides of every word seam (of
    every 32nd row for the vertical one), and the link cells at the ends -- first and last columns (rows) -- are secret in turn.  (grid, far end)."""
    g = gu.serpentine(w, h, vertical) | C_DRAWN
    if vertical:
        for k, x in enumerate(range(0, w, 2)):
            g[(h // 2 + k) % h if h > 2 else 0, x] = (DOOR_WORD, HIDDEN_WORD)[k % 2] | C_DRAWN
        for k, x in enumerate(range(1, w - 1, 2)):
            if k % 3 == 0:
                g[h - 1 if k % 2 == 0 else 0, x] = HIDDEN_WORD | C_DRAWN
        g[h - 1, 0] = STAIR | C_DRAWN
        last = w - 1 - (w - 1) % 2
        far = (last, 0 if ((last // 2) % 2 == 0) else h - 1)
    else:
        for k, y in enumerate(range(0, h, 2)):
            for j, s in enumerate(seams(w) or [w // 2]):
                g[y, s - (k + j) % 2] = (DOOR_WORD, HIDDEN_WORD)[(k + j) % 2] | C_DRAWN
        for k, y in enumerate(range(1, h - 1, 2)):
            if k % 3 == 0:
                g[y, w - 1 if k % 2 == 0 else 0] = DOOR_WORD | C_DRAWN
        g[0, 0] = STAIR | C_DRAWN
        last = h - 1 - (h - 1) % 2
        far = (w - 1 if ((last // 2) % 2 == 0) else 0, last)
    return g, far


def holes_at_seams(w, h):
    """An open floor, drawn, with cells that are not on the map on either side of every word seam in the first, last and a middle row, and in the first and
    last columns; beside them secret cells, so that a frontier cell can be a secret one.  No stairs: only the frontier answers."""
    g = np.full((h, w), FLOOR | C_DRAWN, np.uint16)
    for j, s in enumerate(seams(w) or [w // 2]):
        for y in (0, h - 1, h // 2):
            g[y, s - 1 + (j + y) % 2] = FLOOR                       # unknown
            g[y, s - (j + y) % 2] = DOOR_WORD | C_DRAWN             # a known secret beside it
    g[h // 3, 0] = FLOOR
    g[2 * h // 3, w - 1] = FLOOR
    g[h // 3 + 1, 0] = HIDDEN_WORD | C_DRAWN
    return g


def shape_envs(name):
    """(grids, players, dead, cells, names) of one shape.  Env order in fours, so that every wave of four (H <= 16) or two (H <= 32) envs holds a pair in
    both orders."""
    w, h = gu.SHAPES[name][:2]
    rng = np.random.RandomState(2000 + 3 * w + h)
    known = np.full((h, w), FLOOR | C_DRAWN, np.uint16)
    t0 = known.copy()
    t0[h - 1, w - 1] = STAIR | C_DRAWN                                 # the stairs on the map: tier 0
    t1_last, t1_first = known.copy(), known.copy()
    t1_last[h - 1, :] = FLOOR
    t1_last[h - 1, w // 2] = STAIR                                     # the last row -- the stairs in it -- not on the map: the frontier (row h - 2) answers
    t1_first[0, :] = FLOOR
    t1_first[0, w // 2] = STAIR
    bare = known.copy()                                                # everything known, no stairs: nothing answers -- unless a neighbour's unknown row leaks in
    snake_h, far_h = snake_with_doors(w, h, False)
    snake_v, far_v = snake_with_doors(w, h, True)
    half = gu.serpentine(w, h) | C_DRAWN                               # the far half of a plain serpentine not on the map, stairs included
    half[h // 2:, :] &= ~np.uint16(C_DRAWN)
    half[h - 1 - (h - 1) % 2, w // 2] = STAIR
    holes = holes_at_seams(w, h)
    envs = [("tier 0", t0, (0, 0)), ("tier 1 last row", t1_last, (0, 0)), ("tier 1 first row", t1_first, (w - 1, h - 1)), ("tier 0 again", t0, (w // 2, h // 2)),
            ("unknown last row", t1_last, (w - 1, 0)), ("bare", bare, (w // 2, 0)), ("bare again", bare, (w // 2, h - 1)), ("unknown first row", t1_first, (0, h - 1)),
            ("snake far end", snake_h, far_h), ("snake beside a door", snake_h, (w - 1, 2)), ("snake vertical far end", snake_v, far_v),
            ("snake vertical start", snake_v, (0, h - 1)),
            ("half known", half, (0, 0)), ("holes", holes, (0, 0)), ("holes from the far corner", holes, (w - 1, h - 1)),
            ("random 0.55", gu.random_words(w, h, rng, 0.55), None), ("random 0.75", gu.random_words(w, h, rng, 0.75), None), ("random 0.9", gu.random_words(w, h, rng, 0.9), None)]
    grids, players, names = [], [], []
    for nm, g, p in envs:
        if p is None:
            ys, xs = np.nonzero(~np.isin(g & 7, (gu.WALLX, gu.WALLY, NONE)))
            i = rng.randint(0, len(ys))
            p = (int(xs[i]), int(ys[i]))
        grids.append(g)
        players.append(p)
        names.append(nm)
    n = len(grids)
    dead = np.zeros(n, np.uint32)
    dead[[3, 16]] = 1
    cells = np.stack([rng.randint(-1, h + 1, n), rng.randint(-1, w + 1, n)], axis=1).astype(np.int32)
    return np.stack(grids), players, dead, cells, names


@pytest.fixture(scope="module")
def lib():
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def named_answers(lib, name, grids, players, dead, names):
    """What the grids were built for, by the host entry: {(goals, fallback, mode): (dist, keys, tier)} of the combinations it asks."""
    w, h = gu.SHAPES[name][:2]
    env = {nm: i for i, nm in enumerate(names)}
    by_host = {c: ru.host_answers(lib, grids, players, dead, c[0], c[1], c[2]) for c in (EXPLORE, WITH_SECRETS, (GOAL_STAIRS, 0, 0), (GOAL_FRONTIER, 0, KNOWN | SECRETS))}
    d, k, t = by_host[EXPLORE]
    assert t[env["tier 0"]] == 0 and d[env["tier 0"]] == max(w, h) - 1 and t[env["tier 0 again"]] == 0 and k[env["tier 0 again"]] == ord(".")  # (dead)
    assert (t[env["tier 1 last row"]], d[env["tier 1 last row"]]) == (1, h - 2) and (t[env["tier 1 first row"]], d[env["tier 1 first row"]]) == (1, h - 2)
    assert (t[env["unknown last row"]], t[env["unknown first row"]]) == (1, 1)
    for nm in ("bare", "bare again"):
        assert (d[env[nm]], k[env[nm]], t[env[nm]]) == (-1, ord("s"), NO_TIER), nm
    assert t[env["half known"]] == 1 and d[env["half known"]] > w and t[env["holes"]] == 1
    d, k, t = by_host[WITH_SECRETS]
    plain = by_host[GOAL_STAIRS, 0, 0][0]
    for nm in ("snake far end", "snake vertical far end"):  # a walk through every corridor and all of its doors; without SECRETS the first door ends it
        assert d[env[nm]] >= (w // 2) * (h // 2) and t[env[nm]] == 0 and plain[env[nm]] == -1, (nm, d[env[nm]])
    assert k[env["snake beside a door"]] == ord("s") and d[env["snake beside a door"]] > 0
    return by_host


@pytest.mark.parametrize("name", list(gu.SHAPES))
def test_constructed_grids(lib, name):
    torch_mod()
    grids, players, dead, cells, names = shape_envs(name)
    n = len(grids)
    hip = HipBatch(gu.shape_config(name), [3000 + i for i in range(n)], max_steps=1000, auto_reset=True)
    gu.inject(hip, grids, players, dead, check_every=4)
    hd = hip.h
    by_host = named_answers(lib, name, grids, players, dead, names)
    # the kernel against the host entry: every legal (goals, fallback, mode)
    seen, tiers = set(), set()
    for combo in ru.combos():
        cc = cells if (combo[0] | combo[1]) & GOAL_CELL else None
        got = route_call(hd, combo[0], combo[1], combo[2], cc)
        want = by_host[combo] if combo in by_host else ru.host_answers(lib, grids, players, dead, combo[0], combo[1], combo[2], cc)
        for i in range(n):
            assert (got[0][i], got[1][i], got[2][i]) == (want[0][i], want[1][i], want[2][i]), "%s env %d (%s) player %s goals %d fallback %d mode %d: kernel dist %d key %r tier %d, host entry dist %d key %r tier %d" % (
                name, i, names[i], players[i], combo[0], combo[1], combo[2], got[0][i], chr(got[1][i]), got[2][i], want[0][i], chr(want[1][i]), want[2][i])
        seen |= set(bytes(got[1]).decode())
        tiers |= set(got[2].tolist())
    assert tiers == {0, 1, NO_TIER} and seen >= set("s.") and len(seen & set("kjhlyubn")) >= 4, (seen, tiers)
