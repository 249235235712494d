"""Constructed grids for rg_path and rg_action_mask, and the injector that puts them into a handle's envs through its state records.

A generated dungeon never has a walkable border, a locked cell beside a word seam or a walk of thousands of moves; the grids here have.  Plain numpy and
ctypes: importable without a GPU.  Cell words are in rg_debug_fetch's layout (rg_state.h): surface in bits 0-2, door mark bit 3, CellAttr << 4, maze mark
bit 10, gold bit 11."""
import ctypes as C

import numpy as np

import mask_util as mu
import path_util as pu
from path_util import GOAL_CELL, GOAL_GOLD, GOAL_STAIRS, INF

PASSAGE, FLOOR, WALLX, WALLY, STAIR, DOOR, TRAP, NONE = range(8)   # Surface enum order (rg_state.h)
C_DOOR, C_VISITED, C_HIDDEN, C_VISIBLE, C_DRAWN, C_LOCKED, C_DARK, C_MAZE, C_GOLD = 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800
NAMED_BITS = {"hidden": C_HIDDEN, "locked": C_LOCKED, "gold": C_GOLD, "door": C_DOOR, "maze": C_MAZE}
IGNORED_BITS = {"visited": C_VISITED, "visible": C_VISIBLE, "drawn": C_DRAWN, "dark": C_DARK}
RG_FLAG_DEAD = 0x2
RG_FLAG_ERR_STATE = 0x00100000
P_WALK = (0.55, 0.75, 0.9)
GOAL_SETS = (GOAL_STAIRS, GOAL_GOLD, GOAL_STAIRS | GOAL_GOLD, GOAL_CELL, GOAL_CELL | GOAL_STAIRS)  # those of test_kernel_equals_host_entry_equals_numpy

# name -> (W, H, room_num_x, room_num_y): what only this shape reaches in k_path (min_room_size 4 x 4 needs W / rx > 4 and H / ry > 5)
SHAPES = {
    "32x16": (32, 16, 2, 2),    # WN = 1, four envs per wave, H == GS == 16: a DPP row per env
    "33x17": (33, 17, 2, 2),    # odd H * W = 561: every m16 residue, rows loaded cell by cell, GS = 32 half empty
    "64x32": (64, 32, 2, 3),    # WN = 2 full words, H == GS == 32: two envs per wave held apart only by `there`
    "96x32": (96, 32, 3, 3),    # WN = 3 full words, H == GS
    "80x24": (80, 24, 3, 3),    # the benchmarked size
    "104x20": (104, 20, 3, 2),  # WN = 5, fourth word 8 columns wide, fifth empty, vector loads
    "128x16": (128, 16, 4, 2),  # WN = 5 + the high planes in LDS with four groups per wave
    "97x33": (97, 33, 3, 3),    # WN = 5, one column in the fourth word, cell by cell, GS = 64, odd H * W
    "160x48": (160, 48, 4, 4),  # the maximum; the only grid that reaches plane 9
}


def shape_config(name):
    """A config of that size without enemies (smaller records)."""
    w, h, rx, ry = SHAPES[name]
    return {"width": w, "height": h, "dungeon": {"style": "rogue", "room_num_x": rx, "room_num_y": ry, "min_room_size": {"x": 4, "y": 4}},
            "enemies": {"enemies": []}}


# ---------------------------------------------------------------------------------------------
# grid constructors: u16 [H][W]
# ---------------------------------------------------------------------------------------------
def open_floor(w, h):
    """Every cell floor, borders included."""
    return np.full((h, w), FLOOR, np.uint16)


def blocked(w, h, surface=WALLX, cells=()):
    """Every cell `surface` (a wall, or Surface::None); the (x, y) of `cells` are made floor."""
    g = np.full((h, w), surface, np.uint16)
    for x, y in cells:
        g[y, x] = FLOOR
    return g


def serpentine(w, h, vertical=False):
    """Corridor rows (0, 2, 4 ...) alternate with wall rows, linked at alternating ends: one walk through every corridor.  vertical: the same by columns."""
    if vertical:
        return np.ascontiguousarray(serpentine(h, w).T)
    g = np.full((h, w), WALLX, np.uint16)
    g[0::2] = FLOOR
    for k, y in enumerate(range(1, h - 1, 2)):
        g[y, w - 1 if k % 2 == 0 else 0] = FLOOR
    return g


def diagonal_bands(w, h, mirrored=False):
    """Cells with (x - y) % 3 != 2 are floor, the rest wall; every wall diagonal x - y = 3 k + 2 is opened at one end cell, its first (least x) for even k,
    its last for odd k.  The corner rule forbids every diagonal move inside a band, so a walk covers about two thirds of the grid by the four orthogonal
    moves, across every word seam.  mirrored: the same with x + y (the grid flipped left to right)."""
    if mirrored:
        return np.ascontiguousarray(diagonal_bands(w, h)[:, ::-1])
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.where((xx - yy) % 3 != 2, FLOOR, WALLX).astype(np.uint16)
    for k in range(-(h // 3) - 2, w // 3 + 2):
        c = 3 * k + 2
        y0, y1 = max(0, -c), min(h - 1, w - 1 - c)
        if y0 > y1:
            continue
        y = y0 if k % 2 == 0 else y1
        g[y, y + c] = FLOOR
    return g


def random_words(w, h, rng, p_walk):
    """Every cell, borders included, from the whole palette: surfaces 0..7 (walkable with probability p_walk), independently the hidden, locked, gold, door
    and maze bits, and the attribute bits the rule ignores."""
    n = w * h
    walk = rng.choice([PASSAGE, FLOOR, STAIR, DOOR, TRAP], size=n, p=[0.3, 0.48, 0.02, 0.1, 0.1])
    wall = rng.choice([WALLX, WALLY, NONE], size=n)
    g = np.where(rng.rand(n) < p_walk, walk, wall).astype(np.uint16)
    for bit, p in ((C_HIDDEN, 0.08), (C_LOCKED, 0.08), (C_GOLD, 0.06), (C_DOOR, 0.2), (C_MAZE, 0.3), (C_VISITED, 0.5), (C_VISIBLE, 0.5), (C_DRAWN, 0.5), (C_DARK, 0.5)):
        g |= np.where(rng.rand(n) < p, bit, 0).astype(np.uint16)
    return g.reshape(h, w)


NB_OFFSETS = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]
N_PATCHES = 3 ** 8


def neighbourhoods():
    """u16 [2 * 3^8][3][3]: every assignment of {walkable and free, walkable but hidden or locked (alternating by index), wall} to the eight neighbours of a
    cell; the centre is floor in the first 6 561 patches and stairs in the second."""
    out = np.empty((2 * N_PATCHES, 3, 3), np.uint16)
    for a in range(N_PATCHES):
        p = np.empty((3, 3), np.uint16)
        v = a
        for j, (dx, dy) in enumerate(NB_OFFSETS):
            s, v = v % 3, v // 3
            p[1 + dy, 1 + dx] = (FLOOR, (FLOOR | C_HIDDEN) if (a + j) % 2 == 0 else (DOOR | C_LOCKED), WALLX if (a + j) % 2 else WALLY)[s]
        p[1, 1] = FLOOR
        out[a] = p
        p = p.copy()
        p[1, 1] = STAIR
        out[N_PATCHES + a] = p
    return out


def stamp_position(j, w, h):
    """(px, py, interior) of patch j's centre: positions cycle through the interior (eight of sixteen), the four corners and the four edges; the stairs copy
    of a patch is half a cycle away from its floor copy, so every assignment stands in the interior at least once."""
    a = j % N_PATCHES
    kind = (a + (8 if j >= N_PATCHES else 0)) % 16
    if kind < 8:
        return 1 + (a * 5 + kind) % (w - 2), 1 + (a * 3 + kind) % (h - 2), True
    if kind < 12:
        return ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))[kind - 8] + (False,)
    ex, ey = 1 + (a // 16) % (w - 2), 1 + (a // 16) % (h - 2)
    return ((ex, 0), (ex, h - 1), (0, ey), (w - 1, ey))[kind - 12] + (False,)


def stamped(w=32, h=16):
    """(grids u16 [13 122][h][w], players [(px, py)], interior bool [13 122]): every neighbourhood written over a random background with its centre at
    stamp_position; a neighbour outside the grid does not exist."""
    patches = neighbourhoods()
    back = random_words(w, h, np.random.RandomState(77), 0.75)
    grids = np.empty((len(patches), h, w), np.uint16)
    players, interior = [], np.zeros(len(patches), bool)
    for j, p in enumerate(patches):
        px, py, interior[j] = stamp_position(j, w, h)
        g = back.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= px + dx < w and 0 <= py + dy < h:
                    g[py + dy, px + dx] = p[1 + dy, 1 + dx]
        grids[j] = g
        players.append((px, py))
    return grids, players, interior


def rule_rows(grids, players, dead=None):
    """mask_util.rule of every (grid, player) -> u8 [n][11]."""
    out = np.empty((len(grids), len(mu.KEYS)), np.uint8)
    for i, (g, (px, py)) in enumerate(zip(grids, players)):
        surf, attr = pu.split(g)
        out[i] = mu.rule(surf, attr, px, py, 0 if dead is None else int(dead[i]))
    return out


def direction_pattern(rows):
    """The eight move keys of mask rows as one number per row (bit i: KEYS[1 + i])."""
    return (rows[:, 1:9].astype(np.int64) << np.arange(8)).sum(axis=1)


# ---------------------------------------------------------------------------------------------
# the grids, players and cells of one shape, shared by the host test and the GPU test
# ---------------------------------------------------------------------------------------------
class Ref:
    """One grid with its path_util.Graph; fields are computed once per goal set and shared by the players asked of it."""

    def __init__(self, name, grid):
        self.name, self.grid = name, np.array(grid, np.uint16, order="C")  # (a copy: the caller's array stays writable)
        self.grid.setflags(write=False)
        self.graph = pu.Graph(self.grid)
        self._fields = {}

    def answer(self, px, py, dead, goals, cell=None):
        """(field, distance, key byte) of the numpy rule."""
        key = self.graph.goal_mask(px, py, goals, cell).tobytes()
        if key not in self._fields:
            f = self.graph.field(px, py, goals, cell)
            f.setflags(write=False)
            self._fields[key] = f
        f = self._fields[key]
        return f, pu.dist_of(f, px, py), pu.key_of(self.graph.surf, self.graph.attr, f, px, py, dead, goals)

    def farthest(self, goals=GOAL_STAIRS, cell=None):
        """(largest finite distance, (x, y) of a cell that has it) of the field of a goal set that does not depend on the player."""
        assert not goals & GOAL_GOLD
        f = self.answer(0, 0, 0, goals, cell)[0]
        fin = np.where(f == INF, -1, f.astype(np.int64))
        y, x = np.unravel_index(int(fin.argmax()), fin.shape)
        return int(fin.max()), (int(x), int(y))


def far_corner(grid):
    """(y, x) of the corner from which the farthest finite distance is largest."""
    h, w = grid.shape
    r = Ref("", grid)
    return max(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)), key=lambda c: r.farthest(GOAL_CELL, c)[0])


def shape_grids(name):
    """[Ref] of one shape.  The order makes every four neighbours -- a wave of H <= 16 -- a long snake, an open floor, a blocked grid and a random grid."""
    w, h = SHAPES[name][:2]
    rng = np.random.RandomState(1000 + 7 * w + h)
    snake = serpentine(w, h)
    snake[0, 0] = STAIR                                   # the walk's start: the far end is the whole walk away
    snake[0, w // 2] |= C_GOLD
    plain = open_floor(w, h)
    plain[h - 1, w - 1] = STAIR                           # a goal on two borders
    plain[0, 0] |= C_GOLD
    wall = blocked(w, h, WALLX, [(0, 0), (1, 0), (1, 1), (w - 1, h - 1), (w - 2, h - 1)])
    wall[0, 0] = STAIR
    wall[h - 1, w - 1] |= C_GOLD
    bands = diagonal_bands(w, h)
    y, x = far_corner(bands)                              # the corner with the longest walk: 4 982 moves at 160 x 48
    bands[y, x] = STAIR
    bands[h - 1 - y, w - 1 - x] |= C_GOLD
    golden = open_floor(w, h) | C_GOLD                    # gold on every cell, stairs on the top and left borders
    golden[0, w // 2] = STAIR
    golden[h // 2, 0] = STAIR
    none = blocked(w, h, NONE, [(w // 2, 0), (w // 2, 1), (0, h - 1)])
    none[0, w // 2] = STAIR
    tall = serpentine(w, h, vertical=True)
    tall[h - 1, 0] = STAIR
    tall[h // 2, w - 1 - (w - 1) % 2] |= C_GOLD
    mirror = diagonal_bands(w, h, mirrored=True)
    y, x = far_corner(mirror)
    mirror[y, x] = STAIR
    mirror[h - 1 - y, w - 1 - x] |= C_GOLD
    bare = open_floor(w, h)                               # no goal at all: every field of stairs and gold stays 0xFFFF
    out = [("serpentine", snake), ("open", plain), ("blocked wall", wall), ("random 0.55", random_words(w, h, rng, 0.55)),
           ("bands", bands), ("open gold", golden), ("blocked none", none), ("random 0.75", random_words(w, h, rng, 0.75)),
           ("serpentine vertical", tall), ("open bare", bare), ("bands mirrored", mirror), ("random 0.9", random_words(w, h, rng, 0.9))]
    return [Ref(n, g) for n, g in out]


def shape_players(name, ref, rng):
    """[(px, py)]: the cell farthest from the grid's stairs and a stairs cell (where the grid has stairs), then the four corners, the four edge midpoints,
    both sides of every word seam and a few random rg_path_ok cells."""
    w, h = SHAPES[name][:2]
    out = []
    if (ref.graph.surf == STAIR).any():
        ys, xs = np.nonzero(ref.graph.surf == STAIR)
        out += [ref.farthest()[1], (int(xs[0]), int(ys[0]))]
    out += [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2)]
    for k, seam in enumerate(s for s in (32, 64, 96, 128) if s < w):
        y = (0, h - 1, h // 2, h // 3)[k]
        out += [(seam - 1, y), (seam, y)]
    ys, xs = np.nonzero(ref.graph.ok)
    for i in rng.randint(0, len(ys), 3) if len(ys) else ():
        out.append((int(xs[i]), int(ys[i])))
    return out


def shape_cell(name, px, py, k, diagonal=None):
    """The caller's cell (y, x) of RG_GOAL_CELL.  diagonal = None: cycling through a corner, a cell outside the grid, the opposite corner, the player's own
    cell, a wall of the snake and outside again.  diagonal = 0..3: the end of one of the player's four diagonals, that one first -- on an open floor only a
    diagonal key leads there."""
    w, h = SHAPES[name][:2]
    if diagonal is not None:
        for j in range(4):
            sx, sy = ((-1, -1), (1, -1), (-1, 1), (1, 1))[(diagonal + j) % 4]
            t = min(px if sx < 0 else w - 1 - px, py if sy < 0 else h - 1 - py)
            if t > 0:
                return py + sy * t, px + sx * t
    return ((0, 0), (-1, 3), (h - 1, w - 1), (py, px), (1, w // 2), (h, w))[k % 6]


def shape_cases(name, per_grid=None):
    """[(Ref, px, py, dead, cell)] of one shape in env order: round k gives each of the twelve grids, in turn, its k-th player (per_grid = None: every
    player of every grid, the host test) or, of per_grid rounds, the farthest cell, the stairs cell and then every fifth of the rest.  Every fourth env is
    dead, another grid's in every round.  The open floors get a diagonal cell in every other round."""
    refs = shape_grids(name)
    rng = np.random.RandomState(len(name) + SHAPES[name][0])
    players = [shape_players(name, r, rng) for r in refs]
    rounds = max(len(p) for p in players) if per_grid is None else per_grid
    out = []
    for k in range(rounds):
        for gi, r in enumerate(refs):
            p = players[gi]
            px, py = p[k % len(p)] if per_grid is None or k < 2 else p[(2 + (k - 2) * 5 + gi) % len(p)]
            i = len(out)
            diagonal = (k // 2 + gi // 4) % 4 if r.name.startswith("open") and k % 2 == 0 else None
            out.append((r, px, py, int((i + k) % 4 == 3), shape_cell(name, px, py, i + k, diagonal)))
    return out


def border_pairs(name):
    """[(Ref, px, py, dead, cell)] x 4 for the shapes with H == GS: A (an open floor with stairs in the bottom row), B, B, A' (stairs in the top row), B an
    open floor without any goal -- neighbours in a wave in both orders.  Only the shift's own zeros keep A's frontier out of B."""
    w, h = SHAPES[name][:2]
    a_bottom, a_top = open_floor(w, h), open_floor(w, h)
    a_bottom[h - 1, w // 2] = STAIR
    a_top[0, w // 2] = STAIR
    a_bottom, a_top, bare = Ref("A stairs in the bottom row", a_bottom), Ref("A stairs in the top row", a_top), Ref("B no goal", open_floor(w, h))
    return [(a_bottom, 0, 0, 0, (-1, -1)), (bare, w // 2, 0, 0, (-1, -1)), (bare, w // 2, h - 1, 0, (-1, -1)), (a_top, w - 1, h - 1, 0, (-1, -1))]


# ---------------------------------------------------------------------------------------------
# the record layout and the injector
# ---------------------------------------------------------------------------------------------
def pad16(b):
    return (b + 15) & ~15


def record_offsets(rec):
    """(o_cell, o_words, H, W) of a record, from its header (the layout of include/rogue_gym_hip.h / rg_state_io.h)."""
    hd = np.frombuffer(bytes(rec[:64]), "<u4")
    H, W, nr, sec = int(hd[3] & 0xFFFF), int(hd[3] >> 16), int(hd[4]), int(hd[5])
    hw = H * W
    off = 64
    o_cell = off
    off += pad16(2 * hw) + 2 * pad16(hw)
    if sec & 1:
        off += pad16(2 * 9 * hw)
    if sec & 2:
        off += pad16(4 * 9 * H * (2 if W <= 64 else 3))
    off += 48
    if sec & 4:
        off += pad16(4 * ((nr * 2 + 1 + (nr + 3) // 4 + 3) & ~3))
    return o_cell, off, H, W


WORD_POS, WORD_FLAGS = 0, 10  # the SoA section's words, in state_prepare's order (rg_api_state.cpp): p_pos first, the flag word eleventh


def inject(hip, grids, players, dead, check_every=1):
    """Put grids[i] (u16 [H][W]), players[i] = (px, py) and dead[i] into env i of a HipBatch: its records are saved, the cell section, the position word and
    RG_FLAG_DEAD of each are replaced on the host -- every other byte stays, so room tables, RNG words and mirrors remain those of a valid state -- and
    loaded back.  Then the envs are read back (every check_every-th by rg_debug_fetch, the flag words of all) and must hold exactly what was injected.
    An injected handle must not be stepped, reset, saved again or asked for an observation: its grid does not match its room tables.  rg_path,
    rg_action_mask, rg_debug_fetch, rg_fetch_states, rg_dev_read and rg_sync read the game state only."""
    import torch
    from rogue_gym_python._rogue_gym import RgDebugState

    hd = hip.h
    L, n = hd.L, hd.n
    grids = np.ascontiguousarray(grids, np.uint16)
    dead = np.asarray(dead, np.uint32)
    assert len(grids) == n and len(players) == n and len(dead) == n
    H, W = hd.height, hd.width
    for px, py in players:
        assert 0 <= px < W and 0 <= py < H, "a player outside the grid"
    R = L.rg_state_record_bytes(hd.h)
    recs = torch.empty((n, R), dtype=torch.uint8, device="cuda:%d" % hd.device)
    hd.check(L.rg_state_save(hd.h, None, n, 0, C.c_void_p(recs.data_ptr())))
    host = np.empty((n, R), np.uint8)
    hd.check(L.rg_dev_read(hd.h, C.c_void_p(recs.data_ptr()), host.ctypes.data, host.nbytes))
    o_cell, o_words, rh, rw = record_offsets(host[0])
    assert (rh, rw) == (H, W) and grids.shape == (n, H, W) and o_cell % 2 == 0 and o_words % 4 == 0 and R % 4 == 0
    host.view(np.uint16)[:, o_cell // 2:o_cell // 2 + H * W] = grids.reshape(n, H * W)
    words = host.view(np.uint32)
    words[:, o_words // 4 + WORD_POS] = np.array([px << 8 | py for px, py in players], np.uint32)
    flag = words[:, o_words // 4 + WORD_FLAGS]
    words[:, o_words // 4 + WORD_FLAGS] = (flag & ~np.uint32(RG_FLAG_DEAD)) | (dead * np.uint32(RG_FLAG_DEAD))
    recs.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    hd.check(L.rg_state_load(hd.h, C.c_void_p(recs.data_ptr()), R, None, n, 0))
    hd.check(L.rg_sync(hd.h))
    flags = np.empty(n, np.uint32)
    hd.check(L.rg_fetch_states(hd.h, None, None, None, flags.ctypes.data))
    assert not (flags & RG_FLAG_ERR_STATE).any(), "a record was refused"
    assert np.array_equal((flags & RG_FLAG_DEAD) != 0, dead != 0), "dead bits after the load"
    for i in range(0, n, check_every):
        st, cells = RgDebugState(), np.empty((H, W), np.uint16)
        hd.check(L.rg_debug_fetch(hd.h, i, C.byref(st), cells.ctypes.data))
        assert (int(st.px), int(st.py)) == tuple(players[i]), "env %d: player %s after the load, injected %s" % (i, (st.px, st.py), players[i])
        assert np.array_equal(cells, grids[i]), "env %d: grid after the load" % i
