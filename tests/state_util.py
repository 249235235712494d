"""Whole game states built from a plain description, for the turn (k_step): the injector that writes them into a handle's envs through its state records,
the Shadow (tests/shadow_turn.py) filled from the same description, and the comparison of the two after a key.

grid_util.inject replaces cells and the player's position, which is enough for the readers (rg_path, rg_action_mask).  A handle that is STEPPED needs the
whole record to be one valid state: scalars, RNG words, room tables, monsters, gold, an empty DistCache, the status section, the observation record and the
overlay positions.  The records are saved from a freshly built handle and their sections replaced, so header, fingerprint and layout stay the handle's own;
the room lattice (the assigned areas) follows from the config alone, as on the device (rg_device.h room_id_of).

Plain numpy and ctypes: importable without a GPU.  The layout mirrored here is rg_api_state.cpp (state_layout, state_prepare) and rg_state_io.h."""
import ctypes as C

import numpy as np

import grid_util as gu
import shadow_turn as st

RG_DIST_SLOTS = 9
RG_OVL_MAX = 9
SEC_DCMAP, SEC_DCWALK, SEC_OBSREC, SEC_OVL = 1, 2, 4, 8
RG_FLAG_REDRAW, RG_FLAG_HIST_DIRTY = 0x4, 0x20
MF_ALIVE, MF_ACTIVE = 1, 2
RM_DARK, RM_VISITED = 0x04, 0x08
OVL_UNKNOWN, OVL_NONE = 0x40, 0xFFFF
HUNGER_TIME = 1300                       # player.hunger_time of scenario_config (the reference's default, stated so that both sides read the same number)
# `rarelity` of the builtin monsters A..Z (character/enemies.rs:474-761): the device's monster type is the index into the table sorted by it (enemies.rs:250-261)
RARITY = dict(zip("ABCDEFGHIJKLMNOPQRSTUVWXYZ", (12, 2, 10, 25, 1, 15, 23, 4, 5, 24, 0, 9, 21, 13, 7, 18, 11, 6, 3, 16, 20, 22, 17, 19, 14, 8)))

# name -> (W, H, room_num_x, room_num_y) and the step class it reaches (rg_state.h RG_PARTIAL_MAPS, rg_kernels.hip)
SHAPES = {
    "32x16": (32, 16, 4, 2),    # k_step_w32 with the incremental mirror, 8 monster slots
    "32x20": (32, 20, 4, 2),    # k_step_w32 with more than 16 rows: whole-wave row shifts in its BFS, two envs per wave
    "33x17": (33, 17, 2, 2),    # partial maps, odd width
    "64x32": (64, 32, 2, 3),    # partial maps, two row words
    "80x24": (80, 24, 3, 3),    # partial maps, three row words, the benchmarked size
    "128x16": (128, 16, 4, 2),  # the general class
    "160x48": (160, 48, 4, 4),  # the maximum (more than RG_OVL_MAX rooms: every Redraw drawn from the tiles)
}
PARTIAL = ("33x17", "64x32", "80x24")


def scenario_config(shape, seed=1):
    """The config of a shape: the builtin monsters A..L (mask_util.ENEMIES), searches that open at once, the default pack."""
    w, h, rx, ry = SHAPES[shape]
    return {"width": w, "height": h, "seed": seed,
            "dungeon": {"style": "rogue", "room_num_x": rx, "room_num_y": ry, "min_room_size": {"x": 4, "y": 4}, "passage_unlock_rate_inv": 1, "door_unlock_rate_inv": 1},
            "enemies": {"enemies": list(range(12))}, "player": {"hunger_time": HUNGER_TIME}}


def assigned_areas(shape):
    """Room::assigned_area of every room id (rooms.rs:192-209), half-open (x0, y0, x1, y1): row 0 and, where the rooms reach it, row H - 1 belong to none."""
    w, h, rx, ry = SHAPES[shape]
    sx, sy = w // rx, h // ry
    out = []
    for cy in range(ry):
        for cx in range(rx):
            y1 = (cy + 1) * sy
            out.append((cx * sx, 1 if cy == 0 else cy * sy, (cx + 1) * sx, y1 - 1 if y1 == h else y1))
    return out


def room_of(shape, x, y):
    for i, (x0, y0, x1, y1) in enumerate(assigned_areas(shape)):
        if x0 <= x < x1 and y0 <= y < y1:
            return i
    return None


def rng_words(seed):
    """12 non-zero stream words (dungeon, item, enemy) from a seed."""
    return [int(v) | 1 for v in np.random.RandomState(seed).randint(1, 2 ** 32, 12, dtype=np.uint64)]


class State:
    """One env's game state as plain data.
    cells: u16 [H][W] in rg_state.h's word format (grid_util's constants); the gold bit is set from `gold`.
    rooms: one dict(range=(x0, y0, x1, y1), kind, dark, visited) per room id; None = every room normal, lit, visited, its range the assigned area.
    monsters: one entry per monster SLOT (at most rooms): None or dict(x, y, glyph, active, hp, exp).
    gold: [(x, y, amount)], at most rooms."""

    def __init__(self, shape, cells, pos, monsters=(), gold=(), rooms=None, hp=200, hp_max=None, plevel=1, exp=0, food=HUNGER_TIME, quiet=0, pack_gold=0,
                 dlevel=1, seed=1):
        self.shape = shape
        self.W, self.H, rx, ry = SHAPES[shape]
        self.nr = rx * ry
        self.cells = np.array(cells, np.uint16)
        assert self.cells.shape == (self.H, self.W)
        self.pos = tuple(pos)
        self.monsters = list(monsters) + [None] * (self.nr - len(monsters))
        self.gold = list(gold)
        areas = assigned_areas(shape)
        self.rooms = [dict(range=a, kind=0, dark=False, visited=True) for a in areas] if rooms is None else [dict(r) for r in rooms]
        self.hp, self.hp_max, self.plevel, self.exp, self.food, self.quiet, self.pack_gold, self.dlevel = hp, hp if hp_max is None else hp_max, plevel, exp, food, quiet, pack_gold, dlevel
        self.rng = rng_words(seed)
        for x, y, _ in self.gold:
            self.cells[y, x] |= gu.C_GOLD
        self.validate()

    def validate(self):
        """What the reference's own states always satisfy, and the turn relies on."""
        W, H = self.W, self.H
        assert len(self.monsters) == self.nr and len(self.gold) <= self.nr and len(self.rooms) == self.nr
        surf = self.cells & 7
        walk = ~np.isin(surf, (gu.WALLX, gu.WALLY, gu.NONE))
        px, py = self.pos
        assert 0 <= px < W and 0 <= py < H and walk[py, px] and not self.cells[py, px] & (gu.C_HIDDEN | gu.C_LOCKED), "the player stands on a walkable, open cell"
        seen = {self.pos}
        for m in self.monsters:
            if m is not None:
                p = (m["x"], m["y"])
                assert 0 <= p[0] < W and 0 <= p[1] < H and walk[p[1], p[0]] and p not in seen, "a monster per walkable cell, none on the player: %s" % (p,)
                assert m["glyph"] in "ABCDEFGHIJKL" and m["hp"] >= 1
                seen.add(p)
        assert ((self.cells & gu.C_GOLD) != 0).sum() == len({(x, y) for x, y, _ in self.gold}) == len(self.gold), "the gold bits are the gold table"
        for y, x in zip(*np.nonzero(self.cells & gu.C_DOOR)):   # Floor::with_current_room panics for a door cell without a room (floor.rs:201-229)
            assert room_of(self.shape, int(x), int(y)) is not None, "a door cell outside every assigned area: (%d, %d)" % (x, y)
        for r, a in zip(self.rooms, assigned_areas(self.shape)):
            x0, y0, x1, y1 = r["range"]
            assert a[0] <= x0 < x1 <= a[2] and a[1] <= y0 < y1 <= a[3], "a room lies inside its assigned area"

    # ---- the device's words ----
    def mon_word(self, m):
        if m is None:
            return 0
        order = sorted("ABCDEFGHIJKL", key=lambda g: RARITY[g])   # (a stable sort of distinct rarities)
        return (m["x"] << 8 | m["y"]) | order.index(m["glyph"]) << 16 | (MF_ALIVE | (MF_ACTIVE if m["active"] else 0)) << 24

    def room_words(self):
        rect = [x0 | y0 << 8 | x1 << 16 | y1 << 24 for x0, y0, x1, y1 in (r["range"] for r in self.rooms)]
        meta = [r["kind"] | (RM_DARK if r["dark"] else 0) | (RM_VISITED if r["visited"] else 0) for r in self.rooms]
        return rect, meta

    def status(self):
        """write_status (rg_kernels.hip; RunTime::player_status, core/src/lib.rs:345-356)."""
        hunger = HUNGER_TIME // 10
        return [self.dlevel, self.pack_gold, self.hp, self.hp_max, 16, 16, 0, self.plevel, self.exp, 2 if self.food <= hunger else (1 if self.food <= 2 * hunger else 0)]

    # ---- the Shadow of the same state ----
    def shadow(self, cls=st.Shadow):
        s = cls(self.W, self.H, HUNGER_TIME, 1, 1)
        flat = self.cells.reshape(-1)
        s.surface = [int(v) & 7 for v in flat]
        s.attr = [(int(v) >> 4) & 0x3F for v in flat]
        s.doors = {i for i, v in enumerate(flat) if int(v) & gu.C_DOOR}
        s.items = {y * self.W + x: int(a) for x, y, a in self.gold}
        s.rooms = [dict(kind=r["kind"], dark=r["dark"], visited=r["visited"], has_gold=False, range=tuple(r["range"]), assigned=a) for r, a in zip(self.rooms, assigned_areas(self.shape))]
        s.placed, s.active = {}, {}
        for m in self.monsters:
            if m is not None:
                _, _, defense, _, level = st.BUILTIN[m["glyph"]]
                (s.active if m["active"] else s.placed)[(m["x"], m["y"])] = st.Monster(m["glyph"], m["hp"], m["exp"], level, defense, bool(m["active"]))
        s.pos, s.level = self.pos, self.dlevel
        s.rng_dungeon, s.rng_enemy, s.rng_item_words = st.Rng(self.rng[0:4]), st.Rng(self.rng[8:12]), list(self.rng[4:8])
        s.hp, s.hp_max, s.exp, s.plevel, s.food_left, s.quiet, s.gold, s.dead = self.hp, self.hp_max, self.exp, self.plevel, self.food, self.quiet, self.pack_gold, False
        s.dist_cache = []
        s.mirror = st.Mirror(s, self.status())   # what fill_record puts into the record: these status words and a pending Redraw, drawn here
        return s


class CountingShadow(st.Shadow):
    """Shadow with the event counts the scenarios are judged by; the turn itself is the parent's."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ev = dict(maps=0, evicted=0, cache_max=0, overwritten=0, kills=0, heal_draws=0, stale_moves=0, activated=0)
        self.probe_stale = False   # count the moves a cached map decides otherwise than a map of the present cells would (a second BFS per move)

        self.stood, self.mon_stood, self.min_mon_hp = set(), set(), 1   # cells the player / a monster stood on after a turn; the least monster hit points seen

    def after_turn(self):
        died = super().after_turn()
        self.stood.add(self.pos)
        self.mon_stood.update(self.active)
        self.mon_stood.update(self.placed)
        for m in list(self.active.values()) + list(self.placed.values()):
            self.min_mon_hp = min(self.min_mon_hp, m.hp)
        return died

    def make_dist_map(self, origin):
        self.ev["maps"] += 1
        return super().make_dist_map(origin)

    def cached_dist_map(self, cd):
        miss, before = all(key != cd for _, key in self.dist_cache), len(self.dist_cache)
        m = super().cached_dist_map(cd)
        self.ev["evicted"] += int(miss and before == 9)
        self.ev["cache_max"] = max(self.ev["cache_max"], len(self.dist_cache))
        return m

    def move_enemy(self, cur, target, skip):
        n0 = self.ev["maps"]
        res = super().move_enemy(cur, target, skip)
        if self.probe_stale and self.ev["maps"] == n0:   # a cached map: would the map of the cells as they are now send this monster elsewhere?
            cached = next(m for m, key in self.dist_cache if key == target)
            fresh = st.Shadow.make_dist_map(self, target)
            if fresh != cached:
                keep, self.dist_cache = self.dist_cache, [(fresh, target)]
                other = st.Shadow.move_enemy(self, cur, target, skip)
                self.dist_cache = keep
                self.ev["stale_moves"] += int(other != res)
        return res

    def move_actives(self):
        n0 = len(self.active)
        out = super().move_actives()
        self.ev["overwritten"] += n0 - len(self.active)
        return out

    def activate(self, place):
        self.ev["activated"] += int(place in self.placed)
        super().activate(place)

    def level_up(self, exp):
        self.ev["kills"] += 1
        return super().level_up(exp)

    def heal(self):
        s0 = list(self.rng_enemy.s)
        out = super().heal()
        self.ev["heal_draws"] += int(self.rng_enemy.s != s0)
        return out


# ---------------------------------------------------------------------------------------------
# the record layout (rg_api_state.cpp state_layout) and the injector
# ---------------------------------------------------------------------------------------------
def record_layout(rec):
    """Offsets of a record's sections, from its header."""
    hd = np.frombuffer(bytes(rec[:64]), "<u4")
    H, W, nr, sec = int(hd[3] & 0xFFFF), int(hd[3] >> 16), int(hd[4]), int(hd[5])
    hw = H * W
    L = dict(H=H, W=W, nr=nr, sec=sec, o_cell=64)
    off = 64 + gu.pad16(2 * hw)
    L["o_screen"] = off
    off += gu.pad16(hw)
    L["o_hist"] = off
    off += gu.pad16(hw)
    for name, bit, size in (("dcmap", SEC_DCMAP, 2 * RG_DIST_SLOTS * hw), ("dcwalk", SEC_DCWALK, 4 * RG_DIST_SLOTS * H * (2 if W <= 64 else 3))):
        L["o_" + name], L["b_" + name] = off, size if sec & bit else 0
        off += gu.pad16(L["b_" + name])
    L["o_status"] = off
    off += 48
    L["o_obsrec"], L["b_obsrec"] = off, 4 * ((nr * 2 + 1 + (nr + 3) // 4 + 3) & ~3) if sec & SEC_OBSREC else 0
    off += gu.pad16(L["b_obsrec"])
    L["o_words"] = off
    L["n_words"] = 13 + 12 + 1 + RG_DIST_SLOTS + 4 + 7 * nr + (nr + 1 if sec & SEC_OVL else 0)
    return L


# the SoA section's words in state_prepare's order (rg_api_state.cpp)
W_POS, W_HP, W_HPMAX, W_LVL, W_EXP, W_FOOD, W_QUIET, W_GOLD, W_DLEVEL, W_STEPS, W_FLAGS, W_REWARD, W_DONE, W_RNG, W_MONCNT, W_DCKEY = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 25, 26
W_DCHEAD, W_ROOMS = W_DCKEY + RG_DIST_SLOTS, W_DCKEY + RG_DIST_SLOTS + 4   # dc_head, dc_len, dc_part, dc_own; then 7 tables of nr words and the overlay positions


def fill_record(rec, s):
    """Replace the sections of one saved record (u8 [R], writable) by the state `s`."""
    L = record_layout(rec)
    H, W, nr = L["H"], L["W"], L["nr"]
    assert (H, W, nr) == (s.H, s.W, s.nr), "the record is of another shape"
    rec[L["o_cell"]:L["o_cell"] + 2 * H * W] = s.cells.reshape(-1).view(np.uint8)
    for name in ("dcmap", "dcwalk"):   # DistCache empty: no map, no saved mask
        rec[L["o_" + name]:L["o_" + name] + L["b_" + name]] = 0
    rec[L["o_status"]:L["o_status"] + 40] = np.array(s.status(), np.int64).astype(np.uint32).view(np.uint8)
    mons = [s.mon_word(m) for m in s.monsters]
    rect, meta = s.room_words()
    pos = s.pos[0] << 8 | s.pos[1]
    if L["b_obsrec"]:   # rg_obs.hip ObsTabs: nr monster words, the player's position, nr room rects, the room metas one byte each
        o = np.zeros(L["b_obsrec"] // 4, np.uint32)
        o[:nr], o[nr], o[nr + 1:2 * nr + 1] = mons, pos, rect
        o[2 * nr + 1:].view(np.uint8)[:nr] = meta
        rec[L["o_obsrec"]:L["o_obsrec"] + L["b_obsrec"]] = o.view(np.uint8)
    w = np.zeros(L["n_words"], np.uint32)
    w[W_POS:W_DLEVEL + 1] = [pos, s.hp, s.hp_max, s.plevel, s.exp, s.food, s.quiet, s.pack_gold, s.dlevel]
    w[W_FLAGS] = RG_FLAG_REDRAW | RG_FLAG_HIST_DIRTY   # mirrors drawn from the tiles, the history plane with them
    w[W_RNG:W_RNG + 12] = s.rng
    alive = [m for m in s.monsters if m is not None]
    w[W_MONCNT] = len(alive) | sum(1 for m in alive if m["active"]) << 8
    t = W_ROOMS
    gold = list(s.gold) + [None] * (nr - len(s.gold))
    for table in (rect, meta, mons, [m["hp"] if m else 0 for m in s.monsters], [m["exp"] if m else 0 for m in s.monsters],
                  [(g[0] << 8 | g[1]) | 0x10000 if g else 0 for g in gold], [g[2] if g else 0 for g in gold]):
        w[t:t + nr] = table
        t += nr
    if L["sec"] & SEC_OVL:   # where the overlays stand, how they show unknown (the generator's copy-out, rg_kernels.hip gen_service)
        w[t:t + nr] = [(v & 0xFFFF) | OVL_UNKNOWN if v else OVL_NONE for v in mons]
        w[t + nr] = pos | OVL_UNKNOWN
    rec[L["o_words"]:L["o_words"] + 4 * L["n_words"]] = w.view(np.uint8)


def save_records(hd):
    """rg_state_save of every env of a _Handle -> (torch u8 [n][R] on the device, numpy copy)."""
    import torch

    R = hd.L.rg_state_record_bytes(hd.h)
    recs = torch.empty((hd.n, R), dtype=torch.uint8, device="cuda:%d" % hd.device)
    hd.check(hd.L.rg_state_save(hd.h, None, hd.n, 0, C.c_void_p(recs.data_ptr())))
    host = np.empty((hd.n, R), np.uint8)
    hd.check(hd.L.rg_dev_read(hd.h, C.c_void_p(recs.data_ptr()), host.ctypes.data, host.nbytes))
    return recs, host


def build_records(hd, states):
    """Records of `states` (one per env of the _Handle) made from the handle's own saved records."""
    assert len(states) == hd.n
    _, host = save_records(hd)
    for i, s in enumerate(states):
        fill_record(host[i], s)
    return host


def load_records(hd, host):
    import torch

    recs = torch.from_numpy(host).to("cuda:%d" % hd.device)
    torch.cuda.synchronize()
    hd.check(hd.L.rg_state_load(hd.h, C.c_void_p(recs.data_ptr()), host.shape[1], None, hd.n, 0))
    hd.check(hd.L.rg_sync(hd.h))
    flags = np.empty(hd.n, np.uint32)
    hd.check(hd.L.rg_fetch_states(hd.h, None, None, None, flags.ctypes.data))
    assert not (flags & gu.RG_FLAG_ERR_STATE).any(), "a record was refused"


def fetched(hd, i):
    """rg_debug_fetch of env i as plain data, in the form `expected` gives for a Shadow."""
    d, cells = hd.debug_state(i)
    return dict(pos=(d.px, d.py), level=d.dungeon_level, hp=d.hp, hp_max=d.hp_max, exp=d.exp, plevel=d.player_level, food_left=d.food_left, quiet=d.quiet, gold=d.pack_gold,
                rng_dungeon=list(d.rng[0:4]), rng_item=list(d.rng[4:8]), rng_enemy=list(d.rng[8:12]),
                monsters=[(d.mon_x[k], d.mon_y[k], chr(65 + d.mon_type[k]), d.mon_active[k], d.mon_hp[k], d.mon_exp[k]) for k in range(d.n_monsters)],
                gold_table=sorted((d.gold_x[k], d.gold_y[k], d.gold_amount[k]) for k in range(d.n_gold)),
                visited=[bool(d.room_meta[k] & RM_VISITED) for k in range(d.n_rooms)], rects=[int(d.room_rect[k]) for k in range(d.n_rooms)],
                surface=(cells & 7).reshape(-1).tolist(), door=((cells >> 3) & 1).reshape(-1).tolist(), attr=((cells >> 4) & 0x3F).reshape(-1).tolist(),
                gold_bit=((cells >> 11) & 1).reshape(-1).tolist()), int(d.steps)


def expected(sh):
    """The same of a Shadow."""
    W = sh.W
    n = W * sh.H
    snap = sh.snapshot()
    return dict(pos=snap["pos"], level=snap["level"], hp=snap["hp"], hp_max=snap["hp_max"], exp=snap["exp"], plevel=snap["plevel"], food_left=snap["food_left"], quiet=snap["quiet"],
                gold=snap["gold"], rng_dungeon=snap["rng_dungeon"], rng_item=list(sh.rng_item_words), rng_enemy=snap["rng_enemy"], monsters=snap["monsters"],
                gold_table=sorted((i % W, i // W, a) for i, a in sh.items.items()), visited=[bool(r["visited"]) for r in sh.rooms],
                rects=[x0 | y0 << 8 | x1 << 16 | y1 << 24 for x0, y0, x1, y1 in (r["range"] for r in sh.rooms)],
                surface=list(sh.surface), door=[int(i in sh.doors) for i in range(n)], attr=list(sh.attr), gold_bit=[int(i in sh.items) for i in range(n)])


def differences(got, want):
    """The fields that differ, cells as (x, y, got, want) of the first few."""
    out = {}
    for k in want:
        if got[k] != want[k]:
            out[k] = (got[k], want[k]) if k not in ("surface", "door", "attr", "gold_bit") else [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:6]
    return out


def inject(hd, states):
    """Load `states` into the envs of a _Handle and check what the issue asks: no record refused, and rg_debug_fetch of every env gives back the description."""
    load_records(hd, build_records(hd, states))
    for i, s in enumerate(states):
        got, steps = fetched(hd, i)
        diff = differences(got, expected(s.shadow()))
        assert not diff and steps == 0, "env %d after the load: %s" % (i, diff)
