"""Helpers shared by the monster-table tests: a numpy restatement of the rule (include/rogue_gym_hip.h, rg_monsters) on rg_debug_fetch's / the CPU engine's
layouts, written from RunTime::draw_screen and Floor::in_same_room and not from csrc/rg_monsters.h; the call of the host entry; the feeds that turn an engine
or an rg_debug_fetch result into its arguments; and the injector for the monster words of a state record.  Plain numpy and ctypes: importable without a GPU."""
import ctypes as C

import numpy as np

import mask_util as mu

C_VISIBLE, C_DRAWN, C_GOLD = 0x40, 0x80, 0x800
SHOWN, ALL = 0, 1                      # RG_MON_*
MODES = (("shown", SHOWN), ("all", ALL))
MAX_CAP, COLS = 16, 8
MF_ALIVE, MF_ACTIVE = 1, 2
MOVE_KEYS = "hjklnbuy"                 # RG_ACTION_KEYS[1:9]: bit i of the attack mask
SENTINEL16, SENTINEL32 = 0x5A5A, 0x5A5A5A5A
SENT16 = np.uint16(SENTINEL16).view(np.int16)
SENT32 = np.uint32(SENTINEL32).view(np.int32)


class Feed:
    """One env as the rule sees it: cells u16 [H][W], the player, dead, the monsters as arrays in rg_debug_state's layout (type = tile - 'A') plus the slot
    each answers in column 7, and the rooms: packed rects, metas, the room grid and the assigned areas (half-open x0, y0, x1, y1)."""

    def __init__(self, cells, px, py, dead, mx, my, mtype, mactive, mhp, rnx, rny, rect, meta, assigned=None, slots=None, alive=None):
        self.cells = np.ascontiguousarray(cells, np.uint16)
        self.px, self.py, self.dead = int(px), int(py), int(bool(dead))
        self.mx, self.my, self.mtype, self.mactive, self.mhp = (np.ascontiguousarray(a, np.int32) for a in (mx, my, mtype, mactive, mhp))
        self.alive = None if alive is None else np.ascontiguousarray(alive, np.int32)
        self.rnx, self.rny = int(rnx), int(rny)
        self.rect, self.meta = np.ascontiguousarray(rect, np.uint32), np.ascontiguousarray(meta, np.int32)
        h, w = self.cells.shape
        self.assigned = assigned_areas(w, h, self.rnx, self.rny) if assigned is None else assigned
        self.slots = np.arange(len(self.mx)) if slots is None else np.asarray(slots)
        self.ptrs = None   # host_call's argument prefix


def assigned_areas(w, h, rnx, rny):
    """Room::assigned_area of every room id (rooms.rs:192-209): the grid cut into rnx x rny areas of (w // rnx) x (h // rny), without row 0 and the last row."""
    sx, sy = w // rnx, h // rny
    out = []
    for i in range(rnx * rny):
        cx, cy = i % rnx, i // rnx
        y0, y1 = (1 if cy == 0 else cy * sy), (cy + 1) * sy
        out.append((cx * sx, y0, cx * sx + sx, y1 - 1 if y1 == h else y1))
    return out


def _inside(r, x, y):
    return r[0] <= x < r[2] and r[1] <= y < r[3]


def _room_of(f, x, y):
    for i, a in enumerate(f.assigned):   # Floor::cd_to_room_id: the first area that holds the cell
        if _inside(a, x, y):
            return i
    return -1


def same_room(f, ax, ay, bx, by):
    """Floor::in_same_room (floor.rs:381-393)."""
    i = _room_of(f, ax, ay)
    if i < 0 or _room_of(f, bx, by) != i:
        return False
    if int(f.meta[i]) & 3 == 2:
        return True
    r = int(f.rect[i])
    rect = (r & 0xFF, (r >> 8) & 0xFF, (r >> 16) & 0xFF, r >> 24)
    return _inside(rect, ax, ay) == _inside(rect, bx, by)


def drawn_letter(f, k, but_for_gold=False):
    """What RunTime::draw_screen puts on the cell of monster k, in its own order: nothing outside rows 1 .. H-2 or on a cell that is neither visible nor
    drawn; the player; gold; the monster's letter when it is near or in the player's room -- True iff that is the letter.  but_for_gold: as if the cell
    held no gold."""
    h, w = f.cells.shape
    x, y = int(f.mx[k]), int(f.my[k])
    if not 1 <= y <= h - 2:
        return False
    c = int(f.cells[y, x])
    if not c & (C_VISIBLE | C_DRAWN):
        return False
    if (x, y) == (f.px, f.py):
        return False
    if c & C_GOLD and not but_for_gold:
        return False
    dx, dy = f.px - x, f.py - y
    return dx * dx + dy * dy <= 2 or same_room(f, f.px, f.py, x, y)


def rule_list(f, mode):
    """(rows i16 [q][8] of every qualifier in order, threat i32 [4], monsters that only the gold on their cell hides) -- the whole list, before any cap."""
    rows, threat, under_gold = [], [0, -1, 0, 0], 0
    if f.dead:
        return np.zeros((0, COLS), np.int16), np.array(threat, np.int32), 0
    for k in range(len(f.mx)):
        if f.alive is not None and not f.alive[k]:
            continue
        x, y = int(f.mx[k]), int(f.my[k])
        dx, dy = x - f.px, y - f.py
        cheb, shown = max(abs(dx), abs(dy)), drawn_letter(f, k)
        if not shown and drawn_letter(f, k, but_for_gold=True):
            under_gold += 1
        if shown:
            threat[1] = cheb if threat[1] < 0 else min(threat[1], cheb)
            if cheb == 1:
                threat[0] += 1
                key = [c for c, d in mu.DIRS.items() if d == (dx, dy)][0]
                threat[2] |= 1 << MOVE_KEYS.index(key)
        if shown or mode == ALL:
            threat[3] += 1
            full = mode == ALL
            rows.append(((cheb, dx * dx + dy * dy, x << 8 | y), [ord("A") + int(f.mtype[k]), dx, dy, cheb, int(shown), int(bool(f.mactive[k])) if full else 0,
                                                               max(min(int(f.mhp[k]), 32767), -32768) if full else 0, int(f.slots[k]) if full else 0]))
    rows.sort(key=lambda r: r[0])
    return np.array([r[1] for r in rows], np.int16).reshape(-1, COLS), np.array(threat, np.int32), under_gold


def capped(rows, cap):
    out = np.zeros((cap, COLS), np.int16)
    k = min(cap, len(rows))
    out[:k] = rows[:k]
    return out


def host_call(lib, f, mode, cap, table=True, threat=True):
    """rg_monsters_host on one Feed -> (table i16 [cap][8] or None, threat i32 [4] or None); raises with the library's message on a refusal."""
    t = np.full((max(cap, 1), COLS), SENT16, np.int16) if table else None
    th = np.full(4, SENT32, np.int32) if threat else None
    h, w = f.cells.shape
    if f.ptrs is None:   # (the addresses of a Feed's arrays, taken once: a lock-step run calls this a hundred thousand times)
        p = lambda a: None if a is None or len(a) == 0 else a.ctypes.data  # noqa: E731
        f.ptrs = (f.cells.ctypes.data, h, w, f.px, f.py, f.dead, len(f.mx), p(f.mx), p(f.my), p(f.mtype), p(f.mactive), p(f.mhp), p(f.alive), f.rnx, f.rny, f.rect.ctypes.data,
                  f.meta.ctypes.data)
    rc = lib.rg_monsters_host(*f.ptrs, mode, cap, None if t is None else t.ctypes.data, None if th is None else th.ctypes.data)
    if rc:
        raise RuntimeError(lib.rg_last_error(None).decode())
    return t, th


def room_grid(cfg):
    d = cfg.get("dungeon", {})
    return int(d.get("room_num_x", 3)), int(d.get("room_num_y", 3))


_ORC_BUF = {}


def feed_of_oracle(o, cfg):
    """The CPU engine's state as a Feed: orc_grid, orc_monsters, orc_rooms, orc_scalars; the assigned areas are the engine's own.  (The engine's calls go
    through buffers kept here: OracleEnv.monsters() / rooms() build 512-entry buffers per call, which a lock-step run cannot afford.)"""
    from oracle.pyoracle import OrcMonster
    rnx, rny = room_grid(cfg)
    nr = rnx * rny
    if nr not in _ORC_BUF:
        _ORC_BUF[nr] = ((OrcMonster * (2 * nr + 2))(), np.zeros(12 * nr, np.int32))
    mbuf, rbuf = _ORC_BUF[nr]
    sc = o.scalars()
    mons = mbuf[:o._L.orc_monsters(o._e, mbuf, len(mbuf))]
    assert o._L.orc_rooms(o._e, rbuf.ctypes.data, nr) == nr
    q = rbuf.reshape(nr, 12)
    rect = q[:, 4].astype(np.uint32) | q[:, 5].astype(np.uint32) << 8 | q[:, 6].astype(np.uint32) << 16 | q[:, 7].astype(np.uint32) << 24
    meta = q[:, 0] | q[:, 1] << 2 | q[:, 2] << 3 | q[:, 3] << 4
    return Feed(mu.cell_words(*o.grid()), sc["px"], sc["py"], o.flags()["dead"], [m.x for m in mons], [m.y for m in mons], [m.type for m in mons],
                [m.active for m in mons], [m.hp for m in mons], rnx, rny, rect, meta, assigned=[tuple(int(v) for v in r[8:12]) for r in q])


def feed_of_debug(d, cells, dead, rnx, rny, slots=None):
    """An rg_debug_fetch result as a Feed: the arrays go in as they are."""
    n = d.n_monsters
    assert d.n_rooms == rnx * rny
    a = lambda v: np.ctypeslib.as_array(v)[:n].copy()  # noqa: E731
    return Feed(cells, d.px, d.py, dead, a(d.mon_x), a(d.mon_y), a(d.mon_type), a(d.mon_active), a(d.mon_hp), rnx, rny,
                np.ctypeslib.as_array(d.room_rect)[:d.n_rooms].copy(), np.ctypeslib.as_array(d.room_meta)[:d.n_rooms].copy(), slots=slots)


def letters_on(screen):
    """{(x, y): letter byte} of the monster letters a screen mirror carries."""
    ys, xs = np.nonzero((screen >= ord("A")) & (screen <= ord("Z")))
    return {(int(x), int(y)): int(screen[y, x]) for y, x in zip(ys, xs)}


def listed(f, rows):
    """{(x, y): tile} of table rows."""
    return {(f.px + int(r[1]), f.py + int(r[2])): int(r[0]) for r in rows if r[0]}


# ---------------------------------------------------------------------------------------------
# the monster words of a state record (the SoA section's words in state_prepare's order, rg_api_state.cpp): 13 scalars, 12 RNG words, mon_cnt, 9 dist-cache
# keys, dc_head, dc_len, dc_part, dc_own, then per room: rect, meta, mon_w0, mon_hp, mon_exp, gold_pos, gold_amt
# ---------------------------------------------------------------------------------------------
WORD_MON_CNT = 25
WORD_ROOMS = 39


def word_w0(nr, s):
    return WORD_ROOMS + 2 * nr + s


def word_hp(nr, s):
    return WORD_ROOMS + 3 * nr + s


def pack_w0(x, y, kind, alive=True, active=False):
    return (x << 8 | y) | kind << 16 | ((MF_ALIVE if alive else 0) | (MF_ACTIVE if active else 0)) << 24


def inject_monsters(hip, w0, hp, rect=None, meta=None):
    """Replace the monster words of every env of a HipBatch through its state records: w0 u32 [n][rooms] (pack_w0), hp i32 [n][rooms]; mon_cnt follows them.
    rect u32 [n][rooms] (x0 | y0 << 8 | x1 << 16 | y1 << 24) and meta [n][rooms] (RM_*: kind in bits 0..1) replace the room words likewise when given.
    Everything else stays (call grid_util.inject first for cells, player and the dead bit).  As there: such a handle is only read, never stepped."""
    import torch
    import grid_util as gu

    hd = hip.h
    L, n = hd.L, hd.n
    w0, hp = np.asarray(w0, np.uint32), np.asarray(hp, np.int32)
    nr = w0.shape[1]
    R = L.rg_state_record_bytes(hd.h)
    recs = torch.empty((n, R), dtype=torch.uint8, device="cuda:%d" % hd.device)
    hd.check(L.rg_state_save(hd.h, None, n, 0, C.c_void_p(recs.data_ptr())))
    host = np.empty((n, R), np.uint8)
    hd.check(L.rg_dev_read(hd.h, C.c_void_p(recs.data_ptr()), host.ctypes.data, host.nbytes))
    hdr = np.frombuffer(bytes(host[0, :64]), "<u4")
    assert int(hdr[4]) == nr, "the record's room count"
    o_words = gu.record_offsets(host[0])[1] // 4
    words = host.view(np.uint32)
    words[:, o_words + word_w0(nr, 0):o_words + word_w0(nr, 0) + nr] = w0
    words[:, o_words + word_hp(nr, 0):o_words + word_hp(nr, 0) + nr] = hp.view(np.uint32)
    if rect is not None:
        words[:, o_words + WORD_ROOMS:o_words + WORD_ROOMS + nr] = np.asarray(rect, np.uint32)
    if meta is not None:
        words[:, o_words + WORD_ROOMS + nr:o_words + WORD_ROOMS + 2 * nr] = np.asarray(meta, np.uint32)
    alive, act = ((w0 >> 24) & MF_ALIVE) != 0, ((w0 >> 24) & MF_ACTIVE) != 0
    words[:, o_words + WORD_MON_CNT] = (alive.sum(1) | (alive & act).sum(1) << 8).astype(np.uint32)
    recs.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    hd.check(L.rg_state_load(hd.h, C.c_void_p(recs.data_ptr()), R, None, n, 0))
    hd.check(L.rg_sync(hd.h))
    flags = np.empty(n, np.uint32)
    hd.check(L.rg_fetch_states(hd.h, None, None, None, flags.ctypes.data))
    assert not (flags & gu.RG_FLAG_ERR_STATE).any(), "a record was refused"


def record_monster_words(hip):
    """(p_pos u32 [n], w0 u32 [n][rooms], hp i32 [n][rooms]) of every env, read from its state records: the device's own slots."""
    import torch
    import grid_util as gu

    hd = hip.h
    L, n = hd.L, hd.n
    R = L.rg_state_record_bytes(hd.h)
    recs = torch.empty((n, R), dtype=torch.uint8, device="cuda:%d" % hd.device)
    hd.check(L.rg_state_save(hd.h, None, n, 0, C.c_void_p(recs.data_ptr())))
    host = np.empty((n, R), np.uint8)
    hd.check(L.rg_dev_read(hd.h, C.c_void_p(recs.data_ptr()), host.ctypes.data, host.nbytes))
    nr = int(np.frombuffer(bytes(host[0, :64]), "<u4")[4])
    o_words = gu.record_offsets(host[0])[1] // 4
    words = host.view(np.uint32)
    return words[:, o_words].copy(), words[:, o_words + word_w0(nr, 0):o_words + word_w0(nr, 0) + nr].copy(), words[:, o_words + word_hp(nr, 0):o_words + word_hp(nr, 0) + nr].view(np.int32).copy()
