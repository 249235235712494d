"""Helpers shared by the route tests: a numpy restatement of rg_route's rule (include/rogue_gym_hip.h) -- pass / corner / known, the frontier, the two
tiers, distance, key and tier -- on cell words in rg_debug_fetch's layout, the call of the host entry, and the call of rg_route on a handle."""
from collections import deque

import numpy as np

import mask_util as mu
import path_util as pu
from path_util import DIR_KEYS, DIR_VECS, INF

GOAL_STAIRS, GOAL_GOLD, GOAL_CELL, GOAL_FRONTIER = 1, 2, 4, 8   # RG_GOAL_*
SECRETS, KNOWN = 1, 2                                           # RG_ROUTE_*
NO_TIER = 255
C_HIDDEN, C_VISIBLE, C_DRAWN, C_LOCKED, C_GOLD = 0x20, 0x40, 0x80, 0x100, 0x800
SLACK = 64


def combos(cell=True):
    """Every legal (goals, fallback, mode): all modes, every non-empty goal word and every fallback word (0 included), the frontier only under KNOWN."""
    words = [g for g in range(16) if cell or not g & GOAL_CELL]
    out = []
    for mode in range(4):
        for goals in words[1:]:
            for fb in words:
                if ((goals | fb) & GOAL_FRONTIER) and not mode & KNOWN:
                    continue
                out.append((goals, fb, mode))
    return out


class Rule:
    """The rule on one grid with the player at (px, py), for one mode."""

    def __init__(self, cells, px, py, mode):
        self.cells = np.ascontiguousarray(cells, np.uint16)
        self.h, self.w = self.cells.shape
        self.px, self.py, self.mode = px, py, mode
        c = self.cells
        self.surf = (c & 7).astype(np.uint8)
        self.walk = ~np.isin(self.surf, (mu.S_WALLX, mu.S_WALLY, mu.S_NONE))
        self.secret = (c & (C_HIDDEN | C_LOCKED)) != 0
        self.known = (c & (C_DRAWN | C_VISIBLE)) != 0
        self.known[py, px] = True
        self.K = self.known if mode & KNOWN else np.ones_like(self.known)
        self.corner = self.walk & self.K
        self.passable = self.K & np.where(self.secret, bool(mode & SECRETS), self.walk)   # a secret keeps a wall / bare surface until it is found
        unk = ~self.known
        beside = pu._shift(unk, 1, 0) | pu._shift(unk, -1, 0) | pu._shift(unk, 0, 1) | pu._shift(unk, 0, -1)
        self.frontier = self.passable & beside
        self._fields = {}

    def goal_mask(self, goals, cell=None):
        g = np.zeros((self.h, self.w), bool)
        if goals & GOAL_STAIRS:
            g |= (self.surf == mu.S_STAIR) & self.K
        if goals & GOAL_GOLD:
            gold = ((self.cells & C_GOLD) != 0) & self.K
            gold[self.py, self.px] = False
            g |= gold
        if goals & GOAL_CELL and cell is not None and 0 <= cell[0] < self.h and 0 <= cell[1] < self.w:
            g[cell[0], cell[1]] = True
        if goals & GOAL_FRONTIER:
            g |= self.frontier
        return g

    def move(self, x, y, dx, dy):
        """Is (x, y) -> (x + dx, y + dy) a move of the search graph (the source's own word aside)?"""
        tx, ty = x + dx, y + dy
        if not (0 <= tx < self.w and 0 <= ty < self.h) or not self.passable[ty, tx]:
            return False
        return not (dx and dy) or bool(self.corner[y, tx] and self.corner[ty, x])

    def field(self, goals, cell=None):
        """u16 [H][W] of one goal word; computed once per (goals, cell) and shared (read-only)."""
        key = (goals, None if cell is None or not goals & GOAL_CELL else tuple(cell))
        if key not in self._fields:
            self._fields[key] = self._search(goals, cell)
            self._fields[key].setflags(write=False)
        return self._fields[key]

    def _search(self, goals, cell):
        d = np.full((self.h, self.w), INF, np.uint16)
        gm = self.goal_mask(goals, cell)
        d[gm] = 0
        q = deque((int(y), int(x)) for y, x in zip(*np.nonzero(gm)))
        while q:
            by, bx = q.popleft()
            if not self.passable[by, bx]:
                continue
            for dx, dy in DIR_VECS:
                ax, ay = bx - dx, by - dy
                if 0 <= ax < self.w and 0 <= ay < self.h and d[ay, ax] == INF and self.passable[ay, ax] and self.move(ax, ay, dx, dy):
                    d[ay, ax] = d[by, bx] + 1
                    q.append((ay, ax))
        return d

    def answer(self, goals, fallback, dead, cell=None):
        """(field of the answering tier, distance, key byte, tier)."""
        px, py = self.px, self.py
        tier, gw = NO_TIER, goals
        for t, w in enumerate((goals, fallback)):
            if t and not w:
                break
            gw, f = w, self.field(w, cell)
            if f[py, px] != INF:
                tier = t
                break
        d = int(f[py, px])
        if dead:
            key = "."
        elif d == 0:
            key = ">" if (gw & GOAL_STAIRS) and self.surf[py, px] == mu.S_STAIR else "s" if (gw & GOAL_FRONTIER) and self.frontier[py, px] else "."
        elif d == INF:
            key = "s"
        else:
            key = "s"
            for k, (dx, dy) in zip(DIR_KEYS, DIR_VECS):
                if self.move(px, py, dx, dy) and f[py + dy, px + dx] == d - 1 and not self.secret[py + dy, px + dx]:
                    key = k
                    break
        return f, (-1 if d == INF else d), ord(key), tier


def host(lib, cells, px, py, goals, fallback=0, mode=0, dead=0, cell=(-1, -1), want=(True, True, True, True)):
    """rg_route_host on one grid -> (field u16 [H][W], distance, key byte, tier), None for an output that is not asked for; raises with the library's
    message on a refusal."""
    cells = np.ascontiguousarray(cells, np.uint16)
    h, w = cells.shape
    f = np.full((h, w), 0xAAAA, np.uint16)
    d, k, t = np.full(1, -7, np.int32), np.full(1, 0xAA, np.uint8), np.full(1, 0xAA, np.uint8)
    if lib.rg_route_host(cells.ctypes.data, h, w, int(px), int(py), int(dead), int(goals), int(fallback), int(mode), int(cell[0]), int(cell[1]),
                         f.ctypes.data if want[0] else None, d.ctypes.data if want[1] else None, k.ctypes.data if want[2] else None, t.ctypes.data if want[3] else None):
        raise RuntimeError(lib.rg_last_error(None).decode())
    return (f if want[0] else None), (int(d[0]) if want[1] else None), (int(k[0]) if want[2] else None), (int(t[0]) if want[3] else None)


def route_call(hd, goals, fallback=0, mode=0, cells=None):
    """rg_route on a raw handle into buffers pre-filled with 0xAA -> (dist i32 [n], keys u8 [n], tier u8 [n]); every byte behind the last env must keep
    its fill."""
    import torch
    n, dev = hd.n, "cuda:%d" % hd.device
    d = torch.full((n + SLACK,), 0xAAAAAAAA - (1 << 32), dtype=torch.int32, device=dev)
    k = torch.full((n + SLACK,), 0xAA, dtype=torch.uint8, device=dev)
    t = torch.full((n + SLACK,), 0xAA, dtype=torch.uint8, device=dev)
    c = None if cells is None else torch.as_tensor(np.ascontiguousarray(cells, np.int32), device=dev)
    torch.cuda.synchronize()
    hd.check(hd.L.rg_route(hd.h, goals, fallback, mode, pu.ptr(c), pu.ptr(d), pu.ptr(k), pu.ptr(t)))
    db, kb, tb = pu.read(hd, d).view(np.int32), pu.read(hd, k), pu.read(hd, t)
    assert (db[n:].view(np.uint32) == 0xAAAAAAAA).all() and (kb[n:] == 0xAA).all() and (tb[n:] == 0xAA).all(), "the pass wrote behind the last env"
    return db[:n].copy(), kb[:n].copy(), tb[:n].copy()


def host_answers(lib, grids, pos, dead, goals, fallback, mode, cells=None):
    """The host entry on every env of a fetched batch -> (dist i32 [n], keys u8 [n], tier u8 [n])."""
    n = len(grids)
    d, k, t = np.empty(n, np.int32), np.empty(n, np.uint8), np.empty(n, np.uint8)
    for e in range(n):
        _, d[e], k[e], t[e] = host(lib, grids[e], pos[e][0], pos[e][1], goals, fallback, mode, int(dead[e]), (-1, -1) if cells is None else tuple(cells[e]),
                                   want=(False, True, True, True))
    return d, k, t
