"""Helpers shared by the object-table tests: a numpy restatement of rg_objects' rule (include/rogue_gym_hip.h) -- the kinds, the walk from the player's cell
over route_util.Rule's move, the order and the counts -- on cell words in rg_debug_fetch's layout, the call of the host entry, and the call of rg_objects
on a handle.  Plain numpy and ctypes: importable without a GPU."""
from collections import deque

import numpy as np

import mask_util as mu
import path_util as pu
import route_util as ru
from path_util import DIR_VECS, INF
from route_util import KNOWN, SECRETS

STAIRS, GOLD, DOOR, FRONTIER = 1, 2, 4, 8      # RG_OBJ_*
MAX_CAP, COLS = 32, 8
S_DOOR = 5
C_GOLD = 0x800
SLACK = 64                                      # rows of the table / words-of-four of the counts behind the last env: they keep their fill
SENT16 = np.uint16(0x5A5A).view(np.int16)
SENT32 = np.uint32(0x5A5A5A5A).view(np.int32)
MODES = (0, SECRETS, KNOWN, KNOWN | SECRETS)


def kind_sets(mode):
    """The kind words the tests ask in a mode: each kind alone, all three, and -- under KNOWN -- the frontier alone and all four."""
    return (STAIRS, GOLD, DOOR, STAIRS | GOLD | DOOR) + ((FRONTIER, STAIRS | GOLD | DOOR | FRONTIER) if mode & KNOWN else ())


class Objects:
    """The rule on one grid with the player at (px, py) in one mode: `kind` u8 [H][W], every kind a cell satisfies (the frontier under KNOWN only), and
    `walk` u16 [H][W], the moves from the player's cell, 0xFFFF where the search does not come.  Computed once, shared by every kind word and cap."""

    def __init__(self, cells, px, py, dead, mode):
        r = ru.Rule(cells, px, py, mode)
        self.px, self.py, self.dead, self.mode = int(px), int(py), int(bool(dead)), mode
        gold = ((r.cells & C_GOLD) != 0)
        gold[py, px] = False                      # gold is taken by moving ONTO it
        kind = ((r.surf == mu.S_STAIR) & r.K) * np.uint8(STAIRS) | (gold & r.K) * np.uint8(GOLD) | ((r.surf == S_DOOR) & r.K) * np.uint8(DOOR)
        if mode & KNOWN:
            kind = kind | r.frontier * np.uint8(FRONTIER)
        self.kind = kind.astype(np.uint8)
        walk = np.full((r.h, r.w), INF, np.uint16)
        walk[py, px] = 0                          # the own cell starts the search whatever its word
        q = deque([(int(px), int(py))])
        while q:
            x, y = q.popleft()
            for dx, dy in DIR_VECS:
                if r.move(x, y, dx, dy) and walk[y + dy, x + dx] == INF:
                    walk[y + dy, x + dx] = walk[y, x] + 1
                    q.append((x + dx, y + dy))
        self.walk = walk

    def rows(self, kinds):
        """i16 [q][8]: every listed object in order, before any cap."""
        if self.dead:
            return np.zeros((0, COLS), np.int16)
        ys, xs = np.nonzero(((self.kind & kinds) != 0) & (self.walk != INF))   # (row-major: y, then x)
        order = np.argsort(self.walk[ys, xs], kind="stable")
        out = np.zeros((len(ys), COLS), np.int16)
        for i, j in enumerate(order):
            x, y = int(xs[j]), int(ys[j])
            dx, dy = x - self.px, y - self.py
            out[i] = (int(self.kind[y, x]) & kinds, dx, dy, int(self.walk[y, x]), x, y, max(abs(dx), abs(dy)), 0)
        return out

    def count(self, kinds):
        """i32 [4]: the qualifying cells per kind bit, reached or not."""
        if self.dead:
            return np.zeros(4, np.int32)
        return np.array([int(((self.kind & kinds & (1 << b)) != 0).sum()) for b in range(4)], np.int32)


def capped(rows, cap):
    out = np.zeros((cap, COLS), np.int16)
    k = min(cap, len(rows))
    out[:k] = rows[:k]
    return out


def host(lib, cells, px, py, dead, kinds, mode, cap, table=True, count=True):
    """rg_objects_host on one grid -> (table i16 [cap][8] or None, count i32 [4] or None); raises with the library's message on a refusal."""
    cells = np.ascontiguousarray(cells, np.uint16)
    h, w = cells.shape
    t = np.full((max(cap, 1), COLS), SENT16, np.int16) if table else None
    c = np.full(4, SENT32, np.int32) if count else None
    if lib.rg_objects_host(cells.ctypes.data, h, w, int(px), int(py), int(dead), int(kinds), int(mode), int(cap), None if t is None else t.ctypes.data,
                           None if c is None else c.ctypes.data):
        raise RuntimeError(lib.rg_last_error(None).decode())
    return t, c


def objects_call(hd, kinds, mode, cap, table=True, count=True):
    """rg_objects on a raw handle into buffers pre-filled with a sentinel -> (table i16 [n][cap][8] or None, count i32 [n][4] or None); the SLACK entries
    behind the last env of both outputs must keep their fill."""
    import torch
    n, dev = hd.n, "cuda:%d" % hd.device
    t = torch.full(((n * cap + SLACK) * COLS,), int(SENT16), dtype=torch.int16, device=dev) if table else None
    c = torch.full(((n + SLACK) * 4,), int(SENT32), dtype=torch.int32, device=dev) if count else None
    torch.cuda.synchronize()
    hd.check(hd.L.rg_objects(hd.h, int(kinds), int(mode), int(cap), pu.ptr(t), pu.ptr(c)))
    to = co = None
    if table:
        tb = pu.read(hd, t).view(np.int16)
        assert (tb[n * cap * COLS:] == SENT16).all(), "the pass wrote behind the last env's rows"
        to = tb[:n * cap * COLS].reshape(n, cap, COLS).copy()
    if count:
        cb = pu.read(hd, c).view(np.int32)
        assert (cb[n * 4:] == SENT32).all(), "the pass wrote behind the last env's counts"
        co = cb[:n * 4].reshape(n, 4).copy()
    return to, co


def host_tables(lib, grids, pos, dead, kinds, mode, cap):
    """The host entry on every env of a batch -> (table i16 [n][cap][8], count i32 [n][4])."""
    n = len(grids)
    t, c = np.empty((n, cap, COLS), np.int16), np.empty((n, 4), np.int32)
    for e in range(n):
        t[e], c[e] = host(lib, grids[e], pos[e][0], pos[e][1], int(dead[e]), kinds, mode, cap)
    return t, c
