"""Helpers shared by the path tests: a numpy restatement of the shortest-path rule (include/rogue_gym_hip.h, rg_path) -- field, distance, teacher key and
the own-cell gold exclusion -- on cell words in rg_debug_fetch's layout, the call of the host entry, and the call of rg_path on a handle."""
import ctypes as C
from collections import deque

import numpy as np

import mask_util as mu

GOAL_STAIRS, GOAL_GOLD, GOAL_CELL = 1, 2, 4   # RG_GOAL_*
INF = 0xFFFF                                  # RG_PATH_UNREACHABLE
DIR_KEYS = "kjhlyubn"                         # Direction enum order: Up Down Left Right LeftUp RightUp LeftDown RightDown
DIR_VECS = [mu.DIRS[k] for k in DIR_KEYS]     # (dx, dy)
C_GOLD = 0x0800
SLACK = 64  # elements behind the last env of every output buffer of path_call: they keep their fill


def split(cells):
    """(surf u8 [H][W], attr u8 [H][W]) of cell words, as OracleEnv.grid() gives them."""
    cells = np.asarray(cells, np.uint16)
    return (cells & 7).astype(np.uint8), ((cells >> 4) & 0x3F).astype(np.uint8)


def _shift(a, dx, dy):
    """b[y, x] = a[y + dy, x + dx], False outside the grid."""
    h, w = a.shape
    b = np.zeros_like(a)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    b[yd, xd] = a[ys, xs]
    return b


class Graph:
    """The player's move graph of one grid, built once and shared by the goal sets asked of it."""

    def __init__(self, cells):
        self.cells = np.ascontiguousarray(cells, np.uint16)
        self.h, self.w = self.cells.shape
        self.surf, self.attr = split(self.cells)
        walk = ~np.isin(self.surf, (mu.S_WALLX, mu.S_WALLY, mu.S_NONE))
        self.ok = walk & ((self.attr & (mu.A_HIDDEN | mu.A_LOCKED)) == 0)
        idx = np.arange(self.h * self.w).reshape(self.h, self.w)
        src, dst = [], []
        for dx, dy in DIR_VECS:  # a move a -> a + d: the target inside and ok; a diagonal's two orthogonal neighbours walkable by surface only
            can = _shift(self.ok, dx, dy)
            if dx and dy:
                can = can & _shift(walk, dx, 0) & _shift(walk, 0, dy)
            can = can & self.ok  # (only an ok cell is given a distance as a source)
            a = idx[can]
            src.append(a)
            dst.append(a + dy * self.w + dx)
        src, dst = np.concatenate(src), np.concatenate(dst)
        order = np.argsort(dst, kind="stable")
        self._src = src[order].tolist()
        self._start = np.searchsorted(dst[order], np.arange(self.h * self.w + 1)).tolist()
        self._ok = self.ok.ravel().tolist()

    def goal_mask(self, px, py, goals, cell=None):
        g = np.zeros((self.h, self.w), bool)
        if goals & GOAL_STAIRS:
            g |= self.surf == mu.S_STAIR
        if goals & GOAL_GOLD:
            gold = (self.cells & C_GOLD) != 0
            gold[py, px] = False  # gold is taken by moving ONTO it: the gold under the player is no goal
            g |= gold
        if goals & GOAL_CELL and cell is not None and 0 <= cell[0] < self.h and 0 <= cell[1] < self.w:
            g[cell[0], cell[1]] = True
        return g

    def field(self, px, py, goals, cell=None):
        """u16 [H][W]: 0 on every goal cell, the least number of moves to one from every other ok cell that has a path, 0xFFFF elsewhere."""
        d = [INF] * (self.h * self.w)
        q = deque(np.flatnonzero(self.goal_mask(px, py, goals, cell)).tolist())
        for b in q:
            d[b] = 0
        src, start, ok = self._src, self._start, self._ok
        while q:
            b = q.popleft()
            if not ok[b]:
                continue  # nobody can step onto it: not expanded
            nd = d[b] + 1
            for a in src[start[b]:start[b + 1]]:
                if d[a] == INF:
                    d[a] = nd
                    q.append(a)
        return np.array(d, np.uint16).reshape(self.h, self.w)

    def answer(self, px, py, dead, goals, cell=None):
        """(field, distance, key byte) of the rule."""
        f = self.field(px, py, goals, cell)
        return f, dist_of(f, px, py), key_of(self.surf, self.attr, f, px, py, dead, goals)


def dist_of(field, px, py):
    return -1 if field[py, px] == INF else int(field[py, px])


def key_of(surf, attr, field, px, py, dead, goals):
    """The teacher key byte."""
    if dead:
        return ord(".")
    d = int(field[py, px])
    if d == 0:
        return ord(">") if (goals & GOAL_STAIRS) and surf[py, px] == mu.S_STAIR else ord(".")
    if d == INF:
        return ord("s")
    for k, (dx, dy) in zip(DIR_KEYS, DIR_VECS):
        if mu.judge_move(surf, attr, px, py, dx, dy)[0] and field[py + dy, px + dx] == d - 1:
            return ord(k)
    raise AssertionError("no move from (%d, %d) at distance %d lands on a cell at %d" % (px, py, d, d - 1))


def host(lib, cells, px, py, goals, dead=0, cell=(-1, -1), want=(True, True, True)):
    """rg_path_host on one grid -> (field u16 [H][W], distance, key byte), None for an output that is not asked for; raises with the library's message
    on a refusal."""
    cells = np.ascontiguousarray(cells, np.uint16)
    h, w = cells.shape
    f = np.full((h, w), 0xAAAA, np.uint16)
    d, k = np.full(1, -7, np.int32), np.full(1, 0xAA, np.uint8)
    if lib.rg_path_host(cells.ctypes.data, h, w, int(px), int(py), int(dead), int(goals), int(cell[0]), int(cell[1]), f.ctypes.data if want[0] else None,
                        d.ctypes.data if want[1] else None, k.ctypes.data if want[2] else None):
        raise RuntimeError(lib.rg_last_error(None).decode())
    return (f if want[0] else None), (int(d[0]) if want[1] else None), (int(k[0]) if want[2] else None)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def read(hd, t):
    """Host copy of device tensor `t`, byte for byte, through the handle (rg_dev_read waits for the handle's stream)."""
    out = np.empty(t.numel() * t.element_size(), np.uint8)
    hd.check(hd.L.rg_dev_read(hd.h, ptr(t), out.ctypes.data, out.nbytes))
    return out


def path_call(hd, goals, cells=None, field=True, hw=None):
    """rg_path on a raw handle into buffers pre-filled with 0xAA -> (field u16 [n][H][W] or None, dist i32 [n], keys u8 [n]); every byte behind the last
    env must keep its fill."""
    import torch
    n, dev = hd.n, "cuda:%d" % hd.device
    hw = hd.height * hd.width if hw is None else hw
    f = torch.full((n * hw + SLACK,), 0xAAAA - 0x10000, dtype=torch.int16, device=dev) if field else None
    d = torch.full((n + SLACK,), 0xAAAAAAAA - (1 << 32), dtype=torch.int32, device=dev)
    k = torch.full((n + SLACK,), 0xAA, dtype=torch.uint8, device=dev)
    c = None if cells is None else torch.as_tensor(np.ascontiguousarray(cells, np.int32), device=dev)
    torch.cuda.synchronize()
    hd.check(hd.L.rg_path(hd.h, goals, ptr(c), ptr(f), ptr(d), ptr(k)))
    fo = None
    if field:
        fb = read(hd, f).view(np.uint16)
        assert (fb[n * hw:] == 0xAAAA).all(), "the field pass wrote behind the last env"
        fo = fb[:n * hw].reshape(n, hd.height, hd.width)
    db, kb = read(hd, d).view(np.int32), read(hd, k)
    assert (db[n:].view(np.uint32) == 0xAAAAAAAA).all() and (kb[n:] == 0xAA).all(), "a pass wrote behind the last env"
    return fo, db[:n].copy(), kb[:n].copy()
