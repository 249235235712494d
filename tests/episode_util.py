"""Helpers shared by the episode-accounting tests: a numpy restatement of the rule (include/rogue_gym_hip.h, rg_episode_update / rg_episode_cut /
rg_scout_host) on cell words in rg_debug_fetch's layout, the call of the host entry, and the CPU engine's side of a lock-step run, computed once per
process and shared.  Plain numpy and ctypes: importable without a GPU."""
import ctypes as C

import numpy as np

import mask_util as mu

C_VISIBLE, C_DRAWN = 0x40, 0x80
DIED, TIME_LIMIT, CUT = 1, 2, 3   # RG_EP_*
SLACK = 64                        # envs of slack behind every array of the handle
REC = np.dtype([("serial", "<u4"), ("env", "<i4"), ("ret", "<f4"), ("length", "<i4"), ("depth", "<i4"), ("cause", "<u4"), ("scout", "<i4"), ("zero", "<u4")])
POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def seen_bytes(hw):
    return 16 * ((hw + 127) // 128)


def known_bits(cells):
    """u8 [SB]: the known cells of one grid as the bitmap -- rows 1 .. H-2 only, bit b of byte j = cell 8 j + b, pad bits 0."""
    cells = np.asarray(cells, np.uint16)
    h, w = cells.shape
    k = (cells & (C_VISIBLE | C_DRAWN)) != 0
    k[0] = False
    k[h - 1] = False
    bits = np.zeros(8 * seen_bytes(h * w), bool)
    bits[:h * w] = k.reshape(-1)
    return np.packbits(bits, bitorder="little")


def popcount(a):
    return int(POP8[np.asarray(a, np.uint8)].sum())


def scout_step(known, seen):
    """The bitmap step, in place on `seen`: returns the number of known cells that were not in it."""
    fresh = known & ~seen
    seen |= fresh
    return popcount(fresh)


def scout_host(lib, cells, seen):
    """rg_scout_host on one grid, in place on `seen` (u8 [SB]); raises with the library's message on a refusal."""
    cells = np.ascontiguousarray(cells, np.uint16)
    fresh = C.c_int32(-7)
    if lib.rg_scout_host(cells.ctypes.data, cells.shape[0], cells.shape[1], seen.ctypes.data, C.byref(fresh)):
        raise RuntimeError(lib.rg_last_error(None).decode())
    return fresh.value


def random_known(rng, w, h, p):
    """Random cell words whose C_VISIBLE / C_DRAWN bits are set with probability p each, rows 0 and H - 1 included."""
    import grid_util as gu
    g = gu.random_words(w, h, rng, 0.7) & ~np.uint16(C_VISIBLE | C_DRAWN)
    g |= np.where(rng.rand(h, w) < p, C_VISIBLE, 0).astype(np.uint16) | np.where(rng.rand(h, w) < p, C_DRAWN, 0).astype(np.uint16)
    g[0] |= C_DRAWN          # border rows full of bits that must not count
    g[h - 1, ::2] |= C_VISIBLE
    return g


def abA(w, h, rng):
    """Grid A, B = A with about a third of A's known cells removed and others added, and the counts the rule must pay for A, B, A in turn."""
    a = random_known(rng, w, h, 0.25)
    b = a.copy()
    known_a = (a & (C_VISIBLE | C_DRAWN)) != 0
    drop = known_a & (rng.rand(h, w) < 0.35)
    b[drop] &= ~np.uint16(C_VISIBLE | C_DRAWN)
    add = ~known_a & (rng.rand(h, w) < 0.2)
    b[add] |= C_DRAWN
    inner = np.zeros((h, w), bool)
    inner[1:h - 1] = True
    known_b = (b & (C_VISIBLE | C_DRAWN)) != 0
    return a, b, int((known_a & inner).sum()), int((known_b & ~known_a & inner).sum())


class Lanes:
    """The rule for n lanes: the arrays a handle keeps, advanced by update() / cut() from what the caller read off an engine."""

    def __init__(self, n, hw, max_steps):
        self.n, self.sb, self.max_steps = n, seen_bytes(hw), max_steps
        self.ret, self.len, self.depth, self.level, self.scout_sum = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.died, self.time_limit = np.zeros(n, bool), np.zeros(n, bool)
        self.last_return, self.last_length, self.last_depth, self.last_cause = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        self.scout, self.seen = np.zeros(n, np.float32), np.zeros((n, self.sb), np.uint8)
        self.serial, self.episodes = 0, []

    def _finish(self, e, cause):
        self.last_return[e], self.last_length[e], self.last_depth[e], self.last_cause[e] = self.ret[e], self.len[e], self.depth[e], cause
        self.episodes.append((self.serial, e, np.float32(self.ret[e]), int(self.len[e]), int(self.depth[e]), cause, int(self.scout_sum[e])))

    def _rebase(self, e, level, length, known):
        self.ret[e], self.len[e], self.depth[e], self.level[e], self.scout_sum[e] = 0, length, level, level, 0
        self.seen[e] = known
        self.scout[e] = 0

    def begin(self):
        """One update or cut call begins."""
        self.serial += 1

    def update(self, e, reward, done, level, known):
        self.ret[e] = np.float32(self.ret[e]) + np.float32(reward)   # one f32 add
        self.len[e] += 1
        tl = bool(done) and int(self.len[e]) >= self.max_steps
        self.died[e], self.time_limit[e] = bool(done) and not tl, tl
        if done:
            self._finish(e, TIME_LIMIT if tl else DIED)
            self._rebase(e, level, 0, known)
            return
        if level != self.level[e]:
            self.seen[e] = 0
            self.level[e] = level
            self.depth[e] = max(int(self.depth[e]), level)
        self.scout[e] = scout_step(known, self.seen[e])
        self.scout_sum[e] += int(self.scout[e])

    def cut(self, e, record, level, steps, known):
        if record and self.len[e] > 0:
            self._finish(e, CUT)
        self._rebase(e, level, steps, known)

    def snapshot(self):
        return {k: getattr(self, k).copy() for k in ("ret", "len", "depth", "died", "time_limit", "last_return", "last_length", "last_depth", "last_cause", "scout", "seen")}

    def records(self):
        """The finished episodes as the log delivers them: (serial, env) order."""
        out = np.zeros(len(self.episodes), REC)
        for i, r in enumerate(sorted(self.episodes, key=lambda r: (r[0], r[1]))):
            out[i] = r + (0,)
        return out


def engine_cells(o):
    return mu.cell_words(*o.grid())


def engine_level(o):
    return int(o.status_arr()[0])   # the status mirror's dungeon_level: what the device rule reads


class Run:
    """The CPU engine's side of a lock-step run: every env is stepped with react() and reset by hand when it reports is_terminal -- exactly what the
    auto-resetting step does -- so that `dead`, the step count and the level are still readable before the reset.  Per step a snapshot of the rule's arrays;
    counts for the floors the tests assert."""

    def __init__(self, cfg, seeds, table, max_steps, on_step=None):
        from parity_util import make_oracles
        n, T = len(seeds), len(table)
        self.oracles = make_oracles(cfg, seeds, max_steps=max_steps)
        h, w = self.oracles[0].h, self.oracles[0].w
        self.lanes = Lanes(n, h * w, max_steps)
        self.deaths = self.time_limits = self.descents = self.last_step_deaths = self.new_cells = 0
        self.dead_at_end = np.zeros((T, n), bool)       # the engine's own `dead` in the step that ended an episode
        self.last_step_death = np.zeros((T, n), bool)   # ... dead AND out of steps in the same step
        self.snaps = []
        for e, o in enumerate(self.oracles):            # the enable: a cut without record
            self.lanes.cut(e, False, engine_level(o), o.flags()["steps"], known_bits(engine_cells(o)))
        self.snaps.append(self.lanes.snapshot())
        for t in range(T):
            self.lanes.begin()
            for e, o in enumerate(self.oracles):
                gold0, lvl0 = int(o.status_arr()[1]), o.scalars()["level"]
                o.react(int(table[t][e]))
                f = o.flags()
                done = f["is_terminal"]
                if done:
                    out_of_steps = f["steps"] >= max_steps
                    self.dead_at_end[t, e] = f["dead"]
                    self.last_step_death[t, e] = f["dead"] and out_of_steps
                    self.deaths += int(f["dead"] and not out_of_steps)
                    self.time_limits += int(out_of_steps and not f["dead"])
                    self.last_step_deaths += int(f["dead"] and out_of_steps)
                    o.reset()
                else:
                    self.descents += int(o.scalars()["level"] > lvl0)
                reward = max(0, int(o.status_arr()[1]) - gold0)
                before = (self.lanes.seen[e].copy(), int(self.lanes.level[e])) if on_step is not None else None
                self.lanes.update(e, reward, done, engine_level(o), known_bits(engine_cells(o)))
                if not done:
                    self.new_cells += int(self.lanes.scout[e])
                if on_step is not None:
                    on_step(t, e, o, self.lanes, done, before)
            self.snaps.append(self.lanes.snapshot())

    def floors(self):
        return dict(deaths=self.deaths, time_limits=self.time_limits, descents=self.descents, last_step_deaths=self.last_step_deaths, new_cells=self.new_cells)


# The lock-step runs of the GPU test (and, on the CPU, of the host-entry test): name -> (config builder, envs, seed base, max_steps, steps, key table seed,
# key table width).  The width is the env count the run's floors were first measured with; a narrower batch plays the first columns of that table, so env i
# plays the same keys in the odd-sized GPU batches and the rare cases the measured runs hold -- a death on the last allowed step -- are in both.
def _mini(goldens):
    return dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)


def _shape(name):
    def build(goldens):
        import grid_util as gu
        return dict(gu.shape_config(name), enemies=mu.ENEMIES)
    return build


RUNS = {
    "mini60": (_mini, 135, 9000, 60, 130, 1, 136),
    "mini25": (_mini, 135, 9000, 25, 60, 1, 136),
    "80x24": (lambda goldens: dict(mu.DEFAULT_SIZE), 71, 9100, 40, 90, 1, 72),
    "97x33": (_shape("97x33"), 71, 9200, 30, 70, 3, 71),
    "33x17": (_shape("33x17"), 135, 9200, 30, 70, 3, 135),
}
_CACHE = {}


def run_setup(goldens, name, n=None):
    build, n0, seed0, max_steps, T, rs, width = RUNS[name]
    n = n0 if n is None else n
    assert n <= width
    return build(goldens), [seed0 + i for i in range(n)], np.ascontiguousarray(mu.key_table(rs, T, width)[:, :n]), max_steps


def engine_run(goldens, name):
    """The Run of a named lock-step run, computed once per process and shared (read-only)."""
    if name not in _CACHE:
        cfg, seeds, table, max_steps = run_setup(goldens, name)
        _CACHE[name] = Run(cfg, seeds, table, max_steps)
    return _CACHE[name]
