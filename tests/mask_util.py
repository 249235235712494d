"""Helpers shared by the action-mask tests: a numpy restatement of the legal-action rule (include/rogue_gym_hip.h, rg_action_mask) on the CPU oracle's
internal state, the cell-word builder, the sampling function in Python integers, and the key tables and lock-step runs the host and GPU tests share."""
import numpy as np

KEYS = b".hjklnbuy>s"  # RG_ACTION_KEYS: RogueEnv.ACTIONS in index order
RUN_A = dict(n=136, seed0=9000, max_steps=60, T=120, rs=1, auto_reset=True)       # mini + enemies 0..11
RUN_B = dict(n=72, seed0=9100, max_steps=1000, T=100, rs=1, auto_reset=True)      # 80 x 24 + enemies 0..11
RUN_C = dict(n=128, seed0=7000, max_steps=100000, T=300, rs=2, auto_reset=False)  # mini + enemies 0..11; envs die and stay dead
ENEMIES = {"enemies": list(range(12))}
DEFAULT_SIZE = {"width": 80, "height": 24, "enemies": ENEMIES}

# KeyMap::ai (input.rs:73-100): j is down, k is up; (dx, dy)
DIRS = {"h": (-1, 0), "j": (0, 1), "k": (0, -1), "l": (1, 0), "y": (-1, -1), "u": (1, -1), "b": (-1, 1), "n": (1, 1)}
S_WALLX, S_WALLY, S_STAIR, S_NONE = 2, 3, 4, 7   # Surface enum order (rogue/mod.rs:137-147)
A_HIDDEN, A_LOCKED = 0x02, 0x10                  # CellAttr bits (field.rs:107-124)
M64 = (1 << 64) - 1


def walkable(s):
    return s not in (S_WALLX, S_WALLY, S_NONE)


def judge_move(surf, attr, px, py, dx, dy):
    """Floor::can_move_impl as the player (floor.rs:169-182) -> (legal, why): why is "ok", "out" (target outside the grid), "wall", "hidden" (a walkable
    target that is hidden or locked) or "corner" (refused by the corner-cutting rule alone)."""
    h, w = surf.shape
    x, y = px + dx, py + dy
    if not (0 <= x < w and 0 <= y < h):
        return False, "out"
    if not walkable(surf[y, x]):
        return False, "wall"
    if attr[y, x] & (A_HIDDEN | A_LOCKED):
        return False, "hidden"
    if dx and dy and not (walkable(surf[py, x]) and walkable(surf[y, px])):  # (both inside the grid whenever the target is)
        return False, "corner"
    return True, "ok"


def rule(surf, attr, px, py, dead, keys=KEYS, why=None):
    """u8 [len(keys)]: the mask row of one env.  why (a dict, optional) counts the reasons of this row's move keys."""
    out = np.zeros(len(keys), np.uint8)
    for k, key in enumerate(bytes(keys)):
        c = chr(key)
        if c.lower() in DIRS:
            ok, reason = judge_move(surf, attr, px, py, *DIRS[c.lower()])
            if why is not None:
                why[reason] = why.get(reason, 0) + 1
        elif c == ">":
            ok = surf[py, px] == S_STAIR
        elif c in ".s":
            ok = True
        else:
            raise ValueError("not a key of KeyMap::ai: %r" % c)
        out[k] = 0 if dead else int(ok)
    return out


def oracle_row(o, keys=KEYS, why=None):
    surf, attr, _, _ = o.grid()
    sc = o.scalars()
    return rule(surf, attr, sc["px"], sc["py"], o.flags()["dead"], keys, why)


def cell_words(surf, attr, doors, gold):
    """u16 [H][W] in rg_debug_fetch's layout, from OracleEnv.grid(): surface | doors << 3 | attr << 4 | gold bit 11 (parity_util.compare_internal)."""
    return np.ascontiguousarray(surf.astype(np.uint16) | (doors.astype(np.uint16) << 3) | (attr.astype(np.uint16) << 4) | ((gold >= 0).astype(np.uint16) << 11))


def host_row(lib, cells, px, py, dead, keys=KEYS):
    """rg_action_mask_host on one grid; raises with the library's message on a refusal."""
    cells = np.ascontiguousarray(cells, np.uint16)
    out = np.full(max(len(keys), 1), 0xAA, np.uint8)
    if lib.rg_action_mask_host(cells.ctypes.data, cells.shape[0], cells.shape[1], int(px), int(py), int(dead), bytes(keys), len(keys), out.ctypes.data):
        raise RuntimeError(lib.rg_last_error(None).decode())
    return out[:len(keys)]


def host_row_of_oracle(lib, o, keys=KEYS):
    sc = o.scalars()
    return host_row(lib, cell_words(*o.grid()), sc["px"], sc["py"], o.flags()["dead"], keys)


def sample_reference(seed, env, draw, count):
    """rg_sample_index in Python integers."""
    z = (seed + 0x9E3779B97F4A7C15 * (env + 1) + 0xD1B54A32D192ED03 * draw) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (((z >> 32) * count) >> 32) if count else 0


def sample_of_rows(rows, keys, seed, draw):
    """What sample_dev must hold for mask rows u8 [n][n_keys]: per env the key at its (sample_reference + 1)-th set entry, keys[0] for an empty row."""
    out = np.empty(len(rows), np.uint8)
    for e, row in enumerate(rows):
        on = np.flatnonzero(row)
        out[e] = keys[on[sample_reference(seed, e, draw, len(on))]] if len(on) else keys[0]
    return out


def key_table(rs, t, n):
    """u8 [t][n] key bytes, indexed [step, env]."""
    return np.frombuffer(KEYS, np.uint8)[np.random.RandomState(rs).randint(0, 11, size=(t, n))]


def run_config(goldens, run):
    """(config, seeds, key table) of RUN_A / RUN_B / RUN_C."""
    cfg = DEFAULT_SIZE if run is RUN_B else dict(goldens["configs"]["mini"], enemies=ENEMIES)
    return cfg, [run["seed0"] + i for i in range(run["n"])], key_table(run["rs"], run["T"], run["n"])


class Stats:
    """Counts over the rows a run compared, for the floors the tests assert."""

    def __init__(self):
        self.rows = self.stairs = self.deep = 0
        self.why = {}

    def add(self, o, row):
        self.rows += 1
        self.stairs += int(row[KEYS.index(b">")])
        self.deep += int(o.scalars()["level"] >= 2)

    def __str__(self):
        return "rows %d, '>' legal %d, rows on level >= 2 %d, move keys by reason %s" % (self.rows, self.stairs, self.deep, dict(sorted(self.why.items())))


def step_oracles(oracles, keys, auto_reset):
    """One step of the table on every oracle.  Without auto-reset a dead env is stepped no further (orc_react refuses it)."""
    for o, k in zip(oracles, keys):
        if auto_reset:
            o.step_autoreset(int(k))
        elif not o.flags()["dead"]:
            o.react(int(k))


_RUNS = {}


def oracle_run(goldens, run):
    """The oracle's side of a run, computed once per process and shared (read-only): (rows u8 [T + 1][n][11] -- before every step and after the last --,
    dead bool [T + 1][n], Stats, key table)."""
    key = run["seed0"]
    if key not in _RUNS:
        from parity_util import make_oracles
        cfg, seeds, table = run_config(goldens, run)
        oracles = make_oracles(cfg, seeds, max_steps=run["max_steps"])
        rows, dead, st = np.zeros((run["T"] + 1, run["n"], len(KEYS)), np.uint8), np.zeros((run["T"] + 1, run["n"]), bool), Stats()
        for t in range(run["T"] + 1):
            for i, o in enumerate(oracles):
                rows[t, i] = oracle_row(o, why=st.why)
                dead[t, i] = o.flags()["dead"]
                st.add(o, rows[t, i])
            if t < run["T"]:
                step_oracles(oracles, table[t], run["auto_reset"])
        rows.setflags(write=False)
        dead.setflags(write=False)
        _RUNS[key] = (rows, dead, st, table)
    return _RUNS[key]
