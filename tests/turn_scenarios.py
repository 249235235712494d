"""Constructed states and key scripts for the turn (k_step), one env per scenario variant.

A generated dungeon has one monster per room, no walkable border, walks of a few dozen moves and players below level 8; the states here have what it has
not.  Each scenario says in one line what it reaches and carries the event counts (`claims`) that tests/test_turn_scenarios_host.py demands of its run
through the Shadow alone -- a scenario that does not reach its event is a failure of the scenario.  tests/test_gpu_turn_scenarios.py then plays the same
scripts on the device, key by key, against the Shadow.

Not a scenario: exp that would pass the last LEVEL_EXPS entry (0xFFFFFFFF) -- the sum overflows u32, which the reference does not survive in a checked build;
a monster or the player on a wall; a door cell outside every assigned area (Floor::with_current_room panics, floor.rs:201-229).  The pack's gold ends at
2^31 - 1, the largest value the device documents: its status mirror and the reward's gold difference are i32 (rg_state.h status, rg_kernels.hip)."""
import numpy as np

import grid_util as gu
import state_util as su

LIT = gu.C_VISIBLE | gu.C_DRAWN
KEY_OF = {(-1, 0): "h", (0, 1): "j", (0, -1): "k", (1, 0): "l", (-1, -1): "y", (1, -1): "u", (-1, 1): "b", (1, 1): "n"}


def key(dx, dy, run=False):
    k = KEY_OF[(dx, dy)]
    return k.upper() if run else k


def mon(x, y, glyph, active=True, hp=20, exp=None):
    return dict(x=x, y=y, glyph=glyph, active=active, hp=hp, exp=su.st.BUILTIN[glyph][3] if exp is None else exp)


class Scenario:
    def __init__(self, name, line, state, keys, claims=None):
        assert 20 <= len(keys) <= 60, (name, len(keys))
        self.name, self.line, self.state, self.keys, self.claims = name, line, state, keys, dict(claims or {})


class Play:
    """A scenario played on a Shadow, key by key: what the key's step must report, and the events the scenario is judged by."""

    def __init__(self, sc, cls=su.CountingShadow):
        self.sc, self.sh = sc, sc.state.shadow(cls)
        self.t, self.over = 0, False
        self.died_in_run, self.level_jump, self.hp_rose, self.rewards = False, 0, False, []
        if hasattr(self.sh, "stood"):
            self.sh.stood.add(self.sh.pos)
            self.sh.mon_stood.update(list(self.sh.active) + list(self.sh.placed))

    def step(self):
        """Play the next key (a NoOp when the script is over, or after the player's death) -> (key, reward, done)."""
        if self.over or self.t >= len(self.sc.keys):
            self.t += 1
            return ".", 0, False
        k = self.sc.keys[self.t]
        self.t += 1
        sh = self.sh
        gold0, lvl0, hp0 = sh.gold, sh.plevel, sh.hp
        grave = sh.process_action(k, None)
        self.level_jump = max(self.level_jump, sh.plevel - lvl0)
        self.hp_rose = self.hp_rose or sh.hp > hp0
        self.rewards.append(sh.gold - gold0)
        if grave:   # the episode ends here: the device resets the env, which then only gets NoOps
            self.over = True
            self.died_in_run = k.isupper()
        return k, sh.gold - gold0, bool(grave)

    def events(self):
        sh = self.sh
        ev = dict(getattr(sh, "ev", {}))
        ev.update(died=self.over, died_in_run=self.died_in_run, level_jump=self.level_jump, hp_rose=self.hp_rose, max_reward=max(self.rewards or [0]),
                  min_mon_hp=getattr(sh, "min_mon_hp", 1), gold=sh.gold, food=sh.food_left & 0xFFFFFFFF,
                  mon_x_span=(min((x for x, _ in sh.mon_stood), default=0), max((x for x, _ in sh.mon_stood), default=0)) if hasattr(sh, "mon_stood") else (0, 0))
        return ev


def border_classes(shape, cells):
    """The classes of border cells among `cells`: the four corners and the four edges."""
    w, h = su.SHAPES[shape][:2]
    out = set()
    for x, y in cells:
        ex, ey = {0: "l", w - 1: "r"}.get(x, ""), {0: "t", h - 1: "b"}.get(y, "")
        if ex or ey:
            out.add(ey + ex)
    return out


ALL_BORDER_CLASSES = {"t", "b", "l", "r", "tl", "tr", "bl", "br"}


# ---------------------------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------------------------
def lit(g):
    return (np.asarray(g, np.uint16) | LIT).astype(np.uint16)


def frame(w, h, dark=False):
    """Floor within three cells of the border, rows 0 / H - 1 and columns 0 / W - 1 included, nothing inside; a door tile (not a door of the room table) every
    sixth border cell stops a run there."""
    g = np.full((h, w), gu.NONE, np.uint16)
    g[:3] = g[-3:] = gu.FLOOR
    g[:, :3] = g[:, -3:] = gu.FLOOR
    for x in range(6, w - 3, 6):
        g[0, x] = g[h - 1, x] = gu.DOOR
    for y in range(6, h - 3, 6):
        g[y, 0] = g[y, w - 1] = gu.DOOR
    g = lit(g)
    if dark:
        g[(g & 7) == gu.FLOOR] |= gu.C_DARK
    return g


def block(w, h, x0, y0, bw, bh):
    """A floor block of bw x bh at (x0, y0), nothing else."""
    g = np.full((h, w), gu.NONE, np.uint16)
    g[y0:y0 + bh, x0:x0 + bw] = gu.FLOOR
    return lit(g)


# ---------------------------------------------------------------------------------------------
# (a) borders
# ---------------------------------------------------------------------------------------------
def borders(shape):
    w, h = su.SHAPES[shape][:2]
    out = []
    for k, (cx, cy) in enumerate(((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))):
        ix, iy = (1 if cx == 0 else -1), (1 if cy == 0 else -1)
        keys = (key(-ix, -iy, True) + key(ix, 0, True) + key(-ix, 0, True) + key(0, iy, True) + key(0, -iy, True) + key(-ix, -iy) + key(-ix, 0) + key(0, -iy) +
                key(ix, 0) + key(-ix, -iy) + key(ix, -iy) + key(ix, 0) + key(-ix, 0) + key(-ix, 0) + "s" + key(0, iy) + key(-ix, iy) + key(0, -iy) + key(ix, iy, True) +
                key(-ix, -iy, True) + key(ix, 0, True) + key(0, iy) + key(0, -iy))
        mons = [mon(cx + 9 * ix, cy, "E", hp=30), mon(cx, cy + 5 * iy, "B", hp=30), mon(w - 1 - cx, h - 1 - cy, "K", hp=30), mon(cx + 13 * ix, cy + iy, "H", hp=30)]
        out.append(Scenario("borders %s" % ("tl", "tr", "bl", "br")[k],
                            "runs and walks along both edges of a corner and into it; chasers and a bat come along the border rows and columns, one from the far corner",
                            su.State(shape, frame(w, h, dark=k % 2 == 1), (cx + 2 * ix, cy + 2 * iy), mons, hp=900, seed=100 + k), keys, {"border_part": True}))
    return out


# ---------------------------------------------------------------------------------------------
# (b) seams
# ---------------------------------------------------------------------------------------------
def seams(shape):
    w, h = su.SHAPES[shape][:2]
    out = []
    for s in (x for x in (32, 64, 96, 128) if x < w):
        for mirrored in (False, True):
            g = lit(gu.diagonal_bands(w, h, mirrored))
            walk = (g & 7) == gu.FLOOR
            y = h // 2
            # the player two cells beyond the seam on one side (the left one in the mirrored grid, or where the grid ends right behind the seam), the chaser about
            # nine cells away on the other
            on_left = mirrored or s + 2 >= w
            if on_left:
                p = (next(x for x in range(s - 3, -1, -1) if walk[y, x]), y)
                c = (next(x for x in range(min(w - 1, s + 8), s - 1, -1) if walk[y, x]), y)
            else:
                p = (next(x for x in range(s + 2, w) if walk[y, x]), y)
                c = (next(x for x in range(s - 9, -1, -1) if walk[y, x]), y)
            out.append(Scenario("seam %d %s" % (s, "mirrored" if mirrored else "bands"),
                                "a chaser crosses columns %d / %d over the bands, where only the corner rule keeps it off the diagonals" % (s - 1, s),
                                su.State(shape, g, p, [mon(c[0], c[1], "H", hp=25), mon(c[0], c[1] + (1 if walk[c[1] + 1, c[0]] else -1), "K", hp=25)], hp=600, seed=200 + s + mirrored),
                                "lhjklhkjhlssjkhlyubnlhss", {"crossed": s}))
    return out


# ---------------------------------------------------------------------------------------------
# (c) long walks
# ---------------------------------------------------------------------------------------------
def long_walks(shape, only_short=False):
    w, h = su.SHAPES[shape][:2]
    out = []
    for vertical in ((False,) if only_short else (False, True)):
        g = lit(gu.serpentine(w, h, vertical))
        probe = su.State(shape, g, (0, 0)).shadow()
        dist = probe.make_dist_map((0, 0))
        far = max((d, i) for i, d in enumerate(dist) if d != su.st.INF)
        fx, fy = far[1] % w, far[1] // w
        run = key(0, 1, True) if vertical else key(1, 0, True)
        back = key(0, -1) if vertical else key(-1, 0)
        fwd = back.translate(str.maketrans("hk", "lj"))
        if only_short or (not vertical and w > 33):
            keys = (fwd * 3 + back * 2 + fwd + "s" + back + fwd * 2 + back) * 2  # a handful of cells: every new one costs the Shadow a walk of the whole snake
        else:
            keys = (fwd + back + run + back * 3 + fwd * 2 + "s" + run + back) * 2
        out.append(Scenario("serpentine %s" % ("vertical" if vertical else "horizontal"),
                            "a chaser %d moves away follows the maps of a player who %s" % (far[0], "steps to and fro" if run not in keys else "runs a whole corridor, a turn per cell"),
                            su.State(shape, g, (0, 0), [mon(fx, fy, "K", hp=10)], hp=100, seed=300 + vertical), keys, {"far": far[0]}))
    return out


# ---------------------------------------------------------------------------------------------
# (d) stale cache
# ---------------------------------------------------------------------------------------------
def stale_cache(shape):
    w, h = su.SHAPES[shape][:2]
    ox, oy = 1, 2
    out = []
    for variant in ("one chaser", "two chasers", "locked door", "eight cells", "woken sleeper"):
        g = np.full((h, w), gu.NONE, np.uint16)
        g[oy, ox:ox + 21] = gu.FLOOR                                   # the long way round: row 0, columns 0 and 20
        g[oy:oy + 3, ox] = g[oy:oy + 3, ox + 20] = gu.FLOOR
        g[oy + 2, ox:ox + 6] = g[oy + 3, ox:ox + 5] = gu.FLOOR         # the player's side; A = (4, 2), B = (5, 2)
        g[oy + 2, ox + 7:ox + 21] = gu.FLOOR                           # the chasers' corridor
        g = lit(g)
        g[oy + 2, ox + 6] = gu.NONE | (gu.C_LOCKED if variant == "locked door" else gu.C_HIDDEN)   # the wall between them, as the generator leaves such a cell (floor.rs:92-100)
        start = (ox + 3, oy + 2)
        if variant == "woken sleeper":
            g[(g & 7) == gu.NONE] &= ~np.uint16(LIT)                    # (nothing seen but the corridors: entering the room draws its whole range)
            g[oy + 3, ox] |= gu.C_DOOR                                  # a door of the room table: stepping on it wakes the mean sleeper of its assigned area
            g[oy + 4:oy + 6, ox + 2] = gu.FLOOR | LIT                   # a pocket below the player's side: the chaser in it never leaves, a sleeper (not mean) plugs it
            mons = [mon(ox + 2, oy + 5, "F", hp=900), mon(ox + 12, oy + 2, "E", active=False, hp=30), mon(ox + 2, oy + 4, "C", active=False, hp=900)]
            keys = "ll" + "s" + "h" + "hhhh" + "j" + "k" + "llll" + "l" + "hlhlhl"
            same_area = su.room_of(shape, ox, oy + 3) == su.room_of(shape, ox + 12, oy + 2)
            claims = {"activated": 1, "stale_moves": 1} if same_area else {}
            line = "a near chaser keeps the maps short; a search opens the wall, a door wakes a far sleeper: the maps from before the opening are continued over the old walls"
        else:
            mons = [mon(ox + 16, oy + 2, "K", hp=30)] + ([mon(ox + 18, oy + 2, "H", hp=30)] if variant == "two chasers" else [])
            # to A, to B, search, back to A (the old map), nine further cells (eight: A is the oldest map and goes, B stays), back to A (rebuilt)
            keys = "ll" + "s" + "h" + "hhhh" + "j" + ("lll" + "u" if variant == "eight cells" else "llll" + "k") + "l" + "hlhlhl"
            claims = {"cache_max": 9, "evicted": 1, "stale_moves": 1}
            line = "a map cached while the wall was closed sends the chaser the long way round after a search opened it, until nine (eight) further maps evict it"
        rooms = None
        if variant == "woken sleeper":   # the door's room: not visited, lit -- entering it draws its range
            rooms = [dict(range=a, kind=0, dark=False, visited=i != su.room_of(shape, ox, oy + 3)) for i, a in enumerate(su.assigned_areas(shape))]
        out.append(Scenario("stale cache, " + variant, line, su.State(shape, g, start, mons, rooms=rooms, hp=500, seed=400 + len(variant)), keys, claims))
    return out


# ---------------------------------------------------------------------------------------------
# (e) crowds
# ---------------------------------------------------------------------------------------------
def crowds(shape):
    w, h, rx, ry = su.SHAPES[shape]
    nr = rx * ry
    out = []
    kinds = "AFKEAFHK" * 2
    # in line in a corridor one cell wide, the player at the end the BTreeMap order reaches last
    g = np.full((h, w), gu.NONE, np.uint16)
    g[3, 2:nr + 8] = gu.FLOOR
    out.append(Scenario("crowd in a row", "every slot in line: the nearest reaches the player, stays and is inserted over the one that stepped onto its cell",
                        su.State(shape, lit(g), (2 + nr, 3), [mon(2 + k, 3, kinds[k], hp=40) for k in range(nr)], hp=600, seed=500), "sss" + "h" + "ss" + "l" + "L" + "sh" + "ssHsslshsL", {"overwritten": 2}))
    g = np.full((h, w), gu.NONE, np.uint16)
    g[1:nr + 6, 5] = gu.FLOOR
    out.append(Scenario("crowd in a column", "the same along a column: the order within one x is by y",
                        su.State(shape, lit(g), (5, 1 + nr), [mon(5, 1 + k, kinds[k], hp=40) for k in reversed(range(nr))], hp=600, seed=501), "sss" + "k" + "ss" + "j" + "J" + "sk" + "ssKssjsksJ",
                        {"overwritten": 2}))
    # a ring at distance two: the run's first step brings three attackers next to the player
    cx, cy = 7, 6
    ring = [(2, 0), (2, -2), (2, 2), (0, -2), (0, 2), (-2, 0), (-2, -2), (-2, 2)][:nr]
    out.append(Scenario("ring", "dragons all around kill the player inside a run key, which goes on after the death",
                        su.State(shape, block(w, h, cx - 4, cy - 4, 9, 9), (cx, cy), [mon(cx + dx, cy + dy, "D", hp=80) for dx, dy in ring], hp=7, seed=502), "LLH" + "s" * 17, {"died_in_run": True}))
    # sleepers the player attacks
    sl = [(1, 0, "C"), (-1, 0, "I"), (0, -2, "J"), (3, 1, "L"), (-3, -1, "C"), (2, 2, "I"), (-2, 2, "B"), (0, 3, "C")][:nr]
    out.append(Scenario("sleepers", "asleep monsters are hit, wake up, and keep `damage - cur` hit points: negative, so the next hit kills",
                        su.State(shape, block(w, h, cx - 4, cy - 4, 9, 9), (cx, cy), [mon(cx + dx, cy + dy, gl, active=False, hp=45) for dx, dy, gl in sl], hp=600, seed=503),
                        "llllll" + "hhhhhh" + "ll" + "sk" + "kk" + "jj", {"activated": 2, "negative_hp": True}))
    return out


# ---------------------------------------------------------------------------------------------
# (f) player extremes
# ---------------------------------------------------------------------------------------------
def extremes(shape):
    w, h = su.SHAPES[shape][:2]
    ax, ay = w - 9, h - 7       # an arena of 7 x 5 cells in the far corner of the grid
    g = block(w, h, ax, ay, 7, 5)
    p = (ax + 3, ay + 2)
    exps = su.st.LEVEL_EXPS
    out = []
    for lvl, exp, gain in ((7, exps[6] - 1, 5000), (8, exps[7] - 1, 5000), (12, exps[11] - 1, 200000), (21, 8_000_000, 3_000_000)):
        claims = {"kills": 1, "level_jump": 3} if lvl < 21 else {"kills": 1}
        if lvl >= 8:
            claims["heal_draws"] = 1
        out.append(Scenario("level %d" % lvl, "one kill with exp just below the next entry of the table%s" % ("" if lvl < 8 else "; from level 8 on healing draws from the enemy stream"),
                            su.State(shape, g, p, [mon(p[0] + 1, p[1], "C", active=False, hp=1, exp=gain)], hp=20, hp_max=150, plevel=lvl, exp=exp, seed=600 + lvl), "llllll" + "s" * 14, claims))
    for food in (1, 2):
        out.append(Scenario("food %d" % food, "food_left reaches 0 (no healing that turn) and wraps", su.State(shape, g, p, hp=5, hp_max=12, food=food, quiet=30, seed=630 + food), "ss.hls" + "ssssss" + "hlhlhlhl", {"food_wrapped": True}))
    out.append(Scenario("hp 1", "one hit point next to an attacker", su.State(shape, g, p, [mon(p[0] - 1, p[1] - 1, "H", hp=30)], hp=1, hp_max=12, seed=640), "s" * 20, {"died": True}))
    for quiet in (17, 18):
        out.append(Scenario("quiet %d" % quiet, "a level 1 player heals when quiet reaches 19", su.State(shape, g, p, hp=5, hp_max=12, quiet=quiet, seed=650 + quiet), "ssls" + "s" * 16, {"hp_rose": True}))
    out.append(Scenario("gold", "a pickup that fills the pack to 2^31 - 1", su.State(shape, g, p, gold=[(p[0] + 1, p[1], 150), (p[0] - 2, p[1] + 1, 7)], pack_gold=2 ** 31 - 1 - 150, seed=660),
                        "lhhL" + "hlHs" * 4, {"max_reward": 150, "gold": 2 ** 31 - 1}))
    return out


def scenarios(shape):
    """The scenarios of one shape, in env order."""
    if shape == "160x48":   # the Shadow's walk of 3 840 cells per map: one scenario, a short script
        return long_walks(shape, only_short=True)
    return borders(shape) + seams(shape) + long_walks(shape) + stale_cache(shape) + crowds(shape) + extremes(shape)
