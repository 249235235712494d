"""Constructed states and key scripts for what Python SEES of the turn: the screen, history and status mirrors and every observation pass that draws them.

tests/turn_scenarios.py pins the game state after every key; here the states are built for RunTime::draw_screen and the "who redraws when" rule (the Shadow's
draw_screen / Mirror, tests/shadow_turn.py): the same-room rule with the player outside a room's rect, the player > gold > monster priority, rows 0 and H - 1
that are never drawn, mirrors that lag the state for many keys, and monsters that change between shown and hidden far from the player.  Same form as the turn
scenarios: one line, a state, 20 to 60 keys, and `claims` -- here name -> predicate over the scenario's Trace -- that tests/test_draw_scenarios_host.py demands
of the run through the Shadow alone.  tests/test_gpu_draw_scenarios.py then plays them, with the turn scenarios, through every observation path of the device.

Everything stands in assigned area 0 (and its right and lower neighbours), which is at least 8 columns by rows 1 .. 7 on every shape.  Sleepers are of the kinds
that are not MEAN (B C I J), or stand where no door of their area is stepped on: nothing wakes them, so most scenarios cost the Shadow no dist map -- 160x48
runs the whole set.  No 'L': it is the last symbol of scenario_config, which PlayerState::symbol_image refuses like a 'Z' (python/src/lib.rs:96-102, symbols - 1)."""
import numpy as np

import grid_util as gu
import state_util as su
import turn_scenarios as ts
from turn_scenarios import LIT, Scenario, mon

DRAWN = gu.C_DRAWN


class Frame:
    """What stands after one key: the Mirror (stale by rule) and a fresh draw / status of the state."""

    def __init__(self, key, sh, reactions):
        H, W = sh.H, sh.W
        self.key, self.reactions, self.pos = key, list(reactions), sh.pos
        self.screen, self.hist, self.status = sh.mirror.screen.reshape(H, W).copy(), sh.mirror.hist.reshape(H, W).copy(), list(sh.mirror.status)
        self.fresh, self.fresh_status = sh.draw_screen().reshape(H, W), sh.status()
        self.monsters = {p: m.glyph for p, m in list(sh.placed.items()) + list(sh.active.items())}
        self.stale_screen, self.stale_status = not np.array_equal(self.screen, self.fresh), self.status != self.fresh_status

    def at(self, x, y):
        return chr(self.screen[y, x])


class Trace:
    """A scenario played on a Shadow with its Mirror, key by key.  frames[0] is the loaded state (the record's pending Redraw drawn); a scenario whose Shadow died
    stops at its death key: from there on the env holds another episode."""

    def __init__(self, sc, cls=su.CountingShadow):
        self.sc, self.play = sc, ts.Play(sc, cls)
        sh = self.play.sh
        self.frames = [Frame(None, sh, [su.st.REDRAW])]
        self.died_at = None

    def step(self):
        """The next key -> (key, Frame or None when the scenario is out of the comparison)."""
        p = self.play
        was_over = p.over
        k, _, _ = p.step()
        if was_over:
            return k, None
        if p.over:
            self.died_at = p.t - 1
            return k, None
        if p.t <= len(self.sc.keys):
            p.sh.mirror.react(p.sh)
            self.frames.append(Frame(k, p.sh, p.sh.reactions))
        else:   # a NoOp behind the script's end (the batch's longest script is still running): no reaction
            self.frames.append(Frame(k, p.sh, []))
        return k, self.frames[-1]

    def run(self):
        while self.play.t < len(self.sc.keys):
            self.step()
        return self


def play(sc, cls=su.CountingShadow):
    return Trace(sc, cls).run()


def pad(keys, filler="s."):
    while len(keys) < 20:
        keys += filler
    return keys


def area(shape):
    """(sx, sy): assigned area 0 is columns 0 .. sx - 1, rows 1 .. sy - 1; area 1 begins at column sx, the area below at row sy."""
    w, h, rx, ry = su.SHAPES[shape]
    return w // rx, h // ry


def rooms_with(shape, first):
    return [dict(first) if i == 0 else dict(range=a, kind=0, dark=False, visited=True) for i, a in enumerate(su.assigned_areas(shape))]


def chunks(items, n):
    return [items[i:i + n] for i in range(0, len(items), n)]


# ---------------------------------------------------------------------------------------------
# (a) the same-room rule
# ---------------------------------------------------------------------------------------------
RECT = (3, 2, 8, 7)   # the room's range: walls on columns 3 / 7 and rows 2 / 6, the door in the west wall at (3, 4)


def same_room(shape):
    w, h = su.SHAPES[shape][:2]
    nr = su.SHAPES[shape][2] * su.SHAPES[shape][3]
    sx, sy = area(shape)
    out = []
    for variant in ("lit room", "empty room", "dark room"):
        g = np.full((h, w), gu.NONE, np.uint16)
        x0, y0, x1, y1 = RECT
        g[y0, x0:x1] = g[y1 - 1, x0:x1] = gu.WALLX
        g[y0 + 1:y1 - 1, x0] = g[y0 + 1:y1 - 1, x1 - 1] = gu.WALLY
        g[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = gu.FLOOR | (gu.C_DARK if variant == "dark room" else 0)
        g[4, 3] = gu.DOOR | gu.C_DOOR
        g[1:sy + 3, 1] = gu.PASSAGE        # the passage outside the rect, on into the area below
        g[4, 2] = g[sy, 2] = gu.PASSAGE
        g[g != gu.NONE] |= LIT
        g[sy - 2, 0] = gu.PASSAGE          # neither IS_VISIBLE nor HAS_DRAWN, diagonal to the player: Cell::approached never reaches a diagonal passage cell
        start = (1, sy - 1)
        mons = [mon(1, 1, "C", active=False, hp=900),        # far away in the same passage: both outside the rect -> shown
                mon(6, 3, "I", active=False, hp=900),        # inside the rect -> hidden
                mon(1, sy + 2, "J", active=False, hp=900),   # the area below, three cells away -> hidden
                mon(2, sy, "K", active=False, hp=900),       # the area below, diagonally adjacent -> shown (asleep: no door of ITS area is stepped on)
                mon(0, sy - 2, "B", active=False, hp=900)]   # adjacent, on a cell with neither attribute bit -> hidden
        want0 = {(1, 1): "C", (6, 3): "I" if variant == "empty room" else ".", (1, sy + 2): "#", (2, sy): "K", (0, sy - 2): " "}
        # inside the rect (on the door and behind it) every one of them flips -- but for an Empty room, which has no range: the whole area counts
        want_in = {(1, 1): "C" if variant == "empty room" else "#", (6, 3): "I", (1, sy + 2): "#", (2, sy): "#"}
        up = sy - 5
        keys = pad(".s" + "k" * up + "lll" + "s" + "hhh" + "j" * up + "." + "lh")
        room = dict(range=RECT, kind=2 if variant == "empty room" else 0, dark=variant == "dark room", visited=True)
        for part, ms in enumerate(chunks(mons, nr) if nr < len(mons) else [mons]):
            cells = [(m["x"], m["y"]) for m in ms]

            def shown_as_claimed(tr, cells=cells, want0=want0, want_in=want_in, up=up):
                f0, fin = tr.frames[0], tr.frames[2 + up + 3]   # the loaded state; behind the door
                return all(f0.at(*c) == want0[c] for c in cells) and fin.pos == (4, 4) and all(fin.at(*c) == want_in[c] for c in cells if c in want_in)

            def flips_back(tr, cells=cells, want0=want0, dark=variant == "dark room"):
                f = tr.frames[-1]   # (the bat's cell was approached on the way: it shows from then on; leaving a dark room takes IS_VISIBLE from its inside, floor.rs:249-261)
                return all(f.at(*c) == (" " if dark and c == (6, 3) else want0[c]) for c in cells if c != (0, sy - 2))

            out.append(Scenario("same room, %s%s" % (variant, "" if part == 0 else " (%d)" % (part + 1)),
                                "the player in a passage outside the room's rect inside one assigned area, then through the door and back: shown and hidden monsters flip",
                                su.State(shape, g, start, ms, rooms=rooms_with(shape, room), hp=600, seed=700 + len(variant) + part), keys,
                                {"shown and hidden as the rule says, and flipped behind the door": shown_as_claimed, "back as loaded after the way out": flips_back}))
    return out


# ---------------------------------------------------------------------------------------------
# (b) priority
# ---------------------------------------------------------------------------------------------
def priority(shape):
    w, h = su.SHAPES[shape][:2]
    g = np.full((h, w), gu.NONE, np.uint16)
    g[2:7, 1:7] = gu.FLOOR | LIT
    g[2, 5] = g[6, 6] = gu.FLOOR | DRAWN     # HAS_DRAWN without IS_VISIBLE: the object over a blank
    mons = [mon(4, 4, "C", active=False, hp=900), mon(5, 2, "I", active=False, hp=900), mon(6, 6, "J", active=False, hp=900)]
    gold = [(4, 4, 11), (5, 2, 12), (3, 4, 13)]

    def loaded(tr):
        f = tr.frames[0]
        return f.at(4, 4) == "*" and f.at(5, 2) == "*" and f.at(6, 6) == "J" and f.at(3, 4) == "*" and f.at(2, 4) == "@" and f.at(6, 5) == "."

    def stepped_on_gold(tr):
        f = tr.frames[3]
        return f.pos == (3, 4) and f.at(3, 4) == "@" and f.status[1] == 13 and su.st.STATUS in f.reactions

    def monster_left_its_gold(tr):   # the woken monster steps off its gold and is drawn, the gold stays a '*'
        return any(f.at(4, 4) == "*" and "C" in {chr(v) for v in f.screen.reshape(-1)} for f in tr.frames[4:])

    return [Scenario("priority", "gold under a sleeping monster shows the gold, on a cell that is only HAS_DRAWN over a blank; the player steps onto gold; a hit wakes the monster off its gold",
                     su.State(shape, g, (2, 4), mons, gold=gold, hp=600, seed=720), ".s" + "l" + "ll" + "s" + "hs" + "ls" + "kjs" + "hls" + ".s" + "ls",
                     {"gold over the monster, objects over blanks": loaded, "the player on the gold's cell": stepped_on_gold, "the monster beside its gold": monster_left_its_gold})]


# ---------------------------------------------------------------------------------------------
# (c) rows 0 and H - 1 are never drawn, columns 0 and W - 1 are
# ---------------------------------------------------------------------------------------------
def trimmed(shape):
    w, h = su.SHAPES[shape][:2]
    g = ts.frame(w, h)
    for k in range(8):                       # every surface, visible and not, on the two trimmed rows, the rows next to them and the two border columns
        for y in (0, 1, h - 2, h - 1):
            g[y, 8 + 2 * k] = k | LIT
            g[y, 9 + 2 * k] = k | (DRAWN if k % 2 else 0)
        g[4 + k, 0] = k | (LIT if k % 2 == 0 else DRAWN)
        g[4 + k, w - 1] = k | (LIT if k % 2 else 0)
    mons = [mon(5, 0, "C", active=False, hp=900), mon(5, h - 1, "I", active=False, hp=900), mon(0, 3, "J", active=False, hp=900), mon(w - 1, 3, "K", active=False, hp=900)]
    gold = [(3, 0, 21), (3, h - 1, 22), (0, 2, 23), (w - 1, 2, 24)]
    out = []

    def rows_blank(tr):
        return all(not (f.screen[0] != 32).any() and not (f.screen[h - 1] != 32).any() for f in tr.frames)

    def columns_drawn(tr):
        f = tr.frames[0]
        return (f.at(0, 2), f.at(w - 1, 2), f.at(0, 4), f.at(0, 5), f.at(w - 1, 4), f.at(w - 1, 5), f.at(10, h - 2), f.at(11, h - 2)) == ("*", "*", "#", " ", " ", ".", ".", " ")

    for name, start, ix, iy in (("row 0", (4, 0), 1, 1), ("row H-1", (4, h - 1), 1, -1)):
        keys = pad("s." + ts.key(0, iy) + "s" + ts.key(0, -iy) + "s" + ts.key(-ix, 0) + "s" + ts.key(ix, 0) + ts.key(0, iy) + ts.key(ix, iy) + ts.key(0, -iy) + ts.key(0, -iy) + "s" + ts.key(-ix, 0, True) + "s")

        def no_player(tr):
            on_row = [f for f in tr.frames[1:] if f.pos[1] in (0, h - 1) and su.st.REDRAW in f.reactions]
            return len(on_row) >= 3 and all(not (f.screen == ord("@")).any() for f in on_row) and any((f.screen == ord("@")).any() for f in tr.frames)

        def took_gold(tr, start=start):
            return any(f.pos == (3, start[1]) and su.st.STATUS in f.reactions for f in tr.frames[1:])

        out.append(Scenario("trimmed, " + name, "gold, a sleeper and the player on a row that is never drawn: no '@' at all, the gold is taken there all the same",
                            su.State(shape, g, start, mons, gold=gold, hp=600, seed=730 + iy), keys,
                            {"rows 0 and H - 1 blank on every frame": rows_blank, "a Redraw with the player on the row: no '@'": no_player, "gold taken on the row": took_gold,
                             "columns 0 and W - 1 drawn": columns_drawn}))
    for name, cx, ix in (("column 0", 0, 1), ("column W-1", w - 1, -1)):
        keys = pad("s." + ts.key(-ix, 0) + "s" + ts.key(0, -1) + ts.key(0, -1) + "s" + ts.key(0, 1) + ts.key(0, 1) + "s." + ts.key(ix, 0) + ts.key(-ix, -1) + ts.key(-ix, -1) + "s" + ts.key(ix, 1))

        def on_column(tr, cx=cx):
            return any(f.pos == (cx, 2) and f.at(cx, 2) == "@" and su.st.STATUS in f.reactions for f in tr.frames[1:]) and any(f.pos == (cx, 0) and not (f.screen == ord("@")).any() for f in tr.frames)

        out.append(Scenario("trimmed, " + name, "the player takes gold on a border column (drawn) and walks into the corner on row 0 (not drawn)",
                            su.State(shape, g, (cx + ix, 2), mons, gold=gold, hp=600, seed=740 + ix), keys,
                            {"rows 0 and H - 1 blank on every frame": rows_blank, "'@' on the border column, none in the corner": on_column, "columns 0 and W - 1 drawn": columns_drawn}))
    return out


# ---------------------------------------------------------------------------------------------
# (d) stale mirrors
# ---------------------------------------------------------------------------------------------
def arena(shape):
    w, h = su.SHAPES[shape][:2]
    return ts.block(w, h, 1, 2, 6, 5)   # columns 1 .. 6, rows 2 .. 6; column 0 is not walkable: 'h' from column 1 is a blocked move


def stale(shape):
    w, h = su.SHAPES[shape][:2]
    out = []
    exps = su.st.LEVEL_EXPS

    def stale_run(tr, n=4):   # n keys in a row after which the screen mirror is older than the state
        best = cur = 0
        for f in tr.frames[1:]:
            cur = cur + 1 if f.stale_screen else 0
            best = max(best, cur)
        return best >= n

    def caught_up(tr):
        return any(a.stale_screen and not b.stale_screen and su.st.REDRAW in b.reactions for a, b in zip(tr.frames, tr.frames[1:]))

    # a corridor along row 4 through the areas; the player walks into the wall at its west end while two chasers come along it
    g = np.full((h, w), gu.NONE, np.uint16)
    end = min(w - 2, 20)
    g[4, 1:end + 1] = gu.FLOOR | LIT
    out.append(Scenario("stale, blocked moves", "blocked moves pass turns without a Redraw: the chasers approach and hit while the screen keeps the old picture until a search",
                        su.State(shape, g, (1, 4), [mon(6, 4, "C", hp=40), mon(7, 4, "K", hp=40)], hp=900, seed=750), "hhhhhh" + "s" + "hhh" + "." + "s" + "hh" + "s" + "...." + "hh" + "s",
                        {"the screen lags for six keys": lambda tr: stale_run(tr, 6), "a search catches up": caught_up,
                         "a hit refreshes the status, not the screen": lambda tr: any(f.stale_screen and su.st.STATUS in f.reactions and su.st.REDRAW not in f.reactions for f in tr.frames[1:])}))
    out.append(Scenario("stale, screen to the end", "one search, then blocked moves to the end of the script while a chaser comes up the corridor: the last screen is fifteen turns old",
                        su.State(shape, g, (1, 4), [mon(7, 4, "K", hp=40)], hp=900, seed=757), "...." + "s" + "h" * 15,
                        {"the screen is stale at the end": lambda tr: tr.frames[-1].stale_screen and stale_run(tr, 15)}))
    a = arena(shape)
    out.append(Scenario("stale, status to the end", "a kill below the next level among the last keys: the status mirror ends with the old exp",
                        su.State(shape, a, (2, 4), [mon(3, 4, "C", active=False, hp=1, exp=10)], hp=150, plevel=5, exp=exps[3] + 20, seed=758), "s" * 14 + "llllll",
                        {"the status is stale at the end": lambda tr: tr.frames[-1].stale_status and tr.frames[-1].fresh_status[8] == exps[3] + 30}))
    out.append(Scenario("stale, hits that do not kill", "hits on a monster of 900 hit points push no Redraw; it wakes and a second chaser arrives unseen",
                        su.State(shape, a, (2, 4), [mon(3, 4, "C", active=False, hp=900), mon(6, 2, "E", hp=40)], hp=900, seed=751), "llll" + "s" + "lll" + "." + "ll" + "s" + "llll" + "." + "s" + "ll",
                        {"the screen lags for three keys": lambda tr: stale_run(tr, 3), "a search catches up": caught_up}))
    # a kill worth experience but no level: Redraw, no StatusUpdated -- the status keeps the old exp until the next heal
    out.append(Scenario("stale, exp without a level", "a kill below the next level pushes a Redraw and no StatusUpdated: the status mirror keeps the old exp until a heal",
                        su.State(shape, a, (2, 4), [mon(3, 4, "C", active=False, hp=1, exp=10)], hp=20, hp_max=150, plevel=5, exp=exps[3] + 20, seed=752), "llllll" + "h" * 8 + "s" * 12,
                        {"the status mirror keeps the old exp": lambda tr: any(f.status[8] == exps[3] + 20 and f.fresh_status[8] == exps[3] + 30 and su.st.REDRAW in f.reactions for f in tr.frames[1:]),
                         "a heal brings it": lambda tr: tr.frames[-1].status[8] == exps[3] + 30}))
    hunger = su.HUNGER_TIME // 10
    for food in (2 * hunger + 3, hunger + 3):
        out.append(Scenario("stale, food %d" % food, "food_left passes exactly %d: the Hungry event of that turn refreshes the status" % (food - 3),
                            su.State(shape, a, (1, 4), hp=12, hp_max=12, food=food, seed=753 + food), "h.h" + "h" * 9 + "s" * 8,
                            {"the hunger word changes on the third turn, by a StatusUpdated without a Redraw":
                             lambda tr: [f.status[9] for f in tr.frames[:5]] == [tr.frames[0].status[9]] * 4 + [tr.frames[0].status[9] + 1] and tr.frames[4].reactions == [su.st.STATUS]}))
    out.append(Scenario("stale, heal", "a heal on a blocked move: StatusUpdated alone", su.State(shape, a, (1, 4), hp=5, hp_max=12, quiet=16, seed=756), "hh.h" + "h" * 16 + "ss",
                        {"hp rises by a StatusUpdated without a Redraw": lambda tr: any(b.status[2] == a_.status[2] + 1 and b.reactions == [su.st.STATUS] for a_, b in zip(tr.frames, tr.frames[1:]))}))
    return out


# ---------------------------------------------------------------------------------------------
# (e) far overlays
# ---------------------------------------------------------------------------------------------
def far_overlays(shape):
    w, h = su.SHAPES[shape][:2]
    sx, sy = area(shape)
    out = []
    # the player crosses from area 0 into area 1 and back along row 4; one sleeper far behind, one just beside the boundary
    g = np.full((h, w), gu.NONE, np.uint16)
    g[4, 1:sx + 5] = gu.FLOOR | LIT
    g[5, sx - 1] = gu.FLOOR | LIT
    far, near = (1, 4), (sx - 1, 5)

    def far_flip(tr):   # shown -> hidden more than two cells from the player, on one Redraw
        return any(a_.at(*far) == "C" and b.at(*far) == "." and abs(b.pos[0] - far[0]) > 2 and abs(a_.pos[0] - far[0]) > 2 for a_, b in zip(tr.frames, tr.frames[1:]))

    def near_flip(tr):  # the same within the 5 x 5 window, and not adjacent
        return any(a_.at(*near) == "I" and b.at(*near) == "." and max(abs(b.pos[0] - near[0]), abs(b.pos[1] - near[1])) == 2 for a_, b in zip(tr.frames, tr.frames[1:]))

    out.append(Scenario("far overlays, area boundary", "the player steps over an area boundary and back: a sleeper five cells behind and one two cells away turn hidden and shown again",
                        su.State(shape, g, (sx - 3, 4), [mon(far[0], far[1], "C", active=False, hp=900), mon(near[0], near[1], "I", active=False, hp=900)], hp=600, seed=760),
                        pad("s" + "llll" + "s" + "hhhh" + "." + "lll" + "s" + "l" + "hh" + "s"),
                        {"a far monster turns hidden outside the 5 x 5 window": far_flip, "a near one inside it": near_flip,
                         "and shown again": lambda tr: tr.frames[-1].at(*far) == "C"}))
    # chasers come down a block row by row while the player searches and walks into the wall
    g = ts.block(w, h, 1, 1, 5, 7)
    out.append(Scenario("far overlays, image rows", "two chasers come down from row 1 to the player on row 7, a row per turn: drawn on searches, stale on blocked moves",
                        su.State(shape, g, (3, 7), [mon(1, 1, "K", hp=40), mon(5, 1, "E", hp=40)], hp=900, seed=761), "sjsjjs" + "sjjs" + ".s" + "jjjs" + "sjsj",
                        {"the monsters are drawn on four different rows": lambda tr: len({y for f in tr.frames for y in range(h) for v in f.screen[y] if chr(v) in "KE"}) >= 4}))
    return out


def scenarios(shape):
    """The draw scenarios of one shape, in env order (behind the turn scenarios in a batch)."""
    return same_room(shape) + priority(shape) + trimmed(shape) + stale(shape) + far_overlays(shape)


def all_scenarios(shape):
    """What one batch of tests/test_gpu_draw_scenarios.py holds: the turn scenarios as they are, then the draw scenarios."""
    return ts.scenarios(shape) + scenarios(shape)
