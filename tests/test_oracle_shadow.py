"""Differential test of the C oracle's TURN against a second, independently written restatement (tests/shadow_turn.py).

profiles/r05_pin_map.txt lists the readings of the reference no reference golden pins: they are all in the turn (combat, level-up, healing, erratic
monsters, search, turn structure, the monsters' overwrite / corner-cutting rules, the never-invalidated DistCache) plus three generator sites.  For the
turn, the C oracle (oracle/rogue_oracle.c) and the Python model (written from the Rust text without the C) play the same keys from the same levels and
must agree on the whole state after every key.  tools/shadow_soak.py runs the same harness for 10^6 env-steps (profiles/r05_shadow_diff.txt); this
file keeps a slice of it in the CPU suite -- and checks that the harness is able to see a difference at all (the oracle's mutants must be caught)."""
import json
import os

import numpy as np
import pytest

from oracle.pyoracle import OracleEnv
from shadow_turn import KEYMAP, Mirror, Shadow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_KEYS = "hjklyubnhjklyubnHJKLYUBN.s>"
DIRS8 = {(0, -1): "k", (0, 1): "j", (-1, 0): "h", (1, 0): "l", (-1, -1): "y", (1, -1): "u", (-1, 1): "b", (1, 1): "n"}


def _seeker_key(o, rng, stuck):
    """Test policy: '>' on the stairs, else a greedy step towards them over walkable, known-passable cells, else search / wander."""
    surf, attr, _, _ = o.grid()
    sc = o.scalars()
    px, py = sc["px"], sc["py"]
    h, w = surf.shape
    if surf[py, px] == 4:
        return ">"
    walk = ~np.isin(surf, (2, 3, 7)) & ((attr & 0x12) == 0)
    ys, xs = np.nonzero(surf == 4)
    if len(xs) and stuck[0] < 6:
        dist = np.full((h, w), 1 << 20, np.int32)
        dist[ys[0], xs[0]] = 0
        front = [(int(xs[0]), int(ys[0]))]
        while front:
            nxt = []
            for (x, y) in front:
                for (dx, dy) in DIRS8:
                    nx, ny = x + dx, y + dy
                    if 0 <= nx < w and 0 <= ny < h and walk[ny, nx] and dist[ny, nx] > dist[y, x] + 1 and (not (dx and dy) or (walk[y, nx] and walk[ny, x])):
                        dist[ny, nx] = dist[y, x] + 1
                        nxt.append((nx, ny))
            front = nxt
        best, key = dist[py, px], None
        for (dx, dy), k in DIRS8.items():
            nx, ny = px + dx, py + dy
            if 0 <= nx < w and 0 <= ny < h and walk[ny, nx] and dist[ny, nx] < best and (not (dx and dy) or (walk[py, nx] and walk[ny, px])):
                best, key = dist[ny, nx], k
        if key:
            stuck[0] = 0
            return key
    stuck[0] = (stuck[0] + 1) % 24
    return "s" if stuck[0] % 3 == 0 else "hjklyubn"[rng.randint(0, 8)]


def run_differential(cfg, seeds, steps, max_steps, policy, rng, weapon=(2, 4, 1, 1), armor=4, grid_every=1, stats=None):
    """Plays `steps` keys per seed on the C oracle and on the Python model; raises AssertionError at the first difference.  Returns env-steps played."""
    d = cfg.get("dungeon", {})
    played = 0
    for seed in seeds:
        o = OracleEnv(cfg, max_steps=max_steps, seed=seed)
        sh = Shadow(o.w, o.h, cfg.get("player", {}).get("hunger_time", 1300), d.get("passage_unlock_rate_inv", 3), d.get("door_unlock_rate_inv", 5), weapon, armor)
        sh.new_game(o)
        mirror = Mirror(sh)
        episode, n_steps, stuck = [], 0, [0]
        for t in range(steps):
            key = policy(o, rng, stuck)

            def new_level():
                twin = OracleEnv(cfg, max_steps=10 ** 9, seed=seed)   # the primary, replayed up to this key, takes actions::new_level alone (orc_debug_descend)
                for k in episode:
                    twin.react(k)
                twin.debug_descend()
                sh.load_level(twin)
                if stats is not None:
                    stats["descents"] = stats.get("descents", 0) + 1
            lvl0, plv0, floors0 = sh.plevel, sh.level, len(sh.past_floors)
            died = sh.process_action(key, new_level)
            o.react(key)
            episode.append(key)
            n_steps += 1
            played += 1
            if stats is not None:
                stats["level_ups"] = stats.get("level_ups", 0) + (sh.plevel > lvl0)
                stats["max_plevel"] = max(stats.get("max_plevel", 1), sh.plevel)
                stats["max_dlevel"] = max(stats.get("max_dlevel", 1), sh.level)
                stats["deaths"] = stats.get("deaths", 0) + int(died)
            sc, (words, _), got = o.scalars(), o.rng(), sh.snapshot()
            where = "seed %d key %d (%r)" % (seed, t, key)
            want = dict(pos=(sc["px"], sc["py"]), hp=sc["hp"], hp_max=sc["hp_max"], exp=sc["exp"], plevel=sc["plevel"], food_left=sc["food_left"], quiet=sc["quiet"],
                        gold=sc["gold"], level=sc["level"], rng_dungeon=[int(v) for v in words[0]], rng_enemy=[int(v) for v in words[2]],
                        monsters=sorted((m["x"], m["y"], chr(65 + m["type"]), m["active"], m["hp"], m["exp"]) for m in o.monsters()), dead=o.flags()["dead"])
            assert got == want, "%s: %s" % (where, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
            assert [int(v) for v in words[1]] == sh.rng_item_words, where + ": the turn drew on the item stream"
            if t % grid_every == 0 or died:
                surf, attr, _, gold = o.grid()
                assert sh.surface == [int(v) for v in surf.reshape(-1)], where + ": surface"
                assert sh.attr == [int(v) for v in attr.reshape(-1)], where + ": attr"
                assert sh.items == {i: int(v) for i, v in enumerate(gold.reshape(-1)) if v >= 0}, where + ": items"
            # what Python sees: the Shadow's draw, history and status under its own reaction list against the oracle's mirrors (stale by rule, both)
            mirror.react(sh)
            assert np.array_equal(mirror.screen, o.screen().reshape(-1)), "%s: screen (reactions %s)\nShadow:\n%s\noracle:\n%s" % (
                where, sh.reactions, "\n".join(bytes(r).decode() for r in mirror.screen.reshape(o.h, o.w)), "\n".join(o.dungeon()))
            assert np.array_equal(mirror.hist, o.hist().reshape(-1)), "%s: history (reactions %s)" % (where, sh.reactions)
            assert [v & M32 for v in mirror.status] == [int(v) for v in o.status_arr()], "%s: status %s, the oracle's %s (reactions %s)" % (where, mirror.status, o.status_arr(), sh.reactions)
            if stats is not None:
                stats["stale_screens"] = stats.get("stale_screens", 0) + int(not np.array_equal(mirror.screen, sh.draw_screen()))
                stats["stale_status"] = stats.get("stale_status", 0) + int(mirror.status != sh.status())
                if len(sh.past_floors) > floors0:   # a descent's Redraw comes before its StatusUpdated: the history drawn is the floor's that was left
                    stats["past_hist"] = stats.get("past_hist", 0) + int(np.array_equal(mirror.hist, sh.past_floors[-1]) and not np.array_equal(mirror.hist, sh.history_map()))
            assert o.flags()["is_terminal"] == (died or n_steps >= max_steps), where
            if o.flags()["is_terminal"]:
                o.reset()
                sh.new_game(o)
                mirror = Mirror(sh)
                episode, n_steps = [], 0
    return played


def random_policy(o, rng, stuck):
    return ALL_KEYS[rng.randint(0, len(ALL_KEYS))]


def mixed_policy(o, rng, stuck):
    return _seeker_key(o, rng, stuck) if rng.randint(0, 4) else random_policy(o, rng, stuck)


@pytest.fixture(scope="module")
def cfgs(goldens):
    mini = dict(goldens["configs"]["mini"])
    strong = dict(mini, player={"init_hp": 60, "init_items": [{"Weapon": {"name": "two-handed-sword", "num_plus": 0, "hit_plus": 3, "dam_plus": 3}},
                                                              {"Armor": {"name": "plate mail", "def_plus": 2}}]})
    default = dict(goldens["configs"]["seed1"])
    return mini, strong, default


def test_turn_matches_the_second_restatement(cfgs):
    mini, strong, default = cfgs
    rng = np.random.RandomState(7)
    stats = {}
    n = run_differential(mini, range(40), 400, 300, random_policy, rng, stats=stats)
    n += run_differential(mini, range(100, 120), 500, 400, mixed_policy, rng, stats=stats)
    # a two-handed sword 4d4 +3,+3 and plate mail 7 + 2 (weapon.rs:254-264, armor.rs:213-218): kills, level-ups, deep levels
    n += run_differential(strong, range(200, 216), 700, 600, mixed_policy, rng, weapon=(4, 4, 3, 3), armor=9, stats=stats)
    n += run_differential(default, range(300, 306), 400, 400, mixed_policy, rng, grid_every=4, stats=stats)
    assert n >= 37000
    assert stats["descents"] >= 30 and stats["level_ups"] >= 10 and stats["deaths"] >= 20, stats
    # the mirrors were compared while they lagged the state: a screen older than the state, a status older than the player, a history of the floor that was left
    print(stats)
    assert stats["stale_screens"] >= 100 and stats["stale_status"] >= 100 and stats["past_hist"] >= 30, stats


@pytest.mark.parametrize("k", [34, 36, 37, 38, 39, 40, 43, 46, 48, 50, 51, 56, 58, 62, 63, 64, 65])
def test_the_harness_sees_the_unpinned_mutants(cfgs, k, tmp_path):
    """The differential must be able to fail: every turn mutant the reference's goldens miss (profiles/r05_pin_map.txt) differs from the Python model within a few
    thousand keys.  (The rest -- M35, M41 / M42: a player of level 8, M47: a chase across a descent onto a cached coordinate, M57: a search next to a locked door,
    M68: 1 300 turns without a reset -- need the longer runs of tools/shadow_soak.py, which records for each whether it was caught.)"""
    import subprocess
    import sys
    from oracle_mutants import build_mutant
    so = build_mutant(k, str(tmp_path))
    code = ("import sys, json, numpy as np\nsys.path[:0] = [%r, %r]\nimport test_oracle_shadow as T\n"
            "g = json.load(open(%r))\nmini = dict(g['configs']['mini'])\n"
            "strong = dict(mini, player={'init_hp': 60, 'init_items': [{'Weapon': {'name': 'two-handed-sword', 'num_plus': 0, 'hit_plus': 3, 'dam_plus': 3}}, {'Armor': {'name': 'plate mail', 'def_plus': 2}}]})\n"
            "hard = dict(mini, dungeon=dict(mini['dungeon'], hidden_passage_rate_inv=2, locked_door_rate_inv=2, dark_level=1))\n"
            "rng = np.random.RandomState(3)\n"
            "try:\n"
            "    T.run_differential(mini, range(30), 400, 300, T.random_policy, rng)\n"
            "    T.run_differential(strong, range(200, 212), 600, 600, T.mixed_policy, rng, weapon=(4, 4, 3, 3), armor=9)\n"
            "    T.run_differential(hard, range(400, 420), 400, 300, T.mixed_policy, rng)\n"
            "    print('AGREE')\n"
            "except AssertionError as e:\n"
            "    print('DIFFER', str(e)[:200])\n") % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "reference_goldens.json"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ROGUE_ORACLE_SO=so), capture_output=True, text=True, timeout=600)
    assert "DIFFER" in r.stdout, (k, r.stdout[-500:], r.stderr[-500:])


def test_unpinned_generator_sites(goldens):
    """The generator sites no REFERENCE golden pins (profiles/r05_pin_map.txt: M2, M28, M45; M26 / M27 / M59 are noticed by probe-derived fixtures only), each
    re-derived from the text and checked against what the C oracle generates:
      * rooms.rs:175-190 -- `rng.range(0..=max_empty_rooms)` (u32), then `rng.select(0..room_num).take(empty_num)`: RandomSelecter::next draws
        `gen_range(0, num_rests)` over usize (rng.rs:128-143), i.e. 64 bits, and removes the nth remaining id;
      * gold.rs:18-24, weapon.rs:148-159 -- the item stream of a build: per room that has a free cell `does_happen(rate_inv)` and ONLY THEN the amount
        `range(0..base + per_level * level) + minimum` (both u32), then one `rng.range(init_num)` (u32) per initial weapon;
      * floor.rs:92-100 -- a corridor cell whose gen_attr came back hidden / locked keeps the surface it had (Surface::None for a cell nothing else painted)."""
    from shadow_turn import Rng
    rnd = np.random.RandomState(11)
    base = dict(goldens["configs"]["seed1"])                      # 80 x 24, 3 x 3 rooms, max_empty_rooms 3 by default
    n_empty_seen, gold_rooms, hidden_cells, hidden_unpainted = 0, 0, 0, 0
    for trial in range(400):
        seed = int(rnd.randint(1, 2 ** 62)) * 4 + int(rnd.randint(0, 4))     # full-width seeds: small ones start with a run of zero draws
        cfg = dict(base, dungeon=dict(base.get("dungeon", {}), max_empty_rooms=int(rnd.randint(0, 9)), dark_level=2, hidden_passage_rate_inv=3, locked_door_rate_inv=3,
                                      maze_rate_inv=1000000))
        o = OracleEnv(cfg, seed=seed)
        rooms, n_rooms = o.rooms(), 9
        words = [seed & M32, (seed >> 32) & M32, (seed >> 64) & M32, (seed >> 96) & M32]
        # -- the empty rooms
        r = Rng(words)
        empty_num = min(r.gen_range(0, cfg["dungeon"]["max_empty_rooms"] + 1, 32), n_rooms - 1)
        rest, empty = list(range(n_rooms)), set()
        for _ in range(empty_num):
            empty.add(rest.pop(r.gen_range(0, len(rest), 64)))
        assert empty == {i for i, q in enumerate(rooms) if q["kind"] == 2}, (seed, empty)
        n_empty_seen += len(empty)
        # -- the item stream of the build (level 1): gold per non-empty room in id order, then mace / bow / arrow counts
        it = Rng(words)
        _, _, _, gold = o.grid()
        for q in rooms:
            if q["kind"] == 2:
                continue
            x0, y0, x1, y1 = q["range"]
            found = [int(v) for v in gold[y0:y1, x0:x1].reshape(-1) if v >= 0]
            if it.does_happen(2):
                amount = it.gen_range(0, 50 + 10 * 1, 32) + 2      # gold::Config defaults (gold.rs:38-52): base 50, per_level 10, minimum 2
                assert found == [amount], (seed, q, found, amount)
                gold_rooms += 1
            else:
                assert found == [], (seed, q, found)
        for lo, hi in ((1, 2), (1, 2), (8, 17)):                    # mace, bow, arrow init_num (weapon.rs:179-213), Player::init_items order (player.rs:136-153)
            it.gen_range(lo, hi, 32)
        assert it.s == [int(v) for v in o.rng()[0][1]], (seed, "item stream after the build")
        # -- hidden / locked corridor cells: not painted.  (A cell two corridors share may have been painted by the first; those are the few exceptions.)
        for _ in range(3):
            o.debug_descend()
        surf, attr, _, _ = o.grid()
        in_room = np.zeros_like(surf, bool)
        for q in o.rooms():
            if q["kind"] != 2:
                x0, y0, x1, y1 = q["range"]
                in_room[y0:y1, x0:x1] = True
        hid = ((attr & 0x12) != 0) & ~in_room
        hidden_cells += int(hid.sum())
        hidden_unpainted += int((hid & (surf == 7)).sum())
    assert n_empty_seen > 300 and gold_rooms > 1000 and hidden_cells > 2000, (n_empty_seen, gold_rooms, hidden_cells)
    assert hidden_unpainted >= 0.97 * hidden_cells, (hidden_unpainted, hidden_cells)


M32 = 0xFFFFFFFF


@pytest.mark.parametrize("k", [2, 26, 27, 28, 45, 59])
def test_generator_checks_catch_their_mutants(k, tmp_path):
    """... and those checks do fail for the misreadings they are there for."""
    import subprocess
    import sys
    from oracle_mutants import build_mutant
    so = build_mutant(k, str(tmp_path))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_oracle_shadow.py"), "-q", "-x", "-k", "test_unpinned_generator_sites", "-p", "no:cacheprovider"],
                       env=dict(os.environ, ROGUE_ORACLE_SO=so), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert "1 failed" in r.stdout, (k, r.stdout[-400:])
