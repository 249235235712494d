"""The constructed turn scenarios (tests/turn_scenarios.py) through the Shadow alone: every scenario reaches what its line claims, and no assertion of the
Shadow fires on the way (Floor::with_current_room's among them).  No GPU.  Run with -s for the event counts per scenario."""
import pytest

import state_util as su
import turn_scenarios as ts


def run(sc, probe_stale=False):
    p = ts.Play(sc)
    p.sh.probe_stale = probe_stale
    while p.t < len(sc.keys):
        p.step()
    return p


def check_claims(sc, ev):
    c = sc.claims
    # (overwritten: active monsters that vanished inside move_actives -- no kill is made there)
    for k in ("overwritten", "evicted", "cache_max", "stale_moves", "activated", "kills", "heal_draws", "level_jump", "max_reward"):
        if k in c:
            assert ev[k] >= c[k], "%s: %s = %d, claimed >= %d" % (sc.name, k, ev[k], c[k])
    for k in ("died", "died_in_run", "hp_rose"):
        if k in c:
            assert ev[k], "%s: %s did not happen" % (sc.name, k)
    if "negative_hp" in c:
        assert ev["min_mon_hp"] < 0, "%s: no monster was left with damage - cur < 0 hit points" % sc.name
    if "food_wrapped" in c:
        assert ev["food"] > 2 ** 31, "%s: food_left = %d" % (sc.name, ev["food"])
    if "gold" in c:
        assert ev["gold"] == c["gold"], "%s: gold = %d" % (sc.name, ev["gold"])
    if "crossed" in c:
        lo, hi = ev["mon_x_span"]
        assert lo <= c["crossed"] - 1 and hi >= c["crossed"], "%s: the monsters stood on columns %d .. %d only" % (sc.name, lo, hi)
    if "far" in c:
        assert c["far"] >= (1000 if sc.state.shape == "160x48" else 100), "%s: the walk is %d moves" % (sc.name, c["far"])
        assert ev["maps"] >= 3


@pytest.mark.parametrize("shape", list(su.SHAPES))
def test_every_scenario_reaches_its_event(shape):
    scs = ts.scenarios(shape)
    assert len({s.name for s in scs}) == len(scs)
    stood, mon_stood = set(), set()
    for sc in scs:
        p = run(sc, probe_stale="stale_moves" in sc.claims)
        ev = p.events()
        print("%-7s %-28s keys %2d  %s" % (shape, sc.name, len(sc.keys), {k: v for k, v in sorted(ev.items()) if v not in (0, False, (0, 0), 1) or k in sc.claims}))
        check_claims(sc, ev)
        if "border_part" in sc.claims:
            stood |= ts.border_classes(shape, p.sh.stood)
            mon_stood |= ts.border_classes(shape, p.sh.mon_stood)
    if shape != "160x48":
        assert stood == ts.ALL_BORDER_CLASSES, "the player never stood on %s" % sorted(ts.ALL_BORDER_CLASSES - stood)
        assert mon_stood == ts.ALL_BORDER_CLASSES, "no monster ever stood on %s" % sorted(ts.ALL_BORDER_CLASSES - mon_stood)


def test_scenarios_tell_two_readings_apart():
    """The scripts distinguish the readings a kernel could get wrong: a Shadow whose movers skip cells still in `taken` (no overwrite), and one whose cache
    evicts the least recently used map, each end at least one scenario in another state."""
    class NoOverwrite(su.CountingShadow):
        def move_actives(self):
            attacks, taken, self.active = [], self.active, {}
            for path in sorted(taken):
                enemy = taken[path]
                res = self.move_enemy(path, self.pos, lambda p: p in self.active or p in self.placed or (p in taken and p > path))
                if res == "reach":
                    attacks.append(enemy)
                self.active[path if res in ("reach", "cant") else res] = enemy
            return attacks

    class Lru(su.CountingShadow):
        def cached_dist_map(self, cd):
            for i, (m, k) in enumerate(self.dist_cache):
                if k == cd:
                    self.dist_cache.append(self.dist_cache.pop(i))
                    return m
            return super().cached_dist_map(cd)

    def final(sc, cls):
        p = ts.Play(sc, cls)
        while p.t < len(sc.keys):
            p.step()
        return su.expected(p.sh)

    scs = ts.scenarios("80x24")
    for cls, names in ((NoOverwrite, ("crowd in a row", "crowd in a column")), (Lru, ("stale cache, eight cells",))):
        differing = [sc.name for sc in scs if sc.name in names and final(sc, cls) != final(sc, su.CountingShadow)]
        assert differing, "%s: no scenario of %s tells it from the reference's reading" % (cls.__name__, names)
