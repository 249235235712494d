"""The draw scenarios (tests/draw_scenarios.py) through the Shadow and its Mirror alone: every scenario reaches what it claims, only the scenarios that claim a
death drop out of a batch, and the set can see wrong readings of the draw and of the reaction rule -- each of six misreadings, as a subclass of the Shadow, ends
at least one scenario of every shape with another mirror.  No GPU.  Run with -s for a line per scenario."""
import pytest

import draw_scenarios as ds
import state_util as su
import turn_scenarios as ts

st = su.st


@pytest.mark.parametrize("shape", list(su.SHAPES))
def test_every_draw_scenario_reaches_its_claims(shape):
    scs = ds.scenarios(shape)
    assert len({s.name for s in scs} | {s.name for s in ts.scenarios(shape)}) == len(scs) + len(ts.scenarios(shape))
    stale_screens = stale_status = 0
    for sc in scs:
        tr = ds.play(sc)
        assert tr.died_at is None, "%s %s: the player died at key %d" % (shape, sc.name, tr.died_at)
        n_scr, n_st = sum(f.stale_screen for f in tr.frames), sum(f.stale_status for f in tr.frames)
        stale_screens, stale_status = stale_screens + n_scr, stale_status + n_st
        print("%-7s %-36s keys %2d  Redraws %2d  StatusUpdated %2d  frames with a stale screen %2d, a stale status %2d" % (
            shape, sc.name, len(sc.keys), sum(st.REDRAW in f.reactions for f in tr.frames[1:]), sum(st.STATUS in f.reactions for f in tr.frames[1:]), n_scr, n_st))
        assert not (tr.frames[0].stale_screen or tr.frames[0].stale_status), "%s %s: the loaded mirror is not the draw of the loaded state" % (shape, sc.name)
        assert not any(chr(v) == "Z" for f in tr.frames for v in f.screen.reshape(-1)), "%s %s shows a 'Z'" % (shape, sc.name)
        for what, holds in sc.claims.items():
            assert holds(tr), "%s %s does not reach: %s\n%s" % (shape, sc.name, what, "\n".join(
                "%r %s %s\n%s" % (f.key, f.reactions, f.pos, "\n".join(bytes(r).decode() for r in f.screen[:12, :24])) for f in tr.frames[:12]))
    # a key after which the Mirror differs from a fresh draw of the state / from the state's status: many of them
    assert stale_screens >= 20 and stale_status >= 5, (shape, stale_screens, stale_status)


@pytest.mark.parametrize("shape", list(su.SHAPES))
def test_only_the_scenarios_that_claim_a_death_drop_out(shape):
    """tests/test_gpu_draw_scenarios.py drops a scenario from its death key on; the scenarios that do are exactly those that claim it."""
    scs = ds.all_scenarios(shape)
    died = [sc.name for sc in scs if ds.play(sc).died_at is not None]
    claimed = [sc.name for sc in scs if sc.claims.get("died") or sc.claims.get("died_in_run")]
    assert died == claimed, (shape, died, claimed)
    assert len(died) == (0 if shape == "160x48" else 2)


# ---- six wrong readings of the Rust text ----------------------------------------------------------------------------------------------
class BothInside(su.CountingShadow):       # (a) in_same_room as "both inside the rect"
    def in_same_room(self, a, b):
        rid = self.room_of(a)
        if rid is None or self.room_of(b) != rid:
            return False
        if self.rooms[rid]["kind"] == 2:
            return True
        x0, y0, x1, y1 = self.rooms[rid]["range"]
        return x0 <= a[0] < x1 and y0 <= a[1] < y1 and x0 <= b[0] < x1 and y0 <= b[1] < y1


class MonsterOverGold(su.CountingShadow):  # (b) the monster drawn over gold
    def object_at(self, p):
        if p == self.pos:
            return "@"
        m = self.placed.get(p) or self.active.get(p)
        if m is not None and self.draw_enemy(p):
            return m.glyph
        return "*" if self.idx(*p) in self.items else None


class RedrawEveryKey(su.CountingShadow):   # (c) a Redraw after every key
    def process_action(self, key, new_level):
        grave = super().process_action(key, new_level)
        self.reactions.append(st.REDRAW)
        return grave


class StatusEveryKey(su.CountingShadow):   # (d) the status refreshed after every key
    def process_action(self, key, new_level):
        grave = super().process_action(key, new_level)
        self.reactions.append(st.STATUS)
        return grave


class AllRows(su.CountingShadow):          # (e) rows 0 and H - 1 drawn
    def draw_rows(self):
        return range(0, self.H)


class VisibleOnly(su.CountingShadow):      # (f) objects drawn only on IS_VISIBLE cells
    def obj_visible(self, attr):
        return bool(attr & st.VISIBLE)


MISREADINGS = (BothInside, MonsterOverGold, RedrawEveryKey, StatusEveryKey, AllRows, VisibleOnly)


def final_mirror(sc, cls):
    m = ds.play(sc, cls).play.sh.mirror
    return m.screen.tobytes(), m.hist.tobytes(), tuple(m.status)


@pytest.fixture(scope="module")
def right_mirrors():
    return {shape: [final_mirror(sc, su.CountingShadow) for sc in ds.scenarios(shape)] for shape in su.SHAPES}


@pytest.mark.parametrize("cls", MISREADINGS, ids=[c.__name__ for c in MISREADINGS])
def test_the_set_sees_every_wrong_reading(cls, right_mirrors):
    for shape in su.SHAPES:
        scs = ds.scenarios(shape)
        differing = [sc.name for sc, right in zip(scs, right_mirrors[shape]) if final_mirror(sc, cls) != right]
        print("%-16s %-7s ends with another mirror in: %s" % (cls.__name__, shape, differing))
        assert differing, "%s: no draw scenario of %s ends with another mirror" % (cls.__name__, shape)
