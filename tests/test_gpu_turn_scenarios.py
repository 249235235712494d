"""k_step's turn on constructed states (tests/turn_scenarios.py) against the second restatement of the reference's turn (tests/shadow_turn.py), bit for bit.

Every other parity test of the turn plays dungeons the level generator made; these states have walkable borders, chasers on both sides of a row-word seam,
walks of hundreds of moves, maps cached before a wall opened, every monster slot alive in one corridor, and players of level 21.  One env per scenario,
loaded through the handle's own state records (tests/state_util.py), then the scripts key by key: after every key the whole rg_debug_fetch state, the cell
words, the gold table and the rooms' visited bits of every env against the Shadow, and the step's reward and done against its gold and Grave result.  At the
end the mirrors against a twin handle that draws every Redraw from the tiles, on the partial-map shapes the whole state against a twin that expands every map
to the end, and the dist-map counter against the Shadow's make_dist_map calls.

The counter (rg_counters [2], rg_kernels.hip n_bfs) counts the turns that built OR CONTINUED a map: cache misses, plus -- on the partial-map shapes only --
every continuation of a cached partial map.  So it equals the Shadow's count of cache misses on the other shapes and on the full-BFS twin, which is asserted;
on the partial-map shapes both figures are printed and the handle's may only be larger."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import state_util as su
import turn_scenarios as ts

pytestmark = pytest.mark.gpu

PUBLIC_FLAGS = 0x00FF7F03  # terminal, dead, message bits, error bits (the mirror bookkeeping bits differ between the twins by construction)


def make_handle(shape, n, env=None):
    from rogue_gym_python import _rogue_gym as inner

    cfgs = [json.dumps(su.scenario_config(shape, seed=4000 + i)) for i in range(n)]
    if env:
        os.environ[env] = "1"
    try:
        return inner._Handle(cfgs, 100000, auto_reset=True)
    finally:
        if env:
            os.environ.pop(env, None)


def step_results(hd):
    """(reward f32 [n], done u8 [n]) of the last step."""
    out = []
    for fn, dt in ((hd.L.rg_reward, np.float32), (hd.L.rg_done, np.uint8)):
        dev = C.c_void_p()
        hd.check(fn(hd.h, C.byref(dev)))
        a = np.empty(hd.n, dt)
        hd.check(hd.L.rg_dev_read(hd.h, dev, a.ctypes.data, a.nbytes))
        out.append(a)
    return out


def counters(hd):
    c = (C.c_uint64 * 8)()
    hd.check(hd.L.rg_counters(hd.h, c, 0))
    return list(c)


@pytest.mark.parametrize("shape", list(su.SHAPES))
def test_turn_on_constructed_states_equals_the_shadow(shape):
    t_start = time.time()
    scs = ts.scenarios(shape)
    n = len(scs)
    states = [sc.state for sc in scs]
    main = make_handle(shape, n)
    twins = {"tiles": make_handle(shape, n, "ROGUE_GYM_HIP_NO_MIRROR_UPDATE")}
    if shape in su.PARTIAL:
        twins["full"] = make_handle(shape, n, "ROGUE_GYM_HIP_FULL_BFS")
    for hd in [main] + list(twins.values()):
        su.inject(hd, states)   # (no record refused; rg_debug_fetch of every env gives back the description)
    base = {name: counters(hd)[2] for name, hd in [("main", main)] + list(twins.items())}
    plays = [ts.Play(sc) for sc in scs]
    compared = 0
    for t in range(max(len(sc.keys) for sc in scs)):
        was_over = [p.over for p in plays]
        want = [p.step() for p in plays]
        keys = np.frombuffer("".join(k for k, _, _ in want).encode(), np.uint8).copy()
        for hd in [main] + list(twins.values()):
            hd.check(hd.L.rg_step(hd.h, keys.ctypes.data, 0))
        reward, done = step_results(main)
        for i, (p, (k, gold, grave)) in enumerate(zip(plays, want)):
            if was_over[i]:
                continue   # its Shadow died on an earlier key: the env was reset and is out of the comparison
            where = "%s env %d (%s) key %d %r" % (shape, i, scs[i].name, t, k)
            assert (float(reward[i]), bool(done[i])) == (float(gold), grave), "%s: reward / done %s, the Shadow's gold / Grave %s" % (where, (reward[i], done[i]), (gold, grave))
            if p.over:
                continue   # died on this key: the env holds its next episode already
            got, steps = su.fetched(main, i)
            diff = su.differences(got, su.expected(p.sh))
            assert not diff and steps == t + 1, "%s: %s steps %d" % (where, diff, steps)
            compared += 1
    # ---- the twins ----
    a = main.fetch()
    for name, hd in twins.items():
        b = hd.fetch()
        for x, y, what in zip(a[:3], b[:3], ("screen", "hist", "status")):
            assert np.array_equal(x, y), "%s: %s differs from the %s twin for envs %s" % (shape, what, name, [i for i in range(n) if not np.array_equal(x[i], y[i])])
        assert np.array_equal(a[3] & PUBLIC_FLAGS, b[3] & PUBLIC_FLAGS), "%s: flags differ from the %s twin" % (shape, name)
    if "full" in twins:
        for i in range(n):
            assert su.fetched(main, i) == su.fetched(twins["full"], i), "%s env %d (%s): partial maps and whole maps end in different states" % (shape, i, scs[i].name)
    # ---- the dist-map counter ----
    shadow_maps = sum(p.sh.ev["maps"] for p in plays)
    cm = counters(main)
    built = cm[2] - base["main"]
    print("%s: %d envs, %d env-keys compared, dist maps: Shadow %d, handle %d (continued over a saved mask: %d)%s, %.1f s" % (
        shape, n, compared, shadow_maps, built, cm[7], "" if "full" not in twins else ", full-BFS twin %d" % (counters(twins["full"])[2] - base["full"]), time.time() - t_start))
    if shape in su.PARTIAL:
        cf = counters(twins["full"])
        assert cf[2] - base["full"] == shadow_maps and cf[7] == 0 and built >= shadow_maps, (shadow_maps, built, cf)
        assert cm[7] >= 1, "no partial map was continued over its saved walkable mask: the woken sleeper did not reach that path"
    else:
        assert built == shadow_maps, (built, shadow_maps)
    for hd in [main] + list(twins.values()):
        hd.check(hd.L.rg_sync(hd.h))
        hd.close()
