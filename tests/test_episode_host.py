"""rg_scout_host (the bitmap rule of the episode accounting on one grid, no GPU) against the numpy restatement of tests/episode_util.py: on the CPU engine's
grids through play, after every step, and on constructed grids of every shape; and the ABI around it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import episode_util as eu
import grid_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def _play(lib, goldens, name, n):
    """After every step of every env the host entry takes the step the numpy rule took -- from the bitmap as it was before the step, emptied where the rule
    empties it (a new game, another level) -- and must leave the same bytes and pay the same."""
    cfg, seeds, table, max_steps = eu.run_setup(goldens, name, n)
    checked = [0]

    def on_step(t, e, o, lanes, done, before):
        seen, level = before
        if done or level != lanes.level[e]:
            seen[:] = 0
        fresh = eu.scout_host(lib, eu.engine_cells(o), seen)
        assert np.array_equal(seen, lanes.seen[e]), (name, t, e)
        if not done:
            assert fresh == lanes.scout[e], (name, t, e, fresh, lanes.scout[e])
        checked[0] += 1

    run = eu.Run(cfg, seeds, table, max_steps, on_step=on_step)
    assert checked[0] == len(seeds) * len(table)
    return run


def test_scout_host_on_the_engine_grids_mini(lib, goldens):
    run = _play(lib, goldens, "mini60", 136)
    f = run.floors()
    print(f)
    # measured with exactly this run: 245 deaths, 167 time limits, 14 descents, 3 016 newly known cells; asserted at half
    assert f["deaths"] >= 122 and f["time_limits"] >= 83 and f["descents"] >= 7 and f["new_cells"] >= 1508, f


def test_scout_host_on_the_engine_grids_33x17(lib, goldens):
    """H * W = 561: a partial last byte and pad bytes."""
    run = _play(lib, goldens, "33x17", 135)
    f = run.floors()
    print(f)
    # measured with exactly this run: 108 deaths, 212 time limits, 7 descents, 1 death on the last allowed step, 1 584 newly known cells; asserted at half
    assert f["deaths"] >= 54 and f["time_limits"] >= 106 and f["descents"] >= 3 and f["new_cells"] >= 792, f


@pytest.mark.parametrize("name", sorted(gu.SHAPES))
def test_scout_host_on_constructed_grids(lib, name):
    w, h = gu.SHAPES[name][:2]
    rng = np.random.RandomState(4000 + w * h)
    for p in (0.05, 0.5, 0.95):
        g = eu.random_known(rng, w, h, p)
        seen_np, seen_h = np.zeros(eu.seen_bytes(w * h), np.uint8), np.full(eu.seen_bytes(w * h), 0, np.uint8)
        fresh = eu.scout_step(eu.known_bits(g), seen_np)
        assert eu.scout_host(lib, g, seen_h) == fresh
        assert np.array_equal(seen_h, seen_np)
        bits = np.unpackbits(seen_h, bitorder="little")
        assert not bits[:w].any() and not bits[(h - 1) * w:].any(), "row 0, row H - 1 and the pad bits stay 0"
        assert eu.scout_host(lib, g, seen_h) == 0 and np.array_equal(seen_h, seen_np)
    a, b, n_a, n_b_only = eu.abA(w, h, rng)
    seen = np.zeros(eu.seen_bytes(w * h), np.uint8)
    assert eu.scout_host(lib, a, seen) == n_a
    assert eu.scout_host(lib, b, seen) == n_b_only        # |B \ A|: what dropped off the map stays seen
    assert eu.scout_host(lib, a, seen) == 0               # ... and is never paid twice
    ref = eu.known_bits(a) | eu.known_bits(b)
    assert np.array_equal(seen, ref)
    dirty = np.full(eu.seen_bytes(w * h), 0xFF, np.uint8)   # a caller's pad bits are written 0
    eu.scout_host(lib, a, dirty)
    bits = np.unpackbits(dirty, bitorder="little")
    assert not bits[:w].any() and not bits[(h - 1) * w:].any() and bits[w:(h - 1) * w].all()


def test_header_symbols_and_record_size(lib):
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for n in ("rg_episode_enable", "rg_episode_update", "rg_episode_cut", "rg_episode_arrays", "rg_episode_log_read", "rg_scout_host"):
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), "missing export %s" % n
    m = re.search(r"typedef struct rg_episode_rec \{([^}]*)\}", hdr)
    fields = [f.split() for f in m.group(1).split(";") if f.strip()]
    size = {"uint32_t": 4, "int32_t": 4, "float": 4}
    assert sum(size[t] for t, _ in fields) == 32 and [n for _, n in fields] == list(eu.REC.names)
    assert eu.REC.itemsize == 32
    from rogue_gym_python import _rogue_gym as inner
    assert np.dtype(inner.EPISODE_REC) == eu.REC
    assert C.sizeof(inner.RgEpisodeArrays) == 11 * 8 + 8
    for name, val in (("RG_EP_STATS", 1), ("RG_EP_SCOUT", 2), ("RG_EP_DIED", 1), ("RG_EP_TIME_LIMIT", 2), ("RG_EP_CUT", 3)):
        assert re.search(r"#define %s\s+%du" % (name, val), hdr), name


def test_scout_host_refusals(lib):
    g = np.zeros((16, 32), np.uint16)
    seen = np.zeros(64, np.uint8)
    fresh = C.c_int32(0)
    for args, frag in (((None, 16, 32, seen.ctypes.data, C.byref(fresh)), "cells"),
                       ((g.ctypes.data, 16, 32, None, C.byref(fresh)), "seen_inout"),
                       ((g.ctypes.data, 0, 32, seen.ctypes.data, C.byref(fresh)), "height"),
                       ((g.ctypes.data, 16, 161, seen.ctypes.data, C.byref(fresh)), "width"),
                       ((g.ctypes.data, 49, 32, seen.ctypes.data, C.byref(fresh)), "height"),
                       ((g.ctypes.data, 16, -1, seen.ctypes.data, C.byref(fresh)), "width")):
        assert lib.rg_scout_host(*args) != 0
        msg = lib.rg_last_error(None).decode()
        assert msg.startswith("rg_scout_host:") and frag in msg, msg
    assert lib.rg_scout_host(g.ctypes.data, 16, 32, seen.ctypes.data, None) == 0   # fresh_out is optional
