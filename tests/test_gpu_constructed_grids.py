"""k_path (rogue-gym_amd/csrc/rg_path.hip) and k_action_mask (rg_action_mask.hip) on grids of the test's own making, loaded as state records
(tests/grid_util.py inject): walks of thousands of moves, which set the high distance planes of the field pass and keep the keys-only pass running for
hundreds of blocks beside a group that finished in block 0; walkable borders, where only the zeros the row shifts bring in and the `there` select keep one
env's frontier out of its neighbour in the wave; every row-word count, wave shape and store alignment; and hidden, locked, stairs and gold words at every
word seam.  The conditions that make these inputs hard are asserted on the reference in tests/test_constructed_grids_host.py; here the kernels' own output
is asserted to have seen them.  An injected handle is only ever read: rg_path, rg_action_mask, rg_debug_fetch, rg_fetch_states, rg_dev_read, rg_sync."""
import time

import numpy as np
import pytest

import grid_util as gu
import mask_util as mu
import path_util as pu
from parity_util import HipBatch
from path_util import GOAL_CELL, INF, path_call, ptr, read

pytestmark = pytest.mark.gpu

# players per grid (twelve grids per shape): the env count leaves the last wave partly empty where a wave holds more than one env
PER_GRID = {"32x16": 8, "33x17": 6, "64x32": 5, "96x32": 4, "80x24": 5, "104x20": 4, "128x16": 5, "97x33": 4, "160x48": 3}


def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def lib():
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def shape_envs(name):
    """[(Ref, px, py, dead, cell)] in env order: on the shapes with H == GS the four border envs A, B, B, A' first -- they fill whole waves --, then the
    twelve grids in turn, less the last env."""
    h = gu.SHAPES[name][1]
    return (gu.border_pairs(name) if h in (16, 32) else []) + gu.shape_cases(name, PER_GRID[name])[:-1]


_HANDLES = {}


def injected(name):
    """(HipBatch, envs) of a shape, injected once per process and shared by the tests that read it."""
    if name not in _HANDLES:
        envs = shape_envs(name)
        hip = HipBatch(gu.shape_config(name), [4000 + i for i in range(len(envs))], max_steps=1000, auto_reset=True)
        assert (hip.h.width, hip.h.height) == gu.SHAPES[name][:2]
        gu.inject(hip, np.stack([e[0].grid for e in envs]), [(e[1], e[2]) for e in envs], [e[3] for e in envs])
        _HANDLES[name] = (hip, envs)
    return _HANDLES[name]


@pytest.mark.parametrize("name", list(gu.SHAPES))
def test_path_on_constructed_grids(lib, name):
    """rg_path with the field and rg_path without it (the pass that stops at the player) against rg_path_host and path_util.Graph, every env: the whole
    field, distance and key, for goals 1, 2, 3, 4 + cell and 5 + cell.  No config of these sizes is refused at creation."""
    torch_mod()
    t0 = time.time()
    hip, envs = injected(name)
    hd, n = hip.h, hip.n
    cells = np.array([e[4] for e in envs], np.int32)
    seen, far, far_field, unreachable = set(), 0, 0, 0
    for goals in gu.GOAL_SETS:
        cc = cells if goals & GOAL_CELL else None
        f, d, k = path_call(hd, goals, cc)
        _, d2, k2 = path_call(hd, goals, cc, field=False)
        for i, (ref, px, py, dead, cell) in enumerate(envs):
            cell = cell if goals & GOAL_CELL else (-1, -1)
            tag = "%s env %d (%s) player (%d, %d) dead %d goals %d cell %s" % (name, i, ref.name, px, py, dead, goals, cell)
            hf, hdist, hk = pu.host(lib, ref.grid, px, py, goals, dead, cell)
            ef, ed, ek = ref.answer(px, py, dead, goals, cell)
            assert np.array_equal(hf, ef) and hdist == ed and hk == ek, tag + ": host entry vs numpy rule"
            if not np.array_equal(f[i], hf):
                bad = np.argwhere(f[i] != hf)
                raise AssertionError("%s: %d field cells differ, first (y, x) = %s: kernel %d, host entry %d" % (tag, len(bad), tuple(bad[0]), f[i][tuple(bad[0])], hf[tuple(bad[0])]))
            assert d[i] == hdist and k[i] == hk, "%s: field pass dist %d key %r, host entry dist %d key %r" % (tag, d[i], chr(k[i]), hdist, chr(hk))
            assert d2[i] == hdist and k2[i] == hk, "%s: keys-only pass dist %d key %r, host entry dist %d key %r" % (tag, d2[i], chr(k2[i]), hdist, chr(hk))
        seen |= set(bytes(k).decode()) | set(bytes(k2).decode())
        far = max(far, int(d.max()), int(d2.max()))
        far_field = max(far_field, int(np.where(f == INF, 0, f).max()))
        unreachable += int((d < 0).sum())
    hip.sync()
    line = "%s: largest distance at a player %d, in a field %d, keys seen %s, unreachable answers %d, envs checked %d x %d goal sets x 2 passes, %.2f s" % (
        name, far, far_field, "".join(sorted(seen)), unreachable, n, len(gu.GOAL_SETS), time.time() - t0)
    print(line)
    bound = 4096 if name == "160x48" else 256
    assert far >= bound and far_field >= bound, line  # (at a player: the keys-only pass ran that far too)
    assert len(seen & set("kjhlyubn")) >= 6 and {">", ".", "s"} <= seen, line
    h = gu.SHAPES[name][1]
    if h in (16, 32):  # B beside A: nothing of A's goal reaches it
        f, d, k = path_call(hd, 1)
        assert (f[1] == INF).all() and (f[2] == INF).all() and d[1] == d[2] == -1 and k[1] == k[2] == ord("s")
        assert f[0].max() < INF and f[3].max() < INF and d[0] > 0 and d[3] > 0


def mask_call(hd):
    """rg_action_mask over mu.KEYS into a buffer pre-filled with 0xAA -> rows u8 [n][11]; the bytes behind the last env keep their fill."""
    import torch
    nk = len(mu.KEYS)
    m = torch.full((hd.n * nk + 64,), 0xAA, dtype=torch.uint8, device="cuda:%d" % hd.device)
    torch.cuda.synchronize()
    hd.check(hd.L.rg_action_mask(hd.h, mu.KEYS, nk, ptr(m), None, 0, 0))
    out = read(hd, m)
    assert (out[hd.n * nk:] == 0xAA).all(), "the mask pass wrote behind the last env"
    return out[:hd.n * nk].reshape(hd.n, nk)


@pytest.mark.parametrize("name", ["32x16", "33x17", "160x48"])
def test_action_mask_on_constructed_grids(lib, name):
    """The same injected handles: rg_action_mask over mu.KEYS against the host entry and the numpy rule, every env."""
    torch_mod()
    hip, envs = injected(name)
    got = mask_call(hip.h)
    why = {}
    for i, (ref, px, py, dead, _) in enumerate(envs):
        exp = mu.rule(ref.graph.surf, ref.graph.attr, px, py, dead, why=why)
        assert np.array_equal(mu.host_row(lib, ref.grid, px, py, dead), exp), "%s env %d: host entry vs numpy rule" % (name, i)
        assert np.array_equal(got[i], exp), "%s env %d (%s) player (%d, %d) dead %d: kernel %s, rule %s" % (name, i, ref.name, px, py, dead, got[i], exp)
    hip.sync()
    print(name, "move keys by reason", dict(sorted(why.items())))
    assert all(why.get(r, 0) > 0 for r in ("ok", "out", "wall", "corner")), why


def test_action_mask_every_neighbourhood():
    """One 32 x 16 handle of 13 122 envs: every assignment of {free, hidden or locked, wall} to the eight neighbours of a floor and of a stairs cell, stamped
    at positions cycling through the interior, the four corners and the four edges.  The mask of every env equals mu.rule, and every one of the 2^8
    direction patterns occurs in the kernel's output.  (Reading 13 122 envs back one by one takes longer than the test may: every 16th env is read back by
    rg_debug_fetch, the flag words of all; the handle does not expose the addresses of its cell and position arrays.)"""
    torch_mod()
    t0 = time.time()
    grids, players, interior = gu.stamped()
    exp = gu.rule_rows(grids, players)
    hip = HipBatch(gu.shape_config("32x16"), [9000 + i for i in range(len(grids))], max_steps=1000, auto_reset=True)
    gu.inject(hip, grids, players, np.zeros(len(grids), np.uint32), check_every=16)
    got = mask_call(hip.h)
    hip.sync()
    if not np.array_equal(got, exp):
        bad = np.flatnonzero((got != exp).any(axis=1))
        raise AssertionError("%d rows differ, first env %d at %s: kernel %s, rule %s" % (len(bad), bad[0], players[bad[0]], got[bad[0]], exp[bad[0]]))
    patterns = set(gu.direction_pattern(got[interior]).tolist())
    alone = set(gu.direction_pattern(gu.rule_rows(gu.neighbourhoods()[:6561], [(1, 1)] * 6561)).tolist())
    line = "every neighbourhood: %d envs, %d direction patterns among the interior ones, '>' legal %d, %.2f s" % (len(grids), len(patterns), int(got[:, 9].sum()), time.time() - t0)
    print(line)
    assert patterns == alone and len(alone) == 256 and int(got[:, 9].sum()) == 6561, line
