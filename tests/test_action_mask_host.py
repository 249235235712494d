"""The legal-action rule without a GPU: rg_action_mask_host (the rule of rogue-gym_amd/csrc/rg_action_mask.h, which the kernel shares) on hand-built grids
and against the CPU oracle in lock-step, rg_sample_index against Python integers, and the refusals of the host entry."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import mask_util as mu
from mask_util import KEYS, RUN_A, RUN_B, RUN_C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rg_action_mask", "rg_action_mask_host", "rg_sample_index")
FLOOR, WALL, STAIR, NONE = 1, 2, 4, 7   # surfaces (rg_state.h)
HIDDEN, LOCKED = 0x20, 0x100            # C_HIDDEN, C_LOCKED


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def test_entry_points_declared_exported_and_bound(lib):
    from rogue_gym_python import _rogue_gym as inner
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for n in NAMES:
        assert re.search(r"^(int|uint32_t) %s\(" % n, hdr, re.M), "not declared: " + n
        assert hasattr(lib, n), "not exported: " + n
        assert getattr(lib, n).argtypes is not None, "no ctypes signature: " + n
    assert '#define RG_ACTION_KEYS ".hjklnbuy>s"' in hdr and "#define RG_MASK_MAX_KEYS 32" in hdr
    assert lib.rg_sample_index.restype is C.c_uint32
    assert "rg_action_mask" in inner._INT_FUNCS and "rg_action_mask_host" in inner._INT_FUNCS and "rg_sample_index" not in inner._INT_FUNCS
    from rogue_gym.envs import RogueEnv
    assert "".join(RogueEnv.ACTIONS).encode() == KEYS and inner.N_ACTION_KEYS == len(KEYS)


def grid5(**cells):
    """5 x 5 of floor with the named cells replaced: grid5(x2y1=WALL)."""
    g = np.full((5, 5), FLOOR, np.uint16)
    for name, v in cells.items():
        x, y = int(name[1]), int(name[3])
        g[y, x] = v
    return g


def legal(lib, g, px, py, key, dead=0):
    return int(mu.host_row(lib, g, px, py, dead, key.encode())[0])


def test_rule_clause_by_clause(lib):
    open5 = grid5()
    assert list(mu.host_row(lib, open5, 2, 2, 0)) == [1] * 9 + [0, 1]  # open floor: everything but '>'
    # a target out of the grid, on each of the four edges (and the diagonals that leave with it)
    for px, py, gone in ((0, 2, "hyb"), (4, 2, "lun"), (2, 0, "kyu"), (2, 4, "jbn")):
        for key in "hjklyubn":
            assert legal(lib, open5, px, py, key) == (key not in gone), (px, py, key)
    assert [legal(lib, open5, 0, 0, k) for k in "hjklyubn"] == [0, 1, 0, 1, 0, 0, 0, 1]
    assert [legal(lib, open5, 4, 4, k) for k in "hjklyubn"] == [1, 0, 1, 0, 1, 0, 0, 0]
    # a wall target (either kind) and a bare cell
    for s in (WALL, 3, NONE):
        assert legal(lib, grid5(x3y2=s), 2, 2, "l") == 0 and legal(lib, grid5(x3y2=s), 2, 2, "h") == 1
    # every other surface can be walked on: passage, floor, stairs, door, trap
    for s in (0, 1, 4, 5, 6):
        assert legal(lib, grid5(x3y2=s), 2, 2, "l") == 1
    # a hidden target with a walkable surface; a locked target
    assert legal(lib, grid5(x3y2=FLOOR | HIDDEN), 2, 2, "l") == 0
    assert legal(lib, grid5(x3y2=5 | LOCKED), 2, 2, "l") == 0
    assert legal(lib, grid5(x2y1=0 | HIDDEN), 2, 2, "k") == 0 and legal(lib, grid5(x2y3=5 | LOCKED), 2, 2, "j") == 0
    # the other attr bits (visited, visible, drawn, dark), the door, maze and gold marks do not matter
    assert legal(lib, grid5(x3y2=FLOOR | 0x10 | 0x40 | 0x80 | 0x200 | 0x8 | 0x400 | 0x800), 2, 2, "l") == 1
    # a diagonal blocked by ONE orthogonal wall, on each side ('n' = right-down: its orthogonals are (3, 2) and (2, 3))
    assert legal(lib, grid5(x3y2=WALL), 2, 2, "n") == 0 and legal(lib, grid5(x2y3=3), 2, 2, "n") == 0
    assert legal(lib, grid5(x1y2=WALL), 2, 2, "y") == 0 and legal(lib, grid5(x2y1=3), 2, 2, "y") == 0
    assert legal(lib, grid5(x3y2=NONE), 2, 2, "u") == 0 and legal(lib, grid5(x2y1=WALL), 2, 2, "u") == 0
    assert legal(lib, grid5(x1y2=WALL), 2, 2, "b") == 0 and legal(lib, grid5(x2y3=WALL), 2, 2, "b") == 0
    assert legal(lib, grid5(x1y2=WALL), 2, 2, "n") == 1  # (a wall that is not one of ITS orthogonals)
    # ... whose orthogonal neighbour is hidden or locked but walkable: legal (surface only, floor.rs:177-180)
    assert legal(lib, grid5(x3y2=FLOOR | HIDDEN, x2y3=5 | LOCKED), 2, 2, "n") == 1
    assert legal(lib, grid5(x3y3=FLOOR | HIDDEN), 2, 2, "n") == 0  # (the target itself is still judged)
    # stairs under the player versus beside them
    st = grid5(x2y2=STAIR)
    assert legal(lib, st, 2, 2, ">") == 1 and legal(lib, st, 1, 2, ">") == 0 and legal(lib, st, 3, 3, ">") == 0
    assert legal(lib, grid5(x2y2=STAIR | HIDDEN), 2, 2, ">") == 1  # (the surface alone)
    # the Grave modal: every key 0, '.' included
    assert not mu.host_row(lib, st, 2, 2, 1).any() and not mu.host_row(lib, st, 2, 2, 1, b"HJKLYUBN").any()
    # every run key equals its lower-case key
    rng = np.random.RandomState(3)
    for _ in range(200):
        g = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 1 | HIDDEN, 5 | LOCKED], np.uint16), size=(5, 5))
        px, py = rng.randint(0, 5, 2)
        low, up = mu.host_row(lib, g, px, py, 0, b"hjklyubn"), mu.host_row(lib, g, px, py, 0, b"HJKLYUBN")
        assert np.array_equal(low, up)
        surf, attr = (g & 7).astype(np.uint8), ((g >> 4) & 0x3F).astype(np.uint8)
        assert np.array_equal(mu.host_row(lib, g, px, py, 0), mu.rule(surf, attr, px, py, False))  # (and the numpy restatement agrees on arbitrary grids)
    # duplicates and order are the caller's
    assert list(mu.host_row(lib, st, 2, 2, 0, b">>.>")) == [1, 1, 1, 1] and list(mu.host_row(lib, open5, 0, 2, 0, b"hlh")) == [0, 1, 0]


def lockstep_host(lib, goldens, run):
    from parity_util import make_oracles
    cfg, seeds, table = mu.run_config(goldens, run)
    oracles = make_oracles(cfg, seeds, max_steps=run["max_steps"])
    st, died_at = mu.Stats(), {}
    for t in range(run["T"] + 1):
        for i, o in enumerate(oracles):
            exp = mu.oracle_row(o, why=st.why)
            got = mu.host_row_of_oracle(lib, o)
            assert np.array_equal(got, exp), "t=%d env %d: %s vs %s" % (t, i, got, exp)
            st.add(o, exp)
            if o.flags()["dead"]:
                died_at.setdefault(i, t)
                assert not got.any(), "t=%d env %d is dead (since t=%d) and has a legal key" % (t, i, died_at[i])
        if t < run["T"]:
            mu.step_oracles(oracles, table[t], run["auto_reset"])
    print(st)
    return st, died_at


def test_host_rule_against_the_oracle_mini_autoreset(lib, goldens):
    """Run a.  On the CPU oracle these inputs gave 16 456 rows, '>' legal in 225, corner-rule-only refusals 6 857, out-of-grid targets 987, rows on
    level >= 2 317: the floors are about half of that, so that a change of inputs cannot quietly empty a case."""
    st, _ = lockstep_host(lib, goldens, RUN_A)
    assert st.rows == 136 * 121
    assert st.stairs >= 100 and st.why.get("corner", 0) >= 3000 and st.why.get("out", 0) >= 400 and st.deep >= 100, str(st)


def test_host_rule_against_the_oracle_80x24(lib, goldens):
    """Run b: hidden-or-locked-but-walkable targets 29, corner 1 834 on the CPU oracle."""
    st, _ = lockstep_host(lib, goldens, RUN_B)
    assert st.rows == 72 * 101
    assert st.why.get("hidden", 0) >= 10 and st.why.get("corner", 0) >= 800, str(st)


def test_host_rule_against_the_oracle_dead_envs(lib, goldens):
    """Run c, no auto-reset: 61 envs die on the CPU oracle; their rows are all zero from the step they die."""
    st, died_at = lockstep_host(lib, goldens, RUN_C)
    assert len(died_at) >= 30, (len(died_at), str(st))


def test_sample_index_matches_python_integers(lib):
    f = lib.rg_sample_index
    rnd = random.Random(11)
    for _ in range(10000):
        seed, env, draw, count = rnd.getrandbits(64), rnd.getrandbits(32), rnd.getrandbits(64), rnd.randint(1, 32)
        got = f(seed, env, draw, count)
        assert got == mu.sample_reference(seed, env, draw, count) and got < count, (seed, env, draw, count, got)
    top = (1 << 64) - 1
    for seed in (0, 1, top, top - 1, 1 << 63):
        for draw in (0, 1, top, top - 7, 1 << 63):
            for env in (0, 1, (1 << 32) - 1, (1 << 31)):
                assert f(seed, env, draw, 0) == 0 and f(seed, env, draw, 1) == 0
                for count in (2, 11, 32, (1 << 32) - 1):
                    got = f(seed, env, draw, count)
                    assert got == mu.sample_reference(seed, env, draw, count) and got < count, (seed, env, draw, count, got)
    # the draws spread: 11 keys over 4096 envs, every index taken, none by more than twice its share
    hist = np.bincount([f(5, e, 9, 11) for e in range(4096)], minlength=11)
    assert hist.min() > 0 and hist.max() < 2 * 4096 / 11, hist


def test_host_entry_refusals_name_the_argument(lib):
    g = grid5()
    out = np.full(40, 0xAA, np.uint8)

    def refused(keys, n):
        rc = lib.rg_action_mask_host(g.ctypes.data, 5, 5, 2, 2, 0, keys, n, out.ctypes.data)
        assert rc != 0 and (out == 0xAA).all()
        return lib.rg_last_error(None).decode()

    msg = refused(b"h", 0)
    assert "rg_action_mask_host" in msg and "n_keys" in msg and "got 0" in msg
    msg = refused(b"h" * 33, 33)
    assert "rg_action_mask_host" in msg and "n_keys" in msg and "33" in msg
    msg = refused(b"hjxk", 4)
    assert "rg_action_mask_host" in msg and "keys[2]" in msg and "0x78" in msg and "'x'" in msg
    for bad in (b"i", b" ", b"<", b"S", b"\x00", b"\xeb", b"K\x0b"):
        assert "keys[%d]" % (len(bad) - 1) in refused(bad, len(bad))
    assert "(px, py)" in (lambda: (lib.rg_action_mask_host(g.ctypes.data, 5, 5, 5, 2, 0, b"h", 1, out.ctypes.data), lib.rg_last_error(None).decode())[1])()
    assert lib.rg_action_mask_host(g.ctypes.data, 5, 5, 2, 2, 0, b"h" * 32, 32, out.ctypes.data) == 0 and (out[:32] == 1).all()  # 32 keys are served
    out[:] = 0xAA
    assert lib.rg_action_mask_host(g.ctypes.data, 5, 5, 2, 2, 0, None, 0, out.ctypes.data) == 0 and list(out[:12]) == [1] * 9 + [0, 1, 0xAA]  # NULL: the 11 default keys
