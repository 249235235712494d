"""The learner's side of the action rule on the CPU (rg_policy_eval_host, rg_policy_grad_host; rogue-gym_amd/csrc/rg_policy_grad.h): the forward against rg_act_host
in RG_ACT_GIVEN mode bit for bit, the special rows, the zero gradients, the 16-bit rounding against Python integers, the gradient against the float64 NaN-safe
torch chain, the refusals, the numpy value form -- and the rule's source in a stand-alone program built with -fsanitize=address,undefined."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mask_util as mu
import policy_edge_rows as pe
import policy_grad_util as pg
import policy_util as pu
from policy_grad_util import BF16, F16, F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rg_policy_eval": 10, "rg_policy_grad": 11, "rg_policy_eval_host": 9, "rg_policy_grad_host": 10}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


@pytest.fixture(scope="module")
def inner():
    from rogue_gym_python import _rogue_gym as inner
    return inner


def test_entry_points_declared_exported_and_bound(lib, inner):
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for n, n_args in ENTRIES.items():
        assert re.search(r"^int %s\(" % n, hdr, re.M), "not declared: " + n
        assert hasattr(lib, n), "not exported: " + n
        assert len(inner._ABI[n][0]) == n_args and n in inner._INT_FUNCS
    import rogue_gym
    from rogue_gym.envs.device import HipVecRogueEnv
    assert callable(rogue_gym.masked_logp) and callable(rogue_gym.masked_logp_np) and callable(HipVecRogueEnv.evaluate)
    assert "masked_logp" in HipVecRogueEnv.act.__doc__


def grids(lib, rng, n):
    """n (grid, key list, legal bool [11]) on policy_util.grid5 grids: random walls around the player, the stairs under it or not; the dead env among them."""
    out = []
    while len(out) < n:
        g = pu.grid5(x2y2=pu.STAIR if rng.randint(2) else pu.FLOOR)
        for x, y in ((1, 1), (2, 1), (3, 1), (1, 2), (3, 2), (1, 3), (2, 3), (3, 3)):
            if rng.randint(3) == 0:
                g[y, x] = pu.WALL
        keys = pu.KEYS if rng.randint(2) else b"hjklnbuy>hj"
        dead = int(len(out) % 16 == 7)
        out.append((g, keys, dead, mu.host_row(lib, g, 2, 2, dead, keys).astype(bool)))
    return out


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_eval_equals_act_host_given_bit_for_bit(lib, inner, dtype):
    rng = np.random.RandomState(3 + dtype)
    cases = grids(lib, rng, 160)
    assert any(not c[3].any() for c in cases) and len({int(c[3].sum()) for c in cases}) >= 6    # a row with no legal key (the dead env) among them
    x = pg.typed_rows(rng, len(cases), 11, dtype)                                     # NaN, +-inf, all -inf, all NaN, +80 against -80, +-3e38 among them
    mask = np.stack([c[3] for c in cases])
    for inv_temp in (1.0, 0.7):
        for given in list(range(-1, 12)) + [-2 ** 31, 2 ** 31 - 1]:
            a = np.full(len(cases), given, np.int32)
            lp, ent = pg.eval_host(lib, x, dtype, mask, a, inv_temp)
            for r, (g, keys, dead, _) in enumerate(cases):
                _, act, lp1, ent1, _ = pu.act_host(lib, inner, g, 2, 2, x[r], keys=keys, dead=dead, dtype=dtype, mode=pu.GIVEN, given=given, inv_temp=inv_temp)
                assert act == (given if mask[r].any() else 0)
                assert pg.bits(lp[r:r + 1])[0] == pg.bits(np.float32(lp1).reshape(1))[0], (r, given, lp[r], lp1)
                assert pg.bits(ent[r:r + 1])[0] == pg.bits(np.float32(ent1).reshape(1))[0], (r, given, ent[r], ent1)
    # a mask byte counts as != 0, NULL outputs are skipped, mask = NULL is every key
    lp, ent = pg.eval_host(lib, x, dtype, mask, np.zeros(len(cases), np.int32))
    lp2, none = pg.eval_host(lib, x, dtype, mask.astype(np.uint8) * 0x80, np.zeros(len(cases), np.int32), want=(True, False))
    assert none is None and (pg.bits(lp) == pg.bits(lp2)).all()
    lp3, ent3 = pg.eval_host(lib, x, dtype, None, np.zeros(len(cases), np.int32))
    lp4, ent4 = pg.eval_host(lib, x, dtype, np.ones_like(mask), np.zeros(len(cases), np.int32))
    assert (pg.bits(lp3) == pg.bits(lp4)).all() and (pg.bits(ent3) == pg.bits(ent4)).all()


def test_special_rows_and_zero_gradients(lib):
    rng = np.random.RandomState(5)
    B, nk = 264, 11
    x = pu.special_rows(rng, B, nk)
    mask = pg.random_masks(rng, B, nk)
    a = pg.actions_for(rng, mask)
    g_lp, g_ent = rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    lp, ent = pg.eval_host(lib, x, F32, mask, a)
    dx = pg.grad_host(lib, x, F32, mask, a, g_lp, g_ent)
    d_lp, d_ent = pg.grad_host(lib, x, F32, mask, a, g_lp, None), pg.grad_host(lib, x, F32, mask, a, None, g_ent)
    assert np.isfinite(dx).all() and np.isfinite(ent).all() and not np.isnan(lp).any()
    weighs = mask & ~np.isnan(x) & (x != -np.inf)
    assert (pg.bits(dx)[~weighs] == 0).all() and (pg.bits(d_lp)[~weighs] == 0).all() and (pg.bits(d_ent)[~weighs] == 0).all()   # exactly +0.0
    seen = set()
    for r in range(B):
        none, flat = not mask[r].any(), not weighs[r].any()
        in_range = 0 <= a[r] < nk
        if none:
            assert lp[r] == 0 and ent[r] == 0
        if flat:                                   # no legal key weighs (all -inf, all NaN, no legal key): every gradient is zero
            assert (pg.bits(dx[r]) == 0).all()
            seen.add("flat")
            continue
        counts = in_range and weighs[r, a[r]] and lp[r] > -np.inf
        if not counts:                             # out of range, illegal or weightless: logp -inf, no gradient through logp, the entropy term still flows
            assert lp[r] == -np.inf and (pg.bits(d_lp[r]) == 0).all() and (pg.bits(dx[r]) == pg.bits(d_ent[r])).all()
            seen.add("a=%d" % min(max(a[r], -1), nk) if not in_range else "illegal")
            if r % 8 == 0 and weighs[r].sum() > 1:
                assert np.abs(d_ent[r]).max() > 0
                seen.add("flows")
        else:
            assert abs(float(d_lp[r].astype(np.float64).sum())) < 1e-5 * max(1.0, abs(g_lp[r]))    # softmax gradients sum to zero
            assert np.sign(d_lp[r, a[r]]) in (0, np.sign(g_lp[r]))
        assert abs(float(d_ent[r].astype(np.float64).sum())) < 1e-5 * max(1.0, abs(g_ent[r]))
    assert {"flat", "a=-1", "a=%d" % nk, "illegal", "flows"} <= seen, seen
    # +inf is the largest finite value: the row is one-hot there, logp 0, entropy 0
    r = np.flatnonzero(np.isinf(x).any(1) & (x == np.inf).any(1) & (mask & (x == np.inf)).any(1))
    assert len(r) and (ent[r] == 0).all()
    # +80 against -80: the small keys weigh nothing, their gradient is +0.0 though they are legal
    r = [i for i in range(B) if i % 8 == 5 and mask[i, np.argmax(x[i])] and mask[i].sum() > 1]
    assert r and all((pg.bits(dx[i])[x[i] == -80.0] == 0).all() for i in r)
    # a NaN or infinite upstream gradient gives the canonical quiet NaN, on legal weighing keys only
    bad = pg.grad_host(lib, x, F32, mask, a, np.full(B, np.nan, np.float32), np.full(B, np.inf, np.float32))
    assert (pg.bits(bad)[~weighs] == 0).all()
    assert set(np.unique(pg.bits(bad)[np.isnan(bad)])) == {0x7FC00000}
    # both upstream gradients absent: all zeros
    assert (pg.bits(pg.grad_host(lib, x, F32, mask, a, None, None)) == 0).all()


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_16_bit_gradients_are_the_f32_result_rounded_to_nearest_even(lib, dtype):
    rng = np.random.RandomState(11 + dtype)
    B, nk = 400, 11
    x = pg.typed_rows(rng, B, nk, dtype)
    mask = pg.random_masks(rng, B, nk, lo=1)
    a = pg.actions_for(rng, mask)
    # upstream gradients over 30 binades: binary16 results from zero through its subnormals to infinity
    g_lp = (rng.standard_normal(B) * 2.0 ** rng.randint(-28, 20, B)).astype(np.float32)
    g_ent = (rng.standard_normal(B) * 2.0 ** rng.randint(-28, 20, B)).astype(np.float32)
    got = pg.bits(pg.grad_host(lib, x, dtype, mask, a, g_lp, g_ent))
    full = pg.bits(pg.grad_host(lib, pg.widen(x, dtype), F32, mask, a, g_lp, g_ent))      # the same rule on the widened values
    want = np.array([[pg.rne16(int(u), dtype) for u in row] for row in full], np.uint16)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    kinds = want[mask]
    if dtype == F16:
        assert ((kinds & 0x7FFF) == 0x7C00).any() and (((kinds & 0x7C00) == 0) & ((kinds & 0x3FF) != 0)).any()   # infinities and subnormals were among them
        f = full.view(np.float32)
        ok = np.isfinite(f) & (np.abs(f) < 65000)
        assert (f[ok].astype(np.float16).view(np.uint16) == want[ok]).all()    # numpy's own rounding agrees with the integers
    # the rounding itself on chosen values: ties, the subnormal border, the overflow border, NaN
    for v, f16_bits, bf16_bits in ((1.0 + 2.0 ** -11, 0x3C00, 0x3F80), (1.0 + 3 * 2.0 ** -11, 0x3C02, 0x3F80), (1.0 + 2.0 ** -8, 0x3C04, 0x3F80),
                                   (1.0 + 3 * 2.0 ** -8, 0x3C0C, 0x3F82), (65519.0, 0x7BFF, 0x4780), (65520.0, 0x7C00, 0x4780), (2.0 ** -24, 0x0001, 0x3380),
                                   (2.0 ** -25, 0x0000, 0x3300), (2.0 ** -25 * 1.5, 0x0001, 0x3340), (-2.0 ** -14, 0x8400, 0xB880), (2.0 ** -14 - 2.0 ** -25, 0x0400, 0x3880)):
        u = int(np.float32(v).view(np.uint32))
        assert pg.rne16(u, F16) == f16_bits and pg.rne16(u, BF16) == bf16_bits, (v, hex(pg.rne16(u, F16)), hex(pg.rne16(u, BF16)))
        # through the library: one key, g_ent absent, logp's gradient is g_lp * (1 - 1) = 0 -- so use two keys of equal logits: dlogit[0] = g_lp / 2
        xx = np.zeros((1, 2), np.float16) if dtype == F16 else np.zeros((1, 2), np.uint16)
        d = pg.bits(pg.grad_host(lib, xx, dtype, None, np.zeros(1, np.int32), np.array([2 * v], np.float32), None))
        assert d[0, 0] == (f16_bits if dtype == F16 else bf16_bits), (v, hex(d[0, 0]))


def accuracy_rows():
    rng = np.random.RandomState(29)
    B, nk = 10000, 11
    x = (rng.standard_normal((B, nk)) * 3).astype(np.float32)
    mask = pg.random_masks(rng, B, nk, lo=1)
    a = np.array([rng.choice(np.flatnonzero(m)) for m in mask], np.int32)
    return x, mask, a, rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)


def test_gradient_accuracy_against_the_float64_chain(lib):
    x, mask, a, g_lp, g_ent = accuracy_rows()
    assert sorted(set(mask.sum(1))) == list(range(1, 12))
    worst = 0.0
    for inv_temp in (1.0,):
        lp64, ent64, dx64 = pg.chain64(x, mask, a, g_lp, g_ent, inv_temp)
        lp, ent = pg.eval_host(lib, x, F32, mask, a, inv_temp)
        dx = pg.grad_host(lib, x, F32, mask, a, g_lp, g_ent, inv_temp)
        worst = max(worst, float(np.abs(dx.astype(np.float64) - dx64).max()))
        print("largest |logp - float64| %.3g, |entropy - float64| %.3g, |dlogits - float64| %.3g" % (np.abs(lp - lp64).max(), np.abs(ent - ent64).max(), worst))
        assert np.abs(lp - lp64).max() <= 4 * 1.09e-6 and np.abs(ent - ent64).max() <= 4 * 2.29e-7    # rg_act's own bounds (tests/test_policy_host.py)
        assert (pg.bits(dx)[~mask] == 0).all()
    assert worst <= 4 * pg.MEASURED_GRAD
    # the parts alone, and a temperature: the same bound (inv_temp 0.7 scales the gradient down)
    for gl, ge, it in ((g_lp, None, 1.0), (None, g_ent, 1.0), (g_lp, g_ent, 0.7)):
        dx64 = pg.chain64(x, mask, a, gl, ge, np.float32(it))[2]
        part = float(np.abs(pg.grad_host(lib, x, F32, mask, a, gl, ge, it).astype(np.float64) - dx64).max())
        print("g_lp %s, g_ent %s, inv_temp %g: |dlogits - float64| %.3g" % (gl is not None, ge is not None, it, part))
        assert part <= 4 * pg.MEASURED_GRAD


def test_the_weight_cut_off_on_either_side(lib):
    """policy_edge_rows.cutoff_pair: against a key at 0, d_in weighs 2^-125 and has a gradient that is not zero; d_out, one float32 further, weighs nothing:
    logp -inf, gradient exactly +0.0, and as an action it does not count (the g_lp term of the whole row is +0.0)."""
    d_in, d_out = pe.cutoff_pair()
    x = np.array([[0.0, d_in], [0.0, d_out]], np.float32)
    a = np.ones(2, np.int32)
    one = np.ones(2, np.float32)
    lp, ent = pg.eval_host(lib, x, F32, None, a)
    assert np.isfinite(lp[0]) and abs(float(lp[0]) - float(d_in)) <= 1e-5 and lp[1] == -np.inf
    d_lp, d_ent = pg.grad_host(lib, x, F32, None, a, one, None), pg.grad_host(lib, x, F32, None, a, None, one)
    # inside: dlogit[1] = 1 - pi = 1 (pi = 2^-125 is lost beside 1), dlogit[0] = 0 - 1; the entropy term is -pi * (lp + H), about 86.6 * 2^-125
    assert d_lp[0, 1] == 1.0 and d_lp[0, 0] == -1.0
    assert d_ent[0, 1] != 0 and abs(float(d_ent[0, 1]) / (2.0 ** -125 * -float(d_in)) - 1) < 1e-5
    # outside: every gradient of the light key is +0.0, and the action does not count
    assert (pg.bits(d_lp[1]) == 0).all() and pg.bits(d_ent[1:2, 1])[0] == 0
    # ... while as a bystander of action 0 the inside key still gets its -pi, the outside one +0.0
    by = pg.grad_host(lib, x, F32, None, np.zeros(2, np.int32), one, None)
    assert abs(float(by[0, 1]) / -(2.0 ** -125) - 1) < 1e-5 and pg.bits(by[1:2, 1])[0] == 0


def test_binary16_gradients_on_exact_subnormal_ties(lib):
    """policy_edge_rows.tie_values: f32 gradients exactly half way between two subnormal binary16 values, the lower neighbour even and odd, the tie at 2^-25 and the
    one under the smallest normal, both signs -- through g_lp on two equal legal logits (pi = 1/2 exactly) -- against rne16 and against the values by hand."""
    ties = pe.tie_values()
    by_hand = {0.5: 0x0000, 1.5: 0x0002, 2.5: 0x0002, 3.5: 0x0004, 100.5: 0x0064, 101.5: 0x0066, 511.5: 0x0200, 512.5: 0x0200, 1022.5: 0x03FE, 1023.5: 0x0400}
    assert sorted(by_hand) == sorted(pe.TIE_UNITS)
    B = len(ties)
    x = np.full((B, 3), 0.25, np.float16)
    mask = np.tile(np.array([True, False, True]), (B, 1))            # the illegal key in between stays +0.0
    for act, col, sign in ((0, 0, 1.0), (0, 2, -1.0), (2, 2, 1.0)):   # dlogit[a] = g_lp / 2, the other legal key's = -g_lp / 2
        a = np.full(B, act, np.int32)
        got = pg.bits(pg.grad_host(lib, x, F16, mask, a, 2 * ties, None))
        full = pg.grad_host(lib, x.astype(np.float32), F32, mask, a, 2 * ties, None)
        assert (full[:, col] == sign * ties).all() and (pg.bits(full[:, 1]) == 0).all()
        for r in range(B):
            want = pg.rne16(int(pg.bits(full[r:r + 1, col])[0]), F16)
            unit = abs(float(ties[r])) * 2.0 ** 24
            assert want & 0x7FFF == by_hand[unit] and (want >> 15) == int(sign * ties[r] < 0), (unit, hex(want))
            assert got[r, col] == want and got[r, 1] == 0, (r, unit, hex(got[r, col]), hex(want))
    # with an entropy term of exactly zero upstream the tie stays a tie
    got = pg.bits(pg.grad_host(lib, x, F16, mask, np.zeros(B, np.int32), 2 * ties, np.zeros(B, np.float32)))
    assert all(got[r, 0] & 0x7FFF == by_hand[abs(float(ties[r])) * 2.0 ** 24] for r in range(B))


def domain_cell(lib, family, inv_temp, n=2000, nk=11):
    """One (family, inv_temp) cell of the domain test -> (rows compared / n, worst logp ratio, worst |entropy| error, worst entropy excess over ln count, worst
    gradient ratio).  The reference is float64 on f32(logit * inv_temp), the rule's own first step."""
    rng = np.random.RandomState(1000 + 17 * pe.FAMILIES.index(family) + pe.INV_TEMPS.index(inv_temp))
    x = pe.family_rows(family, rng, n, nk)
    mask = pg.random_masks(rng, n, nk, lo=1)
    a = np.array([rng.choice(np.flatnonzero(m)) for m in mask], np.int32)
    g_lp, g_ent = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    it = np.float32(inv_temp)
    xs = (x * it).astype(np.float32)
    lp64, ent64, dxs64 = pg.chain64(xs, mask, a, g_lp, g_ent)
    dx64 = dxs64 * float(it)                                          # d / d logit = inv_temp * d / d x
    top = np.where(mask, xs.astype(np.float64), -np.inf).max(1)
    keep = np.exp2((xs[np.arange(n), a].astype(np.float64) - top) * np.log2(np.e)) >= 2.0 ** -120      # below that the rule answers -inf by design
    lp, ent = pg.eval_host(lib, x, F32, mask, a, float(it))
    dx = pg.grad_host(lib, x, F32, mask, a, g_lp, g_ent, float(it)).astype(np.float64)
    assert np.isfinite(ent).all() and np.isfinite(dx).all() and np.isfinite(lp[keep]).all()
    r_lp = np.abs(lp.astype(np.float64) - lp64) / np.maximum(1.0, np.abs(lp64))
    e_ent = np.abs(ent.astype(np.float64) - ent64)
    excess = ent.astype(np.float64) - np.log(mask.sum(1))
    scale = float(it) * (np.abs(g_lp) + np.abs(g_ent) * np.maximum(1.0, np.abs(lp64 + ent64)))
    r_dx = np.abs(dx - dx64).max(1) / scale
    return float(keep.mean()), float(r_lp[keep].max()), float(e_ent[keep].max()), float(excess[keep].max()), float(r_dx[keep].max())


def test_accuracy_over_the_domain(lib):
    """logp, entropy and gradient against float64 over policy_edge_rows' six families x four inverse temperatures, 1 to 11 legal keys, 2 000 rows each: rows the
    sampled accuracy tests above never draw (|d| up to 86 and beyond the cut-off, logits at 1e6, near ties, subnormal logits and products).  Bounds relative to
    the size of what is computed, measured here (policy_edge_rows.MEASURED_DOMAIN) times 2."""
    worst = np.zeros(4)
    for family in pe.FAMILIES:
        for inv_temp in pe.INV_TEMPS:
            share, *cell = domain_cell(lib, family, inv_temp)
            print("%-20s inv_temp %-5g compared %5.1f %%  logp ratio %.3g  |entropy| %.3g  entropy - ln count %.3g  gradient ratio %.3g" % ((family, inv_temp, 100 * share) + tuple(cell)))
            assert share >= 0.4 or inv_temp > 1, (family, inv_temp, share)
            worst = np.maximum(worst, cell)
    print("worst: logp ratio %.3g, |entropy| %.3g, entropy - ln count %.3g, gradient ratio %.3g" % tuple(worst))
    m = pe.MEASURED_DOMAIN
    assert worst[0] <= 2 * m["logp"] and worst[1] <= 2 * m["entropy"] and worst[2] <= 2 * m["excess"] and worst[3] <= 2 * m["grad"], (worst.tolist(), m)


def test_refusals_name_the_argument_and_write_nothing(lib):
    x, a = np.zeros((4, 11), np.float32), np.zeros(4, np.int32)
    lp, dx = np.full(4, 7.0, np.float32), np.full((4, 11), 7.0, np.float32)

    def refused(words, n_rows=4, nk=11, dtype=0, inv_temp=1.0, logits=True, action=True, dlogits=True):
        for name in ("rg_policy_eval_host", "rg_policy_grad_host"):
            if "eval" in name and not dlogits:
                continue
            args = [n_rows, nk, x.ctypes.data if logits else None, dtype, None, a.ctypes.data if action else None, inv_temp]
            args += [lp.ctypes.data, None] if "eval" in name else [None, None, dx.ctypes.data if dlogits else None]
            rc = getattr(lib, name)(*args)
            msg = lib.rg_last_error(None).decode()
            assert rc != 0 and msg.startswith(name + ":") and all(w in msg for w in words), (name, words, msg)
            assert (lp == 7.0).all() and (dx == 7.0).all()

    refused(("n_keys", "got 0"), nk=0)
    refused(("n_keys", "got 33"), nk=33)
    refused(("dtype", "got 3"), dtype=3)
    refused(("dtype", "got -1"), dtype=-1)
    refused(("n_rows", "-1"), n_rows=-1)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(("inv_temp",), inv_temp=bad)
    refused(("logits",), logits=False)
    refused(("action",), action=False)
    refused(("dlogits",), dlogits=False)
    # no rows: a valid call that writes nothing
    assert lib.rg_policy_eval_host(0, 11, x.ctypes.data, 0, None, a.ctypes.data, 1.0, lp.ctypes.data, None) == 0 and (lp == 7.0).all()
    assert lib.rg_policy_grad_host(0, 11, x.ctypes.data, 0, None, a.ctypes.data, 1.0, None, None, dx.ctypes.data) == 0 and (dx == 7.0).all()


def test_the_numpy_value_form(lib):
    import rogue_gym
    rng = np.random.RandomState(7)
    x = (rng.standard_normal((3, 5, 11)) * 3).astype(np.float32)
    mask = pg.random_masks(rng, 15, 11, lo=1).reshape(3, 5, 11)
    a = np.array([rng.choice(np.flatnonzero(m)) for m in mask.reshape(15, 11)]).reshape(3, 5)
    g = rng.standard_normal((3, 5)).astype(np.float32)
    lp, ent, grad_fn = rogue_gym.masked_logp_np(x, a, mask, temperature=2.0)
    assert lp.shape == ent.shape == (3, 5) and lp.dtype == ent.dtype == np.float32
    lp1, ent1 = pg.eval_host(lib, x.reshape(15, 11), F32, mask.reshape(15, 11), a.reshape(15), 0.5)
    assert (pg.bits(lp.reshape(15)) == pg.bits(lp1)).all() and (pg.bits(ent.reshape(15)) == pg.bits(ent1)).all()
    dx = grad_fn(g, 0.01)
    assert dx.shape == x.shape and dx.dtype == np.float32
    want = pg.grad_host(lib, x.reshape(15, 11), F32, mask.reshape(15, 11), a.reshape(15), g.reshape(15), np.full(15, 0.01, np.float32), 0.5)
    assert (pg.bits(dx.reshape(15, 11)) == pg.bits(want)).all()
    assert grad_fn(g).shape == x.shape and rogue_gym.masked_logp_np(x.astype(np.float16), a)[2](g).dtype == np.float16
    with pytest.raises(ValueError):
        rogue_gym.masked_logp_np(x, a, mask, temperature=0.0)
    with pytest.raises(ValueError):
        rogue_gym.masked_logp_np(x.astype(np.float64), a)
    with pytest.raises(ValueError):
        rogue_gym.masked_logp_np(x, a[:2])


def test_rule_source_under_address_and_undefined_sanitizers(tmp_path):
    """The twins' source (csrc/rg_policy_grad.h and rg_readers_host.h) in a stand-alone program of its own -- nothing sanitized is loaded into python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or ("/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")):
        pytest.skip("no ROCm include directory (the rule headers include hip/hip_runtime.h for __host__ __device__)")
    exe = str(tmp_path / "learn_host_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []   # the runtimes inside the program (clang's default)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "rogue-gym_amd", "csrc"), "-I", os.path.join(ROOT, "rogue-gym_amd"),
                    os.path.join(ROOT, "tests", "learn_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(", 0 bad"), r.stdout


_ = C
