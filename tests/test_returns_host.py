"""Returns and advantages on the CPU (rg_gae_host, rg_vtrace_host; rogue-gym_amd/csrc/rg_returns.h): the twins against the independent float64 statement of
tests/returns_util.py within bounds derived from the roundings of the recurrence, the clipped ratio alone against min(bar, exp(.)) in float64, the cases that
can be answered by hand, containment of NaN and inf inside their episode, the refusals, the exact aliases, the numpy forms, the entry points -- and the rule's
source in a stand-alone program built with -fsanitize=address,undefined."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import returns_util as ru
from returns_util import EPS, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"rg_gae": 13, "rg_vtrace": 18, "rg_gae_host": 12, "rg_vtrace_host": 17}
F = np.float32
# the largest relative error of ratio(bar) against float64 over lt - lb in [-30, 30] and bars 0.5, 1, 2, measured on the twin by the test below
MEASURED_RATIO = 3.2e-6


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def test_entry_points_declared_exported_and_bound(lib):
    from rogue_gym_python import _rogue_gym as inner
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for n, n_args in ENTRIES.items():
        assert re.search(r"^int %s\(" % n, hdr, re.M), "not declared: " + n
        assert hasattr(lib, n), "not exported: " + n
        assert len(inner._ABI[n][0]) == n_args and n in inner._INT_FUNCS and inner._ABI[n][2]
    import rogue_gym
    for n in ("gae", "discounted_returns", "vtrace", "gae_np", "discounted_returns_np", "vtrace_np"):
        assert callable(getattr(rogue_gym, n)), n


@pytest.mark.parametrize("T", [16, 128, 1000])
def test_gae_twin_against_the_float64_statement(lib, T):
    """Each step rounds three times (fma, subtract, fma), each rounding at most 2^-24 of a quantity bounded by S_t = (gamma |boot| + |r| + |v|) + gamma lam
    S_{t+1}, S_{t+1} reset at an end: to first order |adv - adv64| <= 3 * 2^-24 * S_t; asserted with 4 for the second-order terms (and the one rounding of
    gamma * lam).  ret = v + adv rounds once more, on |ret|."""
    rng = np.random.RandomState(100 + T)
    N, worst = 48, 0.0
    for gamma in (0.9, 0.99, 1.0):
        for lam in (0.0, 0.95, 1.0):
            for rate in (0.0, 0.02, 0.3):
                for mode in range(4):   # bit 0: truncations; bit 1: with trunc_value
                    x = ru.rollout(rng, T, N, done_rate=rate, trunc_rate=0.05 if mode & 1 else 0.0)
                    tr, tv = (x["trunc"] if mode & 1 else None), (x["trunc_value"] if mode == 3 else None)
                    if mode == 2:
                        continue
                    adv, ret = ru.gae_host(lib, x["reward"], x["value"], x["last_value"], x["done"], tr, tv, gamma, lam)
                    a64, r64, S = ru.gae64(x["reward"], x["value"], x["last_value"], x["done"], tr, tv, F(gamma), F(lam))
                    err = np.abs(adv - a64)
                    worst = max(worst, float((err / (EPS * S)).max()))
                    assert (err <= 4 * EPS * S).all(), (gamma, lam, rate, mode, float((err / (EPS * S)).max()))
                    assert (np.abs(ret - r64) <= 4 * EPS * S + EPS * (np.abs(r64) + 4 * EPS * S)).all(), (gamma, lam, rate, mode)
    print("T %d: largest |adv - float64| = %.2f * 2^-24 * S_t" % (T, worst))


@pytest.mark.parametrize("T", [16, 128, 1000])
def test_vtrace_twin_against_the_float64_statement(lib, T):
    """The float64 chain takes the twin's own f32 rho, c and rho_pg, widened (the ratio has its own test).  One rounding more per step than GAE, the multiply
    by rho: |acc - acc64| <= 5 * 2^-24 * S_t, S weighted by rho and gamma c.  vs = v + acc rounds once more on |vs|.  pg_adv rounds three times on
    P_t = rho_pg (gamma |vs_boot| + |r| + |v|), once on its own size, and inherits rho_pg * gamma times the error of vs_{t+1} where the episode goes on."""
    rng = np.random.RandomState(200 + T)
    N, worst = 48, 0.0
    for gamma in (0.9, 0.99, 1.0):
        for lam in (0.5, 1.0):
            for rate in (0.0, 0.02, 0.3):
                for bars in ((1.0, 1.0, 1.0), (2.0, 0.5, 1.5)):
                    x = ru.rollout(rng, T, N, done_rate=rate, trunc_rate=0.05)
                    tv = x["trunc_value"] if bars[0] == 2.0 else None
                    vs, pg = ru.vtrace_host(lib, x["lb"], x["lt"], x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], tv, gamma, lam, bars)
                    rho, cr, rpg = (ru.ratio_twin(lib, x["lt"].reshape(-1), x["lb"].reshape(-1), b).reshape(T, N) for b in bars)
                    c = F(lam) * cr                                          # (one f32 multiply, as the rule makes it)
                    assert c.dtype == np.float32
                    vs64, pg64, S, P = ru.vtrace64(rho.astype(np.float64), c.astype(np.float64), rpg.astype(np.float64), x["reward"], x["value"], x["last_value"],
                                                   x["done"], x["trunc"], tv, F(gamma))
                    e_vs = 5 * EPS * S + EPS * (np.abs(vs64) + 5 * EPS * S)
                    err = np.abs(vs - vs64)
                    worst = max(worst, float((err / e_vs).max()))
                    assert (err <= e_vs).all(), (gamma, lam, rate, bars, float((err / e_vs).max()))
                    end = (x["done"] != 0) | (x["trunc"] != 0)
                    nxt = np.vstack([e_vs[1:], np.zeros((1, N))])
                    e_pg = 4 * EPS * P + EPS * np.abs(pg64) + rpg * float(F(gamma)) * np.where(end, 0.0, nxt) * (1 + 8 * EPS)
                    assert (np.abs(pg - pg64) <= e_pg).all(), (gamma, lam, rate, bars, float((np.abs(pg - pg64) / np.maximum(e_pg, 1e-30)).max()))
    print("T %d: largest |vs - float64| = %.2f of its bound" % (T, worst))


def test_the_clipped_ratio_alone(lib):
    """ratio(bar) against min(bar, exp(lt - lb)) in float64 over lt - lb in [-30, 30] and bars 0.5, 1 and 2.  Its relative error is rg_pol_exp2's and one argument
    multiply's: an error of 2^-24 * |e| * log2(e) in the argument of 2^x is a relative error of that times ln 2 in the result, 1.8e-6 at |e| = 30, beside the
    roundings of lt - lb and of ln_bar.  So it is measured here, on the twin: the largest over this sample is 3.16e-6 (MEASURED_RATIO = 3.2e-6).  Asserted: twice that, the
    maximum of a sample not being the supremum."""
    rng = np.random.RandomState(5)
    n = 200000
    worst = 0.0
    for bar in (0.5, 1.0, 2.0):
        lb = -rng.random_sample(n).astype(F) * 30
        lt = (lb.astype(np.float64) + rng.uniform(-30, 30, n)).astype(F)
        got = ru.ratio_twin(lib, lt, lb, bar).astype(np.float64)
        want = ru.ratio64(lt, lb, bar)
        ln_bar = F(np.log(np.float64(F(bar))))
        e = (lt - lb) - ln_bar                                               # f32, as the rule computes it
        rel = np.abs(got - want) / want
        worst = max(worst, float(rel.max()))
        assert (bits(got.astype(F))[e >= 0] == bits(F(bar))).all()                              # capped: exactly bar
        assert (got <= bar).all()
    print("largest relative error of ratio(bar): %.3g" % worst)
    assert worst <= 2 * MEASURED_RATIO, worst
    # below the cut-off exactly 0; at equal log-probabilities and bar 1 exactly 1; a NaN or (-inf) - (-inf) gives the canonical NaN; -inf against finite: 0, bar
    log2e = float(F(1.4426950216293335))
    deep = F(-125.0 / log2e * 1.0001)
    r = ru.ratio_twin(lib, np.array([deep, -200.0, 0.0, -3.25, np.nan, -np.inf, -np.inf, -1.0], F), np.array([0.0, 0.0, 0.0, -3.25, 0.0, -np.inf, -1.0, -np.inf], F), 1.0)
    assert bits(r).tolist() == [0, 0, 0x3F800000, 0x3F800000, ru.QNAN, ru.QNAN, 0, 0x3F800000], bits(r).tolist()


def test_exact_cases_answered_by_hand(lib):
    r = np.array([[1.0], [2.0], [4.0]], F)
    v = np.array([[0.5], [0.25], [8.0]], F)
    last = np.array([16.0], F)
    zero, one = np.zeros((3, 1), np.uint8), np.ones((3, 1), np.uint8)
    # T = 1: delta = r + gamma * last - v
    adv, ret = ru.gae_host(lib, r[:1], v[:1], last, None, None, None, 0.5, 0.5)
    assert adv[0, 0] == 1.0 + 8.0 - 0.5 and ret[0, 0] == 9.0
    # gamma = 0: adv = r - v, whatever lam
    adv, ret = ru.gae_host(lib, r, v, last, zero, None, None, 0.0, 1.0)
    assert (adv == r - v).all() and (ret == r).all()
    # lam = 0: one-step TD, delta_t = r_t + gamma V_{t+1} - V_t
    adv, _ = ru.gae_host(lib, r, v, last, zero, None, None, 0.5, 0.0)
    assert adv[:, 0].tolist() == [1.0 + 0.125 - 0.5, 2.0 + 4.0 - 0.25, 4.0 + 8.0 - 8.0]
    # no done, gamma = lam = 1 (every sum exact): adv_t = sum of the deltas from t on
    adv, ret = ru.gae_host(lib, r, v, last, zero, None, None, 1.0, 1.0)
    d = [1.0 + 0.25 - 0.5, 2.0 + 8.0 - 0.25, 4.0 + 16.0 - 8.0]
    assert adv[:, 0].tolist() == [d[0] + d[1] + d[2], d[1] + d[2], d[2]] and ret[:, 0].tolist() == [23.0, 22.0, 20.0]     # (r-to-go + last)
    # all done: every step is its own episode, nothing is bootstrapped
    adv, ret = ru.gae_host(lib, r, v, last, one, None, None, 1.0, 1.0)
    assert (adv == r - v).all() and (ret == r).all()
    # done at T - 1 alone: last_value is never looked at
    end = np.array([[0], [0], [1]], np.uint8)
    a1, r1 = ru.gae_host(lib, r, v, last, end, None, None, 1.0, 1.0)
    a2, r2 = ru.gae_host(lib, r, v, np.array([np.nan], F), end, None, None, 1.0, 1.0)
    assert (bits(a1) == bits(a2)).all() and r1[:, 0].tolist() == [7.0, 6.0, 4.0]
    # any non-zero byte counts
    for byte in (2, 0x80, 255):
        a3, _ = ru.gae_host(lib, r, v, last, end * byte, None, None, 1.0, 1.0)
        assert (bits(a3) == bits(a1)).all()
    # a time limit at t = 1 where done is not set: with trunc_value the bootstrap is that value, without it the step's own value, and nothing is carried over
    tr = np.array([[0], [1], [0]], np.uint8)
    tv = np.array([[99.0], [32.0], [99.0]], F)
    adv, ret = ru.gae_host(lib, r, v, last, zero, tr, tv, 1.0, 1.0)
    assert adv[:, 0].tolist() == [(1.0 + 0.25 - 0.5) + (2.0 + 32.0 - 0.25), 2.0 + 32.0 - 0.25, 12.0] and ret[1, 0] == 34.0
    adv, ret = ru.gae_host(lib, r, v, last, zero, tr, None, 1.0, 1.0)
    assert adv[1, 0] == 2.0 + 0.25 - 0.25 and ret[1, 0] == 2.25
    # trunc and done both set: the time limit's bootstrap wins
    adv, _ = ru.gae_host(lib, r, v, last, np.array([[0], [1], [0]], np.uint8), tr, tv, 1.0, 1.0)
    assert adv[1, 0] == 2.0 + 32.0 - 0.25
    # value = NULL, lam = 1: discounted reward-to-go from last_value, cut at a done
    _, ret = ru.gae_host(lib, r, None, last, zero, None, None, 0.5, 1.0, want=(False, True))
    assert ret[:, 0].tolist() == [1.0 + 0.5 * (2.0 + 0.5 * (4.0 + 8.0)), 2.0 + 0.5 * (4.0 + 8.0), 4.0 + 8.0]
    _, ret = ru.gae_host(lib, r, None, last, np.array([[0], [1], [0]], np.uint8), None, None, 0.5, 1.0, want=(False, True))
    assert ret[:, 0].tolist() == [2.0, 2.0, 12.0]
    # last_value = NULL is 0
    _, ret = ru.gae_host(lib, r, None, None, None, None, None, 1.0, 1.0, want=(False, True))
    assert ret[:, 0].tolist() == [7.0, 6.0, 4.0]


def test_on_policy_vtrace_is_gae_bit_for_bit(lib):
    rng = np.random.RandomState(9)
    for T, N, lam in ((1, 5, 1.0), (17, 33, 0.95), (100, 64, 0.5)):
        x = ru.rollout(rng, T, N, done_rate=0.05, trunc_rate=0.05, specials=True)
        lp = np.where(np.isfinite(x["lb"]), x["lb"], F(-1.0)).astype(F)
        for tv in (None, x["trunc_value"]):
            _, ret = ru.gae_host(lib, x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], tv, 0.99, lam)
            vs, _ = ru.vtrace_host(lib, lp, lp, x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], tv, 0.99, lam)
            assert (bits(vs) == bits(ret)).all()


def test_nan_and_inf_stay_inside_their_episode(lib):
    rng = np.random.RandomState(13)
    T, N = 60, 40
    x = ru.rollout(rng, T, N, done_rate=0.1, trunc_rate=0.05)
    end = (x["done"] != 0) | (x["trunc"] != 0)
    episode = np.vstack([np.zeros((1, N), int), np.cumsum(end, 0)[:-1]])          # the episode of step t: the ends before it in its column
    base_g = ru.gae_host(lib, x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], x["trunc_value"], 0.99, 0.95)
    base_v = ru.vtrace_host(lib, x["lb"], x["lt"], x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], x["trunc_value"], 0.99, 0.95, (1.0, 1.0, 1.0))
    seen_nan = False
    for poison in (np.nan, np.inf, -np.inf):
        for name in ("reward", "value", "trunc_value", "lt"):
            y = {k: v.copy() for k, v in x.items()}
            hit = np.zeros((T, N), bool)
            for n in range(N):
                t = rng.randint(T)
                y[name][t, n] = poison
                hit[:, n] = episode[:, n] == episode[t, n]
            # the value of the step before an episode's first is its bootstrap: V(s_t) of an episode's first step is read by the step before only if no end stands between
            got_g = ru.gae_host(lib, y["reward"], y["value"], y["last_value"], y["done"], y["trunc"], y["trunc_value"], 0.99, 0.95)
            got_v = ru.vtrace_host(lib, y["lb"], y["lt"], y["reward"], y["value"], y["last_value"], y["done"], y["trunc"], y["trunc_value"], 0.99, 0.95, (1.0, 1.0, 1.0))
            for got, base in ((got_g, base_g), (got_v, base_v)):
                for g, b in zip(got, base):
                    assert (bits(g)[~hit] == bits(b)[~hit]).all(), (poison, name)
                    nan = np.isnan(g)
                    seen_nan = seen_nan or bool(nan.any())
                    assert (bits(g)[nan] == ru.QNAN).all()
    assert seen_nan


def test_refusals_name_the_argument_and_write_nothing(lib):
    T, N = 3, 4
    r, v, tv, lp = (np.zeros((T, N), F) for _ in range(4))
    last, d = np.zeros(N, F), np.zeros((T, N), np.uint8)
    a, b = np.full((T, N), 7.0, F), np.full((T, N), 7.0, F)
    big = np.zeros(2 * T * N + 1, F)
    P = ru._p

    def refused(words, vt=None, **kw):
        for name in ("rg_gae_host", "rg_vtrace_host"):
            if vt is not None and vt != ("vtrace" in name):
                continue
            k = dict(n_steps=T, n_envs=N, lb=P(lp), lt=P(lp), reward=P(r), value=P(v), last=P(last), done=P(d), trunc=P(d), tv=P(tv), gamma=0.9, lam=0.9, bars=(1.0, 1.0, 1.0),
                     a=P(a), b=P(b))
            k.update(kw)
            if "vtrace" in name:
                rc = lib.rg_vtrace_host(k["n_steps"], k["n_envs"], k["lb"], k["lt"], k["reward"], k["value"], k["last"], k["done"], k["trunc"], k["tv"], k["gamma"], k["lam"],
                                        k["bars"][0], k["bars"][1], k["bars"][2], k["a"], k["b"])
            else:
                rc = lib.rg_gae_host(k["n_steps"], k["n_envs"], k["reward"], k["value"], k["last"], k["done"], k["trunc"], k["tv"], k["gamma"], k["lam"], k["a"], k["b"])
            msg = lib.rg_last_error(None).decode()
            assert rc != 0 and msg.startswith(name + ":") and all(w in msg for w in words), (name, words, msg)
            assert (a == 7.0).all() and (b == 7.0).all() and not big.any()

    refused(("n_steps", "-1"), n_steps=-1)
    refused(("n_envs", "-2"), n_envs=-2)
    refused(("reward",), reward=None)
    refused(("value",), vt=True, value=None)
    refused(("logp_behaviour",), vt=True, lb=None)
    refused(("logp_target",), vt=True, lt=None)
    refused(("adv", "ret", "both"), vt=False, a=None, b=None)
    refused(("vs", "pg_adv", "both"), vt=True, a=None, b=None)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        refused(("gamma",), gamma=bad)
        refused(("lam",), lam=bad)
    for i, n in enumerate(("rho_bar", "c_bar", "pg_rho_bar")):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            bars = [1.0, 1.0, 1.0]
            bars[i] = bad
            refused((n,), vt=True, bars=tuple(bars))
    refused(("trunc_value", "trunc"), trunc=None)
    # overlaps that are not exact: one element in, one element out, another array's size
    base = big.ctypes.data
    refused(("overlaps", "reward"), reward=base, a=base + 4)
    refused(("overlaps", "value"), value=base + 4 * T * N, b=base + 4 * T * N - 4)
    refused(("overlaps", "done"), done=base, a=base)
    refused(("overlaps", "last_value"), last=base + 8, b=base)
    refused(("overlaps", "logp_target"), vt=True, lt=base + 4, b=base)
    refused(("overlaps",), a=base, b=base + 4)
    # empty rollouts are valid calls that write nothing
    assert lib.rg_gae_host(0, N, P(r), None, None, None, None, None, 0.9, 0.9, P(a), None) == 0 and lib.rg_gae_host(T, 0, P(r), None, None, None, None, None, 0.9, 0.9, P(a), None) == 0
    assert lib.rg_vtrace_host(0, N, P(lp), P(lp), P(r), P(v), None, None, None, None, 0.9, 0.9, 1.0, 1.0, 1.0, P(a), None) == 0
    assert (a == 7.0).all()
    # the device entries refuse the same way before they touch a device
    assert lib.rg_gae(None, T, N, None, None, None, None, None, None, 0.9, 0.9, P(a), None) != 0 and lib.rg_last_error(None).decode().startswith("rg_gae: reward")
    assert lib.rg_vtrace(None, T, N, P(lp), P(lp), P(r), None, None, None, None, None, 0.9, 0.9, 1.0, 1.0, 1.0, P(a), None) != 0
    assert lib.rg_last_error(None).decode().startswith("rg_vtrace: value")


def test_exact_aliases_give_the_bits_of_separate_outputs(lib):
    rng = np.random.RandomState(21)
    T, N = 33, 20
    x = ru.rollout(rng, T, N, done_rate=0.1, trunc_rate=0.05, specials=True)
    adv, ret = ru.gae_host(lib, x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], x["trunc_value"], 0.99, 0.95)
    vs, pg = ru.vtrace_host(lib, x["lb"], x["lt"], x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], x["trunc_value"], 0.99, 0.95, (1.0, 1.0, 1.0))
    P = ru._p
    for outs in (("reward", "value"), ("value", "reward"), ("trunc_value", "value")):
        y = {k: v.copy() for k, v in x.items()}
        assert lib.rg_gae_host(T, N, P(y["reward"]), P(y["value"]), P(y["last_value"]), P(y["done"]), P(y["trunc"]), P(y["trunc_value"]), 0.99, 0.95, P(y[outs[0]]), P(y[outs[1]])) == 0
        assert (bits(y[outs[0]]) == bits(adv)).all() and (bits(y[outs[1]]) == bits(ret)).all(), outs
    for outs in (("lb", "lt"), ("reward", "value"), ("lt", "trunc_value")):
        y = {k: v.copy() for k, v in x.items()}
        assert lib.rg_vtrace_host(T, N, P(y["lb"]), P(y["lt"]), P(y["reward"]), P(y["value"]), P(y["last_value"]), P(y["done"]), P(y["trunc"]), P(y["trunc_value"]), 0.99, 0.95,
                                  1.0, 1.0, 1.0, P(y[outs[0]]), P(y[outs[1]])) == 0
        assert (bits(y[outs[0]]) == bits(vs)).all() and (bits(y[outs[1]]) == bits(pg)).all(), outs
    # both outputs in one buffer: the second one stands
    y = {k: v.copy() for k, v in x.items()}
    one = np.zeros((T, N), F)
    assert lib.rg_gae_host(T, N, P(y["reward"]), P(y["value"]), None, P(y["done"]), None, None, 0.99, 0.95, P(one), P(one)) == 0
    assert (bits(one) == bits(ru.gae_host(lib, x["reward"], x["value"], None, x["done"], None, None, 0.99, 0.95)[1])).all()


def test_the_numpy_forms(lib):
    import rogue_gym
    rng = np.random.RandomState(31)
    T, N = 20, 7
    x = ru.rollout(rng, T, N, done_rate=0.1, trunc_rate=0.1)
    adv, ret = rogue_gym.gae_np(x["reward"].astype(np.float64), x["value"], x["done"].astype(bool), x["last_value"], truncated=x["trunc"], trunc_values=x["trunc_value"])
    a1, r1 = ru.gae_host(lib, x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], x["trunc_value"], 0.99, 0.95)
    assert adv.dtype == ret.dtype == np.float32 and adv.shape == (T, N) and (bits(adv) == bits(a1)).all() and (bits(ret) == bits(r1)).all()
    # non-contiguous views are copied, not refused
    adv2, _ = rogue_gym.gae_np(np.asfortranarray(x["reward"]), x["value"][:, ::1], x["done"], x["last_value"], truncated=x["trunc"], trunc_values=x["trunc_value"])
    assert (bits(adv2) == bits(a1)).all()
    rtg = rogue_gym.discounted_returns_np(x["reward"], x["done"], x["last_value"], gamma=0.9)
    assert (bits(rtg) == bits(ru.gae_host(lib, x["reward"], None, x["last_value"], x["done"], None, None, 0.9, 1.0, want=(False, True))[1])).all()
    vs, pg = rogue_gym.vtrace_np(x["lb"], x["lt"], x["reward"], x["value"], x["done"], x["last_value"], lam=0.9, rho_bar=2.0, c_bar=1.5, pg_rho_bar=0.5, truncated=x["trunc"])
    v1, p1 = ru.vtrace_host(lib, x["lb"], x["lt"], x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], None, 0.99, 0.9, (2.0, 1.5, 0.5))
    assert (bits(vs) == bits(v1)).all() and (bits(pg) == bits(p1)).all()
    for bad in (lambda: rogue_gym.gae_np(x["reward"], x["value"][:3], x["done"]), lambda: rogue_gym.gae_np(x["reward"], x["value"], x["done"].astype(np.int32)),
                lambda: rogue_gym.gae_np(x["reward"], x["value"], x["done"], gamma=1.5), lambda: rogue_gym.gae_np(x["reward"], x["value"], x["done"], trunc_values=x["value"]),
                lambda: rogue_gym.vtrace_np(x["lb"], x["lt"], x["reward"], None, x["done"]), lambda: rogue_gym.vtrace_np(x["lb"], x["lt"], x["reward"], x["value"], x["done"], rho_bar=0.0),
                lambda: rogue_gym.discounted_returns_np(x["reward"][0], x["done"][0]), lambda: rogue_gym.gae_np(x["reward"], x["value"], x["done"], last_value=x["last_value"][:3])):
        with pytest.raises(ValueError):
            bad()


def test_rule_source_under_address_and_undefined_sanitizers(tmp_path):
    """The twins' source (csrc/rg_returns.h and rg_readers_host.h) in a stand-alone program of its own -- nothing sanitized is loaded into python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or ("/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")):
        pytest.skip("no ROCm include directory (the rule headers include hip/hip_runtime.h for __host__ __device__)")
    exe = str(tmp_path / "returns_host_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []   # the runtimes inside the program (clang's default)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "rogue-gym_amd", "csrc"), "-I", os.path.join(ROOT, "rogue-gym_amd"),
                    os.path.join(ROOT, "tests", "returns_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(", 0 bad"), r.stdout
