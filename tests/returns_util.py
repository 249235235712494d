"""Shared by the returns tests (tests/test_returns_host.py, tests/test_gpu_returns.py): an independent float64 statement of GAE(lambda) and V-trace in numpy,
written from the papers' formulas (Schulman et al. 2016, eq. 16; Espeholt et al. 2018, eq. 1 and remark 2 with the lambda of rlax.vtrace), the a-priori error
bounds of the f32 recurrences, input makers, and ctypes callers of the host twins and the device entries.

An end at step t (done or a time limit) closes the episode: nothing of step t + 1 reaches step t.  A death bootstraps from 0; a time limit from the value of
the state it cut off (trunc_value, else V(s_t): the partial-episode stand-in)."""
import ctypes as C

import numpy as np

EPS = 2.0 ** -24
QNAN = 0x7FC00000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _wide(a, shape, fill=0.0):
    return np.full(shape, fill, np.float64) if a is None else np.asarray(a).astype(np.float64)


def _ends(done, trunc, shape):
    d = np.zeros(shape, bool) if done is None else np.asarray(done) != 0
    tr = np.zeros(shape, bool) if trunc is None else np.asarray(trunc) != 0
    return d, tr


def gae64(reward, value, last_value, done, trunc, trunc_value, gamma, lam):
    """(adv, ret, S): A_t = delta_t + gamma * lam * A_{t+1} with delta_t = r_t + gamma * V(s_{t+1}) - V(s_t), both cut at an end; ret = A + V; and S, the
    bound's scale: S_t = (gamma |boot| + |r| + |v|) + gamma lam S_{t+1}, S_{t+1} reset at an end."""
    r = np.asarray(reward).astype(np.float64)
    T, N = r.shape
    v = _wide(value, (T, N))
    d, tr = _ends(done, trunc, (T, N))
    tv = v if trunc_value is None else np.asarray(trunc_value).astype(np.float64)
    nxt = _wide(last_value, (N,))
    gamma, lam = float(gamma), float(lam)
    adv, S = np.zeros((T, N)), np.zeros((T, N))
    a_next, s_next = np.zeros(N), np.zeros(N)
    for t in range(T - 1, -1, -1):
        boot = np.where(tr[t], tv[t], np.where(d[t], 0.0, nxt))
        live = ~(d[t] | tr[t])
        with np.errstate(all="ignore"):
            delta = r[t] + gamma * boot - v[t]
            adv[t] = delta + gamma * lam * np.where(live, a_next, 0.0)
            S[t] = (gamma * np.abs(boot) + np.abs(r[t]) + np.abs(v[t])) + gamma * lam * np.where(live, s_next, 0.0)
        a_next, s_next, nxt = adv[t], S[t], v[t]
    with np.errstate(all="ignore"):
        return adv, adv + v, S


def vtrace64(rho, c, rho_pg, reward, value, last_value, done, trunc, trunc_value, gamma):
    """(vs, pg_adv, S_vs, S_pg) for GIVEN clipped ratios rho, c (lambda folded in) and rho_pg [T, N] (float64): vs_t - V_t = rho_t delta_t + gamma c_t (vs_{t+1} -
    V_{t+1}); pg_adv_t = rho_pg_t (r_t + gamma vs_{t+1} - V_t), vs_{t+1} being the bootstrap value itself at an end."""
    r = np.asarray(reward).astype(np.float64)
    T, N = r.shape
    v = np.asarray(value).astype(np.float64)
    d, tr = _ends(done, trunc, (T, N))
    tv = v if trunc_value is None else np.asarray(trunc_value).astype(np.float64)
    nxt = _wide(last_value, (N,))
    vs_next = nxt.copy()
    gamma = float(gamma)
    vs, pg, S, Sp = np.zeros((T, N)), np.zeros((T, N)), np.zeros((T, N)), np.zeros((T, N))
    acc, s_next = np.zeros(N), np.zeros(N)
    for t in range(T - 1, -1, -1):
        boot = np.where(tr[t], tv[t], np.where(d[t], 0.0, nxt))
        end = d[t] | tr[t]
        with np.errstate(all="ignore"):
            acc = rho[t] * (r[t] + gamma * boot - v[t]) + gamma * c[t] * np.where(end, 0.0, acc)
            S[t] = np.abs(rho[t]) * (gamma * np.abs(boot) + np.abs(r[t]) + np.abs(v[t])) + gamma * np.abs(c[t]) * np.where(end, 0.0, s_next)
            vs[t] = v[t] + acc
            vb = np.where(end, boot, vs_next)
            pg[t] = rho_pg[t] * (r[t] + gamma * vb - v[t])
            # pg_adv rounds three times on (gamma |vs_boot| + |r| + |v|) and inherits gamma times the error of vs_{t+1}, each times rho_pg
            Sp[t] = np.abs(rho_pg[t]) * (gamma * np.abs(vb) + np.abs(r[t]) + np.abs(v[t]))
        s_next, nxt, vs_next = S[t], v[t], vs[t]
    return vs, pg, S, Sp


def ratio64(lt, lb, bar):
    with np.errstate(all="ignore"):
        return np.minimum(float(bar), np.exp(np.asarray(lt).astype(np.float64) - np.asarray(lb).astype(np.float64)))


def rollout(rng, T, N, done_rate=0.02, trunc_rate=0.0, specials=False):
    """Random f32 rows of one rollout: dict(reward, value, last_value, done, trunc, trunc_value, lb, lt).  specials: NaN, +-inf, -inf log-probabilities and
    the flag bytes 2 and 255 are sprinkled in."""
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    x = dict(reward=f(T, N), value=f(T, N) * 2, last_value=f(N) * 2, trunc_value=f(T, N) * 2,
             done=(rng.random_sample((T, N)) < done_rate).astype(np.uint8), trunc=(rng.random_sample((T, N)) < trunc_rate).astype(np.uint8),
             lb=-np.abs(f(T, N)) - 0.1, lt=-np.abs(f(T, N)) - 0.1)
    if specials and T * N >= 8:
        flat = lambda a: a.reshape(-1)  # noqa: E731
        pick = lambda k: rng.randint(0, T * N, k)  # noqa: E731
        k = max(1, T * N // 40)
        flat(x["reward"])[pick(k)] = np.nan
        flat(x["reward"])[pick(k)] = np.inf
        flat(x["value"])[pick(k)] = -np.inf
        flat(x["value"])[pick(k)] = np.nan
        flat(x["trunc_value"])[pick(k)] = np.inf
        flat(x["lb"])[pick(k)] = -np.inf
        flat(x["lt"])[pick(k)] = -np.inf
        flat(x["lt"])[pick(k)] = np.nan
        x["last_value"][rng.randint(0, N, max(1, N // 20))] = np.nan
        on = np.flatnonzero(flat(x["done"]))
        flat(x["done"])[on[::2]] = 2
        flat(x["done"])[on[1::4]] = 255
        on = np.flatnonzero(flat(x["trunc"]))
        flat(x["trunc"])[on[::2]] = 255
    return x


def _p(a):
    return None if a is None else a.ctypes.data


def gae_host(lib, reward, value, last_value, done, trunc, trunc_value, gamma, lam, want=(True, True)):
    T, N = reward.shape
    adv, ret = (np.full((T, N), 7.0, np.float32) if w else None for w in want)
    rc = lib.rg_gae_host(T, N, _p(reward), _p(value), _p(last_value), _p(done), _p(trunc), _p(trunc_value), gamma, lam, _p(adv), _p(ret))
    assert rc == 0, lib.rg_last_error(None).decode()
    return adv, ret


def vtrace_host(lib, lb, lt, reward, value, last_value, done, trunc, trunc_value, gamma, lam, bars=(1.0, 1.0, 1.0), want=(True, True)):
    T, N = reward.shape
    vs, pg = (np.full((T, N), 7.0, np.float32) if w else None for w in want)
    rc = lib.rg_vtrace_host(T, N, _p(lb), _p(lt), _p(reward), _p(value), _p(last_value), _p(done), _p(trunc), _p(trunc_value), gamma, lam, bars[0], bars[1], bars[2], _p(vs), _p(pg))
    assert rc == 0, lib.rg_last_error(None).decode()
    return vs, pg


def ratio_twin(lib, lt, lb, bar):
    """ratio(bar) alone, read off the twin: one step, reward 1, value 0, no bootstrap, gamma 0: pg_adv = rho_pg * (fma(0, 0, 1) - 0) = rho_pg exactly."""
    lt, lb = np.ascontiguousarray(lt, np.float32).reshape(1, -1), np.ascontiguousarray(lb, np.float32).reshape(1, -1)
    one, zero = np.ones_like(lt), np.zeros_like(lt)
    return vtrace_host(lib, lb, lt, one, zero, None, None, None, None, 0.0, 1.0, bars=(1.0, 1.0, float(bar)), want=(False, True))[1][0]


_ = C
