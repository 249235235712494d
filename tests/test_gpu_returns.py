"""Returns and advantages on the device (rg_gae, rg_vtrace; k_gae, k_vtrace in librogue_gym_returns.so): the kernels against the host twins as bit patterns over
the wave shapes, the pipeline's round sizes, the done rates and every optional array present and absent, with sentinel bytes around every output; the exact
aliases; the torch forms against the float64 statement of tests/returns_util.py; a rollout of real envs end to end; stream order; the refusals."""
import ctypes as C

import numpy as np
import pytest

import returns_util as ru
from returns_util import EPS, bits

pytestmark = pytest.mark.gpu
SENT = 0x5A
F = np.float32
# either side of every pipeline depth the kernels use (16 for rows of at most four words, 8 above) and of two rounds of it
STEPS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100)
RATES = (0.0, 0.02, 0.3, 1.0)


def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def lib_mod():
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Arena:
    """One uint8 device buffer of sentinel bytes with arrays carved out of it: what lies between and behind them must stay as it was."""

    def __init__(self, torch, dev, nbytes):
        self.torch, self.buf, self.used, self.spans = torch, torch.full((nbytes,), SENT, dtype=torch.uint8, device=dev), 0, []

    def carve(self, nbytes, shift=0):
        start = (self.used + 255) // 256 * 256 + shift
        self.used = start + nbytes + 64
        assert self.used <= self.buf.numel()
        self.spans.append((start, start + nbytes))
        return self.buf[start:start + nbytes]

    def put(self, host, shift=0):
        raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        t = self.carve(raw.size, shift)
        t.copy_(self.torch.from_numpy(raw.copy()))
        return t

    def intact(self):
        keep = np.ones(self.buf.numel(), bool)
        for s, e in self.spans:
            keep[s:e] = False
        return bool((self.buf.cpu().numpy()[keep] == SENT).all())


COMBOS = [(v, lv, d, tr, tv) for v in (1, 0) for lv in (1, 0) for d in (1, 0) for tr in (1, 0) for tv in (1, 0) if tr or not tv]     # 24: trunc_value needs trunc


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_kernels_equal_the_host_twins_bit_for_bit(N):
    """Every output of both kernels against the twins; a quarter of the 24 array combinations at each (N, T), so that every combination meets every T modulo 4
    and every N; the done rate and the outputs asked for (both, the first, the second) change with the case.  The outputs lie inside a sentinel-filled buffer:
    no byte before row 0 or behind row T - 1, column N - 1 changes."""
    torch = torch_mod()
    lib = lib_mod()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(50 + N)
    launches, seen = 0, set()
    for iT, T in enumerate(STEPS):
        rate = RATES[(iT + N) % 4]
        x = ru.rollout(rng, T, N, done_rate=rate, trunc_rate=0.1, specials=True)
        ar = Arena(torch, dev, 14 * (4 * T * N + 512) + 4096)
        shift = 4 if iT % 2 else 0                                        # base pointers on a multiple of 256, and one float further
        d = {k: ar.put(x[k], shift if x[k].dtype == F else shift // 4) for k in ("reward", "value", "last_value", "trunc_value", "lb", "lt", "done", "trunc")}
        out = [ar.carve(4 * T * N, shift) for _ in range(4)]
        for k, (v, lv, dn, tr, tv) in enumerate(COMBOS):
            if (k + iT) % 4:
                continue
            want = ((True, True), (True, False), (False, True))[(k // 4 + iT) % 3]
            seen.add((v, lv, dn, tr, tv))
            g = lambda name, on: (x[name], d[name]) if on else (None, None)  # noqa: E731
            (hv, dv), (hl, dl), (hd, dd), (ht, dt), (htv, dtv) = g("value", v), g("last_value", lv), g("done", dn), g("trunc", tr), g("trunc_value", tv)
            gamma, lam = (0.99, 0.95) if k % 2 else (1.0, 1.0)
            for o in out:
                o.fill_(SENT)
            rc = lib.rg_gae(None, T, N, ptr(d["reward"]), ptr(dv), ptr(dl), ptr(dd), ptr(dt), ptr(dtv), gamma, lam, ptr(out[0]) if want[0] else None, ptr(out[1]) if want[1] else None)
            assert rc == 0, lib.rg_last_error(None).decode()
            bars = (1.0, 1.0, 1.0) if k % 3 else (2.0, 0.5, 1.5)
            rc = lib.rg_vtrace(None, T, N, ptr(d["lb"]), ptr(d["lt"]), ptr(d["reward"]), ptr(d["value"]), ptr(dl), ptr(dd), ptr(dt), ptr(dtv), gamma, lam, bars[0], bars[1],
                               bars[2], ptr(out[2]) if want[0] else None, ptr(out[3]) if want[1] else None)
            assert rc == 0, lib.rg_last_error(None).decode()
            launches += 2
            exp = ru.gae_host(lib, x["reward"], hv, hl, hd, ht, htv, gamma, lam, want) + ru.vtrace_host(lib, x["lb"], x["lt"], x["reward"], x["value"], hl, hd, ht, htv, gamma, lam,
                                                                                                         bars, want)
            for i, (o, e) in enumerate(zip(out, exp)):
                got = o.cpu().numpy().view(np.uint32).reshape(T, N)
                bad = np.argwhere(got != (bits(e) if e is not None else 0x5A5A5A5A))
                assert len(bad) == 0, (N, T, rate, (v, lv, dn, tr, tv), want, i, bad[:4])
        torch.cuda.synchronize()
        assert ar.intact(), (N, T)                                        # nothing written before, between or behind the outputs
        for k, t in d.items():                                            # ... and no input changed
            assert (t.cpu().numpy() == np.ascontiguousarray(x[k]).view(np.uint8).reshape(-1)).all(), (N, T, k)
    assert len(seen) == len(COMBOS)
    print("%d launches" % launches)


def test_exact_aliases_give_the_bits_of_separate_outputs():
    torch = torch_mod()
    lib = lib_mod()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(61)
    for T, N in ((1, 1), (17, 65), (40, 257)):
        x = ru.rollout(rng, T, N, done_rate=0.1, trunc_rate=0.05, specials=True)
        adv, ret = ru.gae_host(lib, x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], x["trunc_value"], 0.99, 0.95)
        vs, pg = ru.vtrace_host(lib, x["lb"], x["lt"], x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], x["trunc_value"], 0.99, 0.95, (2.0, 1.0, 1.5))
        for outs in (("reward", "value"), ("value", "reward"), ("trunc_value", "value")):
            d = {k: torch.from_numpy(v.copy()).to(dev) for k, v in x.items()}
            rc = lib.rg_gae(None, T, N, ptr(d["reward"]), ptr(d["value"]), ptr(d["last_value"]), ptr(d["done"]), ptr(d["trunc"]), ptr(d["trunc_value"]), 0.99, 0.95,
                            ptr(d[outs[0]]), ptr(d[outs[1]]))
            assert rc == 0, lib.rg_last_error(None).decode()
            assert (bits(d[outs[0]].cpu().numpy()) == bits(adv)).all() and (bits(d[outs[1]].cpu().numpy()) == bits(ret)).all(), (T, N, outs)
        for outs in (("lb", "lt"), ("reward", "value"), ("lt", "trunc_value")):
            d = {k: torch.from_numpy(v.copy()).to(dev) for k, v in x.items()}
            rc = lib.rg_vtrace(None, T, N, ptr(d["lb"]), ptr(d["lt"]), ptr(d["reward"]), ptr(d["value"]), ptr(d["last_value"]), ptr(d["done"]), ptr(d["trunc"]),
                               ptr(d["trunc_value"]), 0.99, 0.95, 2.0, 1.0, 1.5, ptr(d[outs[0]]), ptr(d[outs[1]]))
            assert rc == 0, lib.rg_last_error(None).decode()
            assert (bits(d[outs[0]].cpu().numpy()) == bits(vs)).all() and (bits(d[outs[1]].cpu().numpy()) == bits(pg)).all(), (T, N, outs)


def test_torch_forms_against_the_float64_statement():
    """The CPU tolerances of tests/test_returns_host.py (4 and 5 roundings of S_t); non-contiguous and bf16 inputs are converted, not refused; no grad_fn."""
    torch = torch_mod()
    import rogue_gym
    lib = lib_mod()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(71)
    T, N = 100, 257
    x = ru.rollout(rng, T, N, done_rate=0.02, trunc_rate=0.02)
    d = {k: torch.from_numpy(v).to(dev) for k, v in x.items()}
    values = d["value"].clone().requires_grad_()
    adv, ret = rogue_gym.gae(d["reward"], values, d["done"].bool(), d["last_value"], gamma=0.99, lam=0.95, truncated=d["trunc"], trunc_values=d["trunc_value"])
    assert adv.grad_fn is None and ret.grad_fn is None and not adv.requires_grad and adv.dtype == torch.float32 and adv.device == dev and tuple(adv.shape) == (T, N)
    a64, r64, S = ru.gae64(x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], x["trunc_value"], F(0.99), F(0.95))
    assert (np.abs(adv.cpu().numpy() - a64) <= 4 * EPS * S).all() and (np.abs(ret.cpu().numpy() - r64) <= 4 * EPS * S + EPS * (np.abs(r64) + 4 * EPS * S)).all()
    a_t, r_t = ru.gae_host(lib, x["reward"], x["value"], x["last_value"], x["done"], x["trunc"], x["trunc_value"], 0.99, 0.95)
    assert (bits(adv.cpu().numpy()) == bits(a_t)).all() and (bits(ret.cpu().numpy()) == bits(r_t)).all()
    # a non-contiguous view (a [N, T] buffer transposed) and float64 rewards: converted
    adv2, _ = rogue_gym.gae(d["reward"].t().contiguous().t().double(), d["value"].t().contiguous().t(), d["done"], d["last_value"], truncated=d["trunc"],
                            trunc_values=d["trunc_value"])
    assert (bits(adv2.cpu().numpy()) == bits(a_t)).all()
    # bf16 values: the rule runs on their f32 widening
    vb = d["value"].bfloat16()
    adv3, _ = rogue_gym.gae(d["reward"], vb, d["done"], d["last_value"].bfloat16())
    a3, _ = ru.gae_host(lib, x["reward"], vb.float().cpu().numpy(), d["last_value"].bfloat16().float().cpu().numpy(), x["done"], None, None, 0.99, 0.95)
    assert (bits(adv3.cpu().numpy()) == bits(a3)).all()
    # reward-to-go
    rtg = rogue_gym.discounted_returns(d["reward"], d["done"], d["last_value"], gamma=0.9)
    _, r64, S = ru.gae64(x["reward"], None, x["last_value"], x["done"], None, None, F(0.9), F(1.0))
    assert rtg.grad_fn is None and (np.abs(rtg.cpu().numpy() - r64) <= 4 * EPS * S + EPS * (np.abs(r64) + 4 * EPS * S)).all()
    # V-trace, the float64 chain on the twin's own ratios
    bars = (2.0, 0.5, 1.5)
    lt = d["lt"].clone().requires_grad_()
    vs, pg = rogue_gym.vtrace(d["lb"], lt, d["reward"], d["value"], d["done"], d["last_value"], gamma=0.99, lam=0.9, rho_bar=bars[0], c_bar=bars[1], pg_rho_bar=bars[2],
                              truncated=d["trunc"])
    assert vs.grad_fn is None and pg.grad_fn is None
    rho, cr, rpg = (ru.ratio_twin(lib, x["lt"].reshape(-1), x["lb"].reshape(-1), b).reshape(T, N) for b in bars)
    vs64, pg64, S, P = ru.vtrace64(rho.astype(np.float64), (F(0.9) * cr).astype(np.float64), rpg.astype(np.float64), x["reward"], x["value"], x["last_value"], x["done"],
                                   x["trunc"], None, F(0.99))
    e_vs = 5 * EPS * S + EPS * (np.abs(vs64) + 5 * EPS * S)
    assert (np.abs(vs.cpu().numpy() - vs64) <= e_vs).all()
    end = (x["done"] != 0) | (x["trunc"] != 0)
    e_pg = 4 * EPS * P + EPS * np.abs(pg64) + rpg * float(F(0.99)) * np.where(end, 0.0, np.vstack([e_vs[1:], np.zeros((1, N))])) * (1 + 8 * EPS)
    assert (np.abs(pg.cpu().numpy() - pg64) <= e_pg).all()
    # empty rollouts, and the wrong device, shape or dtype by name
    assert tuple(rogue_gym.gae(d["reward"][:0], d["value"][:0], d["done"][:0])[0].shape) == (0, N)
    for words, call in ((("values",), lambda: rogue_gym.gae(d["reward"], d["value"][:3], d["done"])), (("dones",), lambda: rogue_gym.gae(d["reward"], d["value"], d["done"].int())),
                        (("rewards",), lambda: rogue_gym.gae(d["reward"].cpu(), d["value"], d["done"])), (("last_value",), lambda: rogue_gym.gae(d["reward"], d["value"], d["done"], d["last_value"].cpu())),
                        (("truncated",), lambda: rogue_gym.gae(d["reward"], d["value"], d["done"], truncated=d["trunc"][0])),
                        (("trunc_values",), lambda: rogue_gym.gae(d["reward"], d["value"], d["done"], trunc_values=d["trunc_value"])),
                        (("logp_target",), lambda: rogue_gym.vtrace(d["lb"], d["lt"][:, :5], d["reward"], d["value"], d["done"])),
                        (("c_bar",), lambda: rogue_gym.vtrace(d["lb"], d["lt"], d["reward"], d["value"], d["done"], c_bar=0.0)),
                        (("gamma",), lambda: rogue_gym.discounted_returns(d["reward"], d["done"], gamma=1.01))):
        with pytest.raises(ValueError) as e:
            call()
        assert all(w in str(e.value) for w in words), (words, str(e.value))


def test_end_to_end_on_a_rollout_of_real_envs(goldens):
    """256 mini envs with monsters, 32 steps, max_steps 20: env.act chooses the keys, the rollout stores reward, done, time_limit and the behaviour logp; gae with
    truncated=time_limit against the float64 statement; vtrace with logp_target = masked_logp(the same logits) equals gae in vs bit for bit."""
    torch = torch_mod()
    import rogue_gym
    import episode_util as eu
    from rogue_gym.envs import HipVecRogueEnv
    n, T = 256, 32
    cfg = eu._mini(goldens)
    env = HipVecRogueEnv([dict(cfg, seed=7000 + i) for i in range(n)], max_steps=20, action_mask=True, episodes=True)
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(3)
    env.reset()
    rew, done, tl, logp_b, logits_b, mask_b, act_b = [], [], [], [], [], [], []
    for t in range(T):
        logits = torch.randn((n, len(env.ACTIONS)), generator=gen, device=dev)
        res = env.act(logits, seed=100 + t)
        mask_b.append(env.action_mask.clone())
        logits_b.append(logits)
        act_b.append(res.actions.clone())
        logp_b.append(res.logp.clone())
        _, reward, d = env.step_keys(res.keys)
        rew.append(reward.float().clone())
        done.append(d.bool().clone())
        tl.append(env.time_limit.clone())
    env.check_errors()
    rew, done, tl, logp_b = torch.stack(rew), torch.stack(done), torch.stack(tl), torch.stack(logp_b)
    n_tl, n_other = int(tl.sum()), int((done & ~tl).sum())
    print("%d time-limit ends, %d other ends" % (n_tl, n_other))
    assert n_tl >= 1 and n_other >= 1 and not (tl & ~done).any()
    values = torch.randn((T, n), generator=gen, device=dev)
    last = torch.randn((n,), generator=gen, device=dev)
    adv, ret = rogue_gym.gae(rew, values, done, last, gamma=0.99, lam=0.95, truncated=tl)
    a64, r64, S = ru.gae64(rew.cpu().numpy(), values.cpu().numpy(), last.cpu().numpy(), done.cpu().numpy(), tl.cpu().numpy(), None, F(0.99), F(0.95))
    assert (np.abs(adv.cpu().numpy() - a64) <= 4 * EPS * S).all() and (np.abs(ret.cpu().numpy() - r64) <= 4 * EPS * S + EPS * (np.abs(r64) + 4 * EPS * S)).all()
    # a time limit treated as a death gives another answer: the flag matters in this run
    adv_d, _ = rogue_gym.gae(rew, values, done, last, gamma=0.99, lam=0.95)
    assert not torch.equal(adv_d, adv)
    logp_t, _ = rogue_gym.masked_logp(torch.stack(logits_b), torch.stack(act_b), torch.stack(mask_b))
    assert torch.equal(logp_t, logp_b)                                    # unchanged weights: the ratio is exactly 1
    vs, pg = rogue_gym.vtrace(logp_b, logp_t, rew, values, done, last, gamma=0.99, lam=0.95, truncated=tl)
    assert (bits(vs.cpu().numpy()) == bits(ret.cpu().numpy())).all()
    env.close()


def test_stream_order_on_a_side_stream():
    """Inside a side stream of the caller's, behind work enqueued there, without a device-wide synchronise: the inputs are produced on that stream by a chain of
    kernels long enough to be still running when the call is enqueued, and the result is read through an event of that stream."""
    torch = torch_mod()
    import rogue_gym
    lib = lib_mod()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(81)
    T, N = 64, 4096
    x = ru.rollout(rng, T, N, done_rate=0.02)
    d = {k: torch.from_numpy(v).to(dev) for k, v in x.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        r = torch.zeros_like(d["reward"])
        for _ in range(200):                                              # (200 small kernels ahead of the call; the rewards are finite, so r stays 0)
            r = r + d["reward"] * 0.0
        r = r + d["reward"]
        adv, ret = rogue_gym.gae(r, d["value"], d["done"], d["last_value"], gamma=0.99, lam=0.95)
        ev = torch.cuda.Event()
        ev.record(side)
    ev.synchronize()
    a_t, r_t = ru.gae_host(lib, x["reward"], x["value"], x["last_value"], x["done"], None, None, 0.99, 0.95)
    assert (bits(adv.cpu().numpy()) == bits(a_t)).all() and (bits(ret.cpu().numpy()) == bits(r_t)).all()


def test_refusals_launch_nothing_and_write_nothing():
    torch = torch_mod()
    lib = lib_mod()
    dev = torch.device("cuda:0")
    T, N = 5, 70
    z = lambda: torch.zeros((T, N), device=dev)  # noqa: E731
    r, v, lp = z(), z(), z()
    flags = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    a, b = torch.full((T, N), 7.0, device=dev), torch.full((T, N), 7.0, device=dev)
    for words, call in (
            (("rg_gae:", "n_steps"), lambda: lib.rg_gae(None, -1, N, ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, ptr(a), ptr(b))),
            (("rg_gae:", "n_envs"), lambda: lib.rg_gae(None, T, -1, ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, ptr(a), ptr(b))),
            (("rg_gae:", "reward"), lambda: lib.rg_gae(None, T, N, None, ptr(v), None, None, None, None, 0.9, 0.9, ptr(a), ptr(b))),
            (("rg_gae:", "both"), lambda: lib.rg_gae(None, T, N, ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, None, None)),
            (("rg_gae:", "gamma"), lambda: lib.rg_gae(None, T, N, ptr(r), ptr(v), None, None, None, None, 1.5, 0.9, ptr(a), ptr(b))),
            (("rg_gae:", "lam"), lambda: lib.rg_gae(None, T, N, ptr(r), ptr(v), None, None, None, None, 0.9, float("nan"), ptr(a), ptr(b))),
            (("rg_gae:", "trunc_value"), lambda: lib.rg_gae(None, T, N, ptr(r), ptr(v), None, None, None, ptr(v), 0.9, 0.9, ptr(a), ptr(b))),
            (("rg_gae:", "overlaps", "reward"), lambda: lib.rg_gae(None, T - 1, N, ptr(a), ptr(v), None, None, None, None, 0.9, 0.9, C.c_void_p(a.data_ptr() + 4 * N), ptr(b))),
            (("rg_gae:", "overlaps", "done"), lambda: lib.rg_gae(None, T, N, ptr(r), ptr(v), None, ptr(a), None, None, 0.9, 0.9, ptr(a), ptr(b))),
            (("rg_vtrace:", "value"), lambda: lib.rg_vtrace(None, T, N, ptr(lp), ptr(lp), ptr(r), None, None, None, None, None, 0.9, 0.9, 1.0, 1.0, 1.0, ptr(a), ptr(b))),
            (("rg_vtrace:", "logp_behaviour"), lambda: lib.rg_vtrace(None, T, N, None, ptr(lp), ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, 1.0, 1.0, 1.0, ptr(a), ptr(b))),
            (("rg_vtrace:", "rho_bar"), lambda: lib.rg_vtrace(None, T, N, ptr(lp), ptr(lp), ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, 0.0, 1.0, 1.0, ptr(a), ptr(b))),
            (("rg_vtrace:", "c_bar"), lambda: lib.rg_vtrace(None, T, N, ptr(lp), ptr(lp), ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, 1.0, float("inf"), 1.0, ptr(a), ptr(b))),
            (("rg_vtrace:", "pg_rho_bar"), lambda: lib.rg_vtrace(None, T, N, ptr(lp), ptr(lp), ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, 1.0, 1.0, -1.0, ptr(a), ptr(b))),
            (("rg_vtrace:", "overlaps"), lambda: lib.rg_vtrace(None, T - 1, N, ptr(lp), ptr(lp), ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, 1.0, 1.0, 1.0, ptr(a),
                                                                 C.c_void_p(a.data_ptr() + 4)))):
        assert call() != 0
        msg = lib.rg_last_error(None).decode()
        assert all(w in msg for w in words), (words, msg)
    # empty rollouts: valid, nothing launched
    assert lib.rg_gae(None, 0, N, ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, ptr(a), ptr(b)) == 0
    assert lib.rg_vtrace(None, T, 0, ptr(lp), ptr(lp), ptr(r), ptr(v), None, None, None, None, 0.9, 0.9, 1.0, 1.0, 1.0, ptr(a), ptr(b)) == 0
    torch.cuda.synchronize()
    assert bool((a == 7.0).all()) and bool((b == 7.0).all()) and not bool(flags.any())
