"""The learner's side of the action rule on the device (rg_policy_eval, rg_policy_grad; k_pg_eval, k_pg_grad in librogue_gym_learn.so): the kernels against the
host twins as bit patterns over every wave shape, key count, dtype and pointer alignment with sentinel bytes around every output; masked_logp against what
env.act answered, bit for bit; the autograd path against the float64 NaN-safe chain; the refusals."""
import ctypes as C

import numpy as np
import pytest

import mask_util as mu
import policy_edge_rows as pe
import policy_grad_util as pg
import policy_util as pu
from policy_grad_util import BF16, F16, F32

pytestmark = pytest.mark.gpu
SENT = 0x5A


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
    """One uint8 device buffer of sentinel bytes with arrays carved out of it at chosen byte offsets: what lies between and behind them must stay as it was."""

    def __init__(self, torch, dev, nbytes):
        self.torch, self.buf, self.used, self.spans = torch, torch.full((nbytes,), SENT, dtype=torch.uint8, device=dev), 0, []

    def carve(self, nbytes, shift=0):
        """nbytes at the next multiple of 256 plus `shift`, 64 sentinel bytes kept behind it."""
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


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_kernels_equal_the_host_twins_bit_for_bit(dtype):
    torch = torch_mod()
    lib = lib_mod()
    dev = torch.device("cuda:0")
    esz = 4 if dtype == F32 else 2
    rng = np.random.RandomState(40 + dtype)
    launches = 0
    for nk in (1, 5, 11, 19, 32):
        for B in (1, 63, 64, 65, 200):   # a lone lane, a partial wave, exactly one wave, a wave and one row, three waves and a tail
            x = pg.typed_rows(rng, B, nk, dtype)             # the special rows among them
            mask = pg.random_masks(rng, B, nk)               # 0 to nk legal keys
            a = pg.actions_for(rng, mask)                    # -1, nk, an illegal key and the ends of int32 among them
            g_lp, g_ent = rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)
            g_lp[B // 2], g_ent[B // 3] = np.nan, np.inf
            for shifted in (False, True):                    # every base pointer on a multiple of 256, and one row further
                ar = Arena(torch, dev, 1 << 17)
                row = nk * esz if shifted else 0
                dx_ = ar.put(x, row)
                dm = ar.put(mask.view(np.uint8), nk if shifted else 0)
                da, dgl, dge = ar.put(a, 4 if shifted else 0), ar.put(g_lp, 4 if shifted else 0), ar.put(g_ent, 4 if shifted else 0)
                olp, oent, odx = ar.carve(4 * B, 4 if shifted else 0), ar.carve(4 * B, 4 if shifted else 0), ar.carve(B * nk * esz, row)
                for inv_temp in (1.0, 0.7):
                    for m_host, m_dev in ((mask, dm), (None, None)):
                        for want in ((True, True), (True, False), (False, True)):
                            olp.fill_(SENT), oent.fill_(SENT)
                            rc = lib.rg_policy_eval(None, B, nk, ptr(dx_), dtype, ptr(m_dev), ptr(da), inv_temp, ptr(olp) if want[0] else None, ptr(oent) if want[1] else None)
                            assert rc == 0, lib.rg_last_error(None).decode()
                            launches += 1
                            exp = pg.eval_host(lib, x, dtype, m_host, a, inv_temp, want)
                            for o, e in zip((olp, oent), exp):
                                got = o.cpu().numpy().view(np.uint32)
                                assert (got == (pg.bits(e) if e is not None else 0x5A5A5A5A)).all(), (nk, B, shifted, inv_temp, m_host is None, want)
                        for gl_host, gl_dev, ge_host, ge_dev in ((g_lp, dgl, g_ent, dge), (g_lp, dgl, None, None), (None, None, g_ent, dge), (None, None, None, None)):
                            odx.fill_(SENT)
                            rc = lib.rg_policy_grad(None, B, nk, ptr(dx_), dtype, ptr(m_dev), ptr(da), inv_temp, ptr(gl_dev), ptr(ge_dev), ptr(odx))
                            assert rc == 0, lib.rg_last_error(None).decode()
                            launches += 1
                            exp = pg.grad_host(lib, x, dtype, m_host, a, gl_host, ge_host, inv_temp)
                            got = odx.cpu().numpy().view(pg.bits(exp).dtype).reshape(B, nk)
                            bad = np.argwhere(got != pg.bits(exp))
                            assert len(bad) == 0, (nk, B, shifted, inv_temp, m_host is None, gl_host is None, ge_host is None, bad[:4])
                torch.cuda.synchronize()
                assert ar.intact(), (nk, B, shifted)          # nothing written before, between or behind the outputs; no input changed
                for t, h in ((dx_, x), (dm, mask), (da, a)):
                    assert (t.cpu().numpy() == np.ascontiguousarray(h).view(np.uint8).reshape(-1)).all()
    print("%d launches" % launches)


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_kernels_equal_the_host_twins_on_the_edge_rows(dtype):
    """policy_edge_rows.edge_batch through k_pg_eval / k_pg_grad: the six logit families (|d| up to 86 and past the cut-off, 1e6, near ties, subnormal logits and
    subnormal products w * inv), the cut-off pair, gradients that are exact binary16 ties, flat rows -- at inverse temperatures 0.01, 1, 7.3 and 100, where the
    host tests hold the twin against float64, the kernels against the twin as bit patterns."""
    torch = torch_mod()
    lib = lib_mod()
    dev = torch.device("cuda:0")
    nk, esz = 11, 4 if dtype == F32 else 2
    for B in (65, 200):                                      # a wave and one row; three waves and a tail
        x32, mask, a, g_lp, g_ent = pe.edge_batch(B, nk, seed=B)
        if dtype == F16:
            with np.errstate(over="ignore"):
                x = x32.astype(np.float16)
        else:
            x = pu.to_bf16(x32) if dtype == BF16 else x32
        ar = Arena(torch, dev, 1 << 16)
        dx_, dm, da, dgl, dge = ar.put(x), ar.put(mask.view(np.uint8)), ar.put(a), ar.put(g_lp), ar.put(g_ent)
        olp, oent, odx = ar.carve(4 * B), ar.carve(4 * B), ar.carve(B * nk * esz)
        for inv_temp in pe.INV_TEMPS:
            olp.fill_(SENT), oent.fill_(SENT)
            rc = lib.rg_policy_eval(None, B, nk, ptr(dx_), dtype, ptr(dm), ptr(da), inv_temp, ptr(olp), ptr(oent))
            assert rc == 0, lib.rg_last_error(None).decode()
            lp, ent = pg.eval_host(lib, x, dtype, mask, a, inv_temp)
            for o, e, what in ((olp, lp, "logp"), (oent, ent, "entropy")):
                bad = np.flatnonzero(o.cpu().numpy().view(np.uint32) != pg.bits(e))
                assert len(bad) == 0, (what, B, inv_temp, bad[:4], [r % 12 for r in bad[:4]])
            for gl_host, gl_dev, ge_host, ge_dev in ((g_lp, dgl, g_ent, dge), (g_lp, dgl, None, None), (None, None, g_ent, dge)):
                odx.fill_(SENT)
                rc = lib.rg_policy_grad(None, B, nk, ptr(dx_), dtype, ptr(dm), ptr(da), inv_temp, ptr(gl_dev), ptr(ge_dev), ptr(odx))
                assert rc == 0, lib.rg_last_error(None).decode()
                exp = pg.grad_host(lib, x, dtype, mask, a, gl_host, ge_host, inv_temp)
                got = odx.cpu().numpy().view(pg.bits(exp).dtype).reshape(B, nk)
                bad = np.argwhere(got != pg.bits(exp))
                assert len(bad) == 0, (B, inv_temp, gl_host is None, ge_host is None, bad[:4], [r % 12 for r, _ in bad[:4]])
            if inv_temp == 1.0 and dtype == F32:             # the rows are what they are meant to be (the twin's answers, which the host tests hold against the rule)
                kind = np.arange(B) % 12
                assert np.isfinite(lp[kind == 6]).all() and (lp[kind == 7] == -np.inf).all() and (ent[kind == 7] == 0).all()
                assert (np.abs(lp[kind == 11] + np.log(mask[kind == 11].sum(1))) < 1e-6).all()
        torch.cuda.synchronize()
        assert ar.intact(), B
        for t, h in ((dx_, x), (dm, mask), (da, a)):
            assert (t.cpu().numpy() == np.ascontiguousarray(h).view(np.uint8).reshape(-1)).all()


@pytest.mark.parametrize("bf16", [False, True])
def test_masked_logp_answers_what_act_answered(goldens, bf16):
    torch = torch_mod()
    import rogue_gym
    from rogue_gym.envs.device import HipVecRogueEnv
    n = 200
    cfgs = [dict(goldens["configs"]["mini"], enemies=mu.ENEMIES, seed=900 + i) for i in range(n)]
    env = HipVecRogueEnv(cfgs, max_steps=60, action_mask=True)
    gen = torch.Generator(device=env.device).manual_seed(5)
    for steps in (0, 30):
        for keys in mu.key_table(8, steps, n):
            env.step_keys(torch.as_tensor(keys).to(env.device))
        for temperature in (1.0, 1.7):
            logits = (torch.randn((n, 11), generator=gen, device=env.device) * 3).to(torch.bfloat16 if bf16 else torch.float32)
            res = env.act(logits, temperature=temperature, epsilon=0.3, seed=steps)     # (logp is under the pure softmax whatever chose the action)
            logp, ent = rogue_gym.masked_logp(logits, res.actions, env.action_mask, temperature=temperature)
            assert logp.dtype == ent.dtype == torch.float32 and tuple(logp.shape) == (n,)
            assert torch.equal(logp.view(torch.int32), res.logp.view(torch.int32)) and torch.equal(ent.view(torch.int32), res.entropy.view(torch.int32))
            assert bool((torch.exp(logp - res.logp) == 1.0).all())
            lp2, ent2 = env.evaluate(logits, res.actions.long(), temperature=temperature)   # mask = env.action_mask, any integer dtype for the actions
            assert torch.equal(lp2, logp) and torch.equal(ent2, ent)
            lp3, _ = rogue_gym.masked_logp(logits, res.actions, env._mask_u8, temperature=temperature)
            assert torch.equal(lp3, logp)
    assert not bool(env.action_mask.all()) and bool(torch.isfinite(res.logp).all())
    env.check_errors()
    env.close()


def rows(B=200, nk=11, seed=3):
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal((B, nk)) * 3).astype(np.float32)
    mask = pg.random_masks(rng, B, nk, lo=1)
    a = np.array([rng.choice(np.flatnonzero(m)) for m in mask], np.int64)
    return x, mask, a, rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)


def test_autograd_against_the_float64_chain():
    torch = torch_mod()
    lib = lib_mod()
    import rogue_gym
    dev = torch.device("cuda:0")
    x, mask, a, g_lp, g_ent = rows()
    B, nk = x.shape
    tol = 4 * pg.MEASURED_GRAD
    lp64, ent64, dx64 = pg.chain64(x, mask, a, g_lp, g_ent)
    xt, mt, at = torch.from_numpy(x).to(dev).requires_grad_(), torch.from_numpy(mask).to(dev), torch.from_numpy(a).to(dev)
    glt, get = torch.from_numpy(g_lp).to(dev), torch.from_numpy(g_ent).to(dev)
    lp, ent = rogue_gym.masked_logp(xt, at, mt)
    assert lp.requires_grad and ent.requires_grad
    ((lp * glt).sum() + (ent * get).sum()).backward()
    got = xt.grad.cpu().numpy()
    print("largest |logits.grad - float64 chain| %.3g (bound %.3g)" % (np.abs(got - dx64).max(), tol))
    assert xt.grad.dtype == torch.float32 and np.abs(got - dx64).max() <= tol
    assert (pg.bits(got)[~mask] == 0).all()                                            # an illegal key: exactly +0.0
    assert (pg.bits(got) == pg.bits(pg.grad_host(lib, x, F32, mask, a, g_lp, g_ent))).all()
    # logp alone and the entropy alone: the unused output's gradient is absent, not a tensor of zeros
    for use_lp in (True, False):
        xt.grad = None
        lp, ent = rogue_gym.masked_logp(xt, at, mt)
        ((lp * glt) if use_lp else (ent * get)).sum().backward()
        got = xt.grad.cpu().numpy()
        assert np.abs(got - pg.chain64(x, mask, a, g_lp if use_lp else None, None if use_lp else g_ent)[2]).max() <= tol
        assert (pg.bits(got) == pg.bits(pg.grad_host(lib, x, F32, mask, a, g_lp if use_lp else None, None if use_lp else g_ent))).all()
    # no mask, a temperature, leading dimensions [4, 50]
    xt.grad = None
    lp, ent = rogue_gym.masked_logp(xt.view(4, 50, nk), at.view(4, 50), None, temperature=2.0)
    assert tuple(lp.shape) == (4, 50)
    (lp * glt.view(4, 50) + ent * get.view(4, 50)).sum().backward()
    assert np.abs(xt.grad.cpu().numpy() - pg.chain64(x, np.ones_like(mask), a, g_lp, g_ent, np.float32(0.5))[2]).max() <= tol
    # bf16 logits get a bf16 gradient: the f32 result rounded to nearest even, the twin's bits
    xb = pg.typed_rows(np.random.RandomState(1), B, nk, BF16)
    xbt = torch.from_numpy(xb.view(np.int16).copy()).to(dev).view(torch.bfloat16).requires_grad_()
    lp, ent = rogue_gym.masked_logp(xbt, at, mt)
    (lp.nan_to_num(neginf=0.0) * glt + ent * get).sum().backward()
    assert xbt.grad.dtype == torch.bfloat16
    assert (xbt.grad.view(torch.int16).cpu().numpy().view(np.uint16) == pg.bits(pg.grad_host(lib, xb, BF16, mask, a, g_lp, g_ent))).all()
    # a non-contiguous input gets its gradient back in its own layout
    base = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev).requires_grad_()           # [nk, B]: logits = base.t() has strides (1, B)
    lp, ent = rogue_gym.masked_logp(base.t(), at, mt)
    ((lp * glt).sum() + (ent * get).sum()).backward()
    assert tuple(base.grad.shape) == (nk, B) and base.grad.is_contiguous()
    assert (pg.bits(base.grad.cpu().numpy().T) == pg.bits(pg.grad_host(lib, x, F32, mask, a, g_lp, g_ent))).all()
    # logits that need no gradient: values only, nothing to differentiate
    lp, ent = rogue_gym.masked_logp(xt.detach(), at, mt)
    assert not lp.requires_grad and not ent.requires_grad


def test_the_gradient_of_a_linear_layer():
    """logits = obs @ W in float64, rounded to float32 for masked_logp: W.grad = obs^T @ dlogits, summed in float64, so it differs from the chain's by no more
    than sum_r |obs[r, i]| times the bound of one gradient."""
    torch = torch_mod()
    import rogue_gym
    dev = torch.device("cuda:0")
    _, mask, a, g_lp, g_ent = rows(seed=9)
    B, nk, F = mask.shape[0], mask.shape[1], 24
    rng = np.random.RandomState(2)
    obs = (rng.rand(B, F) < 0.3).astype(np.float64)
    W = torch.from_numpy(rng.standard_normal((F, nk))).to(dev).requires_grad_()
    logits = (torch.from_numpy(obs).to(dev) @ W).float()
    lp, ent = rogue_gym.masked_logp(logits, torch.from_numpy(a).to(dev), torch.from_numpy(mask).to(dev))
    ((lp * torch.from_numpy(g_lp).to(dev)).sum() + (ent * torch.from_numpy(g_ent).to(dev)).sum()).backward()
    dx64 = pg.chain64(logits.detach().cpu().numpy(), mask, a, g_lp, g_ent)[2]
    want = obs.T @ dx64
    bound = obs.sum(0)[:, None] * 4 * pg.MEASURED_GRAD + 1e-12
    err = np.abs(W.grad.cpu().numpy() - want)
    print("largest |W.grad - chain| %.3g, bound %.3g" % (err.max(), bound.min()))
    assert W.grad.dtype == torch.float64 and (err <= bound).all()


def test_inside_a_stream_of_the_callers():
    torch = torch_mod()
    lib = lib_mod()
    import rogue_gym
    dev = torch.device("cuda:0")
    x, mask, a, g_lp, g_ent = rows(B=4096, seed=12)
    xt, mt, at = torch.from_numpy(x).to(dev).requires_grad_(), torch.from_numpy(mask).to(dev), torch.from_numpy(a).to(dev)
    glt, get = torch.from_numpy(g_lp).to(dev), torch.from_numpy(g_ent).to(dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        lp, ent = rogue_gym.masked_logp(xt, at, mt)
        ((lp * glt).sum() + (ent * get).sum()).backward()
    s.synchronize()                                                                      # this stream alone
    lp1, ent1 = pg.eval_host(lib, x, F32, mask, a)
    assert (pg.bits(lp.detach().cpu().numpy()) == pg.bits(lp1)).all() and (pg.bits(ent.detach().cpu().numpy()) == pg.bits(ent1)).all()
    assert (pg.bits(xt.grad.cpu().numpy()) == pg.bits(pg.grad_host(lib, x, F32, mask, a, g_lp, g_ent))).all()


def test_refusals_launch_nothing():
    torch = torch_mod()
    lib = lib_mod()
    import rogue_gym
    dev = torch.device("cuda:0")
    x, a = torch.zeros((64, 11), device=dev), torch.zeros((64,), dtype=torch.int32, device=dev)
    lp, dx = torch.full((64,), 7.0, device=dev), torch.full((64, 11), 7.0, device=dev)

    def refused(words, n_rows=64, nk=11, dtype=0, inv_temp=1.0, logits=True, action=True, dlogits=True):
        for name in ("rg_policy_eval", "rg_policy_grad"):
            if "eval" in name and not dlogits:
                continue
            args = [None, n_rows, nk, ptr(x) if logits else None, dtype, None, ptr(a) if action else None, inv_temp]
            args += [ptr(lp), None] if "eval" in name else [None, None, ptr(dx) if dlogits else None]
            rc = getattr(lib, name)(*args)
            msg = lib.rg_last_error(None).decode()
            assert rc != 0 and msg.startswith(name + ":") and all(w in msg for w in words), (name, words, msg)
        torch.cuda.synchronize()
        assert bool((lp == 7.0).all()) and bool((dx == 7.0).all())

    refused(("n_keys", "got 0"), nk=0)
    refused(("n_keys", "got 33"), nk=33)
    refused(("dtype", "got 3"), dtype=3)
    refused(("n_rows", "-5"), n_rows=-5)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(("inv_temp",), inv_temp=bad)
    refused(("logits_dev",), logits=False)
    refused(("action_dev",), action=False)
    refused(("dlogits_dev",), dlogits=False)
    # no rows: a valid call that writes nothing
    assert lib.rg_policy_eval(None, 0, 11, ptr(x), 0, None, ptr(a), 1.0, ptr(lp), None) == 0
    assert lib.rg_policy_grad(None, 0, 11, ptr(x), 0, None, ptr(a), 1.0, None, None, ptr(dx)) == 0
    torch.cuda.synchronize()
    assert bool((lp == 7.0).all()) and bool((dx == 7.0).all())
    # the Python form names what it refuses
    for bad in (lambda: rogue_gym.masked_logp(x.double(), a), lambda: rogue_gym.masked_logp(x, a.float()), lambda: rogue_gym.masked_logp(x, a[:3]),
                lambda: rogue_gym.masked_logp(x, a, torch.ones((64, 10), dtype=torch.bool, device=dev)), lambda: rogue_gym.masked_logp(x, a, temperature=0.0),
                lambda: rogue_gym.masked_logp(x.cpu(), a.cpu())):
        with pytest.raises(ValueError):
            bad()
    empty = rogue_gym.masked_logp(x[:0], a[:0])
    assert tuple(empty[0].shape) == (0,)
