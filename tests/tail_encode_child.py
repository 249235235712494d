"""Child process of tests/test_gpu_tail_encode.py: one batch size per process, because the envs per step wave (ROGUE_GYM_HIP_EPW) are read once, when the
library first launches a step.

usage: tail_encode_child.py CHECK N        CHECK = oracle | twins | cadence | nokey | nolive

Every check plays the mini config with per-env seeds = env index and keys drawn from the 11 actions with a fixed numpy seed; every 4th step sends '>'
to every env, so that stair waves run.  HipVecRogueEnv.step_keys is the call under test: on this config it arms the tail encode (rg_step_obs_gray)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rogue-gym_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from oracle.pyoracle import OracleBatch  # noqa: E402
from parity_util import ACTION_KEYS  # noqa: E402
from rogue_gym.envs.device import HipVecRogueEnv  # noqa: E402

MSG_SHIFT, MSG_MASK = 8, 0x7F


def mini():
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        return json.load(f)["configs"]["mini"]


def configs(n):
    cfg = mini()
    return [dict(cfg, seed=i) for i in range(n)]


def threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def draw_keys(rng, n, t):
    keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)].copy()
    if t % 4 == 0:
        keys[:] = ord(">")
    return keys


def dev(env, keys):
    return torch.as_tensor(np.ascontiguousarray(keys, np.uint8), device=env.device)


def bad_envs(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.flatnonzero((a != b).reshape(len(a), -1).any(1))[:8].tolist()


def against_oracle(env, ob, exp, st_prev, where):
    """The observation tensor, reward, done and -- through fetch() -- status, public flag bits and both mirrors of every env against the oracle batch."""
    n = env.num_envs
    got = env.obs.cpu().numpy()
    assert np.array_equal(got, exp), "%s: gray observation differs at envs %s" % (where, bad_envs(got, exp))
    o_scr, o_hist, st, fl = ob.fetch()
    term = fl[:, 0] != 0
    if st_prev is not None:
        exp_reward = np.maximum(0, st[:, 1].astype(np.int64) - st_prev[:, 1].astype(np.int64)).astype(np.float32)
        reward = env.reward.cpu().numpy()
        assert np.array_equal(reward, exp_reward), "%s: reward differs at envs %s" % (where, bad_envs(reward, exp_reward))
        done = env.done.cpu().numpy().astype(bool)
        assert np.array_equal(done, term), "%s: done differs at envs %s" % (where, bad_envs(done, term))
    scr, hist, status, flags = env._h.fetch()
    flags = flags.astype(np.uint32)
    assert np.array_equal(status.astype(np.uint32).reshape(n, 10), st), "%s: status differs at envs %s" % (where, bad_envs(status.astype(np.uint32).reshape(n, 10), st))
    for what, g, e in (("terminal bit", (flags & 1) != 0, term), ("dead bit", (flags & 2) != 0, fl[:, 3] != 0), ("message bits", (flags >> MSG_SHIFT) & MSG_MASK, fl[:, 1]),
                       ("screen mirror", scr, o_scr), ("history mirror", hist, o_hist)):
        assert np.array_equal(g, e), "%s: %s differs at envs %s" % (where, what, bad_envs(g, e))
    return st, term


def check_oracle(n):
    """Lock step with the oracle at every step: 60 steps with max_steps = 7 (mass timeouts, spare takes), then 120 steps with max_steps = 1000 on a second handle."""
    resets = descents = 0
    for max_steps, steps, seed in ((7, 60, 11), (1000, 120, 12)):
        env = HipVecRogueEnv(configs(n), max_steps=max_steps)
        ob = OracleBatch(configs(n), max_steps=max_steps, n_threads=threads())
        exp = np.empty((n, 1, ob.h, ob.w), np.float32)
        rng = np.random.RandomState(seed)
        st_prev = ob.fetch(screen=False, hist=False)[2]
        for t in range(1, steps + 1):
            keys = draw_keys(rng, n, t)
            env.step_keys(dev(env, keys))
            ob.step(keys, exp)
            st, term = against_oracle(env, ob, exp, st_prev, "max_steps %d step %d" % (max_steps, t))
            resets += int(term.sum())
            descents += int(((st[:, 0] > st_prev[:, 0]) & ~term).sum())
            st_prev = st
        env.check_errors()
        env.close()
    print("oracle side: %d resets, %d descents" % (resets, descents))
    # what keeps the run from going hollow, counted on the oracle's side alone (at n = 80: 845 resets and 36 descents; at n = 48: 498 and 17)
    assert resets >= 20 * n // 80 and descents >= 3, (resets, descents)


def make(n, max_steps, tail):
    if not tail:
        os.environ["ROGUE_GYM_HIP_NO_TAIL_ENCODE"] = "1"
    try:
        return HipVecRogueEnv(configs(n), max_steps=max_steps)
    finally:
        os.environ.pop("ROGUE_GYM_HIP_NO_TAIL_ENCODE", None)


def rng_words(env, ids):
    return [list(env._h.debug_state(int(i))[0].rng) for i in ids]


def check_twins(n):
    """(a) the tail encode, (b) ROGUE_GYM_HIP_NO_TAIL_ENCODE=1, (c) rg_step and rg_obs_gray as separate calls: bit-identical at EVERY step (max_steps = 9 reseeds
    an env that went astray within a few steps) -- the images, both mirrors, status, the whole flag words, reward, done, and the state records of every env
    (rg_state_save: canonical, equal states give equal bytes; a record holds the env's three RNG streams beside its grids, tables and dist cache), compared
    on the device.  The RNG words are also read out as such (rg_debug_fetch) for a few envs, the batch's first and last among them."""
    a, b, c = make(n, 9, True), make(n, 9, False), make(n, 9, True)
    rng = np.random.RandomState(21)
    sample = sorted({0, 1, n // 3, n // 2, n - 2, n - 1})
    for t in range(1, 91):
        keys = draw_keys(rng, n, t)
        a.step_keys(dev(a, keys))
        b.step_keys(dev(b, keys))
        kc = dev(c, keys)
        c._h.check(c._h.L.rg_step(c._h.h, C.c_void_p(kc.data_ptr()), 1))
        c._encode()
        torch.cuda.synchronize()
        fa = a._h.fetch()
        for name, o in (("NO_TAIL_ENCODE", b), ("separate calls", c)):
            where = "step %d, tail encode vs %s" % (t, name)
            assert torch.equal(a.obs.view(torch.int32), o.obs.view(torch.int32)), "%s: observation differs at envs %s" % (where, bad_envs(a.obs.cpu().numpy(), o.obs.cpu().numpy()))
            for what, x, y in zip(("screen mirror", "history mirror", "status", "flag words"), fa, o._h.fetch()):
                assert np.array_equal(x, y), "%s: %s differs at envs %s" % (where, what, bad_envs(x, y))
            assert torch.equal(a.reward.view(torch.int32), o.reward.view(torch.int32)) and torch.equal(a.done, o.done), "%s: reward / done" % where
        ra, sa = rng_words(a, sample), a.save_state()
        for name, o in (("NO_TAIL_ENCODE", b), ("separate calls", c)):
            so = o.save_state()
            assert torch.equal(sa, so), "step %d, tail encode vs %s: state records (RNG streams, tables, dist cache) differ at envs %s" % (
                t, name, torch.nonzero((sa != so).any(1)).flatten()[:8].tolist())
            ro = rng_words(o, sample)
            assert ra == ro, "step %d, tail encode vs %s: RNG words differ at envs %s" % (t, name, [e for e, x, y in zip(sample, ra, ro) if x != y][:8])
    for e in (a, b, c):
        e.check_errors()
        e.close()


def check_cadence(n):
    """One handle: fused step, plain rg_step, fused step, rg_obs_gray into ANOTHER tensor, fused step, rg_reset, fused step, reset_envs of a few ids, fused step --
    the oracle's image after every observation call."""
    env = make(n, 9, True)
    ob = OracleBatch(configs(n), max_steps=9, n_threads=threads())
    exp = np.empty((n, 1, ob.h, ob.w), np.float32)
    other = torch.full((n, 1, ob.h, ob.w), -1.0, dtype=torch.float32, device=env.device)
    rng = np.random.RandomState(31)
    t = [0]

    def keys_now():
        t[0] += 1
        return draw_keys(rng, n, t[0])

    def fused(why):
        keys = keys_now()
        env.step_keys(dev(env, keys))
        ob.step(keys, exp)
        against_oracle(env, ob, exp, None, "round %d, fused step %s" % (rnd, why))

    def oracle_image():
        for i in range(n):
            exp[i] = ob.env(i).gray_image().reshape(1, ob.h, ob.w)

    for rnd in range(6):
        fused("first")
        keys = keys_now()
        kd = dev(env, keys)
        env._h.check(env._h.L.rg_step(env._h.h, C.c_void_p(kd.data_ptr()), 1))  # no observation: its Redraws stay pending
        ob.step(keys, None)
        fused("after a plain rg_step")
        env._h.check(env._h.L.rg_obs_gray(env._h.h, 0, 0, C.c_void_p(other.data_ptr())))
        assert torch.equal(other, env.obs), "round %d: rg_obs_gray into another tensor" % rnd
        fused("after rg_obs_gray")
        env.reset()
        for i in range(n):
            ob.env(i).reset()
        oracle_image()
        against_oracle(env, ob, exp, None, "round %d, rg_reset" % rnd)
        fused("after rg_reset")
        ids = sorted(int(i) for i in rng.permutation(n)[:max(3, n // 16)])
        env.reset_envs(env_ids=ids)
        for i in ids:
            ob.env(i).reset()
        oracle_image()
        against_oracle(env, ob, exp, None, "round %d, reset_envs" % rnd)
        fused("after reset_envs")
    env.check_errors()
    env.close()


def check_nokey(n):
    """Keys that do not play: an invalid key byte for three envs.  Every env's image still matches the twin stepped with separate calls; the three keep the screen
    they had; every other env matches the oracle, which plays that step for them alone; and the error is reported as before."""
    a, c = make(n, 1000, True), make(n, 1000, True)
    ob = OracleBatch(configs(n), max_steps=1000, n_threads=threads())
    rng = np.random.RandomState(41)
    for t in range(1, 13):
        keys = draw_keys(rng, n, t)
        a.step_keys(dev(a, keys))
        kc = dev(c, keys)
        c._h.check(c._h.L.rg_step(c._h.h, C.c_void_p(kc.data_ptr()), 1))
        c._encode()
        ob.step(keys, None)
    a.check_errors()
    keys = draw_keys(rng, n, 13)
    bad = [1, n // 2, n - 1]
    keys[bad] = ord("~")
    before = a.obs.clone()
    a.obs.fill_(-1.0)  # (so that an env nobody serves shows)
    a.step_keys(dev(a, keys))
    kc = dev(c, keys)
    c._h.check(c._h.L.rg_step(c._h.h, C.c_void_p(kc.data_ptr()), 1))
    c._encode()
    assert torch.equal(a.obs.view(torch.int32), c.obs.view(torch.int32)), "observation differs at envs %s" % bad_envs(a.obs.cpu().numpy(), c.obs.cpu().numpy())
    assert torch.equal(a.obs[bad], before[bad]), "an env with an invalid key keeps its screen"
    good = [i for i in range(n) if i not in bad]
    exp = np.empty((len(good), 1, ob.h, ob.w), np.float32)
    for j, i in enumerate(good):
        env_i = ob.env(i)
        env_i.step_autoreset(int(keys[i]))
        exp[j] = env_i.gray_image().reshape(1, ob.h, ob.w)
    got = a.obs[good].cpu().numpy()
    assert np.array_equal(got, exp), "the oracle's image differs at envs %s" % [good[j] for j in bad_envs(got, exp)]
    for x, y in zip(a._h.fetch(), c._h.fetch()):
        assert np.array_equal(x, y)
    for e in (a, c):
        try:
            e.check_errors()
        except RuntimeError as ex:
            assert "Invalid input" in str(ex), ex
        else:
            raise AssertionError("the invalid key was not reported")
        e.close()


class _Plain:
    """A handle the vector env never makes -- auto_reset off -- with the tensors the checks read: what HipVecRogueEnv sets up around its _Handle."""

    def __init__(self, n, max_steps, tail):
        from rogue_gym_python import _rogue_gym as inner

        if not tail:
            os.environ["ROGUE_GYM_HIP_NO_TAIL_ENCODE"] = "1"
        try:
            self.h = inner._Handle([json.dumps(c) for c in configs(n)], max_steps, auto_reset=False)
        finally:
            os.environ.pop("ROGUE_GYM_HIP_NO_TAIL_ENCODE", None)
        self.dev = torch.device("cuda", self.h.device)
        with torch.cuda.device(self.dev):
            self.h.check(self.h.L.rg_set_stream(self.h.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.obs = torch.full((n, 1, self.h.height, self.h.width), -1.0, dtype=torch.float32, device=self.dev)

    def keys(self, keys):
        return torch.as_tensor(np.ascontiguousarray(keys, np.uint8), device=self.dev)

    def fused(self, keys):
        k = self.keys(keys)
        self.h.check(self.h.L.rg_step_obs_gray(self.h.h, C.c_void_p(k.data_ptr()), 1, 0, 0, C.c_void_p(self.obs.data_ptr())))

    def separate(self, keys):
        k = self.keys(keys)
        self.h.check(self.h.L.rg_step(self.h.h, C.c_void_p(k.data_ptr()), 1))
        self.h.check(self.h.L.rg_obs_gray(self.h.h, 0, 0, C.c_void_p(self.obs.data_ptr())))

    def state(self):
        """(rg_sync's report, image, screen, hist, status, flags).  Without auto_reset an env whose player died stays dead, and rg_sync reports each key it is
        sent as an ignored input: that report is part of what must be equal."""
        rc = self.h.L.rg_sync(self.h.h)
        msg = self.h.L.rg_last_error(self.h.h).decode() if rc else ""
        assert rc == 0 or "Ignored input" in msg, msg
        return (np.array([rc != 0]), self.obs.cpu().numpy()) + tuple(self.h.fetch())


def check_nolive(n):
    """Keys that do not play: envs past max_steps with auto_reset off (a handle made through _Handle; HipVecRogueEnv always resets).  From step max_steps + 2 on
    no env plays: step_wave leaves through `valid && !live`, stamps nothing, and the residual pass must write every image.  The fused call with the tail
    encode, with ROGUE_GYM_HIP_NO_TAIL_ENCODE=1 and as separate calls: the same images, mirrors, status and flag words at every step; and an env that no
    longer plays keeps the image of its last turn, although the tensor is overwritten before every call."""
    max_steps = 5
    a, b, c = _Plain(n, max_steps, True), _Plain(n, max_steps, False), _Plain(n, max_steps, True)
    rng = np.random.RandomState(51)
    last = None
    for t in range(1, max_steps + 6):
        keys = draw_keys(rng, n, t)
        for p in (a, b, c):
            p.obs.fill_(-1.0)  # (so that an env nobody serves shows)
        a.fused(keys)
        b.fused(keys)
        c.separate(keys)
        sa = a.state()
        for name, o in (("NO_TAIL_ENCODE", b), ("separate calls", c)):
            for what, x, y in zip(("rg_sync's error report", "observation", "screen mirror", "history mirror", "status", "flag words"), sa, o.state()):
                assert np.array_equal(x, y), "step %d, tail encode vs %s: %s differs at envs %s" % (t, name, what, bad_envs(x, y))
        img = sa[1]
        assert (img >= 0).all(), "step %d: envs %s were not served" % (t, bad_envs(img, np.maximum(img, 0)))
        if t > max_steps + 1:  # (steps > max_steps: state_impls.rs:52-54 -- the key is not played)
            assert np.array_equal(img, last), "step %d: an env past max_steps changed its image at envs %s" % (t, bad_envs(img, last))
        last = img
    for p in (a, b, c):
        p.h.close()


if __name__ == "__main__":
    {"oracle": check_oracle, "twins": check_twins, "cadence": check_cadence, "nokey": check_nokey, "nolive": check_nolive}[sys.argv[1]](int(sys.argv[2]))
    print("OK")
