"""Child process of tests/test_gpu_step_enc.py: one batch size per process; the parent chooses the library and the development knobs through the environment.

usage: step_enc_child.py MODE N        MODE = twin | oracle | narrow

Every mode plays the mini config (32 x 16 cells) with per-env seeds = env index, max_steps = 30 -- every env times out three times in 120 steps, so resets,
spare takes and the urgent refill of an env's last spare all occur -- and one key of the 11-action table per env and step, drawn with a fixed numpy seed; an
env whose player stands on the stairs (read from the oracle before the step) gets '>', so that stair blocks run and descend.  HipVecRogueEnv.step_keys is the
call under test: on this config it arms the pre-streamed encode (rg_step_obs_gray), whose step launch is k_step_enc's (rg_step_enc.hip).

After EVERY step, handle A against an OracleBatch: the observation tensor bit for bit, reward, done, the ten status words, the terminal / dead / message bits
and the screen and history mirrors of every env.

twin (the development library): handle B beside it, made with ROGUE_GYM_HIP_STEP_GENERIC=1 -- the same launch under the generic k_step_w32<false, true> -- must
equal A after every step in the observation, the whole flag words, reward, done, both mirrors, status and the saved state records of every env
(rg_state_save: equal states give equal bytes; a record holds the RNG streams beside the grids, tables and dist cache).
oracle: A alone (any library).
narrow: what the dispatch keeps on the generic instance.  A grid of 16 columns and 32 rows has 512 cells too, but no handle can have one -- the config is refused,
as the reference refuses it (screen width below 32), which this mode asserts -- so the launch that pre-streams and is NOT k_step_enc's is the one of a handle
without next-level structures (ROGUE_GYM_HIP_NO_NEXT_LEVELS=1: S.nx_state is NULL, an array the kernel takes for granted -- rgk_step_enc_takes); it must match
the oracle as well."""
import os
import sys

import numpy as np

from tail_encode_child import against_oracle, bad_envs, configs, dev, mini, threads  # noqa: E402  (also puts the package on sys.path)

import torch  # noqa: E402

from oracle.pyoracle import OracleBatch  # noqa: E402
from parity_util import ACTION_KEYS  # noqa: E402
from rogue_gym.envs.device import HipVecRogueEnv  # noqa: E402

MAX_STEPS, STEPS = 30, 120
S_STAIR = 4   # Surface::Stair as the oracle's grid reports it (tests/parity_util.py compare_internal: the low three bits of a tile word)


def make(n, generic=False, **env):
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    if generic:
        os.environ["ROGUE_GYM_HIP_STEP_GENERIC"] = "1"   # read when the handle is made, by the development library alone
    try:
        return HipVecRogueEnv(configs(n), max_steps=MAX_STEPS)
    finally:
        os.environ.pop("ROGUE_GYM_HIP_STEP_GENERIC", None)
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def on_stairs(ob, n):
    out = np.zeros(n, bool)
    for i in range(n):
        o = ob.env(i)
        sc = o.scalars()
        out[i] = o.grid()[0][sc["py"], sc["px"]] == S_STAIR
    return out


def play(n, a, b):
    ob = OracleBatch(configs(n), max_steps=MAX_STEPS, n_threads=threads())
    exp = np.empty((n, 1, ob.h, ob.w), np.float32)
    rng = np.random.RandomState(131)
    st_prev = ob.fetch(screen=False, hist=False)[2]
    resets = descents = forced = 0
    for t in range(1, STEPS + 1):
        keys = ACTION_KEYS[rng.randint(0, len(ACTION_KEYS), n)].copy()
        stairs = on_stairs(ob, n)
        keys[stairs] = ord(">")
        forced += int(stairs.sum())
        a.obs.fill_(-1.0)   # (so that an env nobody serves shows)
        a.step_keys(dev(a, keys))
        ob.step(keys, exp)
        st, term = against_oracle(a, ob, exp, st_prev, "step %d, k_step_enc vs the oracle" % t)
        resets += int(term.sum())
        descents += int(((st[:, 0] > st_prev[:, 0]) & ~term).sum())
        st_prev = st
        if b is None:
            continue
        b.step_keys(dev(b, keys))
        torch.cuda.synchronize()
        where = "step %d, k_step_enc vs the generic instance" % t
        assert torch.equal(a.obs.view(torch.int32), b.obs.view(torch.int32)), "%s: observation differs at envs %s" % (where, bad_envs(a.obs.cpu().numpy(), b.obs.cpu().numpy()))
        assert torch.equal(a.flags, b.flags), "%s: flag words differ at envs %s" % (where, bad_envs(a.flags.cpu().numpy(), b.flags.cpu().numpy()))
        assert torch.equal(a.reward.view(torch.int32), b.reward.view(torch.int32)) and torch.equal(a.done, b.done), "%s: reward / done" % where
        for what, x, y in zip(("screen mirror", "history mirror", "status", "flag words"), a._h.fetch(), b._h.fetch()):
            assert np.array_equal(x, y), "%s: %s differs at envs %s" % (where, what, bad_envs(x, y))
        sa, sb = a.save_state(), b.save_state()
        assert torch.equal(sa, sb), "%s: state records differ at envs %s" % (where, torch.nonzero((sa != sb).any(1)).flatten()[:8].tolist())
    for e in (a, b):
        if e is not None:
            e.check_errors()
    c = a.counters()
    print("%d envs: %d resets and %d descents on the oracle's side, %d keys forced to '>'; device counters %s" % (n, resets, descents, forced, c))
    # what keeps the run from going hollow: every env times out at steps 31, 62 and 93 at the latest (the oracle's count), and the device took spares for them
    assert resets >= 3 * n, (resets, n)
    assert c["resets"] >= 3 * n and c["spares_taken"] > 0, c
    if n >= 65:
        assert descents > 0 and forced > 0 and c["descents"] > 0, (descents, forced, c)
    for e in (a, b):
        if e is not None:
            e.close()


def main(mode, n):
    if mode == "twin":
        play(n, make(n), make(n, generic=True))
    elif mode == "oracle":
        play(n, make(n), None)
    else:
        try:
            HipVecRogueEnv([dict(mini(), width=16, height=32, seed=0)], max_steps=MAX_STEPS)
        except Exception as ex:  # noqa: BLE001
            assert "too narrow" in str(ex), ex
        else:
            raise AssertionError("a 16 x 32 grid was accepted: play it here, it must take the generic instance")
        play(n, make(n, ROGUE_GYM_HIP_NO_NEXT_LEVELS="1"), None)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
    print("OK")
