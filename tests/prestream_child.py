"""Child process of tests/test_gpu_prestream.py: one batch size per process, because the envs per step wave (ROGUE_GYM_HIP_EPW) are read once, when the
library first launches a step; the parent also chooses the library and the development knobs (helper count, helper start delay) through the environment.

usage: prestream_child.py N

Handle A takes HipVecRogueEnv.step_keys, which on the mini config arms the pre-streamed encode (rg_step_obs_gray: helper blocks of the step launch stream
every image from the mirror as they find it, k_obs_resid fixes up the lines the turns touched).  Its twin B is made with ROGUE_GYM_HIP_NO_TAIL_ENCODE=1 --
the two-pass path -- and gets the same keys as rg_step, then rg_obs_gray, so that its flag words can be read between the two: that is where a pending Redraw
shows.  After every step the images, the whole flag words, reward and done must be equal.  A's tensor is overwritten with -1 before every step, so that an
env nobody serves shows.

The run must exercise the three classes the design tells apart, counted per (env, step) from B alone: flagged Redraw (drawn from the tiles by the pass),
changed without a Redraw flag (the turn wrote mirror bytes itself: the masked lines are re-encoded), unchanged (the helper's image stands)."""
import ctypes as C
import sys

import numpy as np

from tail_encode_child import bad_envs, dev, draw_keys, make  # noqa: E402  (also puts the package on sys.path)

import torch  # noqa: E402

RG_FLAG_REDRAW = 0x4
STEPS = 60


def main(n):
    a, b = make(n, 9, True), make(n, 9, False)
    rng = np.random.RandomState(61)
    prev = b._h.fetch()[0]
    unchanged = changed = flagged = 0
    for t in range(1, STEPS + 1):
        keys = draw_keys(rng, n, t)
        a.obs.fill_(-1.0)
        a.step_keys(dev(a, keys))
        kb = dev(b, keys)
        b._h.check(b._h.L.rg_step(b._h.h, C.c_void_p(kb.data_ptr()), 1))
        redraw = ((b.flags.clone().cpu().numpy().astype(np.uint32) & RG_FLAG_REDRAW) != 0)
        b._encode()
        torch.cuda.synchronize()
        where = "step %d" % t
        assert torch.equal(a.obs.view(torch.int32), b.obs.view(torch.int32)), "%s: observation differs at envs %s" % (where, bad_envs(a.obs.cpu().numpy(), b.obs.cpu().numpy()))
        assert torch.equal(a.flags, b.flags), "%s: flag words differ at envs %s" % (where, bad_envs(a.flags.cpu().numpy(), b.flags.cpu().numpy()))
        assert torch.equal(a.reward.view(torch.int32), b.reward.view(torch.int32)), "%s: reward differs at envs %s" % (where, bad_envs(a.reward.cpu().numpy(), b.reward.cpu().numpy()))
        assert torch.equal(a.done, b.done), "%s: done differs at envs %s" % (where, bad_envs(a.done.cpu().numpy(), b.done.cpu().numpy()))
        scr = b._h.fetch()[0]
        moved = (scr != prev).reshape(n, -1).any(1)
        flagged += int(redraw.sum())
        changed += int((~redraw & moved).sum())
        unchanged += int((~redraw & ~moved).sum())
        prev = scr
    sa, sb = a._h.fetch(), b._h.fetch()
    for what, x, y in zip(("screen mirror", "history mirror", "status", "flag words"), sa, sb):
        assert np.array_equal(x, y), "after the run: %s differs at envs %s" % (what, bad_envs(x, y))
    for e in (a, b):
        e.check_errors()
        e.close()
    print("classes: %d unchanged, %d changed without a Redraw flag, %d flagged Redraw" % (unchanged, changed, flagged))
    assert unchanged > 0 and changed > 0 and flagged > 0, (unchanged, changed, flagged)


if __name__ == "__main__":
    main(int(sys.argv[1]))
    print("OK")
