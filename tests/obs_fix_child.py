"""Child process of tests/test_gpu_obs_fix.py: what the groups of the group-wise fix-up pass (rg_obs_fix.hip k_obs_fix) held during a run, counted from a twin on
the two-pass path, beside the comparison tests/prestream_child.py makes.

usage: obs_fix_child.py N GROUP

Handle A takes HipVecRogueEnv.step_keys (the pre-streamed encode: helper blocks, then k_obs_fix); its twin B is made with ROGUE_GYM_HIP_NO_TAIL_ENCODE=1 and
gets the same keys as rg_step, then rg_obs_gray, so that its flag words can be read between the two: that is where a pending Redraw shows.  A's tensor is
overwritten with -1 before every step.  After every step images, flag words, reward and done must be equal.

Per step and group of GROUP consecutive envs, from B alone: the envs with a pending Redraw, and the envs whose screen mirror changed without one (their
masks are not zero: the turn wrote mirror bytes).  The run must hold a step in which a full group had a Redraw pending in every env -- the Redraw loop from
its first env to its last, each draw with the next env's tiles in flight -- and a step in which a group held a Redraw beside envs with masked lines.  With
max_steps = 9 every env is reset at the same step, which gives the first; ordinary play gives the second."""
import ctypes as C
import sys

import numpy as np

from tail_encode_child import bad_envs, dev, draw_keys, make  # noqa: E402  (also puts the package on sys.path)

import torch  # noqa: E402

RG_FLAG_REDRAW = 0x4
STEPS = 40


def main(n, group):
    a, b = make(n, 9, True), make(n, 9, False)
    rng = np.random.RandomState(71)
    prev = b._h.fetch()[0]
    pad = (-n) % group
    full_groups = n // group
    all_redraw = mixed = 0
    most = 0
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
        assert torch.equal(a.reward.view(torch.int32), b.reward.view(torch.int32)) and torch.equal(a.done, b.done), "%s: reward / done" % where
        scr = b._h.fetch()[0]
        masked = ~redraw & (scr != prev).reshape(n, -1).any(1)
        prev = scr
        r = np.pad(redraw, (0, pad)).reshape(-1, group).sum(1)
        m = np.pad(masked, (0, pad)).reshape(-1, group).sum(1)
        most = max(most, int(r.max()))
        all_redraw += int((r[:full_groups] == group).sum())
        mixed += int(((r > 0) & (m > 0)).sum())
    sa, sb = a._h.fetch(), b._h.fetch()
    for what, x, y in zip(("screen mirror", "history mirror", "status", "flag words"), sa, sb):
        assert np.array_equal(x, y), "after the run: %s differs at envs %s" % (what, bad_envs(x, y))
    for e in (a, b):
        e.check_errors()
        e.close()
    print("groups of %d: %d (group, step) with every env a Redraw, %d with a Redraw beside masked envs, at most %d Redraws in a group" % (group, all_redraw, mixed, most))
    assert all_redraw > 0 and mixed > 0, (all_redraw, mixed, most)


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]))
    print("OK")
