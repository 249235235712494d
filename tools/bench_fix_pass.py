"""The fix-up pass of the pre-streamed gray encode (rg_step_obs_gray on the mini config: k_obs_fix, or k_obs_resid in a build that launches it) through
rg_timing's kernel 2, HIP-event pairs around every launch, for one or more batch sizes:

  play   random keys on a HipVecRogueEnv (max_steps = 1000): the pass with the lines and Redraws of ordinary play, and the step launch (kernel 0) beside it
  floor  a handle without auto_reset whose envs are all past max_steps: no env plays, every line mask is 0 and no Redraw is pending, so the pass is its
         dispatch, one round trip for the flag words and masks, and the drain -- what is left of it when there is nothing to fix

Usage: python tools/bench_fix_pass.py [--steps K] [n_envs ...]        (ROGUE_GYM_HIP_LIB selects the build, as everywhere)
One JSON line per batch size.  Event pairs cost a few microseconds of stream time: compare builds with each other, not with a kernel trace."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rogue-gym_amd"))
import numpy as np
import torch

from rogue_gym.envs.device import HipVecRogueEnv
from rogue_gym_python import _rogue_gym as inner

KEYS = np.frombuffer(b".hjklnbuy>s", np.uint8)


def timed(h, step, steps):
    """avg us of kernels 0 and 2 over `steps` calls of step(t), and their launch counts"""
    h.check(h.L.rg_timing_enable(h.h, 1))
    for t in range(steps):
        step(t)
    ms, launches = (C.c_double * 4)(), (C.c_uint64 * 4)()
    h.check(h.L.rg_timing_read(h.h, ms, launches))
    h.check(h.L.rg_timing_enable(h.h, 0))
    return [round(1e3 * ms[k] / max(1, launches[k]), 2) for k in (0, 2)], [int(launches[k]) for k in (0, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("envs", type=int, nargs="*", default=[65536])
    args = ap.parse_args()
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")))["configs"]["mini"]
    for n in args.envs:
        cfgs = [json.dumps(dict(cfg, seed=i)) for i in range(n)]
        rng = np.random.RandomState(0)
        env = HipVecRogueEnv(cfgs, max_steps=1000)
        keys = [torch.as_tensor(KEYS[rng.randint(0, len(KEYS), n)].copy(), device=env.device) for _ in range(16)]
        for t in range(200):
            env.step_keys(keys[t % 16])
        play, launches = timed(env._h, lambda t: env.step_keys(keys[t % 16]), args.steps)
        env.check_errors()
        env.close()
        # no auto_reset, max_steps = 1: from the third step on no env plays (its key is reported as ignored, which rg_sync would say: it is not asked)
        h = inner._Handle(cfgs, 1, auto_reset=False)
        dev = torch.device("cuda", h.device)
        with torch.cuda.device(dev):
            h.check(h.L.rg_set_stream(h.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        obs = torch.zeros((n, 1, h.height, h.width), dtype=torch.float32, device=dev)
        k = torch.as_tensor(KEYS[rng.randint(0, len(KEYS), n)].copy(), device=dev)

        def idle(t):
            h.check(h.L.rg_step_obs_gray(h.h, C.c_void_p(k.data_ptr()), 1, 0, 0, C.c_void_p(obs.data_ptr())))

        for t in range(50):
            idle(t)
        floor, _ = timed(h, idle, args.steps)
        torch.cuda.synchronize()
        h.close()
        print(json.dumps({"envs": n, "steps": args.steps, "launches": launches, "play_step_us": play[0], "play_fix_us": play[1], "floor_step_us": floor[0],
                          "floor_fix_us": floor[1], "lib": os.environ.get("ROGUE_GYM_HIP_LIB", "product")}), flush=True)


if __name__ == "__main__":
    main()
