"""Step + full image against step + player-centred crop (rg_obs_crop, rogue-gym_amd/csrc/rg_crop_typed.hip k_crop_typed with RG_OBS_F32 elements).

Three workloads, each on ONE handle with the same seeds and the same uniform-random policy (a pre-generated table of 512 key rows, cycled):
65 536 mini envs gray with a 9x9 crop, 32 768 default 80x24 envs gray with an 11x11 crop, 32 768 nohide 80x24 envs one-hot symbol with an 11x11
crop.  Per mode: --warmup untimed steps, then --steps timed steps between two device synchronisations; the pre-roll (--preroll untimed steps) brings
the batch into its steady-state episode mix first.  The full-image mode is what HipVecRogueEnv.step_keys does without a crop (rg_step_obs_gray for
gray, rg_step + rg_obs_symbol for one-hot); the crop mode is rg_step + rg_obs_crop.  One JSON line per workload, with the bytes each observation
pass writes per launch (from the shapes).  Kernel times come from a separate profiler run, e.g.

    python tools/bench_crop.py [--steps 1000] [--warmup 100] [--preroll 500] [--only mini|default|nohide-symbol]
    rocprofv3 --kernel-trace --stats -d prof -- python tools/bench_crop.py --steps 200 --warmup 20 --preroll 100
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rogue-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WORKLOADS = (  # name, golden config, envs, one-hot, crop radius
    ("mini", "mini", 65536, False, 4),
    ("default", "default", 32768, False, 5),
    ("nohide-symbol", "nohide", 32768, True, 5),
)


def case(name, cfg, n, sym, r, a):
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    env = HipVecRogueEnv([dict(cfg, seed=i) for i in range(n)], max_steps=1000,
                         image_setting=ImageSetting(DungeonType.SYMBOL if sym else DungeonType.GRAY, StatusFlag.EMPTY, False))
    dev, L, h = env.device, env._h.L, env._h.h
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    crop = torch.empty((n, env.channels, 2 * r + 1, 2 * r + 1), dtype=torch.float32, device=dev)
    centers = torch.empty((n, 2), dtype=torch.int32, device=dev)
    t = [0]

    def full_step():
        env.step_keys(table[t[0] % 512])
        t[0] += 1

    def crop_step():
        env._h.check(L.rg_step(h, C.c_void_p(table[t[0] % 512].data_ptr()), 1))
        env._h.check(L.rg_obs_crop(h, int(sym), r, r, 0, 0, C.c_void_p(crop.data_ptr()), C.c_void_p(centers.data_ptr())))
        t[0] += 1

    for _ in range(a.preroll):
        full_step()
    rates = {}
    for mode, fn in (("full", full_step), ("crop", crop_step)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        rates[mode] = n * a.steps / (time.perf_counter() - t0)
    if sym:
        L.rg_sync(h)  # (drains the tile-error word: 'Z' is a monster of these configs and not a symbol, as in the reference)
    else:
        env.check_errors()
    row = dict(workload=name, n_env=n, obs="symbol" if sym else "gray", crop="%dx%d" % (2 * r + 1, 2 * r + 1), steps=a.steps,
               full_env_steps_per_s=round(rates["full"] / 1e6, 2), crop_env_steps_per_s=round(rates["crop"] / 1e6, 2),
               crop_vs_full=round(rates["crop"] / rates["full"], 2), full_obs_bytes_per_launch=env.obs.numel() * 4,
               crop_bytes_per_launch=crop.numel() * 4 + centers.numel() * 4, unit="M env-steps/s")
    print(json.dumps(row), flush=True)
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--preroll", type=int, default=500)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        cfgs = json.load(f)["configs"]
    for name, cfg_name, n, sym, r in WORKLOADS:
        if a.only and a.only != name:
            continue
        case(name, cfgs[cfg_name], n, sym, r, a)


if __name__ == "__main__":
    main()
