"""Step + observation by element type (rg_step_obs_typed, rogue-gym_amd/csrc/rg_obs.hip k_obs_typed) against step + f32 observation.

The three workloads of tools/bench_crop.py, each on ONE handle with the same seeds and the same uniform-random policy (a pre-generated table of 512
key rows, cycled): 65 536 mini envs gray, 32 768 default 80x24 envs gray, 32 768 nohide 80x24 envs one-hot symbol.  Modes: f32 (what
HipVecRogueEnv.step_keys does: rg_step_obs_gray for gray, rg_step + rg_obs_symbol for one-hot), f16 and bf16 (rg_step_obs_typed), f32 followed by
obs.to(torch.bfloat16) (what a learner does today); on the one-hot workload also the u8 symbol ids, and the gray f32 image of the same handle (the
ids' ceiling: the same screen, four bytes a cell).  Per mode: --warmup untimed steps, then --steps timed steps between two device synchronisations;
the pre-roll (--preroll untimed steps) brings the batch into its steady-state episode mix first.  One JSON line per workload, with the bytes each
observation pass writes per launch (from the shapes).  Kernel times come from a separate profiler run, e.g.

    python tools/bench_obs_dtype.py [--steps 1000] [--warmup 100] [--preroll 500] [--only mini|default|nohide-symbol]
    rocprofv3 --kernel-trace --stats -d prof -- python tools/bench_obs_dtype.py --steps 200 --warmup 20 --preroll 100 --only nohide-symbol
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

WORKLOADS = (  # name, golden config, envs, one-hot
    ("mini", "mini", 65536, False),
    ("default", "default", 32768, False),
    ("nohide-symbol", "nohide", 32768, True),
)
F16, BF16, U8 = 1, 2, 3  # RG_OBS_*


def case(name, cfg, n, sym, a):
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    env = HipVecRogueEnv([dict(cfg, seed=i) for i in range(n)], max_steps=1000,
                         image_setting=ImageSetting(DungeonType.SYMBOL if sym else DungeonType.GRAY, StatusFlag.EMPTY, False))
    dev, L, h = env.device, env._h.L, env._h.h
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    shape = tuple(env.obs.shape)
    out = {F16: torch.empty(shape, dtype=torch.float16, device=dev), BF16: torch.empty(shape, dtype=torch.bfloat16, device=dev)}
    ids = torch.empty((n, 1) + shape[2:], dtype=torch.uint8, device=dev)
    gray = torch.empty((n, 1) + shape[2:], dtype=torch.float32, device=dev)
    t = [0]

    def keys():
        k = table[t[0] % 512]
        t[0] += 1
        return C.c_void_p(k.data_ptr())

    def f32_step():
        env.step_keys(table[t[0] % 512])
        t[0] += 1

    def typed_step(kind, dt, buf):
        def fn():
            env._h.check(L.rg_step_obs_typed(h, keys(), 1, kind, dt, 0, 0, C.c_void_p(buf.data_ptr())))
        return fn

    def f32_to_step():
        f32_step()
        env.obs.to(torch.bfloat16)

    def gray_step():
        env._h.check(L.rg_step_obs_gray(h, keys(), 1, 0, 0, C.c_void_p(gray.data_ptr())))

    modes = [("f32", f32_step, env.obs.numel() * 4), ("f16", typed_step(int(sym), F16, out[F16]), env.obs.numel() * 2),
             ("bf16", typed_step(int(sym), BF16, out[BF16]), env.obs.numel() * 2), ("f32_to_bf16", f32_to_step, env.obs.numel() * 6)]
    if sym:
        modes += [("ids", typed_step(2, U8, ids), ids.numel()), ("gray_f32", gray_step, gray.numel() * 4)]
    for _ in range(a.preroll):
        f32_step()
    rates = {}
    for mode, fn, _ in modes:
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
    row = dict(workload=name, n_env=n, obs="symbol" if sym else "gray", steps=a.steps, unit="M env-steps/s")
    for mode, _, nbytes in modes:
        row[mode + "_env_steps_per_s"] = round(rates[mode] / 1e6, 2)
        row[mode + "_bytes_per_launch"] = nbytes  # (f32_to_bf16: the f32 write, its read back and the bf16 write)
    row["bf16_vs_f32"] = round(rates["bf16"] / rates["f32"], 3)
    row["f16_vs_f32"] = round(rates["f16"] / rates["f32"], 3)
    row["bf16_vs_f32_to_bf16"] = round(rates["bf16"] / rates["f32_to_bf16"], 3)
    if sym:
        row["ids_vs_f32"] = round(rates["ids"] / rates["f32"], 2)
        row["ids_vs_gray_f32"] = round(rates["ids"] / rates["gray_f32"], 3)
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
    for name, cfg_name, n, sym in WORKLOADS:
        if a.only and a.only != name:
            continue
        case(name, cfgs[cfg_name], n, sym, a)


if __name__ == "__main__":
    main()
