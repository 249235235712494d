"""Step + typed player-centred crop (rg_obs_crop_typed) against step + f32 crop (rg_obs_crop): the instances of k_crop_typed in
rogue-gym_amd/csrc/rg_crop_typed.hip, the f32 crop being its RG_OBS_F32 case.

Three workloads, each on ONE handle with the same seeds and the same uniform-random policy (a pre-generated table of 512 key rows, cycled): 65 536
mini envs gray, 32 768 default 80x24 envs gray, 32 768 nohide 80x24 envs one-hot symbol; the window is 11x11 everywhere.  Two kinds of rows, one JSON
line each:

  "rates":  env-steps/s of step + f32 crop (rg_step, rg_obs_crop), step + bf16 crop and step + id crop (rg_step_obs_crop_typed), and step +
            whole-screen ids (rg_step_obs_typed) for scale: --warmup untimed steps, then --steps timed steps between two device synchronisations, after
            a pre-roll of --preroll untimed steps that brings the batch into its steady-state episode mix.
  "passes": the crop pass's own time from HIP events on the stream, on the state the rates left behind (nothing pending: the pass only reads the
            mirrors): every typed instance next to its yardstick, the f32 pass of the same window and image setting on the same handle.  --repeats
            rounds; in each round every variant in turn runs --inner calls (the variants alternate, so drift hits all
            alike), each call between its own pair of events; a round's figure is the median of its calls.  Per variant: the median over the rounds and the
            spread (min, max) in microseconds per call, and the bytes it writes (from the shapes).

    python tools/bench_crop_typed.py [--steps 1000] [--warmup 100] [--preroll 500] [--repeats 7] [--inner 50] [--only mini|default|nohide-symbol]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rogue-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

F32, F16, BF16, U8 = 0, 1, 2, 3
TORCH_OF = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16, U8: torch.uint8}
WORKLOADS = (  # name, golden config, envs, one-hot
    ("mini", "mini", 65536, False),
    ("default", "default", 32768, False),
    ("nohide-symbol", "nohide", 32768, True),
)
R = 5  # 11x11


def case(name, cfg, n, sym, a):
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    env = HipVecRogueEnv([dict(cfg, seed=i) for i in range(n)], max_steps=1000,
                         image_setting=ImageSetting(DungeonType.SYMBOL if sym else DungeonType.GRAY, StatusFlag.EMPTY, False))
    dev, L, h = env.device, env._h.L, env._h.h
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    side = 2 * R + 1
    centers = torch.empty((n, 2), dtype=torch.int32, device=dev)
    bufs = {}

    def buf(kind, dt):
        if (kind, dt) not in bufs:
            c = 1 if kind == 2 else L.rg_obs_channels(h, kind, 0, 0)
            bufs[(kind, dt)] = torch.empty((n, c, side, side), dtype=TORCH_OF[dt], device=dev)
        return bufs[(kind, dt)]

    ids_full = torch.empty((n, 1, env.height, env.width), dtype=torch.uint8, device=dev)
    t = [0]

    def keys():
        k = table[t[0] % 512]
        t[0] += 1
        return C.c_void_p(k.data_ptr())

    def full_step():
        env.step_keys(table[t[0] % 512])
        t[0] += 1

    def f32_crop_step():
        env._h.check(L.rg_step(h, keys(), 1))
        env._h.check(L.rg_obs_crop(h, int(sym), R, R, 0, 0, C.c_void_p(buf(int(sym), F32).data_ptr()), C.c_void_p(centers.data_ptr())))

    def bf16_crop_step():
        env._h.check(L.rg_step_obs_crop_typed(h, keys(), 1, int(sym), BF16, R, R, 0, 0, C.c_void_p(buf(int(sym), BF16).data_ptr()), C.c_void_p(centers.data_ptr())))

    def id_crop_step():
        env._h.check(L.rg_step_obs_crop_typed(h, keys(), 1, 2, U8, R, R, 0, 0, C.c_void_p(buf(2, U8).data_ptr()), C.c_void_p(centers.data_ptr())))

    def ids_full_step():
        env._h.check(L.rg_step_obs_typed(h, keys(), 1, 2, U8, 0, 0, C.c_void_p(ids_full.data_ptr())))

    for _ in range(a.preroll):
        full_step()
    rates = {}
    for mode, fn in (("f32_crop", f32_crop_step), ("bf16_crop", bf16_crop_step), ("id_crop", id_crop_step), ("ids_whole_screen", ids_full_step)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        rates[mode] = round(n * a.steps / (time.perf_counter() - t0) / 1e6, 2)
    L.rg_sync(h)  # (drains the tile-error word: 'Z' is a monster of these configs and not a symbol, as in the reference)
    print(json.dumps(dict(row="rates", workload=name, n_env=n, obs="symbol" if sym else "gray", crop="%dx%d" % (side, side), steps=a.steps, unit="M env-steps/s",
                          bytes_per_launch={"f32_crop": buf(int(sym), F32).numel() * 4, "bf16_crop": buf(int(sym), BF16).numel() * 2, "id_crop": buf(2, U8).numel(),
                                            "ids_whole_screen": ids_full.numel()}, **rates)), flush=True)

    # ---- the passes alone: each typed instance and its f32 yardstick (same window, same image setting, same handle), alternating ----
    def crop_pass(kind, dt):
        out = C.c_void_p(buf(kind, dt).data_ptr())
        if dt == F32:
            return lambda: L.rg_obs_crop(h, kind, R, R, 0, 0, out, C.c_void_p(centers.data_ptr()))
        return lambda: L.rg_obs_crop_typed(h, kind, dt, R, R, 0, 0, out, C.c_void_p(centers.data_ptr()))

    variants = [("gray_f32", 0, F32), ("gray_f16", 0, F16), ("gray_bf16", 0, BF16), ("onehot_f32", 1, F32), ("onehot_f16", 1, F16), ("onehot_bf16", 1, BF16), ("ids_u8", 2, U8)]
    calls = {v: crop_pass(kind, dt) for v, kind, dt in variants}
    env._h.check(L.rg_obs_crop(h, 0, R, R, 0, 0, C.c_void_p(buf(0, F32).data_ptr()), C.c_void_p(centers.data_ptr())))  # (draws what the last step left pending)
    for fn in calls.values():
        for _ in range(a.inner):
            env._h.check(fn())
    us = {v: [] for v, _, _ in variants}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.inner)]
    for _ in range(a.repeats):
        for v, _, _ in variants:
            fn = calls[v]
            torch.cuda.synchronize()
            for e0, e1 in ev:  # one event pair per call: the pass's own time, not the host's launch rate (the id pass is shorter than a launch)
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            us[v].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
    L.rg_sync(h)
    passes = {v: dict(median_us=round(statistics.median(us[v]), 2), min_us=round(min(us[v]), 2), max_us=round(max(us[v]), 2),
                      bytes=buf(kind, dt).numel() * buf(kind, dt).element_size()) for v, kind, dt in variants}
    print(json.dumps(dict(row="passes", workload=name, n_env=n, crop="%dx%d" % (side, side), repeats=a.repeats, calls_per_repeat=a.inner, unit="us per call (HIP events)",
                          yardstick={"gray_f16": "gray_f32", "gray_bf16": "gray_f32", "onehot_f16": "onehot_f32", "onehot_bf16": "onehot_f32", "ids_u8": "onehot_f32"},
                          **passes)), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--preroll", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
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
