"""Step + observation against step + observation + teacher keys (rg_path, rogue-gym_amd/csrc/rg_path.hip k_path).

Two workloads, each on ONE handle with the same seeds: 65 536 mini envs and 32 768 default 80x24 envs, f32 gray image.  Three kinds of rows, one JSON
line each:

  "rates":  env-steps/s of step + observation under the uniform-random policy (rg_step_obs_gray: the yardstick, the path without the pass), of step +
            observation + teacher keys (goal stairs, keys and distances only) under the same policy, and of the guided loop -- every env plays its
            teacher key: --warmup untimed steps, then --steps timed steps between two device synchronisations, after a pre-roll of --preroll untimed
            steps that brings the batch into its steady-state episode mix.
  "passes": the pass's own time from HIP events on the stream, on the state the rates left behind: keys only for goals stairs / gold / stairs + gold,
            and the field pass.  --repeats rounds; in each round every variant in turn runs --inner calls (the variants alternate, so drift hits all
            alike), each call between its own pair of events; a round's figure is the median of its calls.  Per variant: the median over the rounds
            and the spread (min, max) in microseconds per call, and the bytes it writes.
  "k_step": the same process's mean k_step time (rg_timing, every 8th launch bracketed) over --steps uniform-random steps: what the keys-only pass is
            to be read against.

    python tools/bench_path.py [--steps 1000] [--warmup 100] [--preroll 500] [--repeats 7] [--inner 50] [--only mini|default]
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

WORKLOADS = (("mini", "mini", 65536), ("default", "default", 32768))  # name, golden config, envs


def case(name, cfg, n, a):
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    env = HipVecRogueEnv([dict(cfg, seed=i) for i in range(n)], max_steps=1000, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False))
    dev, L, h = env.device, env._h.L, env._h.h
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    keys = torch.full((n,), ord("."), dtype=torch.uint8, device=dev)
    dist = torch.empty((n,), dtype=torch.int32, device=dev)
    field = torch.empty((n, env.height, env.width), dtype=torch.uint16, device=dev)
    obs = C.c_void_p(env.obs.data_ptr())
    pk, pd, pf = C.c_void_p(keys.data_ptr()), C.c_void_p(dist.data_ptr()), C.c_void_p(field.data_ptr())
    t = [0]

    def step():
        k = table[t[0] % 512]
        t[0] += 1
        env._h.check(L.rg_step_obs_gray(h, C.c_void_p(k.data_ptr()), 1, 0, 0, obs))

    def step_path():
        step()
        env._h.check(L.rg_path(h, 1, None, None, pd, pk))

    def guided():
        env._h.check(L.rg_step_obs_gray(h, pk, 1, 0, 0, obs))
        env._h.check(L.rg_path(h, 1, None, None, pd, pk))

    for _ in range(a.preroll):
        step()
    rates = {}
    for mode, fn in (("step_obs", step), ("step_obs_path", step_path), ("step_obs_again", step), ("guided", guided)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        rates[mode] = round(n * a.steps / (time.perf_counter() - t0) / 1e6, 2)
    env.check_errors()
    print(json.dumps(dict(row="rates", workload=name, n_env=n, obs="gray f32", goal="stairs", steps=a.steps, unit="M env-steps/s", yardstick="step_obs",
                          ratio_path=round(rates["step_obs_path"] / rates["step_obs"], 4), **rates)), flush=True)

    # ---- back to the uniform policy's episode mix, then the same process's k_step time ----
    for _ in range(a.preroll):
        step()
    env._h.check(L.rg_timing_enable(h, 8))
    for _ in range(a.steps):
        step()
    ms, launches = (C.c_double * 4)(), (C.c_uint64 * 4)()
    env._h.check(L.rg_timing_read(h, ms, launches))
    env._h.check(L.rg_timing_enable(h, 0))
    print(json.dumps(dict(row="k_step", workload=name, n_env=n, unit="us per launch (HIP events, every 8th launch)", sampled=int(launches[0]),
                          k_step_us=round(ms[0] * 1e3 / max(int(launches[0]), 1), 2), obs_pass_us=round(ms[2] * 1e3 / max(int(launches[2]), 1), 2))), flush=True)

    # ---- the pass alone, the variants alternating ----
    variants = [("keys_stairs", 1, None, n * 5), ("keys_gold", 2, None, n * 5), ("keys_stairs_gold", 3, None, n * 5), ("field_stairs", 1, pf, n * 5 + field.numel() * 2)]
    calls = {v: (lambda g=g, f=f: L.rg_path(h, g, None, f, pd, pk)) for v, g, f, _ in variants}
    for fn in calls.values():
        for _ in range(a.inner):
            env._h.check(fn())
    us = {v: [] for v, _, _, _ in variants}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.inner)]
    for _ in range(a.repeats):
        for v, _, _, _ in variants:
            fn = calls[v]
            torch.cuda.synchronize()
            for e0, e1 in ev:  # one event pair per call: the pass's own time, not the host's launch rate
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            us[v].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
    env.check_errors()
    passes = {v: dict(median_us=round(statistics.median(us[v]), 2), min_us=round(min(us[v]), 2), max_us=round(max(us[v]), 2), bytes=b) for v, _, _, b in variants}
    print(json.dumps(dict(row="passes", workload=name, n_env=n, repeats=a.repeats, calls_per_repeat=a.inner, unit="us per call (HIP events)",
                          reachable=round(float((dist >= 0).float().mean()), 4), mean_dist=round(float(dist[dist >= 0].float().mean()), 2), **passes)), flush=True)
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
    for name, cfg_name, n in WORKLOADS:
        if a.only and a.only != name:
            continue
        case(name, cfgs[cfg_name], n, a)


if __name__ == "__main__":
    main()
