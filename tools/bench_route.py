"""Step + observation against the guided loops of rg_route (rogue-gym_amd/csrc/rg_route.hip k_route).

Two workloads, each on ONE handle with the same seeds: 65 536 mini envs and 32 768 default 80x24 envs, f32 gray image.  Two kinds of rows, one JSON line
each:

  "rates":  env-steps/s of step + observation under the uniform-random policy (rg_step_obs_gray: the yardstick, the path without any pass) and of the three
            guided loops -- every env plays its teacher key: guide="stairs" (rg_path), the same with guide_secrets (rg_route, RG_ROUTE_SECRETS) and
            guide="explore" (rg_route: goals stairs, fallback frontier, RG_ROUTE_KNOWN).  --repeats rounds; in each round every loop in turn runs --warmup
            untimed and --steps timed steps between two device synchronisations (the loops alternate, so drift hits all alike).  Per loop: the median
            over the rounds with its spread (min, max), and the descents per 1 000 env-steps of its timed steps (rg_counters).
  "passes": the pass's own time from HIP events on the stream, on the state the rates left behind: rg_path keys only (stairs), and rg_route for stairs +
            SECRETS and for the explorer.  --repeats rounds of --inner calls per variant, alternating, each call between its own pair of events; a
            round's figure is the median of its calls.  Per variant: the median over the rounds and the spread in microseconds per call.

    python tools/bench_route.py [--steps 500] [--warmup 50] [--preroll 200] [--repeats 5] [--inner 50] [--only mini|default]
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
EXPLORE, SECRETS = (1, 8, 2), (1, 0, 1)  # (goals, fallback_goals, mode) of rg_route


def case(name, cfg, n, a):
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    env = HipVecRogueEnv([dict(cfg, seed=i) for i in range(n)], max_steps=1000, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False))
    dev, L, h = env.device, env._h.L, env._h.h
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    keys = torch.full((n,), ord("."), dtype=torch.uint8, device=dev)
    dist = torch.empty((n,), dtype=torch.int32, device=dev)
    tier = torch.empty((n,), dtype=torch.uint8, device=dev)
    obs = C.c_void_p(env.obs.data_ptr())
    pk, pd, pt = C.c_void_p(keys.data_ptr()), C.c_void_p(dist.data_ptr()), C.c_void_p(tier.data_ptr())
    t = [0]

    def step():
        k = table[t[0] % 512]
        t[0] += 1
        env._h.check(L.rg_step_obs_gray(h, C.c_void_p(k.data_ptr()), 1, 0, 0, obs))

    def teach_path():
        env._h.check(L.rg_path(h, 1, None, None, pd, pk))

    def teach(words):
        return lambda: env._h.check(L.rg_route(h, words[0], words[1], words[2], None, pd, pk, pt))

    def guided(teacher):
        def fn():
            env._h.check(L.rg_step_obs_gray(h, pk, 1, 0, 0, obs))
            teacher()
        return fn

    loops = (("step_obs", step, None), ("guide_stairs", guided(teach_path), teach_path), ("guide_stairs_secrets", guided(teach(SECRETS)), teach(SECRETS)),
             ("guide_explore", guided(teach(EXPLORE)), teach(EXPLORE)))
    for _ in range(a.preroll):
        step()
    rates, descents = {m: [] for m, _, _ in loops}, {m: [] for m, _, _ in loops}
    for _ in range(a.repeats):
        for mode, fn, first in loops:
            if first is not None:
                first()  # the keys of the state the loop starts from
            for _ in range(a.warmup):
                fn()
            env.counters(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            rates[mode].append(n * a.steps / (time.perf_counter() - t0) / 1e6)
            descents[mode].append(1000.0 * env.counters()["descents"] / (n * a.steps))
    env.check_errors()
    out = {m: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2), descents_per_1000_steps=round(statistics.median(descents[m]), 3))
           for m, v in rates.items()}
    print(json.dumps(dict(row="rates", workload=name, n_env=n, obs="gray f32", steps=a.steps, repeats=a.repeats, unit="M env-steps/s", yardstick="step_obs", **out)), flush=True)

    # ---- the pass alone, the variants alternating ----
    variants = [("path_stairs", teach_path), ("route_stairs_secrets", teach(SECRETS)), ("route_explore", teach(EXPLORE))]
    for _, fn in variants:
        for _ in range(a.inner):
            fn()
    us = {v: [] for v, _ in variants}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.inner)]
    for _ in range(a.repeats):
        for v, fn in variants:
            torch.cuda.synchronize()
            for e0, e1 in ev:  # one event pair per call: the pass's own time, not the host's launch rate
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            us[v].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
    env.check_errors()
    passes = {v: dict(median_us=round(statistics.median(us[v]), 2), min_us=round(min(us[v]), 2), max_us=round(max(us[v]), 2)) for v, _ in variants}
    print(json.dumps(dict(row="passes", workload=name, n_env=n, repeats=a.repeats, calls_per_repeat=a.inner, unit="us per call (HIP events)",
                          explore_tier0=round(float((tier == 0).float().mean()), 4), explore_tier1=round(float((tier == 1).float().mean()), 4), **passes)), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
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
