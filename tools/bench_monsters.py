"""Step + observation without and with the monster-table pass (rogue-gym_amd/csrc/rg_monsters.hip k_monsters).

Two workloads, both with enemies 0..11: 65 536 mini envs and 32 768 envs of 80 x 24.  One handle per workload; three variants of the pass on it -- shown / cap 4,
all / cap 4 and all / cap 16 (the 4-row and the 16-row kernel instance).  Two kinds of rows, one JSON line each:

  "rates":  env-steps/s of step + observation under the uniform-random policy, with the pass behind every step ("on") and without it ("off": the same
            launches as a handle built without monsters=).  --repeats rounds; in each round off and on in turn run --warmup untimed and --steps timed
            steps between two device synchronisations (they alternate, so drift hits both alike).  Per loop: the median over the rounds with its spread
            (min, max).  The yardstick is the same handle's "off" loop.
  "passes": the pass's own time from HIP events on the stream, on the states the rates left behind: --repeats rounds of --inner calls per variant,
            alternating, each call between its own pair of events; a round's figure is the median of its calls.  bytes_written_per_env is the table and
            the threat words; what the pass reads depends on how many monsters are alive (two words per env, one to three per slot, one cell per alive slot).

    python tools/bench_monsters.py [--steps 400] [--warmup 50] [--preroll 200] [--repeats 5] [--inner 50] [--only mini|80x24]
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

ENEMIES = {"enemies": list(range(12))}
VARIANTS = (("shown", 4), ("all", 4), ("all", 16))
MAX_STEPS = 1000


def case(name, cfg, n, a):
    from rogue_gym.envs.device import HipVecRogueEnv
    from rogue_gym_python import _rogue_gym as inner

    env = HipVecRogueEnv([dict(cfg, seed=i) for i in range(n)], max_steps=MAX_STEPS, monsters="all", monster_cap=16)
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    tables = {v: torch.zeros((n, v[1], 8), dtype=torch.int16, device=dev) for v in VARIANTS}
    t = [0]

    def refresh(variant):
        mode, cap = inner._monster_args(*variant)
        return lambda: env._h.check(env._h.L.rg_monsters(env._h.h, mode, cap, C.c_void_p(tables[variant].data_ptr()), C.c_void_p(env.threat.data_ptr())))

    calls = {v: refresh(v) for v in VARIANTS}

    def step(variant):
        """variant None: _refresh_views makes exactly the calls of a handle without the pass (the monster pass is all this env registered)."""
        env._refresh[:] = [] if variant is None else [calls[variant]]
        if variant is not None:
            env.monsters = tables[variant]
        env.step_keys(table[t[0] % 512])
        t[0] += 1

    for _ in range(a.preroll):
        step(VARIANTS[0])
    for variant in VARIANTS:
        rates = {"off": [], "on": []}
        for _ in range(a.repeats):
            for m in ("off", "on"):
                v = variant if m == "on" else None
                for _ in range(a.warmup):
                    step(v)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(v)
                torch.cuda.synchronize()
                rates[m].append(n * a.steps / (time.perf_counter() - t0) / 1e6)
        out = {m: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for m, v in rates.items()}
        print(json.dumps(dict(row="rates", workload=name, variant="%s/cap%d" % variant, n_env=n, obs="gray f32", steps=a.steps, repeats=a.repeats, unit="M env-steps/s",
                              yardstick="off", **out)), flush=True)
    env.check_errors()
    counts = env.monster_table("all", 16)[1][:, 3].float()
    shown = env.monster_table("shown", 16)[1][:, 3].float()
    print(json.dumps(dict(row="state", workload=name, n_env=n, alive_per_env=round(float(counts.mean()), 3), shown_per_env=round(float(shown.mean()), 3),
                          max_alive=int(counts.max()))), flush=True)

    # ---- the pass alone, the variants alternating ----
    def call(variant):
        m, cap = inner._monster_args(*variant)
        return lambda: env._h.check(env._h.L.rg_monsters(env._h.h, m, cap, C.c_void_p(tables[variant].data_ptr()), C.c_void_p(env.threat.data_ptr())))

    fns = [("%s/cap%d" % v, call(v)) for v in VARIANTS]
    for _, fn in fns:
        for _ in range(a.inner):
            fn()
    us = {v: [] for v, _ in fns}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.inner)]
    for _ in range(a.repeats):
        for v, fn in fns:
            torch.cuda.synchronize()
            for e0, e1 in ev:  # one event pair per call: the pass's own time, not the host's launch rate
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            us[v].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
    passes = {v: dict(median_us=round(statistics.median(us[v]), 2), min_us=round(min(us[v]), 2), max_us=round(max(us[v]), 2)) for v, _ in fns}
    print(json.dumps(dict(row="passes", workload=name, n_env=n, repeats=a.repeats, calls_per_repeat=a.inner, unit="us per call (HIP events)",
                          bytes_written_per_env={"%s/cap%d" % v: 16 * v[1] + 16 for v in VARIANTS}, **passes)), flush=True)
    env.close()
    del env
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
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
    for name, cfg, n in (("mini", dict(cfgs["mini"], enemies=ENEMIES), 65536), ("80x24", {"width": 80, "height": 24, "enemies": ENEMIES}, 32768)):
        if a.only and a.only != name:
            continue
        case(name, cfg, n, a)


if __name__ == "__main__":
    main()
