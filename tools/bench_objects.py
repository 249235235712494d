"""Step + observation without and with the object-table pass (rogue-gym_amd/csrc/rg_objects.hip k_objects).

Two workloads, both with enemies 0..11: 65 536 mini envs and 32 768 envs of 80 x 24.  One handle per workload; four variants of the pass on it -- known / cap 8,
known / cap 32, all / cap 8 and all / cap 32 (known asks stairs + gold + door + frontier, all asks stairs + gold + door).  Two kinds of rows, one JSON line each:

  "rates":  env-steps/s of step + observation under the uniform-random policy, with the pass behind every step ("on") and without it ("off": the same
            launches as a handle built without objects=).  --repeats rounds; in each round off and on in turn run --warmup untimed and --steps timed
            steps between two device synchronisations (they alternate, so drift hits both alike).  Per loop: the median over the rounds with its spread
            (min, max).  The yardstick is the same handle's "off" loop.
  "passes": the pass's own time from HIP events on the stream, on the states the rates left behind: --repeats rounds of --inner calls per variant,
            alternating, each call between its own pair of events; a round's figure is the median of its calls.  bytes_written_per_env is the table and
            the counts; the pass reads the env's grid once (2 H W bytes) and one cell word more per listed object.

The random policy keeps the players near their start, where little of the map is known: a guided policy knows more of it and lists more.  --guide explore
steps with the explorer's keys instead.

    python tools/bench_objects.py [--steps 400] [--warmup 50] [--preroll 200] [--repeats 5] [--inner 50] [--only mini|80x24] [--guide explore]
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
# (objects=, kinds, cap)
VARIANTS = (("known", "stairs+gold+door+frontier", 8), ("known", "stairs+gold+door+frontier", 32), ("all", "stairs+gold+door", 8), ("all", "stairs+gold+door", 32))
MAX_STEPS = 1000


def label(v):
    return "%s/cap%d" % (v[0], v[2])


def case(name, cfg, n, a):
    from rogue_gym.envs.device import HipVecRogueEnv
    from rogue_gym_python import _rogue_gym as inner

    env = HipVecRogueEnv([dict(cfg, seed=i) for i in range(n)], max_steps=MAX_STEPS, objects="known", object_kinds=VARIANTS[0][1], object_cap=32, guide=a.guide)
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    tables = {v: torch.zeros((n, v[2], 8), dtype=torch.int16, device=dev) for v in VARIANTS}
    args = {v: inner._object_args(v[1], v[0] == "known", False, v[2]) for v in VARIANTS}
    t, others = [0], env._refresh[:-1]  # (the object pass is the last an env registers; a guide's comes before it)

    def refresh(variant):
        kw, mode, cap = args[variant]
        return lambda: env._h.check(env._h.L.rg_objects(env._h.h, kw, mode, cap, C.c_void_p(tables[variant].data_ptr()), C.c_void_p(env.object_count.data_ptr())))

    calls = {v: refresh(v) for v in VARIANTS}

    def step(variant):
        """variant None: _refresh_views makes exactly the calls of a handle without the pass."""
        env._refresh[:] = others if variant is None else others + [calls[variant]]
        if variant is not None:
            env.objects = tables[variant]
        env.step_keys(table[t[0] % 512] if a.guide is None else env.guide_keys)
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
        print(json.dumps(dict(row="rates", workload=name, variant=label(variant), policy=a.guide or "random", n_env=n, obs="gray f32", steps=a.steps, repeats=a.repeats,
                              unit="M env-steps/s", yardstick="off", **out)), flush=True)
    env.check_errors()
    state = {}
    for v in (VARIANTS[1], VARIANTS[3]):
        tb, cnt = env.object_table(v[1], v[0] == "known", False, 32)
        listed = (tb[:, :, 0] != 0).sum(1).float()
        state[v[0]] = dict(listed_per_env=round(float(listed.mean()), 3), cells_per_env=[round(float(c), 3) for c in cnt.float().mean(0)],
                           mean_walk_of_last_row=round(float(tb[:, :, 3].max(1).values.float().mean()), 2), max_walk=int(tb[:, :, 3].max()))
    print(json.dumps(dict(row="state", workload=name, n_env=n, policy=a.guide or "random", **state)), flush=True)

    # ---- the pass alone, the variants alternating ----
    def call(variant):
        kw, mode, cap = args[variant]
        return lambda: env._h.check(env._h.L.rg_objects(env._h.h, kw, mode, cap, C.c_void_p(tables[variant].data_ptr()), C.c_void_p(env.object_count.data_ptr())))

    fns = [(label(v), call(v)) for v in VARIANTS]
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
                          bytes_written_per_env={label(v): 16 * v[2] + 16 for v in VARIANTS}, **passes)), flush=True)
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
    ap.add_argument("--guide", default=None, choices=(None, "explore", "stairs"))
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
