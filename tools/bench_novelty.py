"""Step + observation without and with the novelty pass (rogue-gym_amd/csrc/rg_novelty.hip), the pass alone, and the same counts in torch ops.

65 536 mini envs and 32 768 envs of 80x24, gray f32 observations.  For each `what` (pos, screen, crop of radius 4) and each scope (episode, global, both) ONE
handle (closed before the next is built: handles that live side by side share the process's hardware queues).  Two kinds of rows, one JSON line each:

  "rates":  env-steps/s of step + observation under the uniform-random policy with the update ("on") and without it ("off": exactly the launches of a handle
            that never enabled novelty -- the yardstick).  --repeats rounds; in each round off and on in turn run --warmup untimed and --steps timed steps
            between two device synchronisations (they alternate, so drift hits both alike).  Per loop: the median over the rounds with its spread (min, max).
  "passes": the pass's own time from HIP events on the stream, on the states the rates left behind: rg_novelty_update, and -- on the screen / both handle --
            what a user writes today for the counts of one step: torch.unique over the screens' rows [N, (H-2) * W] with inverse and counts (that gives
            the counts inside ONE step's batch only; a memory across steps needs a host dict on top).  --repeats rounds of --inner calls per variant,
            each call between its own pair of events; a round's figure is the median of its calls.

    python tools/bench_novelty.py [--steps 500] [--warmup 50] [--preroll 200] [--repeats 5] [--inner 50] [--only mini|default] [--slots 1024] [--global-slots 67108864]

The global table is sized for the run (2^26 slots, 1 GB): with the screen key every env of a batch of procedurally generated games shows its own states, a few
hundred per episode, and a table that fills (stats.dropped_global > 0 in the row) makes every new state cost the full probe count.
"""
import argparse
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

WORKLOADS = (("mini", "mini", 65536), ("default", "default", 32768))
WHATS = (("pos", None), ("screen", None), ("crop", 4))
SCOPES = ("episode", "global", "both")
MAX_STEPS = 1000


def case(name, cfg, n, what, crop, scope, a):
    from rogue_gym.envs.device import HipVecRogueEnv

    cfgs = [dict(cfg, seed=i) for i in range(n)]
    env = HipVecRogueEnv(cfgs, max_steps=MAX_STEPS, novelty=what, novelty_crop=crop, novelty_scope=scope, novelty_slots=a.slots, novelty_global_slots=a.global_slots)
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    t, update = [0], list(env._after_step)  # (the novelty update is all this env registered behind its steps)

    def step(on):
        env._after_step[:] = update if on else []  # (off: _step_keys makes exactly the calls of a handle without novelty)
        env._step_keys(table[t[0] % 512])
        t[0] += 1

    for _ in range(a.preroll):
        step(True)
    rates = {"off": [], "on": []}
    for _ in range(a.repeats):
        for m in ("off", "on"):
            for _ in range(a.warmup):
                step(m == "on")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(m == "on")
            torch.cuda.synchronize()
            rates[m].append(n * a.steps / (time.perf_counter() - t0) / 1e6)
    env._after_step[:] = update
    env.check_errors()
    out = {m: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for m, v in rates.items()}
    cost = round(100.0 * (statistics.median(rates["off"]) / statistics.median(rates["on"]) - 1.0), 1)
    stats = env.novelty_stats()
    print(json.dumps(dict(row="rates", workload=name, what=what, scope=scope, n_env=n, slots=a.slots, global_slots=a.global_slots, steps=a.steps, repeats=a.repeats,
                          unit="M env-steps/s", yardstick="off", step_time_added_percent=cost, table_bytes=16 * (a.slots * n * (scope != "global") + a.global_slots * (scope != "episode")),
                          stats=stats, max_count=None if env.visit_count is None else int(env.visit_count.max()), **out)), flush=True)

    # ---- the pass alone (a second update of one step counts the state again: the same work) ----
    variants = [("update", lambda: env._h.check(env._h.L.rg_novelty_update(env._h.h)), a.inner)]
    if what == "screen" and scope == "both":
        w = env.width
        rows = env.screen.view(n, -1)[:, w:-w]
        variants.append(("torch_unique_one_step", lambda: torch.unique(rows, dim=0, return_inverse=True, return_counts=True), max(2, a.inner // 10)))
    us = {}
    for v, fn, inner in variants:
        for _ in range(2):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(inner)]
        us[v] = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            for e0, e1 in ev:  # one event pair per call: the pass's own time, not the host's launch rate
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            us[v].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
    passes = {v: dict(median_us=round(statistics.median(x), 2), min_us=round(min(x), 2), max_us=round(max(x), 2)) for v, x in us.items()}
    print(json.dumps(dict(row="passes", workload=name, what=what, scope=scope, n_env=n, repeats=a.repeats, unit="us per call (HIP events)", **passes)), flush=True)
    env.close()
    del env
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--global-slots", dest="global_slots", type=int, default=1 << 26)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        cfgs = json.load(f)["configs"]
    for name, cfg_name, n in WORKLOADS:
        if a.only and a.only != name:
            continue
        for what, crop in WHATS:
            for scope in SCOPES:
                case(name, cfgs[cfg_name], n, what, crop, scope, a)


if __name__ == "__main__":
    main()
