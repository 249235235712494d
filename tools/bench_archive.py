"""Step + observation + novelty without and with the cell archive (rogue-gym_amd/csrc/rg_archive.hip), the pass alone, and its record writers against
rg_state_save of the same number of records.

65 536 mini envs and 32 768 envs of 80x24, gray f32 observations, `pos` and `screen` keys (episodic novelty), the gold as the score.  ONE handle per case (closed
before the next is built).  JSON lines:

  "rates":  env-steps/s of step + observation + novelty under the uniform-random policy with the archive update ("on") and without it ("off": exactly the
            launches of the same handle had it never enabled the archive -- the yardstick).  --repeats rounds; in each round off and on in turn run --warmup
            untimed and --steps timed steps between two device synchronisations (they alternate, so drift hits both alike).  Per loop: the median over the
            rounds with its spread (min, max).  table "cold": the archive is cleared before every timed "on" run of --cold-steps steps (no warm-up: the first
            steps into an empty table, every offer a new cell or a contested one); table "warm": after --preroll steps.  records_per_step: the records the
            timed "on" runs wrote, per step -- what the pass's cost depends on.
  "passes": HIP events on the stream.  update_in_step: rg_archive_update behind a real step, one event pair per call (the writers have work);
            update_no_writes: the same call again without a step in between (every offer ties with what is stored: the three table launches and two writer
            launches that find an empty list); state_save_k: rg_state_save of k = records_per_step records (the same bodies, the count known to the host).
            The writers' share is update_in_step - update_no_writes, to be held against state_save_k.

    python tools/bench_archive.py [--steps 500] [--warmup 50] [--preroll 200] [--repeats 5] [--inner 50] [--cold-steps 30] [--cells 262144] [--only mini|default]

cells x record bytes of device memory: 3.1 GB at 2^18 mini cells.  With the screen key every env shows states of its own, a few hundred per episode: a table
that fills (stats.dropped > 0 in the row) makes every new state cost the full probe count, as the global novelty table does.
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

WORKLOADS = (("mini", "mini", 65536), ("default", "default", 32768))
WHATS = ("pos", "screen")
MAX_STEPS = 1000


def case(name, cfg, n, what, a):
    from rogue_gym.envs.device import HipVecRogueEnv

    cfgs = [dict(cfg, seed=i) for i in range(n)]
    env = HipVecRogueEnv(cfgs, max_steps=MAX_STEPS, novelty=what, novelty_slots=a.slots, archive=a.cells)
    dev = env.device
    L, h = env._h.L, env._h.h
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    t, after = [0], list(env._after_step)  # (the novelty update, then the archive's: the last registered)

    def step(on):
        env._after_step[:] = after if on else after[:-1]  # (off: _step_keys makes exactly the calls of a handle without the archive)
        env._step_keys(table[t[0] % 512])
        t[0] += 1

    def timed(on, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(on)
        torch.cuda.synchronize()
        return n * steps / (time.perf_counter() - t0) / 1e6

    def summary(rates):
        return {m: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for m, v in rates.items()}

    rows = {}
    for kind in ("cold", "warm"):
        if kind == "warm":
            for _ in range(a.preroll):
                step(True)
        rates, written, on_steps = {"off": [], "on": []}, 0, 0
        for _ in range(a.repeats):
            for m in ("off", "on"):
                if kind == "cold":
                    if m == "on":
                        env.archive_clear()
                    rates[m].append(timed(m == "on", a.cold_steps))
                    if m == "on":
                        written, on_steps = written + env.archive_stats()["written"], on_steps + a.cold_steps
                else:
                    for _ in range(a.warmup):
                        step(m == "on")
                    w0 = env.archive_stats()["written"]
                    rates[m].append(timed(m == "on", a.steps))
                    if m == "on":
                        written, on_steps = written + env.archive_stats()["written"] - w0, on_steps + a.steps
        env.check_errors()
        per_step = written / max(on_steps, 1)
        rows[kind] = per_step
        cost = round(100.0 * (statistics.median(rates["off"]) / statistics.median(rates["on"]) - 1.0), 1)
        print(json.dumps(dict(row="rates", workload=name, what=what, table=kind, n_env=n, cells=a.cells, record_bytes=env.state_bytes,
                              steps=a.cold_steps if kind == "cold" else a.steps, repeats=a.repeats, unit="M env-steps/s", yardstick="off", step_time_added_percent=cost,
                              records_per_step=round(per_step, 1), stats=env.archive_stats(), **summary(rates))), flush=True)

    # ---- the pass alone ----
    def events(fn, before, inner):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(inner)]
        out = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            for e0, e1 in ev:  # one event pair per call: the pass's own time, not the host's launch rate
                before()
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            out.append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
        return dict(median_us=round(statistics.median(out), 2), min_us=round(min(out), 2), max_us=round(max(out), 2))

    update = lambda: env._h.check(L.rg_archive_update(h, None, None, None))
    w0 = env.archive_stats()["written"]
    passes = dict(update_in_step=events(update, lambda: step(False), a.inner))
    k = max(1, round((env.archive_stats()["written"] - w0) / (a.inner * a.repeats)))
    passes["update_no_writes"] = events(update, lambda: None, a.inner)
    ids = torch.randperm(n, generator=gen, device=dev)[:k].to(torch.int32).sort().values.contiguous()
    out = torch.empty((k, env.state_bytes), dtype=torch.uint8, device=dev)
    save = lambda: env._h.check(L.rg_state_save(h, C.c_void_p(ids.data_ptr()), k, 1, C.c_void_p(out.data_ptr())))
    passes["state_save_k"] = events(save, lambda: None, a.inner)
    print(json.dumps(dict(row="passes", workload=name, what=what, n_env=n, cells=a.cells, repeats=a.repeats, k=k, records_per_step=dict(cold=round(rows["cold"], 1), warm=round(rows["warm"], 1)),
                          unit="us per call (HIP events)", **passes)), flush=True)
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
    ap.add_argument("--cold-steps", dest="cold_steps", type=int, default=30)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--cells", type=int, default=1 << 18)
    ap.add_argument("--only", default=None)
    ap.add_argument("--what", default=None)
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        cfgs = json.load(f)["configs"]
    for name, cfg_name, n in WORKLOADS:
        if a.only and a.only != name:
            continue
        for what in WHATS:
            if a.what and a.what != what:
                continue
            case(name, cfgs[cfg_name], n, what, a)


if __name__ == "__main__":
    main()
