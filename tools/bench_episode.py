"""Step + observation without and with the episode accounting (rogue-gym_amd/csrc/rg_episode.hip k_episode).

The three benchmark workloads, each on TWO handles with the same seeds and keys, one after the other (the first is closed before the second is built:
handles that live side by side share the process's hardware queues, and the second one of a pair steps markedly slower whatever it runs): scalars only
(episodes=True), and scalars + scout bitmap (scout=True).  Two kinds of rows, one JSON line each:

  "rates":  env-steps/s of step + observation under the uniform-random policy, on each handle with the update ("on") and without it ("off": the same
            launches as a handle that never enabled the accounting).  --repeats rounds; in each round off and on in turn run --warmup untimed and --steps
            timed steps between two device synchronisations (they alternate, so drift hits both alike).  Per loop: the median over the rounds with its
            spread (min, max).
  "passes": the pass's own time from HIP events on the stream, on the states the rates left behind: rg_episode_update of the handle's instance, and -- on
            the first handle -- the same SCALAR bookkeeping (return, length, end cause, last_*) written in torch ops: what a user writes today, without
            depth and scout.  --repeats rounds of --inner calls per variant, alternating, each call between its own pair of events; a round's figure is
            the median of its calls.

    python tools/bench_episode.py [--steps 500] [--warmup 50] [--preroll 200] [--repeats 5] [--inner 50] [--only mini|default|nohide-symbol]
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

WORKLOADS = (("mini", "mini", 65536, "gray"), ("default", "default", 32768, "gray"), ("nohide-symbol", "nohide", 32768, "symbol"))  # bench.py's three
MAX_STEPS = 1000


class TorchBookkeeping:
    """Return, length, end cause and the last finished episode of every env in torch ops on the env's reward / done tensors: the hand-written version."""

    def __init__(self, env):
        n, dev = env.num_envs, env.device
        self.env = env
        self.ret, self.len = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        self.last_return, self.last_length = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        self.died, self.time_limit = torch.zeros(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)

    def update(self):
        done = self.env.done
        self.ret += self.env.reward
        self.len += 1
        torch.logical_and(done, self.len >= MAX_STEPS, out=self.time_limit)
        torch.logical_and(done, ~self.time_limit, out=self.died)
        self.last_return = torch.where(done, self.ret, self.last_return)
        self.last_length = torch.where(done, self.len, self.last_length)
        self.ret.masked_fill_(done, 0.0)
        self.len.masked_fill_(done, 0)


def case(name, cfg, n, kind, a):
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    st = ImageSetting(DungeonType.SYMBOL if kind == "symbol" else DungeonType.GRAY, StatusFlag.EMPTY, False)
    cfgs = [dict(cfg, seed=i) for i in range(n)]
    for variant, kw in (("episodes", dict(episodes=True)), ("scout", dict(scout=True))):
        env = HipVecRogueEnv(cfgs, max_steps=MAX_STEPS, image_setting=st, **kw)
        dev = env.device
        gen = torch.Generator(device=dev).manual_seed(0)
        table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
        t, update = [0], list(env._after_step)  # (the episode update is all this env registered behind its steps)

        def step(on):
            env._after_step[:] = update if on else []  # (off: _step_keys makes exactly the calls of a handle without the accounting)
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
        if kind == "symbol":
            env._h.L.rg_sync(env._h.h)  # (drains the tile-error word: 'Z' is a monster of these configs and not a symbol, as in the reference)
        else:
            env.check_errors()
        out = {m: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for m, v in rates.items()}
        print(json.dumps(dict(row="rates", workload=name, variant=variant, n_env=n, obs=kind + " f32", steps=a.steps, repeats=a.repeats, unit="M env-steps/s", yardstick="off", **out)),
              flush=True)

        # ---- the pass alone, the variants alternating (a second update of one step accounts the mirrors again: the same work) ----
        variants = [("update_" + variant, lambda: env._h.check(env._h.L.rg_episode_update(env._h.h)))]
        if variant == "episodes":
            variants.append(("torch_ops_scalars", TorchBookkeeping(env).update))
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
        passes = {v: dict(median_us=round(statistics.median(us[v]), 2), min_us=round(min(us[v]), 2), max_us=round(max(us[v]), 2)) for v, _ in variants}
        extra = dict(scout_bytes_read_per_call=n * (2 * env.height * env.width + env.seen_bits.shape[1])) if variant == "scout" else {}
        print(json.dumps(dict(row="passes", workload=name, variant=variant, n_env=n, repeats=a.repeats, calls_per_repeat=a.inner, unit="us per call (HIP events)", **extra, **passes)),
              flush=True)
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
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        cfgs = json.load(f)["configs"]
    for name, cfg_name, n, kind in WORKLOADS:
        if a.only and a.only != name:
            continue
        case(name, cfgs[cfg_name], n, kind, a)


if __name__ == "__main__":
    main()
