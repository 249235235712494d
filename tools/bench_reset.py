"""Cost of resetting chosen envs (rg_reset_mask: rogue-gym_amd/csrc/rg_kernels.hip k_reset_compact / k_build_list + rg_state_io.hip k_state_stairs) next to
rg_reset (k_build) on the same handle in the same run.

For 65 536 mini envs and 32 768 envs on 80x24: the median time of rg_reset_mask with 0 %, 1 %, 10 % and 100 % of the envs set (random envs, fixed
generator seed) and of rg_reset -- HIP events on the handle's stream, --reps samples of one call each, the batch played on for a few steps between the
samples so that every call meets a running batch.  Per mask the implied microseconds per rebuilt env, and for the all-ones mask the ratio to rg_reset
(the yardstick: the same generations plus a compaction and a list indirection).  One JSON line.

    python tools/bench_reset.py [--reps 15] [--only mini|default]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rogue-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRACTIONS = (0.0, 0.01, 0.1, 1.0)


def case(name, cfg, n, reps):
    from rogue_gym.envs.device import HipVecRogueEnv

    cfgs = []
    for i in range(n):
        d = dict(cfg)
        d["seed"] = i
        cfgs.append(d)
    env = HipVecRogueEnv(cfgs, max_steps=1000)
    dev = env.device
    keys = torch.frombuffer(bytearray(b".hjklnbuy>s"), dtype=torch.uint8).to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    L, h = env._h.L, env._h.h
    masks = {}
    for f in FRACTIONS:
        m = torch.zeros(n, dtype=torch.uint8)
        m[torch.randperm(n, generator=g)[: int(round(f * n))]] = 1
        masks[f] = m.to(dev)

    def play(steps):
        for _ in range(steps):
            env.step_keys(keys[torch.randint(0, len(keys), (n,), generator=g).to(dev)])

    def timed(fn):
        s = torch.cuda.current_stream()
        out = []
        for _ in range(reps):
            play(3)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            out.append(a.elapsed_time(b) * 1000.0)
        return float(np.median(out))

    play(20)
    env.check_errors()
    row = dict(case=name, n=n, reps=reps)
    t_reset = timed(lambda: env._h.check(L.rg_reset(h)))
    row["rg_reset_us"] = round(t_reset, 1)
    for f in FRACTIONS:
        k = int(masks[f].sum())
        t = timed(lambda: env._h.check(L.rg_reset_mask(h, C.c_void_p(masks[f].data_ptr()))))
        tag = "mask_%g%%" % (100 * f)
        row[tag + "_envs"] = k
        row[tag + "_us"] = round(t, 1)
        if k:
            row[tag + "_us_per_env"] = round(t / k, 4)
    row["mask_100%_vs_rg_reset"] = round(row["mask_100%_us"] / t_reset, 3)
    row["rg_reset_us_again"] = round(timed(lambda: env._h.check(L.rg_reset(h))), 1)   # (the yardstick's own spread inside this run)
    env.check_errors()
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        cfgs = json.load(f)["configs"]
    rows = []
    for name, n in (("mini", 65536), ("default", 32768)):
        if a.only and a.only != name:
            continue
        rows.append(case(name, cfgs[name], n, a.reps))
    print(json.dumps(dict(tool="bench_reset", cases=rows)), flush=True)


if __name__ == "__main__":
    main()
