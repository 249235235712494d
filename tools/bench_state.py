"""Save / load throughput of the state records (rg_state_save / rg_state_load, rogue-gym_amd/csrc/rg_state_io.hip).

For 65 536 mini envs and 32 768 envs on 80x24, with contiguous ids (NULL = every env in order) and with a random permutation (device ids): bytes
moved, microseconds per call (HIP events on the handle's stream, median of --reps samples of --calls back-to-back calls each) and the ratio to a
device-to-device copy of the same byte count (torch copy_ = hipMemcpyAsync D2D) on the same device.  One JSON line per case.

    python tools/bench_state.py [--reps 25] [--calls 4] [--only mini|default]
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


def timed(fn, reps, calls):
    s = torch.cuda.current_stream()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(calls):
            fn()
        b.record(s)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / calls)
    return float(np.median(out))


def case(name, cfg, n, reps, calls):
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
    for _ in range(20):  # (states of a running batch: dist maps built, monsters awake)
        env.step_keys(keys[torch.randint(0, len(keys), (n,), generator=g).to(dev)])
    env.check_errors()
    L, h = env._h.L, env._h.h
    R = env.state_bytes
    recs = torch.empty((n, R), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(recs)
    perm = torch.randperm(n, generator=g).to(device=dev, dtype=torch.int32)
    rows = []
    for ids_name, ids in (("contiguous", None), ("permuted", perm)):
        ptr = None if ids is None else C.c_void_p(ids.data_ptr())
        on_dev = 0 if ids is None else 1

        def save():
            env._h.check(L.rg_state_save(h, ptr, n, on_dev, C.c_void_p(recs.data_ptr())))

        def load():
            env._h.check(L.rg_state_load(h, C.c_void_p(recs.data_ptr()), R, ptr, n, on_dev))

        save()
        torch.cuda.synchronize()
        t_save = timed(save, reps, calls)
        t_load = timed(load, reps, calls)
        t_copy = timed(lambda: dst.copy_(recs), reps, calls)
        env.check_errors()
        row = dict(case=name, n=n, ids=ids_name, record_bytes=R, bytes=n * R, save_us=round(t_save, 1), load_us=round(t_load, 1),
                   d2d_copy_us=round(t_copy, 1), save_vs_copy=round(t_save / t_copy, 3), load_vs_copy=round(t_load / t_copy, 3),
                   save_GBps=round(2 * n * R / t_save / 1e3, 1), load_GBps=round(2 * n * R / t_load / 1e3, 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
    env.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        cfgs = json.load(f)["configs"]
    for name, n in (("mini", 65536), ("default", 32768)):
        if a.only and a.only != name:
            continue
        case(name, cfgs[name], n, a.reps, a.calls)


if __name__ == "__main__":
    main()
