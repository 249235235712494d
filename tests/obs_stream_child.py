"""Child process of tests/test_gpu_obs_stream.py (run with ROGUE_GYM_HIP_LIB = the development library).

Two handles over the same configs take the same keys; before every observation call of handle B the development knob RG_OBS_STREAM=0 sends the
gray encode to k_obs<0, false> instead of k_obs_stream.  After every observation call the two f32 tensors must agree bit for bit (compared on the
device as int32), and every few calls -- and after every special event -- the mirrors (screen, history, status) and the FULL flag words, the
Redraw bookkeeping bits included.

usage: obs_stream_child.py CONFIG N STEPS [no_mirror]"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rogue-gym_amd"))

import torch  # noqa: E402

from rogue_gym_python import _rogue_gym as inner  # noqa: E402


def main():
    name, n, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    no_mirror = "no_mirror" in sys.argv[4:]
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        cfg = json.load(f)["configs"][name]
    cfgs = [json.dumps(dict(cfg, seed=i % 5000)) for i in range(n)]
    if no_mirror:  # every Redraw is drawn from the tiles by the observation pass (about 43 % of the envs of a step)
        os.environ["ROGUE_GYM_HIP_NO_MIRROR_UPDATE"] = "1"
    a = inner._Handle(cfgs, 40, auto_reset=True)
    b = inner._Handle(cfgs, 40, auto_reset=True)
    os.environ.pop("ROGUE_GYM_HIP_NO_MIRROR_UPDATE", None)
    dev = torch.device("cuda", a.device)
    oa = torch.empty((n, a.height, a.width), dtype=torch.float32, device=dev)
    ob = torch.full((n, a.height, a.width), -1.0, dtype=torch.float32, device=dev)
    rng = np.random.RandomState(5)
    table = np.frombuffer(b"hjklyubnhjklyubnHJKL>s.", np.uint8)
    counts = {"obs": 0, "fetch": 0}

    def observe(t, why):
        a.check(a.L.rg_obs_gray(a.h, 0, 0, ctypes.c_void_p(oa.data_ptr())))
        os.environ["RG_OBS_STREAM"] = "0"
        try:
            b.check(b.L.rg_obs_gray(b.h, 0, 0, ctypes.c_void_p(ob.data_ptr())))
        finally:
            del os.environ["RG_OBS_STREAM"]
        torch.cuda.synchronize()
        counts["obs"] += 1
        same = (oa.view(torch.int32) == ob.view(torch.int32)).flatten(1).all(1)
        if not bool(same.all()):
            bad = torch.nonzero(~same).flatten()[:8].tolist()
            raise AssertionError("step %d (%s): images differ at envs %s" % (t, why, bad))

    def compare_states(t, why):
        counts["fetch"] += 1
        xa, xb = a.fetch(), b.fetch()
        for x, y, what in zip(xa, xb, ("screen", "hist", "status", "flags")):
            if not np.array_equal(x, y):
                raise AssertionError("step %d (%s): %s differs at envs %s" % (t, why, what, [i for i in range(n) if not np.array_equal(x[i], y[i])][:8]))

    # the first pass after creation and after rg_reset: every env's mirror comes from its new level
    observe(-1, "after create")
    compare_states(-1, "after create")
    for t in range(steps):
        keys = np.ascontiguousarray(table[rng.randint(0, len(table), n)])
        if t % 7 == 3:  # a prefix step: only the first n_keys envs get a key
            k = n - 1 - rng.randint(0, n // 3)
            for h in (a, b):
                h.check(h.L.rg_step_prefix(h.h, keys.ctypes.data, k, 0))
        else:
            for h in (a, b):
                h.check(h.L.rg_step(h.h, keys.ctypes.data, 0))
        if t % 5 == 1:  # no observation after this step: its Redraw flags stay pending into the next pass
            continue
        observe(t, "step")
        if t % 20 == 0 or t == steps - 1:
            compare_states(t, "step")
        if t == steps // 2:
            for h in (a, b):
                h.check(h.L.rg_reset(h.h))
            observe(t, "after rg_reset")
            compare_states(t, "after rg_reset")
    a.close()
    b.close()
    print("OK", json.dumps(counts))


if __name__ == "__main__":
    main()
