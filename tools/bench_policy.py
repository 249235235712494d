"""Step + observation fed by env.act (rg_act, rogue-gym_amd/csrc/rg_policy.hip k_act) against the same loop fed by the chain of torch operations it replaces
(masked_fill, Categorical, sample, log_prob, entropy, the key gather).

Two workloads, each on ONE handle with action_mask=True: 65 536 mini envs and 32 768 default 80x24 envs, f32 gray image; logits f32 and bf16, a fixed
random [N, 11] tensor (no network: the loop's cost is the sampler's and the step's).  Two kinds of rows, one JSON line each:

  "rates":  env-steps/s of act + step + observation and of torch chain + step + observation: --warmup untimed steps, then --steps timed steps between two
            device synchronisations, after a pre-roll of --preroll untimed random steps that brings the batch into its steady-state episode mix.  --repeats
            rounds, the two loops alternating; the median over the rounds and the spread (min, max).
  "passes": the sampler alone from HIP events on the stream, on the state the rates left behind: k_act (all five outputs and the mask), k_action_mask on the
            same handle (the mask alone), and the torch chain.  --repeats rounds; in each round every variant in turn runs --inner calls (the variants
            alternate, so drift hits all alike), each call between its own pair of events; a round's figure is the median of its calls.  Per variant: the
            median over the rounds and the spread (min, max) in microseconds per call.

    python tools/bench_policy.py [--steps 300] [--warmup 50] [--preroll 300] [--repeats 5] [--inner 30] [--only mini|default]
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


def spread(xs, nd=2):
    return dict(median=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd))


def case(name, cfg, n, a):
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv
    from rogue_gym_python import _rogue_gym as inner

    env = HipVecRogueEnv([dict(cfg, seed=i) for i in range(n)], max_steps=1000, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), action_mask=True)
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(a.preroll):
        env.step_keys(env.sample_keys())
    for dtype in (torch.float32, torch.bfloat16):
        logits = (torch.randn((n, len(env.ACTIONS)), generator=gen, device=dev) * 2).to(dtype)
        ninf = float("-inf")

        def chain():
            x = logits.masked_fill(~env.action_mask, ninf)
            dist = torch.distributions.Categorical(logits=x)
            act = dist.sample()
            return env._action_keys[act], dist.log_prob(act), dist.entropy()

        def step_act():
            env.step_logits(logits)

        def step_chain():
            env.step_keys(chain()[0])

        rates = {"act": [], "torch_chain": []}
        for _ in range(a.repeats):
            for mode, fn in (("act", step_act), ("torch_chain", step_chain)):
                for _ in range(a.warmup):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                rates[mode].append(n * a.steps / (time.perf_counter() - t0) / 1e6)
        env.check_errors()
        print(json.dumps(dict(row="rates", workload=name, n_env=n, logits=str(dtype).replace("torch.", ""), steps=a.steps, repeats=a.repeats, unit="M env-steps/s",
                              step_obs_act=spread(rates["act"]), step_obs_torch_chain=spread(rates["torch_chain"]))), flush=True)

        # the two kernels through the C-ABI with every buffer made beforehand: between a call's events stands the launch alone
        L, h, P = env._h.L, env._h.h, lambda t: C.c_void_p(t.data_ptr())
        res = env.act(logits)
        opts = inner._act_opts(seed=0, draw=1)
        args = (h, None, 0, P(logits), inner.ACT_DTYPES[str(dtype).replace("torch.", "")], C.byref(opts), None, None, P(res.keys), P(res.actions), P(res.logp), P(res.entropy),
                P(res.source), P(env._mask_u8))
        variants = {"k_act": lambda: L.rg_act(*args), "k_action_mask": lambda: L.rg_action_mask(h, None, 0, P(env._mask_u8), None, 0, 1), "torch_chain": chain}
        for fn in variants.values():
            for _ in range(a.inner):
                fn()
        us = {v: [] for v in variants}
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.inner)]
        for _ in range(a.repeats):
            for v, fn in variants.items():
                torch.cuda.synchronize()
                for e0, e1 in ev:  # one event pair per call
                    e0.record()
                    fn()
                    e1.record()
                torch.cuda.synchronize()
                us[v].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
        env.check_errors()
        print(json.dumps(dict(row="passes", workload=name, n_env=n, logits=str(dtype).replace("torch.", ""), repeats=a.repeats, calls_per_repeat=a.inner,
                              unit="us per call (HIP events)", **{v: spread(us[v]) for v in variants})), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=30)
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
