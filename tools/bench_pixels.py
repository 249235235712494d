"""Step + observation without and with the pixel pass (rogue-gym_amd/csrc/rg_pixels.hip k_pixels), and the pass against two yardsticks.

Four cases, enemies 0..11, the built-in 8 x 8 tileset: 65 536 mini envs with the 11 x 11 window in gray and in RGB, 32 768 envs of 80 x 24 with the 11 x 11
window in gray, and the whole screen in gray at 8 192 mini envs.  One handle per workload.  Two kinds of rows, one JSON line each:

  "rates":  env-steps/s of step + gray f32 observation under the uniform-random policy, with the pass behind every step ("on") and without it ("off": the same
            launches as a handle built without pixels=).  --repeats rounds; in each round off and on in turn run --warmup untimed and --steps timed steps
            between two device synchronisations (they alternate, so drift hits both alike).  Per loop: the median over the rounds with (min, max).
  "passes": from HIP events on the stream, on the states the rates left behind, --repeats rounds of --inner calls each, alternating, each call between its own
            pair of events, a round's figure the median of its calls: the pass ("pixels"); torch.Tensor.fill_ of the same output tensor ("fill": the write
            floor); and the same image built with torch ops from the symbol-id window ("torch": font_bits[ids] gather, expand, where -- what a user does
            without the pass; it starts from rg_obs_crop_typed's id window / rg_obs_typed's id plane, whose time is included).  ratio_to_fill and
            speedup_over_torch are medians over medians.  bytes_per_env is the size of one env's image.

    python tools/bench_pixels.py [--steps 300] [--warmup 30] [--preroll 100] [--repeats 5] [--inner 20] [--only NAME]
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
MAX_STEPS = 1000
# name -> (workload, n_env, pixels=, pixel_crop=)
CASES = (("mini 11x11 gray", "mini", 65536, "gray", 5), ("mini 11x11 rgb", "mini", 65536, "rgb", 5), ("80x24 11x11 gray", "80x24", 32768, "gray", 5),
         ("mini whole gray", "mini", 8192, "gray", None))


def torch_form(env, ids, crop, channels, font_bits, ink, paper):
    """The image from symbol ids with torch ops.  ids u8 [N, 1, hc, wc]; font_bits bool [S, th, 8] and ink u8 [S, C] indexed by symbol id."""
    L, h = env._h.L, env._h.h
    if crop is None:
        env._h.check(L.rg_obs_typed(h, 2, 3, 0, 0, C.c_void_p(ids.data_ptr())))
    else:
        env._h.check(L.rg_obs_crop_typed(h, 2, 3, crop[0], crop[1], 0, 0, C.c_void_p(ids.data_ptr()), None))
    idx = ids[:, 0].long()                                   # [N, hc, wc]
    n, hc, wc = idx.shape
    th = font_bits.shape[1]
    bits = font_bits[idx]                                    # [N, hc, wc, th, 8]
    bits = bits.permute(0, 1, 3, 2, 4).reshape(n, 1, hc * th, wc * 8)
    col = ink[idx].permute(0, 3, 1, 2)                       # [N, C, hc, wc]
    col = col.repeat_interleave(th, 2).repeat_interleave(8, 3)
    return torch.where(bits, col, paper.view(1, channels, 1, 1))


def case(name, workload, cfg, n, pixels, crop, a):
    from rogue_gym.envs.device import HipVecRogueEnv, Tileset
    from rogue_gym.envs import RogueEnv

    env = HipVecRogueEnv([dict(cfg, seed=i) for i in range(n)], max_steps=MAX_STEPS, pixels=pixels, pixel_crop=crop)
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(0)
    table = env._action_keys[torch.randint(0, len(env.ACTIONS), (512, n), generator=gen, device=dev)].contiguous()
    px, channels, radii = env.pixels, 3 if pixels == "rgb" else 1, None if crop is None else env._crop_radii(crop)
    refresh = list(env._refresh)  # (the pixel pass is all this env registered)
    t = [0]

    def step(on):
        """off: _refresh_views makes exactly the calls of a handle without the pass."""
        env._refresh[:] = refresh if on else []
        env.step_keys(table[t[0] % 512])
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
    env._refresh[:] = refresh
    out = {m: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for m, v in rates.items()}
    print(json.dumps(dict(row="rates", case=name, n_env=n, obs="gray f32", steps=a.steps, repeats=a.repeats, unit="M env-steps/s", yardstick="off", **out)), flush=True)
    env.check_errors()

    # ---- the pass alone against the fill and the torch form ----
    ts = Tileset.default()
    syms = [ord(s) for s in RogueEnv.SYMBOLS]                # symbol id -> glyph ('-' and '|' share an id: the torch form draws both as one of them)
    syms = syms + [0x20] * (256 - len(syms))                 # (an id without a symbol: blank)
    font_bits = torch.as_tensor(ts.font[syms], device=dev)
    font_bits = ((font_bits.unsqueeze(-1) >> torch.arange(7, -1, -1, device=dev, dtype=torch.uint8)) & 1).bool()   # [S, th, 8]
    pal = torch.as_tensor(ts.palette, device=dev)
    if channels == 1:
        pal = ((77 * pal[:, 0].int() + 150 * pal[:, 1].int() + 29 * pal[:, 2].int() + 128) >> 8).to(torch.uint8).unsqueeze(1)
    ink, paper = pal[syms].contiguous(), pal[256].contiguous()
    hc, wc = (env.height, env.width) if radii is None else (2 * radii[0] + 1, 2 * radii[1] + 1)
    ids = torch.zeros((n, 1, hc, wc), dtype=torch.uint8, device=dev)
    assert torch_form(env, ids, radii, channels, font_bits, ink, paper).shape == px.shape
    fns = [("pixels", lambda: env._pixel_call(channels, radii, px, env.pixel_center)), ("fill", lambda: px.fill_(7)),
           ("torch", lambda: torch_form(env, ids, radii, channels, font_bits, ink, paper))]
    for _, fn in fns:
        for _ in range(3):
            fn()
    us = {k: [] for k, _ in fns}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.inner)]
    for _ in range(a.repeats):
        for k, fn in fns:
            torch.cuda.synchronize()
            for e0, e1 in ev:  # one event pair per call: the pass's own time, not the host's launch rate
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            us[k].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev))
    passes = {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in us.items()}
    med = {k: statistics.median(v) for k, v in us.items()}
    print(json.dumps(dict(row="passes", case=name, n_env=n, repeats=a.repeats, calls_per_repeat=a.inner, unit="us per call (HIP events)", bytes_per_env=int(px[0].numel()),
                          tensor_MB=round(px.numel() / 1e6, 1), ratio_to_fill=round(med["pixels"] / med["fill"], 3),
                          speedup_over_torch=round(med["torch"] / med["pixels"], 2), write_GBps=round(px.numel() / med["pixels"] / 1e3, 1), **passes)), flush=True)
    env.close()
    del env
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--preroll", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every n_env (a smaller box, or a quick look)")
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        cfgs = json.load(f)["configs"]
    workloads = {"mini": dict(cfgs["mini"], enemies=ENEMIES), "80x24": {"width": 80, "height": 24, "enemies": ENEMIES}}
    for name, workload, n, pixels, crop in CASES:
        if a.only and a.only != name:
            continue
        case(name, workload, workloads[workload], max(1, int(n * a.scale)), pixels, crop, a)


if __name__ == "__main__":
    main()
