"""Returns and advantages of a [T, N] rollout (rg_gae / rg_vtrace, rogue-gym_amd/csrc/rg_returns.hip k_gae and k_vtrace) against the reversed Python loop of
torch operations they replace and against a device-to-device copy of the same byte count, and the pipeline depths and envs-per-lane variants of the kernel
against each other.

(T, N) = (16, 65 536), (128, 65 536), (128, 32 768) and (128, 256); fixed random inputs, 2 % of the steps end an episode.  One JSON line per shape, every
figure in microseconds per call from HIP events on the stream:

  k_gae, k_vtrace      the launch alone through the C-ABI, every buffer made beforehand (reward, value, done and both outputs; V-trace with the two logp rows)
  torch_gae            the loop of examples/a2c_masked.py before this kernel (for t in reversed(range(T)): elementwise torch ops on [N] rows), extended by the
                       GAE terms, the rows stacked at the end
  torch_vtrace         the same loop with the clipped ratios (computed for the whole rollout in three torch ops beforehand, inside the timing)
  copy_gae, copy_vtrace  one device-to-device copy of as many bytes as the kernel reads plus as many as it writes, halved (a copy moves every byte twice)
  gae_d<D>e<E>, vtrace_d<D>e<E>   rgk_gae and rgk_vtrace of a variant library (rogue-gym_amd/variants/librogue_gym_returns_d<D>e<E>.so: -DRG_RET_DEPTH=D -DRG_RET_ENVS=E), built by
                       --build-variants; each variant's outputs are held against the product's bits before anything is timed

--repeats rounds; in each round every variant in turn runs --inner calls (the variants alternate, so drift hits all alike), each call between its own pair of
events; a round's figure is the median of its calls.  Per variant: the median over the rounds and the spread (min, max).

    python tools/bench_returns.py [--repeats 5] [--inner 20] [--shapes 16x65536,128x65536,128x32768,128x256] [--build-variants] [--variants 4x1,8x1,32x1,8x2,16x2,4x4,8x4]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rogue-gym_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GAMMA, LAM = 0.99, 0.95


def spread(xs, nd=2):
    return dict(median=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd))


def variant_path(d, e):
    return os.path.join(PKG, "variants", "librogue_gym_returns_d%de%d.so" % (d, e))


def build_variants(pairs):
    """hipcc, needs no GPU: one library per (depth, envs per lane), side by side."""
    os.makedirs(os.path.join(PKG, "variants"), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "hipcc")
    jobs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-O3", "-shared", "-Wl,-Bsymbolic", "-DRG_RET_DEPTH=%d" % d, "-DRG_RET_ENVS=%d" % e,
                              os.path.join(PKG, "csrc", "rg_returns.hip"), "-o", variant_path(d, e)]) for d, e in pairs]
    if any(j.wait() != 0 for j in jobs):
        raise SystemExit("hipcc failed")


def load_variant(d, e):
    path = variant_path(d, e)
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    vp, i64, f32 = C.c_void_p, C.c_int64, C.c_float
    lib.rgk_gae.argtypes, lib.rgk_gae.restype = [i64, i64, vp, vp, vp, vp, vp, vp, f32, f32, vp, vp, vp], None
    lib.rgk_vtrace.argtypes, lib.rgk_vtrace.restype = [i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp], None
    return lib


def case(T, N, a, pairs):
    import numpy as np
    import torch
    from rogue_gym_python import _rogue_gym as inner
    L = inner.load_library()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rew, val = torch.randn((T, N), generator=gen, device=dev), torch.randn((T, N), generator=gen, device=dev)
    last = torch.randn((N,), generator=gen, device=dev)
    done = torch.rand((T, N), generator=gen, device=dev) < 0.02
    lb, lt = -torch.rand((T, N), generator=gen, device=dev) - 0.1, -torch.rand((T, N), generator=gen, device=dev) - 0.1
    done_u8 = done.view(torch.uint8)
    adv, ret, vs, pg = (torch.empty((T, N), device=dev) for _ in range(4))
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    gl = float(np.float32(GAMMA) * np.float32(LAM))
    bars = (C.c_float * 6)(1.0, 1.0, 1.0, 0.0, 0.0, 0.0)                  # rho_bar, c_bar, pg_rho_bar and their logarithms, as the entry hands them on

    def torch_gae():
        a_next, nxt, rows = torch.zeros_like(last), last, []
        for t in reversed(range(T)):
            live = (~done[t]).float()
            delta = rew[t] + GAMMA * nxt * live - val[t]
            a_next = delta + GAMMA * LAM * a_next * live
            rows.append(a_next)
            nxt = val[t]
        out = torch.stack(rows[::-1])
        return out, out + val

    def torch_vtrace():
        ratio = torch.exp(lt - lb)
        rho, c = ratio.clamp(max=1.0), LAM * ratio.clamp(max=1.0)
        acc, nxt, vs_next, rows, pgs = torch.zeros_like(last), last, last, [], []
        for t in reversed(range(T)):
            live = (~done[t]).float()
            acc = rho[t] * (rew[t] + GAMMA * nxt * live - val[t]) + GAMMA * c[t] * acc * live
            v = val[t] + acc
            pgs.append(rho[t] * (rew[t] + GAMMA * vs_next * live - val[t]))
            rows.append(v)
            nxt, vs_next = val[t], v
        return torch.stack(rows[::-1]), torch.stack(pgs[::-1])

    gae_bytes, vt_bytes = T * N * (4 + 4 + 1 + 8), T * N * (4 * 4 + 1 + 8)
    src, dst = torch.empty((vt_bytes // 2,), dtype=torch.uint8, device=dev), torch.empty((vt_bytes // 2,), dtype=torch.uint8, device=dev)
    variants = {
        "k_gae": lambda: L.rg_gae(None, T, N, P(rew), P(val), P(last), P(done_u8), None, None, GAMMA, LAM, P(adv), P(ret)),
        "k_vtrace": lambda: L.rg_vtrace(None, T, N, P(lb), P(lt), P(rew), P(val), P(last), P(done_u8), None, None, GAMMA, LAM, 1.0, 1.0, 1.0, P(vs), P(pg)),
        "torch_gae": torch_gae, "torch_vtrace": torch_vtrace,
        "copy_gae": lambda: dst[:gae_bytes // 2].copy_(src[:gae_bytes // 2]), "copy_vtrace": lambda: dst.copy_(src),
    }
    # the two paths agree before they are timed, and every variant library answers the product's bits
    variants["k_gae"]()
    variants["k_vtrace"]()
    t_adv, t_ret = torch_gae()
    t_vs, _ = torch_vtrace()
    torch.cuda.synchronize()
    assert float((adv - t_adv).abs().max()) < 1e-3 and float((ret - t_ret).abs().max()) < 1e-3 and float((vs - t_vs).abs().max()) < 1e-3
    for d, e in pairs:
        lib = load_variant(d, e)
        if lib is None:
            continue
        a2, r2 = torch.empty_like(adv), torch.empty_like(ret)
        call = (lambda lib, a2, r2: lambda: lib.rgk_gae(T, N, P(rew), P(val), P(last), P(done_u8), None, None, GAMMA, gl, P(a2), P(r2), None))(lib, a2, r2)
        call()
        torch.cuda.synchronize()
        assert torch.equal(a2.view(torch.int32), adv.view(torch.int32)) and torch.equal(r2.view(torch.int32), ret.view(torch.int32)), (d, e)
        variants["gae_d%de%d" % (d, e)] = call
        v2, p2 = torch.empty_like(vs), torch.empty_like(pg)
        call = (lambda lib, v2, p2: lambda: lib.rgk_vtrace(T, N, P(lb), P(lt), P(rew), P(val), P(last), P(done_u8), None, None, GAMMA, LAM, bars, P(v2), P(p2), None))(lib, v2, p2)
        call()
        torch.cuda.synchronize()
        assert torch.equal(v2.view(torch.int32), vs.view(torch.int32)) and torch.equal(p2.view(torch.int32), pg.view(torch.int32)), (d, e)
        variants["vtrace_d%de%d" % (d, e)] = call
    for fn in variants.values():
        for _ in range(3):
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
    med = {v: statistics.median(us[v]) for v in variants}
    print(json.dumps(dict(steps=T, envs=N, repeats=a.repeats, calls_per_repeat=a.inner, unit="us per call (HIP events)", gae_bytes=gae_bytes, vtrace_bytes=vt_bytes,
                          **{v: spread(us[v]) for v in variants},
                          gae_over_torch=round(med["k_gae"] / med["torch_gae"], 5), vtrace_over_torch=round(med["k_vtrace"] / med["torch_vtrace"], 5),
                          gae_over_copy=round(med["k_gae"] / med["copy_gae"], 3), vtrace_over_copy=round(med["k_vtrace"] / med["copy_vtrace"], 3),
                          gae_TBps=round(gae_bytes / med["k_gae"] * 1e-6, 3), vtrace_TBps=round(vt_bytes / med["k_vtrace"] * 1e-6, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--shapes", default="16x65536,128x65536,128x32768,128x256")
    ap.add_argument("--variants", default="4x1,8x1,32x1,8x2,16x2,4x4,8x4", help="depth x envs per lane of the variant libraries to build or, where built, to time")
    ap.add_argument("--build-variants", action="store_true", help="build the variant libraries (hipcc; no GPU needed) and exit")
    a = ap.parse_args()
    pairs = [tuple(int(v) for v in p.split("x")) for p in a.variants.split(",") if p]
    if a.build_variants:
        build_variants(pairs)
        return
    import __graft_entry__

    __graft_entry__.build()
    for T, N in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
        case(T, N, a, pairs)


if __name__ == "__main__":
    main()
