"""The learner's side of the action rule (rg_policy_eval / rg_policy_grad, rogue-gym_amd/csrc/rg_policy_grad.hip k_pg_eval and k_pg_grad) against the NaN-safe chain
of torch operations it replaces and against a device-to-device copy of the same byte count.

B = 65 536, 1 048 576 and 8 388 608 rows of 11 keys (8.4 M rows = 128 steps of 65 536 envs), logits f32 and bf16, about 60 % of the keys legal, fixed random
inputs.  One JSON line per (B, dtype), every figure in microseconds per call from HIP events on the stream:

  k_pg_eval        the forward through the C-ABI, every buffer made beforehand: between a call's events stands the launch alone
  k_pg_grad        the backward likewise (both upstream gradients present)
  torch_fwd        lp = log_softmax(logits.masked_fill(~mask, -inf)); logp = lp.gather(a); entropy = -(exp(lp) * lp.masked_fill(~mask, 0)).sum(1)
  torch_fwd_bwd    that and (logp * g_lp + entropy * g_ent).sum().backward()
  masked_logp_fwd_bwd   rogue_gym.masked_logp and the same loss and backward: the two kernels with autograd's bookkeeping around them
  copy_eval, copy_grad  one device-to-device copy of as many bytes as the kernel reads plus as many as it writes, halved (a copy moves every byte twice):
                        the floor of a pass that streams its rows once

--repeats rounds; in each round every variant in turn runs --inner calls (the variants alternate, so drift hits all alike), each call between its own pair of
events; a round's figure is the median of its calls.  Per variant: the median over the rounds and the spread (min, max).

    python tools/bench_policy_grad.py [--repeats 5] [--inner 20] [--rows 65536,1048576,8388608]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rogue-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

NK = 11


def spread(xs, nd=2):
    return dict(median=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd))


def case(B, dtype, a):
    import rogue_gym
    from rogue_gym_python import _rogue_gym as inner
    L = inner.load_library()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    logits = (torch.randn((B, NK), generator=gen, device=dev) * 2).to(dtype)
    mask = torch.rand((B, NK), generator=gen, device=dev) < 0.6
    mask[:, NK - 1] = True                                     # ('s' is always legal)
    act = torch.multinomial(mask.float(), 1, generator=gen)[:, 0].to(torch.int32)
    act64 = act.long()[:, None]
    g_lp, g_ent = torch.randn((B,), generator=gen, device=dev), torch.randn((B,), generator=gen, device=dev)
    logp, ent, dlogits = torch.empty((B,), device=dev), torch.empty((B,), device=dev), torch.empty_like(logits)
    mask_u8 = mask.view(torch.uint8)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    code, esz = inner.ACT_DTYPES[str(dtype).replace("torch.", "")], logits.element_size()
    ninf = float("-inf")
    leaf = logits.clone().requires_grad_()

    def chain(x):
        lp = torch.log_softmax(x.masked_fill(~mask, ninf), 1)
        return lp.gather(1, act64)[:, 0], -(lp.exp() * lp.masked_fill(~mask, 0.0)).sum(1)

    def torch_fwd():
        with torch.no_grad():
            chain(logits)

    def torch_fwd_bwd():
        leaf.grad = None
        lp, e = chain(leaf)
        (lp * g_lp + e * g_ent).sum().backward()

    def ours_fwd_bwd():
        leaf.grad = None
        lp, e = rogue_gym.masked_logp(leaf, act, mask_u8)
        (lp * g_lp + e * g_ent).sum().backward()

    # a copy moves each of its bytes twice: as many bytes as the pass reads and writes together, halved
    eval_bytes, grad_bytes = B * (NK * esz + NK + 4 + 8), B * (NK * esz + NK + 4 + 8 + NK * esz)
    src, dst = torch.empty((grad_bytes // 2,), dtype=torch.uint8, device=dev), torch.empty((grad_bytes // 2,), dtype=torch.uint8, device=dev)
    variants = {
        "k_pg_eval": lambda: L.rg_policy_eval(None, B, NK, P(logits), code, P(mask_u8), P(act), 1.0, P(logp), P(ent)),
        "k_pg_grad": lambda: L.rg_policy_grad(None, B, NK, P(logits), code, P(mask_u8), P(act), 1.0, P(g_lp), P(g_ent), P(dlogits)),
        "torch_fwd": torch_fwd, "torch_fwd_bwd": torch_fwd_bwd, "masked_logp_fwd_bwd": ours_fwd_bwd,
        "copy_eval": lambda: dst[:eval_bytes // 2].copy_(src[:eval_bytes // 2]), "copy_grad": lambda: dst.copy_(src),
    }
    for fn in variants.values():
        for _ in range(3):
            fn()
    # the two paths agree before they are timed
    lp_t, e_t = chain(logits.float())
    L.rg_policy_eval(None, B, NK, P(logits), code, P(mask_u8), P(act), 1.0, P(logp), P(ent))
    torch.cuda.synchronize()
    assert float((logp - lp_t).abs().max()) < 1e-4 and float((ent - e_t).abs().max()) < 1e-4
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
    print(json.dumps(dict(rows=B, keys=NK, logits=str(dtype).replace("torch.", ""), repeats=a.repeats, calls_per_repeat=a.inner, unit="us per call (HIP events)",
                          eval_bytes=eval_bytes, grad_bytes=grad_bytes, **{v: spread(us[v]) for v in variants},
                          pair_over_torch_fwd_bwd=round((med["k_pg_eval"] + med["k_pg_grad"]) / med["torch_fwd_bwd"], 4),
                          eval_over_torch_fwd=round(med["k_pg_eval"] / med["torch_fwd"], 4),
                          eval_over_copy=round(med["k_pg_eval"] / med["copy_eval"], 3), grad_over_copy=round(med["k_pg_grad"] / med["copy_grad"], 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rows", default="65536,1048576,8388608")
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    for B in (int(v) for v in a.rows.split(",")):
        for dtype in (torch.float32, torch.bfloat16):
            case(B, dtype, a)


if __name__ == "__main__":
    main()
