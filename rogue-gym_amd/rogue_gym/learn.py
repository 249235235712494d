"""The learner's side of HipVecRogueEnv.act: the log-probability of stored actions and the entropy under stored masks for any number of rows of logits, with a
backward pass -- two HIP kernels (k_pg_eval, k_pg_grad; rogue-gym_amd/csrc/rg_policy_grad.hip) behind one torch.autograd.Function, and a numpy form on the
host twins.  The rule is csrc/rg_policy_grad.h's: the forward is bit for bit what `act` answered for the same logits, mask and action, so the importance
ratio exp(logp_new - logp_old) of a first epoch on unchanged weights is exactly 1.  Stateless: a learner process needs no env."""
import ctypes as C

import numpy as np

from rogue_gym_python import _rogue_gym as inner

_FN = None


def _inv_temp(temperature):
    temperature = float(temperature)
    if not temperature > 0.0:
        raise ValueError("temperature must be > 0, got %r" % (temperature,))
    return float(np.float32(1.0) / np.float32(temperature))   # (the f32 division `act` makes)


def _check(rc):
    if rc:
        raise RuntimeError("Error in rogue-gym: " + inner.load_library().rg_last_error(None).decode())


def _function():
    """The autograd.Function, made on first use (importing this module needs no torch)."""
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from torch.autograd.function import once_differentiable

    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    class MaskedLogp(torch.autograd.Function):
        # x [B, nk] contiguous f32 / f16 / bf16, a int32 [B] contiguous, m uint8 [B, nk] contiguous or None: masked_logp made them
        @staticmethod
        def forward(ctx, x, a, m, inv_temp):
            B, nk = x.shape
            with torch.cuda.device(x.device):
                logp = torch.empty((B,), dtype=torch.float32, device=x.device)
                ent = torch.empty((B,), dtype=torch.float32, device=x.device)
                if B:
                    _check(inner.load_library().rg_policy_eval(C.c_void_p(torch.cuda.current_stream().cuda_stream), B, nk, ptr(x),
                                                               inner.ACT_DTYPES[str(x.dtype).replace("torch.", "")],
                                                               ptr(m), ptr(a), inv_temp, ptr(logp), ptr(ent)))
            ctx.save_for_backward(x, a, *(() if m is None else (m,)))   # the inputs alone: backward recomputes
            ctx.inv_temp = inv_temp
            ctx.set_materialize_grads(False)   # an output that the loss never used arrives as None, not as zeros: the kernel then gets NULL for it
            return logp, ent

        @staticmethod
        @once_differentiable
        def backward(ctx, g_lp, g_ent):
            if not ctx.needs_input_grad[0]:
                return None, None, None, None
            x, a = ctx.saved_tensors[:2]
            m = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
            B, nk = x.shape
            with torch.cuda.device(x.device):
                g_lp, g_ent = (None if g is None else g.to(torch.float32).contiguous() for g in (g_lp, g_ent))
                dx = torch.empty_like(x)
                if B:
                    _check(inner.load_library().rg_policy_grad(C.c_void_p(torch.cuda.current_stream().cuda_stream), B, nk, ptr(x),
                                                               inner.ACT_DTYPES[str(x.dtype).replace("torch.", "")],
                                                               ptr(m), ptr(a), ctx.inv_temp, ptr(g_lp), ptr(g_ent), ptr(dx)))
            return dx, None, None, None

    _FN = MaskedLogp
    return _FN


def masked_logp(logits, actions, mask=None, temperature=1.0):
    """(logp, entropy), float32 tensors [...] on the device: ln pi(actions) and the entropy in nats of pi = the softmax of logits / temperature over the keys
    that `mask` calls legal -- the rule of HipVecRogueEnv.act, bit for bit what it answered for the same logits, mask and actions.  Differentiable with
    respect to `logits` (first derivatives), one kernel forward and one backward whatever the number of rows.
    logits: [..., n_keys] float32, float16 or bfloat16 on a HIP device, n_keys <= 32; actions: an integer tensor [...]; mask: bool or uint8 [..., n_keys],
    what `env.action_mask` holds and a rollout buffer stores (None: every key is legal).  Contiguous copies are made where needed; the gradient comes back in
    the layout and dtype of `logits`.  An illegal key has probability 0 and gradient exactly 0; an illegal or out-of-range action has logp -inf and sends
    no gradient through logp.  It runs on torch's current stream and device."""
    import torch
    if not isinstance(logits, torch.Tensor) or logits.dtype not in (torch.float32, torch.float16, torch.bfloat16) or logits.dim() < 1 or not logits.is_cuda:
        raise ValueError("masked_logp: logits must be a float32 / float16 / bfloat16 device tensor [..., n_keys]")
    lead, nk = tuple(logits.shape[:-1]), int(logits.shape[-1])
    if not isinstance(actions, torch.Tensor) or actions.is_floating_point() or actions.dtype == torch.bool or tuple(actions.shape) != lead or actions.device != logits.device:
        raise ValueError("masked_logp: actions must be an integer tensor %s on %s" % (list(lead), logits.device))
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != tuple(logits.shape)
                             or mask.device != logits.device):
        raise ValueError("masked_logp: mask must be a bool / uint8 tensor %s on %s" % (list(logits.shape), logits.device))
    inv_temp = _inv_temp(temperature)
    x = logits.reshape(-1, nk).contiguous()        # (autograd carries the gradient back through these to `logits` as it is laid out)
    a = actions.reshape(-1).to(torch.int32).contiguous()
    m = None if mask is None else mask.reshape(-1, nk).contiguous()
    if m is not None and m.dtype == torch.bool:
        m = m.view(torch.uint8)
    logp, ent = _function().apply(x, a, m, inv_temp)
    return logp.reshape(lead), ent.reshape(lead)


def masked_logp_np(logits, actions, mask=None, temperature=1.0):
    """(logp, entropy, grad_fn): the value form of masked_logp on the host twins (rg_policy_eval_host, rg_policy_grad_host), for RogueEnv / ParallelRogueEnv
    users and for tests -- the same rule, bit for bit what the device call gives.  logits: a numpy array [..., n_keys] of float32 or float16; actions: integers
    [...]; mask: bool / uint8 [..., n_keys] or None.  logp and entropy are float32 [...]; grad_fn(g_logp=None, g_entropy=None) -> the gradient of
    sum(g_logp * logp + g_entropy * entropy) with respect to logits, in their shape and dtype (an absent upstream gradient counts as 0)."""
    L = inner.load_library()
    logits = np.asarray(logits)
    if logits.dtype not in (np.float32, np.float16) or logits.ndim < 1:
        raise ValueError("masked_logp_np: logits must be a float32 / float16 array [..., n_keys], got %s %s" % (logits.shape, logits.dtype))
    lead, nk = logits.shape[:-1], logits.shape[-1]
    x = np.ascontiguousarray(logits.reshape(-1, nk))
    a = np.ascontiguousarray(np.asarray(actions).reshape(-1), dtype=np.int32)
    if np.asarray(actions).shape != lead:
        raise ValueError("masked_logp_np: actions must have the shape %s, got %s" % (lead, np.asarray(actions).shape))
    m = None
    if mask is not None:
        mask = np.asarray(mask)
        if mask.dtype not in (np.bool_, np.uint8) or mask.shape != logits.shape:
            raise ValueError("masked_logp_np: mask must be a bool / uint8 array %s, got %s %s" % (logits.shape, mask.shape, mask.dtype))
        m = np.ascontiguousarray(mask.reshape(-1, nk)).view(np.uint8)
    inv_temp, dtype, B = _inv_temp(temperature), inner.ACT_DTYPES[x.dtype.name], x.shape[0]
    P = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    logp, ent = np.zeros(B, np.float32), np.zeros(B, np.float32)
    _check(L.rg_policy_eval_host(B, nk, P(x), dtype, P(m), P(a), inv_temp, P(logp), P(ent)))

    def grad_fn(g_logp=None, g_entropy=None):
        g = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), lead).reshape(-1)) for v in (g_logp, g_entropy)]
        dx = np.zeros_like(x)
        _check(L.rg_policy_grad_host(B, nk, P(x), dtype, P(m), P(a), inv_temp, P(g[0]), P(g[1]), P(dx)))
        return dx.reshape(logits.shape)

    return logp.reshape(lead), ent.reshape(lead), grad_fn
