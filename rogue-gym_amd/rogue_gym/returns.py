"""Returns and advantages of a [T, N] rollout on the device: GAE(lambda), discounted reward-to-go and V-trace, each ONE kernel launch for the whole rollout
(k_gae, k_vtrace; rogue-gym_amd/csrc/rg_returns.hip) in place of a Python loop over reversed(range(T)), and numpy forms on the host twins.  The rule is
csrc/rg_returns.h's.  `truncated` marks the ends that were time limits (HipVecRogueEnv.time_limit): the episode ended, the state did not, so such a step
bootstraps -- from `trunc_values` where the learner has the value of the state that the rebuild replaced, else from the step's own value.  Stateless: a
learner process needs no env.  The outputs are targets: they carry no autograd."""
import ctypes as C

import numpy as np

from rogue_gym_python import _rogue_gym as inner


def _check(rc):
    if rc:
        raise RuntimeError("Error in rogue-gym: " + inner.load_library().rg_last_error(None).decode())


def _unit(fn, name, v):
    v = float(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError("%s: %s must lie in [0, 1], got %r" % (fn, name, v))
    return v


def _bar(fn, name, v):
    v = float(v)
    if not (v > 0.0 and v < float("inf")):
        raise ValueError("%s: %s must be finite and > 0, got %r" % (fn, name, v))
    return v


def _torch_args(fn, rewards, floats, flags, last_value):
    """The device arguments of one call: `rewards` fixes shape and device; floats = ((name, tensor or None), ...) [T, N]; flags likewise, bool or uint8.
    -> (T, N, device, f32 contiguous tensors or None in the order given, uint8 likewise, last_value f32 [N] or None)."""
    import torch
    if not isinstance(rewards, torch.Tensor) or rewards.dim() != 2 or not rewards.is_cuda or not (rewards.is_floating_point() or rewards.dtype in (torch.int32, torch.int64)):
        raise ValueError("%s: rewards must be a floating-point or integer device tensor [T, N]" % fn)
    shape, dev = tuple(rewards.shape), rewards.device
    out_f, out_b = [], []
    for name, t in (("rewards", rewards),) + tuple(floats):
        if t is None:
            out_f.append(None)
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.device != dev or not (t.is_floating_point() or t.dtype in (torch.int32, torch.int64)):
            raise ValueError("%s: %s must be a floating-point tensor %s on %s" % (fn, name, list(shape), dev))
        out_f.append(t.detach().to(torch.float32).contiguous())
    for name, t in flags:
        if t is None:
            out_b.append(None)
            continue
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.bool, torch.uint8) or tuple(t.shape) != shape or t.device != dev:
            raise ValueError("%s: %s must be a bool / uint8 tensor %s on %s" % (fn, name, list(shape), dev))
        t = t.detach().contiguous()
        out_b.append(t.view(torch.uint8) if t.dtype == torch.bool else t)
    if last_value is not None:
        if not isinstance(last_value, torch.Tensor) or tuple(last_value.shape) != shape[1:] or last_value.device != dev or not last_value.is_floating_point():
            raise ValueError("%s: last_value must be a floating-point tensor %s on %s" % (fn, list(shape[1:]), dev))
        last_value = last_value.detach().to(torch.float32).contiguous()
    return shape[0], shape[1], dev, out_f, out_b, last_value


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _trunc_pair(fn, truncated, trunc_values):
    if trunc_values is not None and truncated is None:
        raise ValueError("%s: trunc_values needs truncated" % fn)


def gae(rewards, values, dones, last_value=None, gamma=0.99, lam=0.95, truncated=None, trunc_values=None):
    """(advantages, returns), float32 [T, N] on the inputs' device: generalised advantage estimation over a time-major rollout in one kernel launch.
    rewards, values [T, N] (values may be None: 0); dones, truncated [T, N] bool or uint8 (None: never); last_value [N], the value of the state after the
    last step (None: 0); trunc_values [T, N], the value of the state a time-limit end cut off, looked at where `truncated` is set (None: that step's own
    value).  Inputs are detached, converted to float32 and made contiguous where needed; the outputs carry no autograd.  It runs on torch's current stream."""
    import torch
    _trunc_pair("gae", truncated, trunc_values)
    gamma, lam = _unit("gae", "gamma", gamma), _unit("gae", "lam", lam)
    T, N, dev, (r, v, tv), (d, tr), lv = _torch_args("gae", rewards, (("values", values), ("trunc_values", trunc_values)), (("dones", dones), ("truncated", truncated)), last_value)
    with torch.cuda.device(dev):
        adv, ret = torch.empty((T, N), dtype=torch.float32, device=dev), torch.empty((T, N), dtype=torch.float32, device=dev)
        if T and N:
            _check(inner.load_library().rg_gae(C.c_void_p(torch.cuda.current_stream().cuda_stream), T, N, _ptr(r), _ptr(v), _ptr(lv), _ptr(d), _ptr(tr), _ptr(tv), gamma, lam,
                                               _ptr(adv), _ptr(ret)))
    return adv, ret


def discounted_returns(rewards, dones, last_value=None, gamma=0.99, truncated=None, trunc_values=None):
    """returns, float32 [T, N]: the discounted reward-to-go of every step, bootstrapped from last_value [N] (None: 0) and, at a time-limit end, from
    trunc_values (None: 0) -- gae without values and with lam = 1, one kernel launch."""
    import torch
    _trunc_pair("discounted_returns", truncated, trunc_values)
    gamma = _unit("discounted_returns", "gamma", gamma)
    T, N, dev, (r, tv), (d, tr), lv = _torch_args("discounted_returns", rewards, (("trunc_values", trunc_values),), (("dones", dones), ("truncated", truncated)), last_value)
    with torch.cuda.device(dev):
        ret = torch.empty((T, N), dtype=torch.float32, device=dev)
        if T and N:
            _check(inner.load_library().rg_gae(C.c_void_p(torch.cuda.current_stream().cuda_stream), T, N, _ptr(r), None, _ptr(lv), _ptr(d), _ptr(tr), _ptr(tv), gamma, 1.0,
                                               None, _ptr(ret)))
    return ret


def vtrace(logp_behaviour, logp_target, rewards, values, dones, last_value=None, gamma=0.99, lam=1.0, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, truncated=None,
           trunc_values=None):
    """(vs, pg_advantages), float32 [T, N]: the V-trace value targets and policy-gradient advantages (Espeholt et al. 2018, lambda as in rlax) in one kernel
    launch.  logp_behaviour is what `env.act` recorded, logp_target what `rogue_gym.masked_logp` gives under the learner's weights; the importance ratio
    exp(logp_target - logp_behaviour) is clipped at rho_bar, c_bar and pg_rho_bar.  On unchanged weights and bars of 1, vs equals gae's returns bit for bit.
    The other arguments are gae's; `values` is required."""
    import torch
    _trunc_pair("vtrace", truncated, trunc_values)
    gamma, lam = _unit("vtrace", "gamma", gamma), _unit("vtrace", "lam", lam)
    bars = [_bar("vtrace", n, b) for n, b in (("rho_bar", rho_bar), ("c_bar", c_bar), ("pg_rho_bar", pg_rho_bar))]
    if values is None:
        raise ValueError("vtrace: values must be a floating-point tensor [T, N]")
    T, N, dev, (r, lb, lt, v, tv), (d, tr), lv = _torch_args(
        "vtrace", rewards, (("logp_behaviour", logp_behaviour), ("logp_target", logp_target), ("values", values), ("trunc_values", trunc_values)),
        (("dones", dones), ("truncated", truncated)), last_value)
    if lb is None or lt is None:
        raise ValueError("vtrace: logp_behaviour and logp_target must be floating-point tensors [T, N]")
    with torch.cuda.device(dev):
        vs, pg = torch.empty((T, N), dtype=torch.float32, device=dev), torch.empty((T, N), dtype=torch.float32, device=dev)
        if T and N:
            _check(inner.load_library().rg_vtrace(C.c_void_p(torch.cuda.current_stream().cuda_stream), T, N, _ptr(lb), _ptr(lt), _ptr(r), _ptr(v), _ptr(lv), _ptr(d), _ptr(tr),
                                                  _ptr(tv), gamma, lam, bars[0], bars[1], bars[2], _ptr(vs), _ptr(pg)))
    return vs, pg


def _np_args(fn, rewards, floats, flags, last_value):
    rewards = np.asarray(rewards)
    if rewards.ndim != 2 or rewards.dtype.kind not in "fiu":
        raise ValueError("%s: rewards must be a numeric array [T, N], got %s %s" % (fn, rewards.shape, rewards.dtype))
    shape = rewards.shape
    out_f, out_b = [], []
    for name, a in (("rewards", rewards),) + tuple(floats):
        if a is None:
            out_f.append(None)
            continue
        a = np.asarray(a)
        if a.shape != shape or a.dtype.kind not in "fiu":
            raise ValueError("%s: %s must be a numeric array %s, got %s %s" % (fn, name, shape, a.shape, a.dtype))
        out_f.append(np.ascontiguousarray(a, dtype=np.float32))
    for name, a in flags:
        if a is None:
            out_b.append(None)
            continue
        a = np.asarray(a)
        if a.shape != shape or a.dtype not in (np.bool_, np.uint8):
            raise ValueError("%s: %s must be a bool / uint8 array %s, got %s %s" % (fn, name, shape, a.shape, a.dtype))
        out_b.append(np.ascontiguousarray(a).view(np.uint8))
    if last_value is not None:
        last_value = np.asarray(last_value)
        if last_value.shape != shape[1:] or last_value.dtype.kind != "f":
            raise ValueError("%s: last_value must be a floating-point array %s, got %s %s" % (fn, shape[1:], last_value.shape, last_value.dtype))
        last_value = np.ascontiguousarray(last_value, dtype=np.float32)
    return shape[0], shape[1], out_f, out_b, last_value


def _P(a):
    return None if a is None else a.ctypes.data


def gae_np(rewards, values, dones, last_value=None, gamma=0.99, lam=0.95, truncated=None, trunc_values=None):
    """(advantages, returns): the numpy form of gae on the host twin (rg_gae_host) -- the same rule, bit for bit what the device call gives."""
    _trunc_pair("gae_np", truncated, trunc_values)
    gamma, lam = _unit("gae_np", "gamma", gamma), _unit("gae_np", "lam", lam)
    T, N, (r, v, tv), (d, tr), lv = _np_args("gae_np", rewards, (("values", values), ("trunc_values", trunc_values)), (("dones", dones), ("truncated", truncated)), last_value)
    adv, ret = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32)
    _check(inner.load_library().rg_gae_host(T, N, _P(r), _P(v), _P(lv), _P(d), _P(tr), _P(tv), gamma, lam, _P(adv), _P(ret)))
    return adv, ret


def discounted_returns_np(rewards, dones, last_value=None, gamma=0.99, truncated=None, trunc_values=None):
    """returns: the numpy form of discounted_returns on the host twin."""
    _trunc_pair("discounted_returns_np", truncated, trunc_values)
    gamma = _unit("discounted_returns_np", "gamma", gamma)
    T, N, (r, tv), (d, tr), lv = _np_args("discounted_returns_np", rewards, (("trunc_values", trunc_values),), (("dones", dones), ("truncated", truncated)), last_value)
    ret = np.zeros((T, N), np.float32)
    _check(inner.load_library().rg_gae_host(T, N, _P(r), None, _P(lv), _P(d), _P(tr), _P(tv), gamma, 1.0, None, _P(ret)))
    return ret


def vtrace_np(logp_behaviour, logp_target, rewards, values, dones, last_value=None, gamma=0.99, lam=1.0, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, truncated=None,
              trunc_values=None):
    """(vs, pg_advantages): the numpy form of vtrace on the host twin (rg_vtrace_host)."""
    _trunc_pair("vtrace_np", truncated, trunc_values)
    gamma, lam = _unit("vtrace_np", "gamma", gamma), _unit("vtrace_np", "lam", lam)
    bars = [_bar("vtrace_np", n, b) for n, b in (("rho_bar", rho_bar), ("c_bar", c_bar), ("pg_rho_bar", pg_rho_bar))]
    if values is None or logp_behaviour is None or logp_target is None:
        raise ValueError("vtrace_np: logp_behaviour, logp_target and values must be numeric arrays [T, N]")
    T, N, (r, lb, lt, v, tv), (d, tr), lv = _np_args(
        "vtrace_np", rewards, (("logp_behaviour", logp_behaviour), ("logp_target", logp_target), ("values", values), ("trunc_values", trunc_values)),
        (("dones", dones), ("truncated", truncated)), last_value)
    vs, pg = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32)
    _check(inner.load_library().rg_vtrace_host(T, N, _P(lb), _P(lt), _P(r), _P(v), _P(lv), _P(d), _P(tr), _P(tv), gamma, lam, bars[0], bars[1], bars[2], _P(vs), _P(pg)))
    return vs, pg
