"""Helpers of the rg_policy_eval / rg_policy_grad tests: the host twins through ctypes, the float64 NaN-safe torch chain that is the reference of the
gradient, round-to-nearest-even to binary16 / bfloat16 in Python integers, and the row sets the CPU and the GPU tests share."""
import ctypes as C
from fractions import Fraction

import numpy as np

import policy_util as pu

F32, F16, BF16 = 0, 1, 2
# The largest |difference| of the f32 gradient between the host rule and the float64 chain over the 10 000 rows of
# test_policy_grad_host.test_gradient_accuracy_against_the_float64_chain (normal * 3 logits, 1 to 11 legal keys, normal g_lp and g_ent), measured on the CPU.
# A gradient is g * (a few roundings of pi, logp and H): with |g| up to 4 and logp + H up to 25, a few f32 ulps of those.  The tests assert four times it,
# rg_act's own margin for logp: the sample is finite and the polynomials' worst case need not be in it.
MEASURED_GRAD = 6.58e-7


def widen(x, dtype):
    """float32 values of an array of logits: float32 / float16 as they are, uint16 bfloat16 patterns shifted up."""
    x = np.asarray(x)
    return (x.astype(np.uint32) << 16).view(np.float32) if dtype == BF16 else x.astype(np.float32)


def eval_host(lib, x, dtype, mask, a, inv_temp=1.0, want=(True, True)):
    """rg_policy_eval_host -> (logp, entropy) float32 [B] (None where not wanted); x [B, nk] float32 / float16 / uint16 (bf16 patterns)."""
    x = np.ascontiguousarray(x)
    B, nk = x.shape
    a = np.ascontiguousarray(a, np.int32)
    m = None if mask is None else np.ascontiguousarray(mask).view(np.uint8)
    out = [np.full(B, 7.0, np.float32) if w else None for w in want]
    rc = lib.rg_policy_eval_host(B, nk, x.ctypes.data, dtype, None if m is None else m.ctypes.data, a.ctypes.data, inv_temp, *(None if o is None else o.ctypes.data for o in out))
    assert rc == 0, lib.rg_last_error(None).decode()
    return out


def grad_host(lib, x, dtype, mask, a, g_lp, g_ent, inv_temp=1.0):
    """rg_policy_grad_host -> dlogits [B, nk] in the dtype of x."""
    x = np.ascontiguousarray(x)
    B, nk = x.shape
    a = np.ascontiguousarray(a, np.int32)
    m = None if mask is None else np.ascontiguousarray(mask).view(np.uint8)
    g = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (g_lp, g_ent)]
    dx = np.full_like(x, 0x5A5A if x.dtype == np.uint16 else 7.0)
    rc = lib.rg_policy_grad_host(B, nk, x.ctypes.data, dtype, None if m is None else m.ctypes.data, a.ctypes.data, inv_temp, *(None if v is None else v.ctypes.data for v in g),
                                 dx.ctypes.data)
    assert rc == 0, lib.rg_last_error(None).decode()
    return dx


def chain64(x, mask, a, g_lp, g_ent, inv_temp=1.0):
    """The float64 NaN-safe torch chain on the CPU: (logp, entropy, d(sum g_lp * logp + g_ent * entropy) / dx) as float64 numpy arrays.  x finite float32 [B, nk],
    mask bool with at least one legal key per row, a legal."""
    import torch
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    mt = torch.tensor(np.asarray(mask, bool))
    lp = torch.log_softmax((xt * float(inv_temp)).masked_fill(~mt, -float("inf")), 1)
    ent = -(lp.exp() * lp.masked_fill(~mt, 0.0)).sum(1)
    la = lp.gather(1, torch.tensor(np.asarray(a, np.int64))[:, None])[:, 0]
    loss = 0.0
    if g_lp is not None:
        loss = loss + (la * torch.tensor(np.asarray(g_lp, np.float64))).sum()
    if g_ent is not None:
        loss = loss + (ent * torch.tensor(np.asarray(g_ent, np.float64))).sum()
    loss.backward()
    return la.detach().numpy(), ent.detach().numpy(), xt.grad.numpy()


def rne16(bits32, dtype):
    """The binary16 (F16) / bfloat16 (BF16) bit pattern nearest to the float32 with the bits `bits32`, ties to even, in Python integers and fractions."""
    ebits, mbits = (5, 10) if dtype == F16 else (8, 7)
    bias, emax = (1 << (ebits - 1)) - 1, (1 << ebits) - 1
    s, e, m = bits32 >> 31, (bits32 >> 23) & 0xFF, bits32 & 0x7FFFFF
    sign = s << (ebits + mbits)
    if e == 0xFF:
        return (emax << mbits) | (1 << (mbits - 1)) if m else sign | (emax << mbits)   # the canonical quiet NaN has no sign
    v = Fraction(m, 1 << 23) * Fraction(2) ** -126 if e == 0 else (1 + Fraction(m, 1 << 23)) * Fraction(2) ** (e - 127)
    if v == 0:
        return sign
    ex = e - 127 if e else -127                       # floor(log2 v) for a normal float32 (a subnormal is far below either type's range or is bf16's own)
    while Fraction(2) ** ex > v:
        ex -= 1
    while Fraction(2) ** (ex + 1) <= v:
        ex += 1
    q = Fraction(2) ** (max(ex, 1 - bias) - mbits)    # the spacing of the target type at v
    n = v / q
    lo = n.numerator // n.denominator
    r = n - lo
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and lo & 1):
        lo += 1
    # lo * q is the rounded value: lo < 2^mbits = subnormal, else 2^mbits <= lo <= 2^(mbits + 1)
    if lo < (1 << mbits):
        return sign | lo
    et = max(ex, 1 - bias) + bias
    if lo == (1 << (mbits + 1)):
        lo, et = 1 << mbits, et + 1
    if et >= emax:
        return sign | (emax << mbits)
    return sign | (et << mbits) | (lo - (1 << mbits))


def random_masks(rng, B, nk, lo=0):
    """bool [B, nk]: row r has between `lo` and nk legal keys, every count taken."""
    mask = np.zeros((B, nk), bool)
    for r in range(B):
        c = lo + (r % (nk + 1 - lo))
        mask[r, rng.permutation(nk)[:c]] = True
    return mask


def actions_for(rng, mask):
    """int32 [B]: mostly a legal key of the row; every sixteenth row (a plain row of special_rows) one of -1, nk, an illegal key and the ends of int32."""
    B, nk = mask.shape
    a = np.zeros(B, np.int32)
    for r in range(B):
        legal, illegal = np.flatnonzero(mask[r]), np.flatnonzero(~mask[r])
        if r % 16 == 8 or len(legal) == 0:
            a[r] = (-1, nk, int(illegal[0]) if len(illegal) else nk + 7, -2 ** 31, 2 ** 31 - 1)[(r // 16) % 5]
        else:
            a[r] = int(rng.choice(legal))
    return a


def typed_rows(rng, B, nk, dtype):
    """Logit rows with section 23's special values (policy_util.special_rows) in `dtype`: float32, float16, or uint16 bfloat16 patterns."""
    x = pu.special_rows(rng, B, nk)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16)
    return pu.to_bf16(x) if dtype == BF16 else x


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view({2: np.uint16, 4: np.uint32}[v.dtype.itemsize])


_ = C
