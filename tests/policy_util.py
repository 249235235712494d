"""Helpers of the rg_act tests: the host twin through ctypes, the random word of rogue-gym_amd/csrc/rg_policy.h in Python integers, a float64 masked softmax,
and the logit rows with the special values."""
import ctypes as C

import numpy as np

KEYS = b".hjklnbuy>s"
ALL_KEYS = b".hjklnbuy>sHJKLNBUY"                     # every key of KeyMap::ai, run keys included
LISTS = [b"s", b"hl>.j", None, ALL_KEYS, (KEYS * 3)[:32]]   # 1, 5, 11 (the default list), 19 and RG_MASK_MAX_KEYS keys
FLOOR, WALL, STAIR = 1, 2, 4
SAMPLE, GREEDY, GIVEN = 0, 1, 2
M64 = (1 << 64) - 1
DT = {np.dtype(np.float32): 0, np.dtype(np.float16): 1}
BF16 = 2


def grid5(**cells):
    """5 x 5 of floor with the named cells replaced: grid5(x2y1=WALL)."""
    g = np.full((5, 5), FLOOR, np.uint16)
    for name, v in cells.items():
        g[int(name[3]), int(name[1])] = v
    return g


def opts_of(inner, mode=SAMPLE, inv_temp=1.0, epsilon=0.0, beta=0.0, seed=0, draw=0):
    return inner.RgActOpts(inv_temp, epsilon, beta, mode, seed & M64, draw & M64)


def to_bf16(x):
    """float32 -> the bfloat16 bit patterns, round to nearest even (uint16)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def act_host(lib, inner, g, px, py, logits, keys=None, dead=0, env=0, teacher=-1, given=0, dtype=None, **o):
    """rg_act_host for one env -> (key, action, logp, entropy, source); logits float32 / float16, or uint16 bfloat16 patterns with dtype=BF16."""
    logits = np.ascontiguousarray(logits)
    dtype = DT[logits.dtype] if dtype is None else dtype
    nk = len(KEYS) if keys is None else len(keys)
    assert logits.shape == (nk,)
    key, src, act, lp, ent = C.c_uint8(0xAA), C.c_uint8(0xAA), C.c_int32(-7), C.c_float(7.0), C.c_float(7.0)
    opts = opts_of(inner, **o)
    rc = lib.rg_act_host(g.ctypes.data, g.shape[0], g.shape[1], px, py, dead, keys, nk, logits.ctypes.data, dtype, C.byref(opts), env, teacher, given,
                         C.byref(key), C.byref(act), C.byref(lp), C.byref(ent), C.byref(src))
    assert rc == 0, lib.rg_last_error(None).decode()
    return key.value, act.value, np.float32(lp.value), np.float32(ent.value), src.value


def word(seed, env, draw):
    """The random word of (seed, env, draw): rg_policy.h's splitmix64 finalizer with its stream constant."""
    z = (seed + 0x9E3779B97F4A7C15 * (env + 1) + 0xD1B54A32D192ED03 * draw + 0xA0761D6478BD642F) & M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def fields(z):
    """(categorical u in [0, 1), source v in [0, 1), the 16 bits of the uniform index)."""
    return (z >> 40) / float(1 << 24), ((z >> 16) & 0xFFFFFF) / float(1 << 24), z & 0xFFFF


def softmax64(x, legal):
    """float64 masked log-softmax and entropy of one row (x float32 finite, legal bool)."""
    x = np.asarray(x, np.float64)
    m = x[legal].max()
    lse = m + np.log(np.exp(x[legal] - m).sum())
    lp = np.where(legal, x - lse, -np.inf)
    p = np.exp(lp)
    return lp, float(-(p[legal] * lp[legal]).sum())


def special_rows(rng, n, nk):
    """float32 [n, nk] of normal * 3 logits whose rows cycle through: plain, a NaN, a -inf, a +inf, all -inf, +80 against -80, all NaN, huge finite values."""
    x = (rng.standard_normal((n, nk)) * 3).astype(np.float32)
    for e in range(n):
        c, k = e % 8, rng.randint(nk)
        if c == 1:
            x[e, k] = np.nan
        elif c == 2:
            x[e, k] = -np.inf
        elif c == 3:
            x[e, k] = np.inf
        elif c == 4:
            x[e, :] = -np.inf
        elif c == 5:
            x[e, :] = -80.0
            x[e, k] = 80.0
        elif c == 6:
            x[e, :] = np.nan
        elif c == 7:
            x[e, k] = 3.0e38
            x[e, (k + 1) % nk] = -3.0e38
    return x
