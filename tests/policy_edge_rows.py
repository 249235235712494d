"""The edge inputs of the policy rule (rogue-gym_amd/csrc/rg_policy.h, rg_policy_grad.h) that the CPU tests hold against independent statements and the GPU tests
push through k_act / k_pg_eval / k_pg_grad: random words whose bit fields stand exactly on a boundary, the weight cut-off pair, gradients that are exact ties
between two subnormal binary16 values, flat rows, and the six logit families with their measured bounds.  Data and pure numpy only: no library is loaded here."""
import numpy as np

import policy_util as pu

# (seed, env, draw) triples whose word (policy_util.word) carries the named 24-bit field, found by search_words() over draw = 0, 1, ... at seed 0 and envs
# 0 .. 255 (1.5e8 words, 5 s): the first six of each in draw order.  The tests re-derive the fields with word() and fields().
#   u = 0x400000, 0x800000, 0xC00000: u * 4 is exactly 1, 2, 3 -- with four equal logits the running sum EQUALS t at keys 0, 1, 2, and `c > t` takes the next one.
#   u = 11184811 = ceil(2/3 * 2^24), odd: u * 3 rounds to exactly 2.0 (three equal logits: action 2); without its lowest bit it is 1.9999999 (action 1).
#   v = 0x400000 = 0.25 and 0x800000 = 0.5: `v < beta` and `v < beta + epsilon` are false AT the bound.
BOUNDARY_WORDS = {
    ("u", 0x400000): [(0, 55, 42461), (0, 137, 60593), (0, 238, 81751), (0, 123, 109119), (0, 38, 211067), (0, 77, 268597)],
    ("u", 0x800000): [(0, 16, 73861), (0, 250, 81718), (0, 253, 91601), (0, 223, 106589), (0, 156, 223198), (0, 104, 280348)],
    ("u", 0xC00000): [(0, 42, 67402), (0, 161, 128620), (0, 143, 147716), (0, 103, 175146), (0, 148, 186578), (0, 102, 252797)],
    ("u", 11184811): [(0, 173, 156), (0, 216, 28725), (0, 151, 86999), (0, 122, 95964), (0, 235, 108040), (0, 153, 127763)],
    ("v", 0x400000): [(0, 170, 42088), (0, 86, 93709), (0, 31, 94861), (0, 107, 163704), (0, 35, 176707), (0, 229, 210220)],
    ("v", 0x800000): [(0, 34, 51384), (0, 36, 139510), (0, 160, 325730), (0, 179, 426125), (0, 153, 486427), (0, 190, 573247)],
}


def search_words(per=6, n_envs=256, chunk=1 << 16):
    """The search that found BOUNDARY_WORDS: {(field, value): [(0, env, draw), ...]}, vectorised over envs x a chunk of draws."""
    found = {k: [] for k in BOUNDARY_WORDS}
    envs = np.arange(n_envs, dtype=np.uint64)
    d0 = 0
    with np.errstate(over="ignore"):
        base = (np.uint64(0x9E3779B97F4A7C15) * (envs + np.uint64(1)) + np.uint64(0xA0761D6478BD642F))[:, None]
        while any(len(v) < per for v in found.values()):
            z = base + np.uint64(0xD1B54A32D192ED03) * np.arange(d0, d0 + chunk, dtype=np.uint64)[None, :]
            z ^= z >> np.uint64(30)
            z *= np.uint64(0xBF58476D1CE4E5B9)
            z ^= z >> np.uint64(27)
            z *= np.uint64(0x94D049BB133111EB)
            z ^= z >> np.uint64(31)
            f = {"u": (z >> np.uint64(40)).astype(np.uint32), "v": ((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.uint32)}
            for (kind, t), lst in found.items():
                if len(lst) < per:
                    lst.extend((0, int(e), int(d0 + d)) for e, d in np.argwhere(f[kind] == t))
            d0 += chunk
    return {k: sorted(v, key=lambda w: w[2])[:per] for k, v in found.items()}


def field_of(kind, seed, env, draw):
    """The 24-bit field `kind` ('u' / 'v') of the word of (seed, env, draw), as an integer."""
    z = pu.word(seed, env, draw)
    return (z >> 40) if kind == "u" else (z >> 16) & 0xFFFFFF


# u words: (number of equal logits, all legal; the action the comment's "first key whose running sum EXCEEDS t" gives), written out by hand:
#   t = u * 4 = 1, 2, 3 exactly and the running sums are 1, 2, 3, 4: the sum that equals t does not exceed it.  t = f32(11184811 * 2^-24 * 3) = f32(2 + 2^-24 * 1) = 2.
U_EXPECT = {0x400000: (4, 1), 0x800000: (4, 2), 0xC00000: (4, 3), 11184811: (3, 2)}
# v words: the (beta, epsilon) pairs under which v stands exactly on a bound, and the source the comment gives there: `v < beta` and `v < beta + epsilon` are
# false at equality, so 0.25 is neither the teacher's (beta 0.25) nor the uniform draw's (epsilon 0.25), and 0.5 is the policy's under 0.25 + 0.25.
V_EXPECT = {0x400000: ((0.25, 0.0, 0), (0.0, 0.25, 0)), 0x800000: ((0.25, 0.25, 0),)}


LOG2E = np.float32(1.4426950216293335)


def cutoff_pair():
    """(d_in, d_out): adjacent negative float32 with f32(d_in * log2 e) >= -125 > f32(d_out * log2 e), from the f32 product itself.  Against a key at 0 the first
    weighs 2^-125 (a finite logp, a gradient that is not zero), the second weighs nothing (logp -inf, gradient +0.0)."""
    d = np.float32(-125.0) / LOG2E
    while np.float32(d * LOG2E) < np.float32(-125.0):
        d = np.nextafter(d, np.float32(0.0))
    while np.float32(np.nextafter(d, np.float32(-np.inf)) * LOG2E) >= np.float32(-125.0):
        d = np.nextafter(d, np.float32(-np.inf))
    out = np.nextafter(d, np.float32(-np.inf))
    assert np.float32(d * LOG2E) >= -125.0 > np.float32(out * LOG2E) and d.dtype == np.float32
    return d, out


# f32 gradients that are exact ties between two subnormal binary16 values (units of 2^-24), with an even and an odd lower neighbour, the tie at 2^-25 between 0
# and the smallest subnormal, the tie under the smallest normal, and both signs; built through g_lp on two equal legal logits: pi = 1/2 exactly, so
# dlogit[0] = g_lp * (1 - 1/2) and dlogit[1] = g_lp * (0 - 1/2) with g_lp = 2 * tie.
TIE_UNITS = (0.5, 1.5, 2.5, 3.5, 100.5, 101.5, 511.5, 512.5, 1022.5, 1023.5)


def tie_values():
    return np.array([s * q * 2.0 ** -24 for q in TIE_UNITS for s in (1.0, -1.0)], np.float32)


FAMILIES = ("uniform [-86, 0]", "normal * 30", "1e6 + normal * 3", "two levels 60 apart", "5 + normal * 1e-6", "normal * 1e-38")
INV_TEMPS = (0.01, 1.0, 7.3, 100.0)


def family_rows(family, rng, n, nk):
    """float32 [n, nk] logits of one of FAMILIES."""
    i = FAMILIES.index(family)
    if i == 0:
        x = rng.uniform(-86.0, 0.0, (n, nk))
    elif i == 1:
        x = rng.standard_normal((n, nk)) * 30
    elif i == 2:
        x = 1e6 + rng.standard_normal((n, nk)) * 3
    elif i == 3:
        x = np.where(rng.randint(0, 2, (n, nk)) == 1, 0.0, -60.0)
    elif i == 4:
        x = 5 + rng.standard_normal((n, nk)) * 1e-6
    else:
        x = rng.standard_normal((n, nk)) * 1e-38      # around the smallest normal float32 (1.18e-38): subnormal logits among them
    return x.astype(np.float32)


# The bounds of test_policy_grad_host.test_accuracy_over_the_domain: the worst figure that test prints over all 24 (family, inv_temp) cells on the CPU, times
# 2 because the sample is finite (the exhaustive sweeps of tests/policy_poly_main.cpp bound the two polynomials; this bounds their composition).
#   logp:     |logp - logp64| / max(1, |logp64|)
#   entropy:  |H - H64|, and H - ln(count)
#   gradient: |dlogits - chain64| / (inv_temp * (|g_lp| + |g_ent| * max(1, |logp64 + H64|))), the largest over the row
# measured: logp 1.86e-7 (1e6 + normal * 3 at inv_temp 1), entropy 3.22e-7 (1e6 + normal * 3 at 0.01), excess 2.78e-7 (5 + normal * 1e-6 at 1), gradient 1.81e-7
MEASURED_DOMAIN = {"logp": 1.86e-7, "entropy": 3.22e-7, "excess": 2.78e-7, "grad": 1.81e-7}


def edge_batch(B, nk=11, seed=0):
    """The rows of the GPU test, float32 [B, nk] with mask, action, g_lp, g_ent: B rows cycling through the six families, the cut-off pair against 0 (inside and
    outside), the binary16 tie gradients on two equal legal logits, and flat rows (every legal logit NaN, every one -inf, a mix) in GIVEN-like use."""
    import policy_grad_util as pg
    rng = np.random.RandomState(seed)
    fam = [family_rows(f, rng, B, nk) for f in FAMILIES]
    x = np.zeros((B, nk), np.float32)
    mask = pg.random_masks(rng, B, nk, lo=1)
    a = np.array([rng.choice(np.flatnonzero(m)) for m in mask], np.int32)
    g_lp, g_ent = rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    d_in, d_out = cutoff_pair()
    ties = tie_values()
    for r in range(B):
        c = r % 12
        if c < 6:
            x[r] = fam[c][r]
        elif c in (6, 7):                                   # one key at 0, the others at the cut-off; the action is one of those
            x[r] = d_in if c == 6 else d_out
            if nk > 1:
                mask[r, :2] = True
                x[r, 0], a[r] = 0.0, 1
        elif c in (8, 9):                                   # two equal legal logits, g_lp = 2 * tie, the entropy term exactly 0
            x[r] = 0.25
            mask[r] = False
            mask[r, :min(2, nk)] = True
            a[r], g_lp[r], g_ent[r] = (r // 12) % min(2, nk), 2 * ties[((r // 12) * 2 + c - 8) % len(ties)], 0.0
        else:                                               # flat: no legal key weighs
            x[r] = (np.nan, -np.inf)[(r // 12) % 2]
            if (r // 24) % 2:
                x[r, ::2] = -np.inf
            x[r, ~mask[r]] = rng.standard_normal(int((~mask[r]).sum())) * 3      # (what the illegal keys hold does not count)
    return x, mask, a, g_lp, g_ent
