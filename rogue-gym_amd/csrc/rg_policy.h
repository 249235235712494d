// rg_policy.h -- one masked categorical action per env from policy logits (rg_act / rg_act_host): THE statement of the rule.  Host and device: k_act
// (rg_policy.hip, librogue_gym_policy.so) and rgh_act (rg_readers_host.h) both call rg_act_rule, so the rule is written once -- and it is written so that
// the two agree BIT FOR BIT on every output, floats included: a sampled key next to a boundary of the cumulative weights would otherwise differ between
// them.  Hence only integer operations, f32 add / multiply / compare, explicit __builtin_fmaf and ONE f32 division (correctly rounded on both sides); no
// libm, no fast-math intrinsic, contraction off (below), every sum in list order, and no value that could be subnormal.
//
// The legal keys are rg_action_mask.h's (rg_legal_bits, rg_key_bit); the caller hands them over as `row`, bit k = keys[k] is legal now.
//
// LOGITS.  x[k] = widen(logit k) * inv_temp (one f32 multiply; f16 / bf16 widen exactly, by integer operations).  NaN and -inf weigh 0; +inf is FLT_MAX.
//   m = the largest x[k] over the legal keys that weigh; d[k] = x[k] - m <= 0; w[k] = exp2(d[k] * log2 e), and 0 where that argument is below -125 (no
//   subnormal arises; the largest weight is exactly 1).  S = sum of w over the legal keys in list order; pi[k] = w[k] / S, 0 for an illegal key.
//   logp[k] = d[k] - ln S (-inf where w[k] == 0);  entropy = ln S - (sum w[k] * d[k]) / S, not below 0.
//   No legal key weighs: pi is uniform over the `count` legal keys, logp = -ln count, entropy = ln count, and the source is 1.
//   No legal key at all (the Grave modal): action 0, logp 0, entropy 0, source 3 -- keys[0], as rg_action_mask's sample answers.
//
// RANDOMNESS.  One 64-bit word per (seed, env, draw), a splitmix64 finalizer as rg_sample_index_of with a stream constant of its own (RG_ACT_STREAM), so
//   rg_act and rg_action_mask's sample with equal seed and draw are unrelated:
//     z = seed + 0x9E3779B97F4A7C15 * (env + 1) + 0xD1B54A32D192ED03 * draw + RG_ACT_STREAM          (mod 2^64)
//     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
//   bits 63..40  u = field * 2^-24 in [0, 1): the categorical draw.  t = u * S; the first legal key whose running sum of w (list order) exceeds t wins.
//                (t < S always: u <= 1 - 2^-24.  The guard behind the loop answers the last legal key.)
//   bits 39..16  v = field * 2^-24: the source.  v < beta: the teacher key, if it is in the list (its first position) and legal now, else the policy's draw;
//                else v < beta + epsilon (one f32 add): the uniform draw; else the policy's draw.
//   bits 15..0   the uniform draw among the `count` legal keys: the (field * count >> 16)-th of them in list order.
//
// MODES.  RG_ACT_SAMPLE as above.  RG_ACT_GREEDY: the legal key that weighs with the largest x, ties to the lowest index (no key weighs: the lowest legal
//   index, source 1); no draw, no mixing.  RG_ACT_GIVEN: the caller's index, no draw; logp -inf when it is out of range or illegal; source 0.
//   logp and entropy are those of pi whatever chose the action.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rogue_gym_hip.h"
#include "rg_action_mask.h"

#pragma clang fp contract(off)

#define RG_ACT_STREAM 0xA0761D6478BD642Full

struct RgActOut { int32_t action; float logp, entropy; uint32_t source; };

static __host__ __device__ inline float rg_pol_f(uint32_t bits) { return __builtin_bit_cast(float, bits); }
static __host__ __device__ inline uint32_t rg_pol_u(float f) { return __builtin_bit_cast(uint32_t, f); }

// the f32 with the value of a binary16 / bfloat16 bit pattern, exactly (subnormals included); integer operations only
static __host__ __device__ inline float rg_pol_widen(uint32_t h, int dtype) {
    if (dtype == RG_OBS_BF16) return rg_pol_f(h << 16);
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31u) return rg_pol_f(s | 0x7f800000u | (m << 13));
    if (e != 0u) return rg_pol_f(s | ((e + 112u) << 23) | (m << 13));
    if (m == 0u) return rg_pol_f(s);
    const uint32_t sh = (uint32_t)__builtin_clz(m) - 21u;  // m < 2^10: its leading one moves to bit 10
    return rg_pol_f(s | ((113u - sh) << 23) | (((m << sh) & 0x3ffu) << 13));
}
// logit k of a row of `dtype` elements, widened
static __host__ __device__ inline float rg_pol_load(const void *row, int k, int dtype) {
    if (dtype == RG_OBS_F32) return static_cast<const float *>(row)[k];
    return rg_pol_widen(static_cast<const uint16_t *>(row)[k], dtype);
}

// 2^t for -125 <= t <= 0: t = i + f with i = floor(t + 1/2) and |f| <= 1/2 (exact), 2^f = 1 + f * q(f) with q the degree-5 interpolant of (2^f - 1) / f at
// the Chebyshev nodes of [-1/2, 1/2] (3.9e-9 before rounding), and i added into the exponent field.  t = 0 gives exactly 1.  Below -125: 0.
static __host__ __device__ inline float rg_pol_exp2(float t) {
    if (!(t >= -125.0f)) return 0.0f;
    const float h = t + 0.5f;
    int i = (int)h;
    if ((float)i > h) i -= 1;
    const float f = t - (float)i;
    float q = 0.00015453163359779865f;
    q = __builtin_fmaf(q, f, 0.0013390863314270973f);
    q = __builtin_fmaf(q, f, 0.009618083015084267f);
    q = __builtin_fmaf(q, f, 0.055503569543361664f);
    q = __builtin_fmaf(q, f, 0.24022650718688965f);
    q = __builtin_fmaf(q, f, 0.6931471824645996f);
    const float p = __builtin_fmaf(q, f, 1.0f);  // in [0.70, 1.42]
    return rg_pol_f(rg_pol_u(p) + ((uint32_t)i << 23));
}
// ln s for a normal s >= 1: s = 2^e * (1 + u) with the mantissa folded into [sqrt(1/2), sqrt 2), ln(1 + u) = u * q(u) with q the degree-9 interpolant of
// ln(1 + u) / u at the Chebyshev nodes of that interval (1.6e-9 before rounding).  s = 1 gives exactly 0.
static __host__ __device__ inline float rg_pol_ln(float s) {
    const uint32_t b = rg_pol_u(s);
    int e = (int)(b >> 23) - 127;
    uint32_t mant = b & 0x7fffffu;
    uint32_t mb = mant | 0x3f800000u;
    if (mant > 0x3504f3u) { mb = mant | 0x3f000000u; e += 1; }  // above sqrt 2: half of it, one more in the exponent
    const float u = rg_pol_f(mb) - 1.0f;
    float q = -0.07451186329126358f;
    q = __builtin_fmaf(q, u, 0.12806610763072968f);
    q = __builtin_fmaf(q, u, -0.13266031444072723f);
    q = __builtin_fmaf(q, u, 0.14199650287628174f);
    q = __builtin_fmaf(q, u, -0.1660836935043335f);
    q = __builtin_fmaf(q, u, 0.20000939071178436f);
    q = __builtin_fmaf(q, u, -0.2500157952308655f);
    q = __builtin_fmaf(q, u, 0.33333346247673035f);
    q = __builtin_fmaf(q, u, -0.49999988079071045f);
    q = __builtin_fmaf(q, u, 1.0f);
    return __builtin_fmaf((float)e, 0.6931471824645996f, q * u);
}

static __host__ __device__ inline uint64_t rg_act_word(uint64_t seed, uint32_t env, uint64_t draw) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)env + 1ull) + 0xD1B54A32D192ED03ull * draw + RG_ACT_STREAM;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// x[k] of the header comment; `weighs` says whether the key can carry weight
static __host__ __device__ inline float rg_pol_scaled(float logit, float inv_temp, bool &weighs) {
    float x = logit * inv_temp;
    weighs = x == x && x != rg_pol_f(0xff800000u);
    if (x == rg_pol_f(0x7f800000u)) x = rg_pol_f(0x7f7fffffu);
    return x;
}
// the idx-th set bit of row (idx < popcount(row))
static __host__ __device__ inline int rg_pol_nth(uint32_t row, uint32_t idx) {
    for (uint32_t i = 0; i < idx; i++) row &= row - 1;
    return __builtin_ctz(row);
}

// The row's softmax statistics, the part of the rule that the learner's side (rg_policy_grad.h) shares: row != 0.
//   best = where the largest scaled logit among the legal keys that weigh first stands (-1 = none weighs: flat); m = that logit; S and T = the sums of w and
//   w * d in list order; lnS = ln S (flat: ln count); inv = 1 / S, THE division (flat: unused, 0); ent = the entropy, not below 0.
struct RgPolStats { float m, S, T, lnS, inv, ent; int best; bool flat; uint32_t count; };
template <class Fetch>
static __host__ __device__ inline RgPolStats rg_pol_stats(uint32_t row, int n_keys, Fetch fetch, float inv_temp) {
    const float log2e = 1.4426950216293335f;
    const uint32_t count = (uint32_t)__builtin_popcount(row);
    // pass 1: the largest scaled logit among the legal keys that weigh, and where it first stands
    float m = 0.0f;
    int best = -1;
    for (int k = 0; k < n_keys; k++) {
        bool ok;
        const float x = rg_pol_scaled(fetch(k), inv_temp, ok);
        if (((row >> k) & 1u) && ok && (best < 0 || x > m)) { m = x; best = k; }
    }
    const bool flat = best < 0;  // no legal key weighs: the uniform distribution
    // pass 2: S and sum w * d, in list order
    float S = 0.0f, T = 0.0f;
    if (!flat)
        for (int k = 0; k < n_keys; k++) {
            bool ok;
            const float x = rg_pol_scaled(fetch(k), inv_temp, ok);
            if (!(((row >> k) & 1u) && ok)) continue;
            const float d = x - m, w = rg_pol_exp2(d * log2e);
            S = S + w;
            if (w != 0.0f) T = __builtin_fmaf(w, d, T);
        }
    const float lnS = flat ? rg_pol_ln((float)count) : rg_pol_ln(S);
    float ent = lnS, inv = 0.0f;
    if (!flat) {
        inv = 1.0f / S;
        ent = lnS - T * inv;
        if (!(ent > 0.0f)) ent = 0.0f;
    }
    return {m, S, T, lnS, inv, ent, best, flat, count};
}

// One env.  row: bit k = keys[k] is legal (k < n_keys <= 32); fetch(k): logit k widened to f32; teacher: the position of the teacher key in the list, -1 =
// none or not listed; given: the action of RG_ACT_GIVEN.  The options are checked by the caller (rgh_act_opts_check).
template <class Fetch>
static __host__ __device__ inline RgActOut rg_act_rule(uint32_t row, int n_keys, Fetch fetch, const rg_act_opts &o, uint32_t env, int teacher, int given) {
    RgActOut r = {0, 0.0f, 0.0f, 3u};
    if (row == 0u) return r;
    const float ninf = rg_pol_f(0xff800000u), log2e = 1.4426950216293335f;
    const RgPolStats st = rg_pol_stats(row, n_keys, fetch, o.inv_temp);
    const uint32_t count = st.count;
    const float m = st.m, S = st.S, lnS = st.lnS, ent = st.ent;
    const int best = st.best;
    const bool flat = st.flat;
    r.entropy = ent;
    // the action
    const uint64_t z = rg_act_word(o.seed, env, o.draw);
    const int uni = rg_pol_nth(row, (uint32_t)(((z & 0xffffull) * (uint64_t)count) >> 16));
    int a;
    uint32_t src = flat ? 1u : 0u;
    if (o.mode == RG_ACT_GIVEN) {
        a = given;
        src = 0u;
    } else if (o.mode == RG_ACT_GREEDY) {
        a = flat ? __builtin_ctz(row) : best;
    } else {
        int pol = uni;
        if (!flat) {
            const float t = (float)(uint32_t)(z >> 40) * 5.9604644775390625e-08f * S;
            float c = 0.0f;
            pol = -1;
            for (int k = 0; k < n_keys && pol < 0; k++) {
                bool ok;
                const float x = rg_pol_scaled(fetch(k), o.inv_temp, ok);
                if (!(((row >> k) & 1u) && ok)) continue;
                c = c + rg_pol_exp2((x - m) * log2e);
                if (c > t) pol = k;
            }
            if (pol < 0) pol = 31 - __builtin_clz(row);
        }
        const float v = (float)(uint32_t)((z >> 16) & 0xffffffull) * 5.9604644775390625e-08f;
        a = pol;
        if (v < o.beta) {
            if (teacher >= 0 && ((row >> teacher) & 1u)) { a = teacher; src = 2u; }
        } else if (v < o.beta + o.epsilon) {
            a = uni;
            src = 1u;
        }
    }
    r.action = a;
    r.source = src;
    // the log-probability of a under pi
    if (a < 0 || a >= n_keys || !((row >> a) & 1u)) {
        r.logp = ninf;
    } else if (flat) {
        r.logp = 0.0f - lnS;
    } else {
        bool ok;
        const float x = rg_pol_scaled(fetch(a), o.inv_temp, ok);
        const float d = x - m;
        r.logp = (ok && rg_pol_exp2(d * log2e) != 0.0f) ? d - lnS : ninf;
    }
    return r;
}
