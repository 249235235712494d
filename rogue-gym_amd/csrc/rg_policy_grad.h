// rg_policy_grad.h -- the learner's side of rg_policy.h's rule: the log-probability of a STORED action and the entropy under a STORED mask for one row of
// logits, and their gradient with respect to that row (rg_policy_eval / rg_policy_grad and their host twins): THE statement.  Host and device: k_pg_eval and
// k_pg_grad (rg_policy_grad.hip, librogue_gym_learn.so) and rgh_policy_eval / rgh_policy_grad (rg_readers_host.h) call the two functions below, and agree
// bit for bit.  rg_policy.h's discipline holds: integer operations, f32 add / multiply / compare, explicit __builtin_fmaf, ONE f32 division per row (inside
// rg_pol_stats), no libm, no fast-math intrinsic, contraction off, sums in list order.
//
// FORWARD.  rg_pg_eval_rule IS rg_act_rule in RG_ACT_GIVEN mode with the row's legal word and action: what rg_act answered for the same logits, mask and
//   action, bit for bit (no legal key: logp 0, entropy 0; an action out of range or illegal: logp -inf).
//
// BACKWARD, for upstream g_lp and g_ent (an absent one: its term is +0.0).  With x, m, d, w, S, ln S, inv = 1 / S and the entropy H exactly as
//   rg_pol_stats computes them (H after its clamp at 0), for every LEGAL key k that WEIGHS (w[k] != 0), in list order:
//       pi = w[k] * inv                         lp = d[k] - lnS
//       t1 = g_lp * (i - pi)                    i = 1.0 for k == a, else 0.0;  t1 = +0.0 when g_lp is absent or the action does not count (below)
//       t2 = g_ent * (pi * (lp + H))            t2 = +0.0 when g_ent is absent
//       dlogit[k] = inv_temp * (t1 - t2)
//   and dlogit[k] = +0.0 for every other key: an illegal one, a NaN or -inf logit, a weight that underflowed to 0.
//   (d logp[a] / d logit[k] = inv_temp * ([k == a] - pi[k]);  d H / d logit[k] = -inv_temp * pi[k] * (logp[k] + H).)
//   w[k] is recomputed by rg_pol_exp2, a pure function of d[k]: the same bits as in the sums.
// EDGE CASES.
//   A flat row (no legal key weighs: pi is uniform whatever the logits) and a row with no legal key: every gradient is +0.0.
//   The action does not count when it is out of range, illegal or weightless (logp = -inf): the g_lp term is +0.0 for the whole row, g_lp is not looked at,
//   and the entropy term still flows.
//   +inf is FLT_MAX, as in the forward: it stands at d = 0 and every finite key below it weighs 0.
//   A NaN result (a NaN or infinite upstream gradient) is written as the canonical quiet NaN 0x7fc00000, so host and device bit patterns agree.
//   The result is f32; for f16 / bf16 logits it is rounded to that type, to nearest even, by integer operations (rg_pol_narrow, the inverse of rg_pol_widen).
#pragma once
#include "rg_policy.h"

#pragma clang fp contract(off)

// the binary16 / bfloat16 bit pattern nearest to f, ties to even; NaN is the canonical quiet NaN of the type; integer operations only
static __host__ __device__ inline uint32_t rg_pol_narrow(float f, int dtype) {
    const uint32_t u = rg_pol_u(f), a = u & 0x7fffffffu;
    if (dtype == RG_OBS_BF16) {
        if (a > 0x7f800000u) return 0x7fc0u;
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;  // (a carry out of the mantissa moves into the exponent; past the largest finite value that is infinity)
    }
    const uint32_t s = (u >> 16) & 0x8000u;
    if (a > 0x7f800000u) return 0x7e00u;
    if (a >= 0x47800000u) return s | 0x7c00u;           // 2^16 and above, infinity included
    if (a >= 0x38800000u) {                             // 2^-14 and above: a normal binary16 (65520 and above carries into 0x7c00)
        const uint32_t r = a - 0x38000000u;
        return s | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13);
    }
    if (a <= 0x33000000u) return s;                     // 2^-25 and below: zero (the tie at 2^-25 goes to the even 0)
    const uint32_t sh = 126u - (a >> 23), m = (a & 0x7fffffu) | 0x800000u;  // a subnormal binary16: units of 2^-24, 14 <= sh <= 24
    const uint32_t q = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    return s | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
}
static __host__ __device__ inline float rg_pg_canon(float v) { return v == v ? v : rg_pol_f(0x7fc00000u); }
// every key of a list of n_keys legal (mask = NULL)
static __host__ __device__ inline uint32_t rg_pg_all(int n_keys) { return n_keys >= 32 ? 0xffffffffu : (1u << n_keys) - 1u; }

struct RgPgOut { float logp, entropy; };

// FORWARD: one row.  row: bit k = key k is legal; fetch(k): logit k widened to f32; a: the stored action, any int32.
template <class Fetch>
static __host__ __device__ inline RgPgOut rg_pg_eval_rule(uint32_t row, int n_keys, Fetch fetch, float inv_temp, int a) {
    const rg_act_opts o = {inv_temp, 0.0f, 0.0f, RG_ACT_GIVEN, 0ull, 0ull};
    const RgActOut r = rg_act_rule(row, n_keys, fetch, o, 0u, -1, a);
    return {r.logp, r.entropy};
}

// BACKWARD: one row.  put(k, v): the f32 gradient of logit k, called once for every k < n_keys in list order.
template <class Fetch, class Put>
static __host__ __device__ inline void rg_pg_grad_rule(uint32_t row, int n_keys, Fetch fetch, float inv_temp, int a, bool has_lp, float g_lp, bool has_ent, float g_ent, Put put) {
    const float log2e = 1.4426950216293335f;
    RgPolStats st = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1, true, 0u};
    if (row != 0u) st = rg_pol_stats(row, n_keys, fetch, inv_temp);
    if (st.flat) {  // (no legal key among them)
        for (int k = 0; k < n_keys; k++) put(k, 0.0f);
        return;
    }
    // does the action count?  Nothing is indexed by it before its range is known.
    bool counts = false;
    if (has_lp && a >= 0 && a < n_keys && ((row >> a) & 1u)) {
        bool ok;
        const float x = rg_pol_scaled(fetch(a), inv_temp, ok);
        counts = ok && rg_pol_exp2((x - st.m) * log2e) != 0.0f;
    }
    for (int k = 0; k < n_keys; k++) {
        bool ok;
        const float x = rg_pol_scaled(fetch(k), inv_temp, ok);
        float v = 0.0f;
        if (((row >> k) & 1u) && ok) {
            const float d = x - st.m, w = rg_pol_exp2(d * log2e);
            if (w != 0.0f) {
                const float pi = w * st.inv, lp = d - st.lnS;
                const float t1 = counts ? g_lp * ((k == a ? 1.0f : 0.0f) - pi) : 0.0f;
                const float t2 = has_ent ? g_ent * (pi * (lp + st.ent)) : 0.0f;
                v = rg_pg_canon(inv_temp * (t1 - t2));
            }
        }
        put(k, v);
    }
}
