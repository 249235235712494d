// rg_returns.h -- returns and advantages of a [T, N] rollout: GAE(lambda), discounted reward-to-go and V-trace (rg_gae / rg_vtrace and their host twins): THE
// statement.  Host and device: k_gae and k_vtrace (rg_returns.hip, librogue_gym_returns.so) and rgh_gae / rgh_vtrace (rg_readers_host.h) call the step functions
// below, and agree bit for bit.  rg_policy.h's discipline holds: f32 add / multiply / compare, explicit __builtin_fmaf, contraction off, no libm, no fast-math
// intrinsic.  A NaN result is written as the canonical quiet NaN 0x7fc00000 (rg_pg_canon).
//
// All [T, N] arrays are time-major and contiguous: row t is N consecutive elements, one env per column; every float is f32.  Each env's column is scanned from
// t = T - 1 down to 0, in that order and no other (a split of T would reassociate the sums).
//
// GAE.  State: adv_next = +0.0, v_next = last_value[n] (absent: +0.0).  For t = T - 1 .. 0:
//       d   = done && done[t] != 0          tr = trunc && trunc[t] != 0        end = d || tr          (any non-zero byte counts)
//       v   = value ? value[t] : +0.0
//       boot = tr ? (trunc_value ? trunc_value[t] : v) : (d ? +0.0 : v_next)
//       delta = fmaf(gamma, boot, reward[t]) - v
//       carry = end ? +0.0 : adv_next               a select, never a multiply by 0: the NaN / inf of one episode stay inside it
//       adv   = fmaf(gl, carry, delta)              gl = gamma * lam, ONE f32 multiply, made once on the host
//       ret   = v + adv
//       adv_next = adv;  v_next = v
//   value absent and lam = 1 is plain discounted reward-to-go, bootstrapped from last_value.
//   trunc marks a time-limit end: the episode ended, the state did not.  Its bootstrap is the caller's trunc_value[t], the value of the state that the rebuild
//   replaced, for a learner that has it.  Without trunc_value the bootstrap is value[t] itself: the partial-episode approximation V(s_{t+1}) ~ V(s_t), that is
//   delta = r + (gamma - 1) * V(s_t) -- a stand-in, not the true bootstrap.
//
// V-TRACE (Espeholt et al. 2018, lambda as in rlax).  With ln_bar = (float)log((double)bar), made once on the host for each of the three bars:
//       ratio(bar) = e >= 0 ? bar : bar * rg_pol_exp2(e * log2e)        e = (logp_target[t] - logp_behaviour[t]) - ln_bar
//   = min(bar, exp(lt - lb)), the argument of rg_pol_exp2 never above 0 (its domain); below -125 the ratio is 0; a NaN e gives a NaN ratio.
//   rho = ratio(rho_bar), c = lam * ratio(c_bar), rho_pg = ratio(pg_rho_bar).  State: acc = +0.0, v_next = vs_next = last_value[n].  end and boot as in GAE:
//       delta   = rho * (fmaf(gamma, boot, reward[t]) - v)
//       carry   = end ? +0.0 : acc
//       acc     = fmaf(gamma * c, carry, delta)
//       vs      = v + acc
//       vs_boot = end ? boot : vs_next
//       pg_adv  = rho_pg * (fmaf(gamma, vs_boot, reward[t]) - v)
//       vs_next = vs;  v_next = v
//   With logp_target == logp_behaviour and rho_bar == c_bar == 1 every ratio is exactly 1 and vs equals GAE's ret for the same lam, bit for bit.
#pragma once
#include "rg_policy_grad.h"

#pragma clang fp contract(off)

// one row of one column as the step functions take it: absent arrays already replaced (v = +0.0, d = tr = false), tv looked at only where has_tv
struct RgRetRow { float r, v, tv; bool d, tr, has_tv; };
struct RgRetPair { float a, b; };   // (adv, ret) or (vs, pg_adv), canonical NaNs

static __host__ __device__ inline float rg_ret_boot(const RgRetRow &x, float v_next) { return x.tr ? (x.has_tv ? x.tv : x.v) : (x.d ? 0.0f : v_next); }

struct RgGaeState { float adv_next, v_next; };
static __host__ __device__ inline RgRetPair rg_gae_step(RgGaeState &s, const RgRetRow &x, float gamma, float gl) {
    const float boot = rg_ret_boot(x, s.v_next);
    const float delta = __builtin_fmaf(gamma, boot, x.r) - x.v;
    const float carry = (x.d || x.tr) ? 0.0f : s.adv_next;
    const float adv = __builtin_fmaf(gl, carry, delta);
    const float ret = x.v + adv;
    s.adv_next = adv;
    s.v_next = x.v;
    return {rg_pg_canon(adv), rg_pg_canon(ret)};
}

// min(bar, exp(lt - lb)) for a finite bar > 0 with ln_bar = (float)log((double)bar)
static __host__ __device__ inline float rg_vt_ratio(float lt, float lb, float bar, float ln_bar) {
    const float log2e = 1.4426950216293335f;
    const float e = (lt - lb) - ln_bar;
    const bool capped = e >= 0.0f;
    const float w = rg_pol_exp2(capped ? 0.0f : e * log2e);   // (selects, not returns: the device's lanes stay together)
    return capped ? bar : (e != e ? rg_pol_f(0x7fc00000u) : bar * w);
}

struct RgVtState { float acc, v_next, vs_next; };
struct RgVtBars { float rho, c, pg, ln_rho, ln_c, ln_pg; };   // the three bars and their logarithms
static __host__ __device__ inline RgRetPair rg_vtrace_step(RgVtState &s, const RgRetRow &x, float lb, float lt, float gamma, float lam, const RgVtBars &bars) {
    const float rho = rg_vt_ratio(lt, lb, bars.rho, bars.ln_rho), c = lam * rg_vt_ratio(lt, lb, bars.c, bars.ln_c), rho_pg = rg_vt_ratio(lt, lb, bars.pg, bars.ln_pg);
    const bool end = x.d || x.tr;
    const float boot = rg_ret_boot(x, s.v_next);
    const float delta = rho * (__builtin_fmaf(gamma, boot, x.r) - x.v);
    const float carry = end ? 0.0f : s.acc;
    const float acc = __builtin_fmaf(gamma * c, carry, delta);
    const float vs = x.v + acc;
    const float vs_boot = end ? boot : s.vs_next;
    const float pg_adv = rho_pg * (__builtin_fmaf(gamma, vs_boot, x.r) - x.v);
    s.acc = acc;
    s.vs_next = vs;
    s.v_next = x.v;
    return {rg_pg_canon(vs), rg_pg_canon(pg_adv)};
}
