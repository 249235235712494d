// rg_api_learn.cpp -- the learner's side behind the C-ABI: the action rule (rg_policy_eval, rg_policy_grad and their host twins) and the returns and advantages
// of a rollout (rg_gae, rg_vtrace and theirs): stateless entries without a handle -- a learner process may own no env.  The kernels are rg_policy_grad.hip's
// (librogue_gym_learn.so) and rg_returns.hip's (librogue_gym_returns.so), the rules rg_policy_grad.h's and rg_returns.h's, the argument checks and the twins
// rg_readers_host.h's.  Refusals are read through rg_last_error(NULL).  The device entries enqueue on the caller's stream, on the caller's
// current device, and wait for nothing.
#include "rg_handle.h"
#include "rg_launch.h"
#include "rg_readers_host.h"

static int pg_launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    g_create_err = std::string(what) + ": " + hipGetErrorString(e);
    return 1;
}

extern "C" {
int rg_policy_eval(void *hip_stream, int64_t n_rows, int n_keys, const void *logits_dev, int dtype, const uint8_t *mask_dev, const int32_t *action_dev, float inv_temp,
                   float *logp_dev, float *entropy_dev) {
    if (pg_args_check(g_create_err, "rg_policy_eval", "_dev", n_rows, n_keys, logits_dev, dtype, action_dev, inv_temp, false, nullptr)) return 1;
    if (n_rows == 0 || (!logp_dev && !entropy_dev)) return 0;
    rgk_pg_eval(n_rows, n_keys, logits_dev, dtype, mask_dev, action_dev, inv_temp, logp_dev, entropy_dev, static_cast<hipStream_t>(hip_stream));
    return pg_launched("rg_policy_eval");
}
int rg_policy_grad(void *hip_stream, int64_t n_rows, int n_keys, const void *logits_dev, int dtype, const uint8_t *mask_dev, const int32_t *action_dev, float inv_temp,
                   const float *g_logp_dev, const float *g_entropy_dev, void *dlogits_dev) {
    if (pg_args_check(g_create_err, "rg_policy_grad", "_dev", n_rows, n_keys, logits_dev, dtype, action_dev, inv_temp, true, dlogits_dev)) return 1;
    if (n_rows == 0) return 0;
    rgk_pg_grad(n_rows, n_keys, logits_dev, dtype, mask_dev, action_dev, inv_temp, g_logp_dev, g_entropy_dev, dlogits_dev, static_cast<hipStream_t>(hip_stream));
    return pg_launched("rg_policy_grad");
}
int rg_policy_eval_host(int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp, float *logp, float *entropy) {
    return rgh_policy_eval(g_create_err, n_rows, n_keys, logits, dtype, mask, action, inv_temp, logp, entropy);
}
int rg_policy_grad_host(int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp, const float *g_logp,
                        const float *g_entropy, void *dlogits) {
    return rgh_policy_grad(g_create_err, n_rows, n_keys, logits, dtype, mask, action, inv_temp, g_logp, g_entropy, dlogits);
}

// Returns and advantages.  The launchers are weak references (rg_launch.h): a build linked without librogue_gym_returns.so refuses here.
int rg_gae(void *hip_stream, int64_t n_steps, int64_t n_envs, const float *reward, const float *value, const float *last_value, const uint8_t *done, const uint8_t *trunc,
           const float *trunc_value, float gamma, float lam, float *adv, float *ret) {
    if (ret_args_check(g_create_err, "rg_gae", false, n_steps, n_envs, nullptr, nullptr, reward, value, last_value, done, trunc, trunc_value, gamma, lam, nullptr, adv, ret)) return 1;
    if (n_steps == 0 || n_envs == 0) return 0;
    if (!rgk_gae) { g_create_err = "rg_gae: this build is linked without librogue_gym_returns.so (k_gae)"; return 1; }
    rgk_gae(n_steps, n_envs, reward, value, last_value, done, trunc, trunc_value, gamma, ret_gl(gamma, lam), adv, ret, static_cast<hipStream_t>(hip_stream));
    return pg_launched("rg_gae");
}
int rg_vtrace(void *hip_stream, int64_t n_steps, int64_t n_envs, const float *logp_behaviour, const float *logp_target, const float *reward, const float *value,
              const float *last_value, const uint8_t *done, const uint8_t *trunc, const float *trunc_value, float gamma, float lam, float rho_bar, float c_bar, float pg_rho_bar,
              float *vs, float *pg_adv) {
    const float raw[3] = {rho_bar, c_bar, pg_rho_bar};
    if (ret_args_check(g_create_err, "rg_vtrace", true, n_steps, n_envs, logp_behaviour, logp_target, reward, value, last_value, done, trunc, trunc_value, gamma, lam, raw, vs, pg_adv))
        return 1;
    if (n_steps == 0 || n_envs == 0) return 0;
    if (!rgk_vtrace) { g_create_err = "rg_vtrace: this build is linked without librogue_gym_returns.so (k_vtrace)"; return 1; }
    float bars[6];
    ret_bars(rho_bar, c_bar, pg_rho_bar, bars);
    rgk_vtrace(n_steps, n_envs, logp_behaviour, logp_target, reward, value, last_value, done, trunc, trunc_value, gamma, lam, bars, vs, pg_adv, static_cast<hipStream_t>(hip_stream));
    return pg_launched("rg_vtrace");
}
int rg_gae_host(int64_t n_steps, int64_t n_envs, const float *reward, const float *value, const float *last_value, const uint8_t *done, const uint8_t *trunc,
                const float *trunc_value, float gamma, float lam, float *adv, float *ret) {
    return rgh_gae(g_create_err, n_steps, n_envs, reward, value, last_value, done, trunc, trunc_value, gamma, lam, adv, ret);
}
int rg_vtrace_host(int64_t n_steps, int64_t n_envs, const float *logp_behaviour, const float *logp_target, const float *reward, const float *value, const float *last_value,
                   const uint8_t *done, const uint8_t *trunc, const float *trunc_value, float gamma, float lam, float rho_bar, float c_bar, float pg_rho_bar, float *vs,
                   float *pg_adv) {
    return rgh_vtrace(g_create_err, n_steps, n_envs, logp_behaviour, logp_target, reward, value, last_value, done, trunc, trunc_value, gamma, lam, rho_bar, c_bar, pg_rho_bar, vs,
                      pg_adv);
}
}
