// rg_api_learn.cpp -- the learner's side of the action rule behind the C-ABI (rg_policy_eval, rg_policy_grad and their host twins): stateless entries without a
// handle -- a learner process may own no env.  The kernels are rg_policy_grad.hip's (librogue_gym_learn.so), the rule rg_policy_grad.h's, the argument check
// and the twins rg_readers_host.h's.  Refusals are read through rg_last_error(NULL).  The device entries enqueue on the caller's stream, on the caller's
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
}
