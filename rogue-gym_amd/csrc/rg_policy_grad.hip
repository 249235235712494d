// rg_policy_grad.hip -- the learner's side of the action rule on the device (rg_policy_eval, rg_policy_grad; gfx950).
//
//   k_pg_eval<dtype> : one wave per 64 consecutive rows, one row per lane: logp of the stored action and the entropy under the stored mask
//   k_pg_grad<dtype> : the same shape: the gradient of g_lp * logp + g_ent * entropy with respect to the row of logits, in the logits' dtype
//
// A library of its own (librogue_gym_learn.so, which librogue_gym_hip.so links): tests/test_policy_resources.py pins librogue_gym_policy.so to the three k_act
// instances.  The rule is rg_policy_grad.h's, shared with the host twins (rg_policy_eval_host, rg_policy_grad_host); kernel and twin agree bit for bit.
// The rows are user data (a rollout buffer), not game state: an action indexes nothing before the rule has range-checked it, a mask byte counts as != 0, and
// nothing is read or written past row n - 1.
#include "rg_device.h"
#include "rg_policy_grad.h"

struct PgIo {
    const void *logits; const uint8_t *mask; const int32_t *action; const float *g_lp, *g_ent;
    float *logp, *entropy; void *dlogits;
};

template <int DT> struct PgElem { typedef uint16_t T; };
template <> struct PgElem<RG_OBS_F32> { typedef float T; };

// LDS, sized by the launch (64 * n_keys * (sizeof(T) + 1) bytes): the wave's 64 rows of logits as one flat stretch (row r at element r * n_keys: an odd
// n_keys, the product's 11, walks the banks without a conflict), then its 64 rows of mask bytes.
extern __shared__ __align__(16) uint8_t pg_lds[];

// ONE ROUND OF LOADS.  A full wave's 64 rows are one contiguous stretch of 64 * n_keys elements, a multiple of 16 bytes: where it starts on a multiple of 16
// the wave requests it as 16-byte pieces, at most PIECES per lane, and the mask stretch likewise (at most two pieces per lane); nothing waits for anything
// else.  A stretch that does not start on a multiple of 16 (a minibatch slice logits[i0:i1] starts at i0 * 44 bytes) and the partial last wave go lane by lane,
// each lane its own row's elements and nothing behind row n - 1.  Every lane then reads its row from LDS, once per pass of the rule.
template <class T>
__device__ __forceinline__ void pg_stage(const PgIo &io, int64_t base, int cnt, int n_keys, T *lg, uint8_t *rows, int lane) {
    constexpr int PIECES = RG_MASK_MAX_KEYS * (int)sizeof(T) / 16, MPIECES = RG_MASK_MAX_KEYS / 16;
    const T *src = static_cast<const T *>(io.logits) + base * (int64_t)n_keys;
    const uint8_t *msrc = io.mask ? io.mask + base * (int64_t)n_keys : nullptr;
    const bool lstaged = cnt == WAVE && !((uintptr_t)src & 15), mstaged = msrc && cnt == WAVE && !((uintptr_t)msrc & 15);  // (wave-uniform)
    const int pieces = n_keys * (int)sizeof(T) * (WAVE / 16), mpieces = n_keys * (WAVE / 16);
    u4v piece[PIECES], mpiece[MPIECES];
    if (lstaged) {
#pragma unroll
        for (int i = 0; i < PIECES; i++)
            if (lane + i * WAVE < pieces) piece[i] = reinterpret_cast<const u4v *>(src)[lane + i * WAVE];
    }
    if (mstaged) {
#pragma unroll
        for (int i = 0; i < MPIECES; i++)
            if (lane + i * WAVE < mpieces) mpiece[i] = reinterpret_cast<const u4v *>(msrc)[lane + i * WAVE];
    }
    if (lstaged) {
#pragma unroll
        for (int i = 0; i < PIECES; i++)
            if (lane + i * WAVE < pieces) reinterpret_cast<u4v *>(lg)[lane + i * WAVE] = piece[i];
    } else if (lane < cnt) {
        for (int k = 0; k < n_keys; k++) lg[lane * n_keys + k] = src[(int64_t)lane * n_keys + k];
    }
    if (mstaged) {
#pragma unroll
        for (int i = 0; i < MPIECES; i++)
            if (lane + i * WAVE < mpieces) reinterpret_cast<u4v *>(rows)[lane + i * WAVE] = mpiece[i];
    } else if (msrc && lane < cnt) {
        for (int k = 0; k < n_keys; k++) rows[lane * n_keys + k] = msrc[(int64_t)lane * n_keys + k];
    }
    lds_barrier();
}
// the lane's legal word: bit k = its mask byte k is not 0 (no mask: every key)
__device__ __forceinline__ uint32_t pg_row(const uint8_t *rows, bool have_mask, int lane, int n_keys) {
    if (!have_mask) return rg_pg_all(n_keys);
    uint32_t row = 0;
    for (int k = 0; k < n_keys; k++) row |= (rows[lane * n_keys + k] != 0 ? 1u : 0u) << k;
    return row;
}

template <int DT>
__global__ void __launch_bounds__(WAVE) k_pg_eval(PgIo io, int64_t n, int n_keys, float inv_temp) {
    typedef typename PgElem<DT>::T T;
    T *lg = reinterpret_cast<T *>(pg_lds);
    uint8_t *rows = pg_lds + (size_t)WAVE * n_keys * sizeof(T);
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * WAVE;
    const int cnt = n - base < WAVE ? (int)(n - base) : WAVE;
    const int32_t a = lane < cnt ? io.action[base + lane] : 0;
    pg_stage<T>(io, base, cnt, n_keys, lg, rows, lane);
    if (lane >= cnt) return;
    const T *mine = lg + lane * n_keys;
    const RgPgOut r = rg_pg_eval_rule(pg_row(rows, io.mask != nullptr, lane, n_keys), n_keys, [=](int k) -> float {
        if constexpr (DT == RG_OBS_F32) return mine[k];
        else return rg_pol_widen((uint32_t)mine[k], DT);
    }, inv_temp, a);
    if (io.logp) io.logp[base + lane] = r.logp;
    if (io.entropy) io.entropy[base + lane] = r.entropy;
}

// The gradient row takes the place of the lane's logits in LDS (the rule hands key k over after its last look at logit k), and the wave sends its stretch out
// as it came in: 16-byte pieces where the stretch of dlogits starts on a multiple of 16 and the wave is full, else each lane its own row.
template <int DT>
__global__ void __launch_bounds__(WAVE) k_pg_grad(PgIo io, int64_t n, int n_keys, float inv_temp) {
    typedef typename PgElem<DT>::T T;
    constexpr int PIECES = RG_MASK_MAX_KEYS * (int)sizeof(T) / 16;
    T *lg = reinterpret_cast<T *>(pg_lds);
    uint8_t *rows = pg_lds + (size_t)WAVE * n_keys * sizeof(T);
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * WAVE;
    const int cnt = n - base < WAVE ? (int)(n - base) : WAVE;
    const bool live = lane < cnt;
    const int32_t a = live ? io.action[base + lane] : 0;
    const float g_lp = live && io.g_lp ? io.g_lp[base + lane] : 0.0f, g_ent = live && io.g_ent ? io.g_ent[base + lane] : 0.0f;
    pg_stage<T>(io, base, cnt, n_keys, lg, rows, lane);
    T *mine = lg + lane * n_keys;
    if (live)
        rg_pg_grad_rule(pg_row(rows, io.mask != nullptr, lane, n_keys), n_keys, [=](int k) -> float {
            if constexpr (DT == RG_OBS_F32) return mine[k];
            else return rg_pol_widen((uint32_t)mine[k], DT);
        }, inv_temp, a, io.g_lp != nullptr, g_lp, io.g_ent != nullptr, g_ent, [=](int k, float v) {
            if constexpr (DT == RG_OBS_F32) mine[k] = v;
            else mine[k] = (uint16_t)rg_pol_narrow(v, DT);
        });
    lds_barrier();
    T *dst = static_cast<T *>(io.dlogits) + base * (int64_t)n_keys;
    if (cnt == WAVE && !((uintptr_t)dst & 15)) {  // (wave-uniform)
        const int pieces = n_keys * (int)sizeof(T) * (WAVE / 16);
#pragma unroll
        for (int i = 0; i < PIECES; i++)
            if (lane + i * WAVE < pieces) reinterpret_cast<u4v *>(dst)[lane + i * WAVE] = reinterpret_cast<const u4v *>(lg)[lane + i * WAVE];
    } else if (live) {
        for (int k = 0; k < n_keys; k++) dst[(int64_t)lane * n_keys + k] = mine[k];
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launchers: defined here against the prototypes the host units call them by
// ---------------------------------------------------------------------------------------------
#ifndef RG_BUILD_ID
#define RG_BUILD_ID "unstamped"
#endif
extern "C" {
// the build id of this library, readable from the file as librogue_gym_hip.so's is (rg_api.cpp rg_build_id)
const char *rgk_learn_build_id(void) { static const char id[] = "RGBUILDID:" RG_BUILD_ID; return id + 10; }
// n_rows > 0, 1 <= n_keys <= RG_MASK_MAX_KEYS, dtype and inv_temp checked by the caller (pg_args_check); a wave per 64 rows
void rgk_pg_eval(int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp, float *logp, float *entropy,
                 hipStream_t st) {
    const PgIo io = {logits, mask, action, nullptr, nullptr, logp, entropy, nullptr};
    const size_t lds = (size_t)WAVE * n_keys * ((dtype == RG_OBS_F32 ? 4 : 2) + 1);
    auto *kernel = dtype == RG_OBS_F32 ? k_pg_eval<RG_OBS_F32> : dtype == RG_OBS_F16 ? k_pg_eval<RG_OBS_F16> : k_pg_eval<RG_OBS_BF16>;
    rg_launch(kernel, dim3((unsigned)((n_rows + WAVE - 1) / WAVE)), dim3(WAVE), lds, st, nullptr, nullptr, io, n_rows, n_keys, inv_temp);
}
void rgk_pg_grad(int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp, const float *g_lp, const float *g_ent,
                 void *dlogits, hipStream_t st) {
    const PgIo io = {logits, mask, action, g_lp, g_ent, nullptr, nullptr, dlogits};
    const size_t lds = (size_t)WAVE * n_keys * ((dtype == RG_OBS_F32 ? 4 : 2) + 1);
    auto *kernel = dtype == RG_OBS_F32 ? k_pg_grad<RG_OBS_F32> : dtype == RG_OBS_F16 ? k_pg_grad<RG_OBS_F16> : k_pg_grad<RG_OBS_BF16>;
    rg_launch(kernel, dim3((unsigned)((n_rows + WAVE - 1) / WAVE)), dim3(WAVE), lds, st, nullptr, nullptr, io, n_rows, n_keys, inv_temp);
}
}
