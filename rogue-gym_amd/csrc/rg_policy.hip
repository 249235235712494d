// rg_policy.hip -- one masked categorical action per env from policy logits, on the device (rg_act; gfx950).
//
//   k_act<dtype> : one wave per 64 consecutive envs, one env per lane -- k_action_mask's shape
//
// A library of its own (librogue_gym_policy.so, which librogue_gym_hip.so links), as the novelty pass is: its kernels stay out of the code objects whose kernel
// set tests/test_pixels_resources.py pins by name.  The rule is rg_policy.h's, shared with the host twin (rg_act_host), and the two agree bit for bit.
#include "rg_device.h"
#include "rg_policy.h"

// The key list as kernel arguments (k_action_mask's form): the key bytes, eight per word, and each key's bit of rg_legal_bits, sixteen per word.
struct ActKeys {
    uint64_t k0, k1, k2, k3, b0, b1;
    __device__ __forceinline__ uint32_t bit(int k) const { return (uint32_t)((k < 16 ? b0 : b1) >> (4 * (k & 15))) & 15u; }
    __device__ __forceinline__ uint32_t byte(uint32_t k) const { return (uint32_t)((k < 8 ? k0 : k < 16 ? k1 : k < 24 ? k2 : k3) >> (8 * (k & 7))) & 0xffu; }
};
// what the call hands over per env and takes back: every pointer but `logits` may be NULL (`key` in RG_ACT_GIVEN only)
struct ActIo {
    const void *logits; const uint8_t *teacher; const int32_t *given;
    uint8_t *key; int32_t *action; float *logp, *entropy; uint8_t *source, *mask;
};

template <int DT> struct ActElem { typedef uint16_t T; };
template <> struct ActElem<RG_OBS_F32> { typedef float T; };

// ONE ROUND OF LOADS.  The rows of a full wave's 64 envs are one contiguous stretch of 64 * n_keys elements, a multiple of 16 bytes that starts on a multiple
// of 16 (rg_act checks logits_dev): the wave requests it as 16-byte pieces, at most PIECES per lane, then each lane requests its player cell, its flag word,
// its teacher key and given action and the nine clamped cells of its neighbourhood (k_action_mask's loads) -- nothing of all that waits for anything else.  The
// pieces go to LDS and every lane reads its row from there, once per pass of the rule (rg_act_rule walks the row three times; it is never held in registers).
// The last, partial wave and a config group (ext: env e's row is the handle's row ext[e], anywhere) read their own elements only, each lane its row, into
// the same LDS slots.  Results: one store per output per lane, at ext[e] for a group; the optional mask as k_action_mask writes it.
template <int DT>
__global__ void __launch_bounds__(WAVE) k_act(const uint16_t *__restrict__ p_pos, const uint32_t *__restrict__ flags, const uint16_t *__restrict__ cell,
                                             const int32_t *__restrict__ ext, int n, int W, int H, int n_keys, ActKeys K, ActIo io, rg_act_opts o) {
    typedef typename ActElem<DT>::T T;
    constexpr int PIECES = RG_MASK_MAX_KEYS * (int)sizeof(T) / 16;  // per lane: 64 rows of at most RG_MASK_MAX_KEYS elements
    __shared__ __align__(16) T lg[WAVE * RG_MASK_MAX_KEYS];
    __shared__ __align__(16) uint8_t rows[WAVE * RG_MASK_MAX_KEYS];
    const int lane = threadIdx.x, base = blockIdx.x * WAVE;
    const int cnt = n - base < WAVE ? n - base : WAVE;
    const bool staged = !ext && cnt == WAVE;  // (wave-uniform)
    u4v piece[PIECES];
    const int pieces = n_keys * (int)sizeof(T) * (WAVE / 16);
    if (staged) {
        const u4v *src = reinterpret_cast<const u4v *>(static_cast<const T *>(io.logits) + (size_t)base * n_keys);
#pragma unroll
        for (int i = 0; i < PIECES; i++)
            if (lane + i * WAVE < pieces) piece[i] = src[lane + i * WAVE];
    }
    const int e = base + (lane < cnt ? lane : 0);  // (a lane past the end repeats the wave's first env and stores nothing)
    const uint32_t xe = ext ? (uint32_t)ext[e] : (uint32_t)e;
    const uint32_t pos = p_pos[e], fl = flags[e];
    const int tkey = io.teacher ? (int)io.teacher[xe] : -1;
    const int given = io.given ? io.given[xe] : -1;
    const int px = POS_X(pos), py = POS_Y(pos);
    const uint16_t *g = cell + (size_t)e * (size_t)(W * H);
    uint16_t nb[9];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int x = px + i - 1, y = py + j - 1;
            const bool inside = x >= 0 && y >= 0 && x < W && y < H;
            const uint16_t v = g[min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1)];
            nb[j * 3 + i] = inside ? v : (uint16_t)S_NONE;
        }
    T *mine = lg + lane * n_keys;
    if (staged) {
        u4v *dst = reinterpret_cast<u4v *>(lg);
#pragma unroll
        for (int i = 0; i < PIECES; i++)
            if (lane + i * WAVE < pieces) dst[lane + i * WAVE] = piece[i];
    } else if (lane < cnt) {
        const T *src = static_cast<const T *>(io.logits) + (size_t)xe * n_keys;
        for (int k = 0; k < n_keys; k++) mine[k] = src[k];
    }
    lds_barrier();
    if (lane < cnt) {
        const uint32_t bits = rg_legal_bits(nb, 3, 3, 1, 1, (int)(fl & RG_FLAG_DEAD));
        uint32_t row = 0;
        int teacher = -1;
        for (int k = n_keys - 1; k >= 0; k--) {
            const uint32_t v = (bits >> K.bit(k)) & 1u;
            row |= v << k;
            if ((int)K.byte(k) == tkey) teacher = k;  // (its first position in the list)
            if (io.mask) {
                if (ext) io.mask[(size_t)xe * n_keys + k] = (uint8_t)v;
                else rows[lane * n_keys + k] = (uint8_t)v;
            }
        }
        const RgActOut r = rg_act_rule(row, n_keys, [=](int k) -> float {
            if constexpr (DT == RG_OBS_F32) return mine[k];
            else return rg_pol_widen((uint32_t)mine[k], DT);
        }, o, xe, teacher, given);
        if (io.key) io.key[xe] = (uint8_t)K.byte(r.action >= 0 && r.action < n_keys ? (uint32_t)r.action : 0u);
        if (io.action) io.action[xe] = r.action;
        if (io.logp) io.logp[xe] = r.logp;
        if (io.entropy) io.entropy[xe] = r.entropy;
        if (io.source) io.source[xe] = (uint8_t)r.source;
    }
    if (io.mask && !ext) {  // (wave-uniform)
        lds_barrier();
        const int bytes = cnt * n_keys;
        uint8_t *out = io.mask + (size_t)base * n_keys;  // 16-byte aligned (rg_act checks mask_dev)
        for (int p = lane; p * 16 < bytes; p += WAVE) {
            if (p * 16 + 16 <= bytes) {
                *reinterpret_cast<u4v *>(out + p * 16) = *reinterpret_cast<const u4v *>(rows + p * 16);
            } else {
#pragma unroll 1
                for (int b = p * 16; b < bytes; b++) out[b] = rows[b];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launcher: defined here against the prototype the host units call it by
// ---------------------------------------------------------------------------------------------
#ifndef RG_BUILD_ID
#define RG_BUILD_ID "unstamped"
#endif
extern "C" {
// the build id of this library, readable from the file as librogue_gym_hip.so's is (rg_api.cpp rg_build_id)
const char *rgk_act_build_id(void) { static const char id[] = "RGBUILDID:" RG_BUILD_ID; return id + 10; }
// keys: 1 <= n_keys <= RG_MASK_MAX_KEYS keys of KeyMap::ai, dtype and *opts checked by the caller (act_opts_check)
void rgk_act(const RgState *S, const RgConfig *c, const uint8_t *keys, int n_keys, const void *logits, int dtype, const rg_act_opts *opts, const uint8_t *teacher,
             const int32_t *given, uint8_t *key, int32_t *action, float *logp, float *entropy, uint8_t *source, uint8_t *mask, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    if (S->n <= 0) return;
    uint64_t kw[4] = {0, 0, 0, 0}, bw[2] = {0, 0};
    for (int k = 0; k < n_keys; k++) {
        kw[k >> 3] |= (uint64_t)keys[k] << (8 * (k & 7));
        bw[k >> 4] |= (uint64_t)rg_key_bit(keys[k]) << (4 * (k & 15));
    }
    const ActKeys K = {kw[0], kw[1], kw[2], kw[3], bw[0], bw[1]};
    const ActIo io = {logits, teacher, given, key, action, logp, entropy, source, mask};
    const int blocks = (S->n + WAVE - 1) / WAVE;
    auto *kernel = dtype == RG_OBS_F32 ? k_act<RG_OBS_F32> : dtype == RG_OBS_F16 ? k_act<RG_OBS_F16> : k_act<RG_OBS_BF16>;
    rg_launch(kernel, dim3(blocks), dim3(WAVE), 0, st, ev0, ev1, S->p_pos, S->flags, S->cell, S->ext, S->n, (int)c->width, (int)c->height, n_keys, K, io, *opts);
}
}
