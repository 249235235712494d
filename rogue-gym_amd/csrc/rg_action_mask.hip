// rg_action_mask.hip -- legal-action masks and a masked random key per env, on the device (rg_action_mask; gfx950).
//
//   k_action_mask : one wave per 64 consecutive envs, one env per lane
//
// A translation unit of its own, as rg_crop_typed.hip is, so that the code generation of the step and observation kernels -- their register counts are
// pinned by the resource tests -- is not touched by anything here.  The rule itself is rg_action_mask.h's, shared with the host entry point.
#include "rg_device.h"
#include "rg_action_mask.h"

// The key list as kernel arguments: the key bytes, eight per word, and each key's bit of rg_legal_bits, sixteen per word.  Read by shifts, not by
// indexing, so the list stays in scalar registers whatever its length.
struct MaskKeys {
    uint64_t k0, k1, k2, k3, b0, b1;
    __device__ __forceinline__ uint32_t bit(int k) const { return (uint32_t)((k < 16 ? b0 : b1) >> (4 * (k & 15))) & 15u; }
    __device__ __forceinline__ uint32_t byte(uint32_t k) const { return (uint32_t)((k < 8 ? k0 : k < 16 ? k1 : k < 24 ? k2 : k3) >> (8 * (k & 7))) & 0xffu; }
};

// A lane loads its env's player cell and flag word, then the nine cell words of the 3x3 neighbourhood as independent loads: a neighbour outside the grid
// is not read -- the load goes to the clamped cell and the word is replaced by a bare Surface::None, which is what the rule makes of it (not walkable).
// The rule then runs on that 3x3 grid with the player in its middle, every key of the list lands in one bit of `row`, and the draw picks among the set
// bits.  The wave's rows are one contiguous stretch of 64 * n_keys bytes of the output, a multiple of 16 that starts on a multiple of 16: staged in LDS
// and written as 16-byte pieces (the last, partial wave: its own envs' bytes only, the tail of the stretch byte by byte).
// GROUPS (ext: a config group of a handle with several): env e's row goes to the handle's row ext[e] by byte stores, and its draw is env ext[e]'s.
// (The kernel takes the few arrays it reads, not RgState by value, as the observation kernels do.)
__global__ void __launch_bounds__(WAVE) k_action_mask(const uint16_t *__restrict__ p_pos, const uint32_t *__restrict__ flags, const uint16_t *__restrict__ cell,
                                                     const int32_t *__restrict__ ext, int n, int W, int H, int n_keys, MaskKeys K, uint8_t *__restrict__ mask,
                                                     uint8_t *__restrict__ sample, uint64_t seed, uint64_t draw) {
    __shared__ __align__(16) uint8_t rows[WAVE * RG_MASK_MAX_KEYS];
    const int lane = threadIdx.x, base = blockIdx.x * WAVE;
    const int cnt = n - base < WAVE ? n - base : WAVE;
    if (lane < cnt) {
        const int e = base + lane;
        const uint32_t pos = p_pos[e], fl = flags[e];
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
        const uint32_t bits = rg_legal_bits(nb, 3, 3, 1, 1, (int)(fl & RG_FLAG_DEAD));
        const uint32_t xe = ext ? (uint32_t)ext[e] : (uint32_t)e;
        uint32_t row = 0;
        for (int k = 0; k < n_keys; k++) {
            const uint32_t v = (bits >> K.bit(k)) & 1u;
            row |= v << k;
            if (mask) {
                if (ext) mask[(size_t)xe * n_keys + k] = (uint8_t)v;
                else rows[lane * n_keys + k] = (uint8_t)v;
            }
        }
        if (sample) {
            const uint32_t legal = (uint32_t)__popc(row);
            const uint32_t idx = rg_sample_index_of(seed, xe, draw, legal);
            uint32_t r = row;
            for (uint32_t i = 0; i < idx; i++) r &= r - 1;  // drop the idx lowest set entries (idx < legal)
            sample[xe] = (uint8_t)K.byte(legal ? (uint32_t)__builtin_ctz(r) : 0u);
        }
    }
    if (mask && !ext) {  // (wave-uniform)
        lds_barrier();
        const int bytes = cnt * n_keys;
        uint8_t *o = mask + (size_t)base * n_keys;  // 16-byte aligned (rg_action_mask checks mask_dev)
        for (int p = lane; p * 16 < bytes; p += WAVE) {
            if (p * 16 + 16 <= bytes) {
                *reinterpret_cast<u4v *>(o + p * 16) = *reinterpret_cast<const u4v *>(rows + p * 16);
            } else {
#pragma unroll 1
                for (int b = p * 16; b < bytes; b++) o[b] = rows[b];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launcher: defined here against the prototype the host units call it by
// ---------------------------------------------------------------------------------------------
extern "C" {
// keys: 1 <= n_keys <= RG_MASK_MAX_KEYS keys of KeyMap::ai (checked by the caller); mask / sample: either may be NULL
void rgk_action_mask(const RgState *S, const RgConfig *c, const uint8_t *keys, int n_keys, uint8_t *mask, uint8_t *sample, uint64_t seed, uint64_t draw,
                     hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    if (S->n <= 0) return;
    uint64_t kw[4] = {0, 0, 0, 0}, bw[2] = {0, 0};
    for (int k = 0; k < n_keys; k++) {
        kw[k >> 3] |= (uint64_t)keys[k] << (8 * (k & 7));
        bw[k >> 4] |= (uint64_t)rg_key_bit(keys[k]) << (4 * (k & 15));
    }
    const MaskKeys K = {kw[0], kw[1], kw[2], kw[3], bw[0], bw[1]};
    const int blocks = (S->n + WAVE - 1) / WAVE;
    rg_launch(k_action_mask, dim3(blocks), dim3(WAVE), 0, st, ev0, ev1, S->p_pos, S->flags, S->cell, S->ext, S->n, (int)c->width, (int)c->height, n_keys, K, mask, sample, seed,
              draw);
}
}
