// rg_episode.hip -- episode accounting and the scout reward on the device (rg_episode_update / rg_episode_cut; gfx950).
//
//   k_episode<false> : returns, lengths, depths, end causes; one env per lane
//   k_episode<true>  : the same plus the scout bitmap; a group of 16 lanes (one DPP row) per env
//
// A pass of its own behind the step, in a translation unit of its own, as rg_route.hip is: nothing here touches the code generation of the kernels whose
// register counts the resource tests pin.  The rule itself is rg_episode.h's, shared with the host entry point.
#include "rg_device.h"
#include "rg_episode.h"

#define EP_THREADS 256
#define EP_GS 16   // lanes per env of the scout instance: four 16-byte loads per lane cover 512 cells, and 8 cells make exactly one byte of `seen`

// what the pass reads of the game state (the few arrays, not RgState by value, as the observation kernels do), and which envs it serves
struct EpView {
    const uint16_t *cell; const int32_t *status; const float *reward; const uint8_t *done; const uint32_t *steps;
    const int32_t *ids; const uint8_t *mask;   // a cut's envs: a list of `slots` ids, or a mask [n]; both NULL = slot i is env i
    int32_t n, hw, W, slots;
    uint32_t max_steps, serial;
    int32_t cut, record;                       // cut = 0: the update behind a step; 1: the cut behind a rebuild / a load
};

// the sum of v over the DPP row (16 lanes) the lane sits in, in every lane of it: four rotations
static __device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);  // row_ror:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);  // row_ror:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false);  // row_ror:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false);  // row_ror:1
    return v;
}
// eight cell words in four registers -> their known bits
static __device__ __forceinline__ uint32_t known_of8(const u4v v) {
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    uint32_t b = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) b |= rg_ep_known((t & 1) ? q[t >> 1] >> 16 : q[t >> 1] & 0xffffu) << t;
    return b;
}

// Slot s of the launch is one env: env s of an update (the first n_keys envs of the last step), or the s-th env of a cut's list / the envs of its mask.
// SCOUT: the 16 lanes of a group walk the env's `seen` words 16 apart -- word w covers cells 32 w .. 32 w + 31, four 16-byte loads where H * W is a
// multiple of 8 (every env's grid then starts on a multiple of 16 bytes), cell by cell otherwise (rg_ep_known_byte) -- OR and pop-count in registers,
// and the count is summed over the group's DPP row: no LDS, no barrier.  Every lane of the group reads the few scalars that decide whether the bitmap
// starts from nothing (a done, a cut, another level); the group's first lane does the scalar rule and the stores.
// The log: the wave's finished episodes take ONE returning atomic for their slots (ballot + popc), a record past the capacity is dropped -- the counter
// keeps counting, rg_episode_log_read works out how many were.
template <bool SCOUT>
__global__ void __launch_bounds__(EP_THREADS) k_episode(const EpView V, const RgEpisode A) {
    const int gid = blockIdx.x * EP_THREADS + threadIdx.x;
    const int slot = SCOUT ? gid / EP_GS : gid, sub = SCOUT ? gid % EP_GS : 0;
    bool active = slot < V.slots;
    int e = slot;
    if (active && V.ids) { e = V.ids[slot]; active = e >= 0 && e < V.n; }  // (a device-side list is the caller's to get right: an id out of range is skipped)
    if (active && V.mask) active = V.mask[e] != 0;
    if (!active) e = 0;
    const bool lead = active && sub == 0;

    RgEpLane L = {0.f, 0, 0, 0, 0};
    RgEpDone F = {0.f, 0, 0, 0u, 0};
    bool fin = false, drop = false, ended = false;
    int32_t lvl = 0;
    if (active) {
        lvl = V.status[(size_t)e * 10];
        L.ret = A.ret[e]; L.len = A.len[e]; L.depth = A.depth[e]; L.level = A.level[e]; L.scout_sum = A.scout_sum[e];
        if (V.cut) {
            fin = V.record != 0 && L.len > 0;
            F = rg_ep_finish(L, RG_EP_CUT);
            rg_ep_rebase(L, lvl, (int32_t)V.steps[e]);
            drop = true;
        } else {
            rg_ep_account(L, V.reward[e]);
            ended = V.done[e] != 0;
            if (ended) {
                fin = true;
                F = rg_ep_finish(L, rg_ep_cause(L.len, V.max_steps));
                rg_ep_rebase(L, lvl, 0);
                drop = true;
            } else drop = rg_ep_new_level(L, lvl);
        }
    }
    uint32_t cnt = 0;
    if (SCOUT) {
        if (active) {
            const uint16_t *grid = V.cell + (size_t)e * (size_t)V.hw;
            uint32_t *sw = reinterpret_cast<uint32_t *>(A.seen + (size_t)e * (size_t)A.seen_bytes);
            const int nw = A.seen_bytes >> 2;
            const bool aligned = (V.hw & 7) == 0;
            for (int w = sub; w < nw; w += EP_GS) {
                uint32_t known = 0;
                if (aligned) {
                    u4v v[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int c0 = 32 * w + 8 * k;
                        v[k] = c0 < V.hw ? *reinterpret_cast<const u4v *>(grid + c0) : u4v{0u, 0u, 0u, 0u};
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) known |= (known_of8(v[k]) & rg_ep_row_bits(4 * w + k, V.hw, V.W)) << (8 * k);
                } else {
#pragma unroll 1
                    for (int k = 0; k < 4; k++) known |= rg_ep_known_byte(grid, 4 * w + k, V.hw, V.W) << (8 * k);
                }
                const uint32_t was = sw[w];
                uint32_t s = was;
                cnt += (uint32_t)__popc(rg_ep_fresh(known, s, drop));
                if (s != was) sw[w] = s;
            }
        }
        cnt = row_sum(cnt);  // (every lane takes part: the rotations read neighbour lanes)
    }
    if (lead) {
        const int32_t pay = (V.cut || ended) ? 0 : (int32_t)cnt;  // the first view of a new game is not something the old episode earned
        L.scout_sum += pay;
        A.ret[e] = L.ret; A.len[e] = L.len; A.depth[e] = L.depth; A.level[e] = L.level; A.scout_sum[e] = L.scout_sum;
        if (SCOUT) A.scout[e] = (float)pay;
        if (!V.cut) {
            A.died[e] = (uint8_t)(ended && F.cause == RG_EP_DIED);
            A.time_limit[e] = (uint8_t)(ended && F.cause == RG_EP_TIME_LIMIT);
        }
        if (fin) { A.last_return[e] = F.ret; A.last_length[e] = F.len; A.last_depth[e] = F.depth; A.last_cause[e] = (uint8_t)F.cause; }
    }
    if (A.log) {  // (wave-uniform; every lane is still here)
        const bool rec = lead && fin;
        const uint64_t m = __ballot(rec);
        if (m) {
            uint32_t base = 0;
            if ((threadIdx.x & (WAVE - 1)) == 0) base = atomicAdd(&A.log_cnt[0], (uint32_t)__popcll(m));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (rec && at < (uint32_t)A.log_cap) {
                u4v *o = reinterpret_cast<u4v *>(A.log + at);
                o[0] = u4v{V.serial, (uint32_t)e, __float_as_uint(F.ret), (uint32_t)F.len};
                o[1] = u4v{(uint32_t)F.depth, F.cause, (uint32_t)F.scout, 0u};
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launcher: defined here against the prototype the host units call it by
// ---------------------------------------------------------------------------------------------
extern "C" {
// slots: the envs served (an update: the last step's n_keys; a cut: the list's length, or n).  ids / mask: a cut's, both device pointers, at most one of them.
void rgk_episode(const RgState *S, const RgConfig *c, const RgEpisode *A, int slots, const int32_t *ids, const uint8_t *mask, int cut, int record, uint32_t serial,
                 hipStream_t st) {
    if (slots <= 0) return;
    const EpView V = {S->cell, S->status, S->reward, S->done, S->steps, ids, mask, S->n, S->hw, (int32_t)c->width, slots, c->max_steps, serial, cut, record};
    if (A->seen) {
        const int blocks = (int)(((size_t)slots * EP_GS + EP_THREADS - 1) / EP_THREADS);
        hipLaunchKernelGGL((k_episode<true>), dim3(blocks), dim3(EP_THREADS), 0, st, V, *A);
    } else {
        const int blocks = (slots + EP_THREADS - 1) / EP_THREADS;
        hipLaunchKernelGGL((k_episode<false>), dim3(blocks), dim3(EP_THREADS), 0, st, V, *A);
    }
}
}
