// rg_novelty.hip -- count-based novelty on the device: state hashes and visit counts (rg_novelty_update / rg_novelty_cut; gfx950).  The rule: rg_novelty.h.
//
//   k_nov_hash<G, WIDE> : the hash of a screen or a window, G lanes per env (16, 32 or 64: a power-of-two part of a wave).  WIDE: the whole-screen key of a
//                         grid whose rows are multiples of 16 bytes -- every lane loads 16 bytes (two words) at a time; else a lane builds its word byte by
//                         byte through rg_nov_key_word (windows, and screens such as 33x17 whose keys start on no 16-byte boundary).
//   k_nov_insert<POS>   : one env per lane -- the generation, the episodic insert, the global insert; POS hashes the player's cell in the same lane
//   k_nov_count         : the global counts read back, once every env's visit of the call is in
//
// A pass of its own behind the step, in a translation unit AND a shared library of its own (librogue_gym_novelty.so, which librogue_gym_hip.so links: units.sh):
// nothing here touches the code generation of the kernels whose register counts the resource tests pin, nor the set of kernels in that library's code objects.  The launches of one call follow each other on the handle's stream, which orders them; no LDS, no barrier, no loop
// that waits for another lane.
#include "rg_device.h"
#include "rg_novelty.h"

#define NOV_THREADS 256

// what the pass reads of the game state (the few arrays, not RgState by value), and which envs it serves
struct NovView {
    const uint8_t *screen; const int32_t *status; const uint16_t *p_pos; const uint8_t *done;
    const int32_t *ids; const uint8_t *mask;   // a cut's envs: a list of `slots` ids, or a mask [n]; both NULL = slot i is env i
    int32_t n, hw, W, H, slots, cut;           // cut = 0: the update behind a step; 1: the cut behind a rebuild / a load (and the enable)
    uint32_t L, m;                             // key bytes and key words
};

// slot s of a launch is one env, as in k_episode: env s of an update, the s-th env of a cut's list, the envs of its mask
static __device__ __forceinline__ bool nov_env(const NovView &V, int slot, int &e) {
    bool active = slot < V.slots;
    e = slot;
    if (active && V.ids) { e = V.ids[slot]; active = e >= 0 && e < V.n; }  // (a device-side list is the caller's to get right: an id out of range is skipped)
    if (active && V.mask) active = V.mask[e] != 0;
    if (!active) e = 0;
    return active;
}
// one atomic per wave and counter: every lane of the wave is here
static __device__ __forceinline__ void nov_tally(unsigned long long *ctr, bool mine) {
    const uint64_t m = __ballot(mine);
    if (m && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

// The words' terms are independent (rg_novelty.h), so the G lanes of a group take the words G apart, sum their terms and the group adds the sums up with
// log2 G exchanges; the group's first lane finishes the hash with the salt.
template <int G, bool WIDE>
__global__ void __launch_bounds__(NOV_THREADS) k_nov_hash(const NovView V, const RgNovelty A) {
    const int gid = blockIdx.x * NOV_THREADS + threadIdx.x;
    const int slot = gid / G, sub = gid % G;
    int e;
    const bool active = nov_env(V, slot, e);
    uint64_t acc = 0;
    if (active) {
        const uint8_t *scr = V.screen + (size_t)e * (size_t)V.hw;
        if (WIDE) {
            const u4v *key = reinterpret_cast<const u4v *>(scr + V.W);  // (hw and W are multiples of 16: so is the key's address, and its length)
            const uint32_t pieces = V.L >> 4;
            for (uint32_t p = (uint32_t)sub; p < pieces; p += G) {
                const u4v v = key[p];
                acc += rg_nov_term((uint64_t)v.x | ((uint64_t)v.y << 32), 2 * p) + rg_nov_term((uint64_t)v.z | ((uint64_t)v.w << 32), 2 * p + 1);
            }
        } else {
            const uint32_t pos = V.p_pos[e];
            for (uint32_t i = (uint32_t)sub; i < V.m; i += G)
                acc += rg_nov_term(rg_nov_key_word(A.what, scr, V.H, V.W, POS_X(pos), POS_Y(pos), A.ry, A.rx, V.L, i), i);
        }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) acc += __shfl_xor((unsigned long long)acc, off);  // (every lane takes part; a partner stays inside the group)
    if (active && sub == 0) A.hash[e] = rg_nov_finish(acc, rg_nov_salt((uint32_t)A.what, V.status[(size_t)e * 10], V.L));
}

// One lane owns its env's episodic table (rg_nov_insert, no atomics).  The global insert: the hash word is looked at, claimed with one compare-and-swap where it
// is 0, and a probe that finds another hash moves on; a stale 0 only means the swap answers with the hash that got there first.
template <bool POS>
__global__ void __launch_bounds__(NOV_THREADS) k_nov_insert(const NovView V, const RgNovelty A) {
    const int slot = blockIdx.x * NOV_THREADS + threadIdx.x;
    int e;
    const bool active = nov_env(V, slot, e);
    bool drop_e = false, drop_g = false, claimed = false;
    if (active) {
        uint32_t gen = A.gen[e];
        if (V.cut || V.done[e] != 0) { gen += 1; A.gen[e] = gen; }
        uint64_t h;
        if (POS) {
            const uint32_t pos = V.p_pos[e];
            h = rg_nov_finish(rg_nov_term(rg_nov_pos_word(POS_X(pos), POS_Y(pos)), 0u), rg_nov_salt(RG_NOV_POS, V.status[(size_t)e * 10], 8u));
            A.hash[e] = h;
        } else h = A.hash[e];
        if (A.tab) {
            const uint32_t c = rg_nov_insert(A.tab + (size_t)e * (size_t)A.cap, (uint32_t)A.cap, gen, h);
            A.count[e] = (int32_t)c;
            drop_e = c == 0;
        }
        if (A.gtab) {
            const uint32_t gm = (uint32_t)A.gcap - 1u;
            uint32_t at = (uint32_t)h & gm;
            int32_t got = -1;
            const uint32_t last = gm < RG_NOV_GPROBES - 1u ? gm : RG_NOV_GPROBES - 1u;
            for (uint32_t p = 0; p <= last; p++, at = (at + 1u) & gm) {
                unsigned long long *word = reinterpret_cast<unsigned long long *>(&A.gtab[at].hash);
                unsigned long long cur = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == 0ull) {
                    cur = atomicCAS(word, 0ull, (unsigned long long)h);
                    if (cur == 0ull) { claimed = true; cur = h; }
                }
                if (cur == h) { got = (int32_t)at; break; }
            }
            if (got >= 0) atomicAdd(&A.gtab[got].count, 1u);
            else drop_g = true;
            A.gslot[e] = got;
        }
    }
    if (A.gtab) { nov_tally(&A.stat[0], claimed); nov_tally(&A.stat[1], drop_g); }  // (wave-uniform conditions)
    if (A.tab) nov_tally(&A.stat[2], drop_e);
}

__global__ void __launch_bounds__(NOV_THREADS) k_nov_count(const NovView V, const RgNovelty A) {
    const int slot = blockIdx.x * NOV_THREADS + threadIdx.x;
    int e;
    if (!nov_env(V, slot, e)) return;
    const int32_t at = A.gslot[e];
    A.gcount[e] = at >= 0 ? (int32_t)A.gtab[at].count : 0;
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launcher: defined here against the prototype the host units call it by
// ---------------------------------------------------------------------------------------------
template <bool WIDE>
static void launch_hash(int units, int slots, hipStream_t st, const NovView &V, const RgNovelty &A) {
    const int G = units <= 16 ? 16 : units <= 32 ? 32 : 64;  // lanes per env: one round where the key fits
    const int blocks = (int)(((size_t)slots * G + NOV_THREADS - 1) / NOV_THREADS);
    if (G == 16) hipLaunchKernelGGL((k_nov_hash<16, WIDE>), dim3(blocks), dim3(NOV_THREADS), 0, st, V, A);
    else if (G == 32) hipLaunchKernelGGL((k_nov_hash<32, WIDE>), dim3(blocks), dim3(NOV_THREADS), 0, st, V, A);
    else hipLaunchKernelGGL((k_nov_hash<64, WIDE>), dim3(blocks), dim3(NOV_THREADS), 0, st, V, A);
}

#ifndef RG_BUILD_ID
#define RG_BUILD_ID "unstamped"
#endif
extern "C" {
// the build id of this library, readable from the file as librogue_gym_hip.so's is (rg_api.cpp rg_build_id)
const char *rgk_novelty_build_id(void) { static const char id[] = "RGBUILDID:" RG_BUILD_ID; return id + 10; }
// slots: the envs served (an update: the last step's n_keys; a cut: the list's length, or n).  ids / mask: a cut's, both device pointers, at most one of them.
void rgk_novelty(const RgState *S, const RgConfig *c, const RgNovelty *A, int slots, const int32_t *ids, const uint8_t *mask, int cut, hipStream_t st) {
    if (slots <= 0) return;
    const int W = (int)c->width, H = (int)c->height;
    const uint32_t L = rg_nov_key_len(A->what, H, W, A->ry, A->rx), m = (L + 7) / 8;
    const NovView V = {S->screen, S->status, S->p_pos, S->done, ids, mask, S->n, S->hw, W, H, slots, cut, L, m};
    const int blocks = (slots + NOV_THREADS - 1) / NOV_THREADS;
    if (A->what == RG_NOV_POS) hipLaunchKernelGGL((k_nov_insert<true>), dim3(blocks), dim3(NOV_THREADS), 0, st, V, *A);
    else {
        if (A->what == RG_NOV_SCREEN && (S->hw & 15) == 0 && (W & 15) == 0) launch_hash<true>((int)(L >> 4), slots, st, V, *A);
        else launch_hash<false>((int)m, slots, st, V, *A);
        hipLaunchKernelGGL((k_nov_insert<false>), dim3(blocks), dim3(NOV_THREADS), 0, st, V, *A);
    }
    if (A->gtab) hipLaunchKernelGGL(k_nov_count, dim3(blocks), dim3(NOV_THREADS), 0, st, V, *A);
}
}
