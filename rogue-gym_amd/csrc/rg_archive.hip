// rg_archive.hip -- the cell archive on the device: per hashed state the best state record any env has offered (rg_archive_update / rg_archive_restore;
// gfx950).  The rule: rg_archive.h.  A library of its own (librogue_gym_archive.so, which librogue_gym_hip.so links: units.sh), as the novelty pass is: the
// kernel sets and register counts the resource tests pin in the other code objects stay what they are.
//
// One update is five launches on the handle's stream, which orders them; no lane waits for another lane and no loop spins on memory:
//   k_arc_offer    one lane per env: the probe (find the key or claim a zero key with one 64-bit compare-and-swap), seen += 1, and the slot's bid raised with a
//                  64-bit atomic max on the packed (score, ~steps)
//   k_arc_bidders  lanes whose bid is the slot's final bid, where that bid beats the stored offer, take the slot with a 64-bit atomic max on
//                  (serial << 32 | ~env): the lowest env id wins, and a stale word of an earlier call never does
//   k_arc_winners  the lane that took its slot moves (score, steps, when) in, sets stored[e] and enters the device list (ballot + one atomic per wave); every
//                  lane with a slot puts the slot's bid back to 0 for the next call
//   k_arc_rec, k_arc_words   the two record writers, from the device list, straight into records + slot * R: the per-record bodies of rg_state_save's two
//                  kernels (rg_state_io_dev.h), a wave per record and a workgroup per 64 records; the grid is the worst case (every env writes) and the waves past
//                  the count, which they read on the device, leave at once
// Restore: k_arc_gather copies the chosen slots' records into a staging buffer that rg_state_load takes as it is, k_arc_chosen counts the loads that fitted.
#include "rg_device.h"
#include "rg_archive.h"
#include "rg_state_io_dev.h"

#define ARC_THREADS 256

// what an update reads: the offers
struct ArcView {
    const uint64_t *key; const int32_t *score; const uint32_t *gold; const uint32_t *steps; const uint8_t *mask;   // score NULL: the pack gold; mask NULL: every env
    int32_t n; uint32_t serial;
};

// one atomic per wave and counter: every lane of the wave is here
static __device__ __forceinline__ void arc_tally(unsigned long long *ctr, bool mine) {
    const uint64_t m = __ballot(mine);
    if (m && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(ARC_THREADS) k_arc_offer(const ArcView V, const RgArchive A) {
    const int e = blockIdx.x * ARC_THREADS + threadIdx.x;
    if (e == 0) A.cnt[0] = 0;   // (the writers of the last call are done: stream order)
    bool claimed = false, drop = false;
    if (e < V.n) {
        int32_t got = -1;
        if (!V.mask || V.mask[e] != 0) {
            const uint64_t key = rg_arc_key(V.key[e]);
            const int32_t score = V.score ? V.score[e] : (int32_t)V.gold[e];
            const uint32_t steps = V.steps[e];
            A.score_in[e] = score; A.steps_in[e] = steps;
            const uint32_t m = (uint32_t)A.cells - 1u, last = rg_arc_probes((uint32_t)A.cells);
            uint32_t at = (uint32_t)key & m;
            for (uint32_t p = 0; p < last; p++, at = (at + 1u) & m) {
                unsigned long long *word = reinterpret_cast<unsigned long long *>(&A.key[at]);
                unsigned long long cur = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == 0ull) {
                    cur = atomicCAS(word, 0ull, (unsigned long long)key);
                    if (cur == 0ull) { claimed = true; cur = key; }
                }
                if (cur == key) { got = (int32_t)at; break; }
            }
            if (got >= 0) {
                atomicAdd(&A.seen[got], 1u);
                atomicMax(&A.bid[got], (unsigned long long)rg_arc_bid(score, steps));
            } else drop = true;
        }
        A.slot[e] = got;
        A.stored[e] = 0;
    }
    arc_tally(&A.stat[0], claimed);
    arc_tally(&A.stat[1], drop);
}

__global__ void __launch_bounds__(ARC_THREADS) k_arc_bidders(const ArcView V, const RgArchive A) {
    const int e = blockIdx.x * ARC_THREADS + threadIdx.x;
    if (e >= V.n) return;
    const int32_t s = A.slot[e];
    if (s < 0) return;
    const int32_t score = A.score_in[e];
    const uint32_t steps = A.steps_in[e];
    if (rg_arc_bid(score, steps) == A.bid[s] && rg_arc_beats(score, steps, A.when[s], A.score[s], A.steps[s]))
        atomicMax(&A.win[s], ((unsigned long long)V.serial << 32) | (unsigned long long)(~(uint32_t)e));
}

__global__ void __launch_bounds__(ARC_THREADS) k_arc_winners(const ArcView V, const RgArchive A) {
    const int e = blockIdx.x * ARC_THREADS + threadIdx.x, lane = threadIdx.x & (WAVE - 1);
    bool mine = false;
    if (e < V.n) {
        const int32_t s = A.slot[e];
        if (s >= 0) {
            A.bid[s] = 0ull;   // (nobody reads it in this launch; every lane of the slot stores the same word)
            mine = A.win[s] == (((unsigned long long)V.serial << 32) | (unsigned long long)(~(uint32_t)e));
            if (mine) { A.score[s] = A.score_in[e]; A.steps[s] = A.steps_in[e]; A.when[s] = V.serial; A.stored[e] = 1; }
        }
    }
    const uint64_t m = __ballot(mine);
    if (m) {
        uint32_t base = 0;
        if (lane == 0) {
            base = atomicAdd(&A.cnt[0], (uint32_t)__popcll(m));
            atomicAdd(&A.stat[2], (unsigned long long)__popcll(m));
        }
        base = __shfl(base, 0);
        if (mine) A.list[base + __popcll(m & ((1ull << lane) - 1ull))] = e;   // (at most one entry per env: the list holds n)
    }
}

// ---- the record writers: rg_state_save's bodies, the destination records + slot * R, the count on the device ----
// (the grid is sized for the worst case, every env a winner; the waves past the count leave after one load.  The few pointers are passed one by one: RgState
// alone takes most of the scalar registers a kernel has)
__global__ void __launch_bounds__(WAVE * IO_RPB) k_arc_rec(RgState S, RgIoLayout L, const int32_t *__restrict__ list, const uint32_t *__restrict__ cnt,
                                                           const int32_t *__restrict__ slot, uint8_t *__restrict__ records) {
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t r = blockIdx.x * IO_RPB + threadIdx.x / WAVE;
    if (r >= cnt[0]) return;
    const int e = list[r];
    io_rec_save(S, L, e, records + (size_t)slot[e] * L.R, lane);
}

struct ArcSlotDst {  // record l of a block: the slot the block's env list names
    uint8_t *records; const int *at; uint32_t R;
    __device__ __forceinline__ uint8_t *operator()(uint32_t l) const { return records + (size_t)at[l] * R; }
};
__global__ void __launch_bounds__(IO_THREADS) k_arc_words(RgIoLayout L, const uint64_t *__restrict__ desc, const uint32_t *__restrict__ guard, const int32_t *__restrict__ list,
                                                          const uint32_t *__restrict__ cnt, const int32_t *__restrict__ slot, uint8_t *__restrict__ records) {
    __shared__ uint32_t tile[IO_WPB * (IO_CH + 1)];
    __shared__ int env[IO_WPB], at[IO_WPB];
    const int t = threadIdx.x;
    const uint32_t k = cnt[0], r0 = blockIdx.x * IO_WPB;
    if (r0 >= k) return;   // (the whole workgroup: no barrier is left waiting)
    if (t < IO_WPB) {
        const int e = r0 + t < k ? list[r0 + t] : -1;
        env[t] = e;
        at[t] = e >= 0 ? slot[e] : 0;
    }
    __syncthreads();
    io_words_save(L, desc, guard, tile, env, k - r0 < IO_WPB ? k - r0 : IO_WPB, ArcSlotDst{records, at, L.R}, t);
}

// ---- restore ----
// record r of the staging buffer = the record of slot sid[r]; an id out of range gives an all-zero record, which no load takes
__global__ void __launch_bounds__(WAVE * IO_RPB) k_arc_gather(const RgArchive A, const int32_t *__restrict__ sid, int k, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int r = blockIdx.x * IO_RPB + (int)(threadIdx.x / WAVE);
    if (r >= k) return;
    const int32_t s = sid[r];
    const bool in = s >= 0 && s < A.cells;
    const uint4 *src = reinterpret_cast<const uint4 *>(A.records + (size_t)(in ? s : 0) * A.R);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)r * A.R);
    for (uint32_t i = lane; i < A.R / 16; i += WAVE) dst[i] = in ? src[i] : make_uint4(0, 0, 0, 0);
}
__global__ void __launch_bounds__(ARC_THREADS) k_arc_chosen(const RgArchive A, const int32_t *__restrict__ sid, int k, const uint8_t *__restrict__ ok) {
    const int r = blockIdx.x * ARC_THREADS + threadIdx.x;
    if (r >= k || !ok[r]) return;
    const int32_t s = sid[r];
    if (s >= 0 && s < A.cells) atomicAdd(&A.chosen[s], 1u);
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launchers: defined here against the prototypes the host units call them by
// ---------------------------------------------------------------------------------------------
#ifndef RG_BUILD_ID
#define RG_BUILD_ID "unstamped"
#endif
extern "C" {
// the build id of this library, readable from the file as librogue_gym_hip.so's is (rg_api.cpp rg_build_id)
const char *rgk_archive_build_id(void) { static const char id[] = "RGBUILDID:" RG_BUILD_ID; return id + 10; }
void rgk_archive_update(const RgState *S, const RgIoLayout *L, const uint64_t *desc, const uint32_t *guard, const RgArchive *A, const uint64_t *key, const int32_t *score,
                        const uint8_t *mask, uint32_t serial, hipStream_t st) {
    const int n = S->n;
    if (n <= 0) return;
    const ArcView V = {key, score, S->pack_gold, S->steps, mask, n, serial};
    const int blocks = (n + ARC_THREADS - 1) / ARC_THREADS;
    hipLaunchKernelGGL(k_arc_offer, dim3(blocks), dim3(ARC_THREADS), 0, st, V, *A);
    hipLaunchKernelGGL(k_arc_bidders, dim3(blocks), dim3(ARC_THREADS), 0, st, V, *A);
    hipLaunchKernelGGL(k_arc_winners, dim3(blocks), dim3(ARC_THREADS), 0, st, V, *A);
    const int rb = (n + IO_RPB - 1) / IO_RPB, wb = (n + IO_WPB - 1) / IO_WPB;   // the worst case: every env writes
    hipLaunchKernelGGL(k_arc_rec, dim3(rb), dim3(WAVE * IO_RPB), 0, st, *S, *L, A->list, A->cnt, A->slot, A->records);
    if (L->n_words) hipLaunchKernelGGL(k_arc_words, dim3(wb), dim3(IO_THREADS), 0, st, *L, desc, guard, A->list, A->cnt, A->slot, A->records);
}
void rgk_archive_gather(const RgArchive *A, const int32_t *sid, int k, uint8_t *out, hipStream_t st) {
    if (k > 0) hipLaunchKernelGGL(k_arc_gather, dim3((k + IO_RPB - 1) / IO_RPB), dim3(WAVE * IO_RPB), 0, st, *A, sid, k, out);
}
void rgk_archive_chosen(const RgArchive *A, const int32_t *sid, int k, const uint8_t *ok, hipStream_t st) {
    if (k > 0) hipLaunchKernelGGL(k_arc_chosen, dim3((k + ARC_THREADS - 1) / ARC_THREADS), dim3(ARC_THREADS), 0, st, *A, sid, k, ok);
}
}
