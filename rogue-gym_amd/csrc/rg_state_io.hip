// rg_state_io.hip -- batched save / restore of env game states (rg_state_save / rg_state_load, include/rogue_gym_hip.h; record layout: rg_state_io.h).
//
// A record is mostly env-contiguous bytes (the grids; the dist maps alone are ~80 % of a mini record), the rest are words of the SoA arrays at stride n.
// Two kernels per direction:
//   k_state_rec_*    one WAVE per record: header + the env-contiguous sections + the key log, 16-byte loads and stores where both sides are aligned.
//   k_state_words_*  one WORKGROUP per 64 records: a field is read (save) / written (load) with lane = env -- one coalesced access per field when the ids
//                    are ascending -- and transposed through LDS, so that the record side is written (save) / read (load) in whole record lines.
//                    (A wave per env would touch a 128-byte line per 4-byte word.)
// Load adds the header check (a record that does not fit leaves its env untouched and raises RG_FLAG_ERR_STATE) and k_state_stairs, the stair-set
// producer of the next k_step (rg_state.h stair_mark): restored envs from their restored cell and position, all others carried forward.
#include "rg_device.h"
#include "rg_state_io.h"

// The io_* helpers and the per-record bodies of the two save kernels (io_rec_save, io_words_save): rg_state_io_dev.h, shared with the archive's record writers.
#include "rg_state_io_dev.h"

// ---- save ----
__global__ void __launch_bounds__(WAVE * IO_RPB) k_state_rec_save(RgState S, RgIoLayout L, const int32_t *__restrict__ ids, int k, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int r = blockIdx.x * IO_RPB + (int)(threadIdx.x / WAVE);
    if (r >= k) return;
    const int e = io_env(ids, r, S.n);
    uint8_t *rec = out + (size_t)r * L.R;
    if (e < 0) {  // a device-side id out of range: an all-zero record (no magic, so no load takes it) and the error bit
        for (uint32_t i = lane; i < L.R / 16; i += WAVE) reinterpret_cast<uint4 *>(rec)[i] = make_uint4(0, 0, 0, 0);
        if (lane == 0) atomicOr(S.err_any, RG_FLAG_ERR_STATE);
        return;
    }
    io_rec_save(S, L, e, rec, lane);
}

struct IoRowDst {  // record l of a block of rg_state_save: row r0 + l of the caller's buffer
    uint8_t *out; int r0; uint32_t R;
    __device__ __forceinline__ uint8_t *operator()(uint32_t l) const { return out + (size_t)(r0 + l) * R; }
};
__global__ void __launch_bounds__(IO_THREADS) k_state_words_save(int n, RgIoLayout L, const uint64_t *__restrict__ desc, const uint32_t *__restrict__ guard,
                                                                 const int32_t *__restrict__ ids, int k,
                                                                 uint8_t *__restrict__ out) {
    __shared__ uint32_t tile[IO_WPB * (IO_CH + 1)];  // [record][word], odd row pitch: both the column writes and the row reads are conflict-free
    __shared__ int env[IO_WPB];
    const int t = threadIdx.x, r0 = blockIdx.x * IO_WPB;
    if (t < IO_WPB) env[t] = r0 + t < k ? io_env(ids, r0 + t, n) : -1;
    __syncthreads();
    const uint32_t nr = (uint32_t)(k - r0 < IO_WPB ? k - r0 : IO_WPB);
    io_words_save(L, desc, guard, tile, env, nr, IoRowDst{out, r0, L.R}, t);
}

// ---- load ----
__global__ void __launch_bounds__(WAVE * IO_RPB) k_state_rec_load(RgState S, RgIoLayout L, const int32_t *__restrict__ ids, int k, const uint8_t *__restrict__ recs,
                                                                  uint32_t rec_bytes, uint8_t *__restrict__ ok, uint8_t *__restrict__ mark) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int r = blockIdx.x * IO_RPB + (int)(threadIdx.x / WAVE);
    if (r >= k) return;
    const int e = io_env(ids, r, S.n);
    const uint8_t *rec = recs + (size_t)r * rec_bytes;
    const uint32_t *hd = reinterpret_cast<const uint32_t *>(rec);
    const uint32_t cap_r = hd[8], klen = hd[9];
    // the record fits iff everything before its key log is laid out as this handle's: same format, config (fingerprint), geometry and sections
    const bool good = e >= 0 && hd[0] == RG_STATE_MAGIC && hd[1] == RG_STATE_VERSION && hd[2] == rec_bytes && hd[3] == (L.H | (L.W << 16)) && hd[4] == L.rooms &&
                      hd[5] == L.sections && hd[6] == L.fp_lo && hd[7] == L.fp_hi && cap_r <= rec_bytes && rec_bytes - RG_STATE_PAD16(cap_r) == L.base;
    if (lane == 0) ok[r] = good ? 1 : 0;
    if (!good) {
        if (lane == 0) {
            if (e >= 0) S.flags[e] |= RG_FLAG_ERR_STATE;
            atomicOr(S.err_any, RG_FLAG_ERR_STATE);
        }
        return;
    }
    const size_t hw = L.hw;
    io_copy(reinterpret_cast<uint8_t *>(S.cell + (size_t)e * hw), rec + L.o_cell, L.hw * 2, L.hw * 2, lane);
    io_copy(S.screen + (size_t)e * hw, rec + L.o_screen, L.hw, L.hw, lane);
    io_copy(S.hist + (size_t)e * hw, rec + L.o_hist, L.hw, L.hw, lane);
    if (L.sections & RG_SEC_DCMAP) io_copy(reinterpret_cast<uint8_t *>(S.dc_map) + (size_t)e * L.b_dcmap, rec + L.o_dcmap, L.b_dcmap, L.b_dcmap, lane);
    if (L.sections & RG_SEC_DCWALK) io_copy(reinterpret_cast<uint8_t *>(S.dc_walk) + (size_t)e * L.b_dcwalk, rec + L.o_dcwalk, L.b_dcwalk, L.b_dcwalk, lane);
    io_copy(reinterpret_cast<uint8_t *>(S.status + (size_t)e * 10), rec + L.o_status, 40, 40, lane);
    if (L.sections & RG_SEC_OBSREC) io_copy(reinterpret_cast<uint8_t *>(S.obs_rec) + (size_t)e * L.b_obsrec, rec + L.o_obsrec, L.b_obsrec, L.b_obsrec, lane);
    if (S.klog) {  // the running episode's keys, as many as both logs hold; the length stays (beyond the capacity it already means "tail not stored")
        const uint32_t cur = S.klog_cur[e];
        uint32_t nk = klen < cap_r ? klen : cap_r;
        nk = nk < L.klog_cap ? nk : L.klog_cap;
        io_copy(S.klog + ((size_t)e * 2 + cur) * L.klog_cap, rec + rec_bytes - RG_STATE_PAD16(cap_r), nk, nk, lane);
        if (lane == 0) S.klog_len[(size_t)cur * S.n + e] = klen > cap_r ? (klen | RG_KLOG_PARTIAL) : klen;
    }
    if (lane == 0) mark[e] = 1;
}

__global__ void __launch_bounds__(IO_THREADS) k_state_words_load(int n, RgIoLayout L, const uint64_t *__restrict__ desc, const uint32_t *__restrict__ guard,
                                                                 const int32_t *__restrict__ ids, int k,
                                                                 const uint8_t *__restrict__ recs, uint32_t rec_bytes, const uint8_t *__restrict__ ok) {
    __shared__ uint32_t tile[IO_WPB * (IO_CH + 1)];
    __shared__ int env[IO_WPB];
    const int t = threadIdx.x, r0 = blockIdx.x * IO_WPB;
    if (t < IO_WPB) env[t] = (r0 + t < k && ok[r0 + t]) ? io_env(ids, r0 + t, n) : -1;
    __syncthreads();
    const uint32_t nr = (uint32_t)(k - r0 < IO_WPB ? k - r0 : IO_WPB);
    for (uint32_t c0 = 0; c0 < L.n_words; c0 += IO_CH) {
        const uint32_t cn = L.n_words - c0 < IO_CH ? L.n_words - c0 : IO_CH;
        for (uint32_t i = t; i < nr * cn; i += IO_THREADS) {  // record lines in
            const uint32_t l = i / cn, w = i - l * cn;
            if (env[l] >= 0) {
                const uint32_t *rw = reinterpret_cast<const uint32_t *>(recs + (size_t)(r0 + l) * rec_bytes + L.o_words);
                const uint32_t gd = guard[c0 + w];
                uint32_t v = rw[c0 + w];
                if (gd && !(gd & RG_IO_GUARD_RING) && !((rw[(gd & 0xffffffu) - 1] >> (gd >> RG_IO_GUARD_SHIFT)) & 1u)) v = 0;  // an empty slot's stale word
                tile[l * (IO_CH + 1) + w] = v;
            }
        }
        __syncthreads();
        for (uint32_t i = t; i < IO_WPB * cn; i += IO_THREADS) {  // fields out, lane = env
            const uint32_t w = i / IO_WPB, l = i % IO_WPB;
            const int e = env[l];
            if (e >= 0) io_st(desc[c0 + w], e, tile[l * (IO_CH + 1) + w]);
        }
        __syncthreads();
    }
}

// The stair set for the next k_step (rg_state.h; the producer protocol of k_build / k_debug_descend, rg_kernels.hip stair_publish / stair_recycle): every
// env gets its byte -- a restored env from the tile under its restored player, every other one its byte of the current set -- and the marked envs
// are listed.  A restored env's next-level structure is dropped, as at any new level (RG_NX_DROP: CLAIMED -> DROP, else -> NONE).
__global__ void __launch_bounds__(IO_THREADS) k_state_stairs(RgState S, RgIoLayout L, uint8_t *__restrict__ mark) {
    const int e = blockIdx.x * IO_THREADS + threadIdx.x, lane = threadIdx.x & (WAVE - 1);
    const int g = S.stair_gen;
    const bool mine = e < S.n;
    bool on = false;
    if (mine) {
        if (mark[e]) {
            mark[e] = 0;
            const uint32_t p = S.p_pos[e];
            const uint32_t x = (uint32_t)POS_X(p), y = (uint32_t)POS_Y(p);
            on = x < L.W && y < L.H && (S.cell[(size_t)e * L.hw + y * L.W + x] & C_SURF_MASK) == S_STAIR;
            if (S.nx_state) (void)__hip_atomic_fetch_and(&S.nx_state[e], RG_NX_DROP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            on = S.stair_mark[(size_t)(g & 1) * S.n + e] != 0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the counter nobody reads or writes right now, and its take counter
        S.stair_cnt[(g + 2) % 3] = 0;
        S.stair_cnt[4 + (g + 2) % 3] = 0;
    }
    const int w = (g + 1) & 1;
    if (mine) S.stair_mark[(size_t)w * S.n + e] = on ? 1 : 0;
    const uint64_t m = __ballot(mine && on);
    if (m) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&S.stair_cnt[(g + 1) % 3], (uint32_t)__popcll(m));
        base = __shfl(base, 0);
        if (mine && on) S.stair_list[(size_t)w * S.n + base + __popcll(m & ((1ull << lane) - 1ull))] = e;
    }
}
#include "rg_launch.h"  // host-callable launchers: defined here against the prototypes the host units call them by
extern "C" {
void rgk_state_save(const RgState *S, const RgIoLayout *L, const uint64_t *desc, const uint32_t *guard, const int32_t *ids, int k, uint8_t *out, hipStream_t st) {
    if (k <= 0) return;
    hipLaunchKernelGGL(k_state_rec_save, dim3((k + IO_RPB - 1) / IO_RPB), dim3(WAVE * IO_RPB), 0, st, *S, *L, ids, k, out);
    if (L->n_words) hipLaunchKernelGGL(k_state_words_save, dim3((k + IO_WPB - 1) / IO_WPB), dim3(IO_THREADS), 0, st, S->n, *L, desc, guard, ids, k, out);
}
// (S->stair_gen: set by the host to this producer's number)
void rgk_state_load(const RgState *S, const RgIoLayout *L, const uint64_t *desc, const uint32_t *guard, const int32_t *ids, int k, const uint8_t *recs, uint32_t rec_bytes, uint8_t *ok,
                    uint8_t *mark, hipStream_t st) {
    if (k > 0) {
        hipLaunchKernelGGL(k_state_rec_load, dim3((k + IO_RPB - 1) / IO_RPB), dim3(WAVE * IO_RPB), 0, st, *S, *L, ids, k, recs, rec_bytes, ok, mark);
        if (L->n_words) hipLaunchKernelGGL(k_state_words_load, dim3((k + IO_WPB - 1) / IO_WPB), dim3(IO_THREADS), 0, st, S->n, *L, desc, guard, ids, k, recs, rec_bytes, ok);
    }
    hipLaunchKernelGGL(k_state_stairs, dim3((S->n + IO_THREADS - 1) / IO_THREADS), dim3(IO_THREADS), 0, st, *S, *L, mark);
}
// the stair set behind any other partial writer of player positions that marked its envs (the list-driven build of rg_reset_envs / rg_reset_mask)
void rgk_state_stairs(const RgState *S, const RgIoLayout *L, uint8_t *mark, hipStream_t st) {
    hipLaunchKernelGGL(k_state_stairs, dim3((S->n + IO_THREADS - 1) / IO_THREADS), dim3(IO_THREADS), 0, st, *S, *L, mark);
}
}
