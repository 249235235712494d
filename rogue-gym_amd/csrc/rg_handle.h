// rg_handle.h -- what the host units of librogue_gym_hip.so (rg_api*.cpp) share: the handle, the launch timer, the error macros, the allocation helper and the
// few helpers that more than one unit calls.  Host only.  Everything declared below the includes has hidden visibility: none of it is a dynamic symbol.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/rogue_gym_hip.h"
#include "rg_state.h"
#include "rg_episode.h"
#include "rg_novelty.h"
#include "rg_archive.h"

// (rg_api_comm.cpp spells out the few RCCL declarations it needs; the handle holds the communicator)
extern "C" { typedef struct ncclComm *ncclComm_t; }

#pragma GCC visibility push(hidden)
#define RG_TIMED_KERNELS 5   // k_step, k_render, k_obs (or the unfused encode), k_build, k_regen
struct rg_handle {
    RgParsed parsed;             // config of env 0 (all envs agree except for the seed)
    RgConfig cfg;
    RgState S;
    RgState SP;                  // spare view: core pointers address the pre-generated next level-1 state (k_regen)
    bool spares = false;
    uint32_t *lane_q = nullptr; int32_t *lane_list = nullptr;  // its claim list (one launch at a time: the generator's stream serialises them)
    hipStream_t side3 = nullptr; // ... alternating with side2 (a launch may outlast a step)
    hipStream_t side2 = nullptr; // stream of the level-per-lane spare producer (LOW priority; its launches are long and far apart, the next-level structures' short and with every step)
    int lane_flip = 0;           // which of the two carries the next launch (each with its own claim list)
    uint64_t lane_last = 0;      // step_count of its last launch
    uint8_t *pin_keys = nullptr;   // rg_step_fetch: the keys of the call in pinned, device-visible host memory (k_step reads them across PCIe: no copy call)
    uint32_t *pin_err = nullptr;   // ... and where k_export leaves the error word
    bool lane_regen = false;     // the consumed spares are rebuilt one level per LANE (rg_regen_lanes.hip) instead of one per wave (k_regen); ROGUE_GYM_HIP_WAVE_REGEN=1 keeps the latter
    uint64_t step_count = 0;
    hipStream_t side = nullptr;  // stream of the background generator (LOW priority: the step kernel's blocks are placed first, k_regen takes what is left; rg_step_prefix)
    int regen_idle_after = -1;   // ROGUE_GYM_HIP_KEEP_SPARES with fixed seeds only: > 0 = that many more k_regen launches (after creation / rg_seed), 0 = none needed, -1 = off
    int regen_bulk = 0;          // that many of the next k_regen launches rebuild EVERY consumed spare they find (after rg_seed dropped them all), not one per wave
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    uint32_t *d_err = nullptr;
    uint8_t *d_keys = nullptr;
    bool render_pending = false;
    // rg_obs_bind: the caller's standing observation tensor and whether its contents are the current screens of every env up to the SCR_CHANGED / REDRAW flags
    float *bound_out = nullptr; int bound_kind = 0; bool bound_valid = false;
    int32_t *obs_list_mem = nullptr; uint32_t *obs_cnt_mem = nullptr; float *gray_lut_mem = nullptr;
    // the pre-streamed encode (rg_state.h enc_out): helper blocks of rg_step_obs_gray's step launch stream every env's image beside the turns, the pass behind it
    // fixes up the lines the turns touched and draws the Redraws.  Whether it applies is decided when the handle is created (the grid and step-kernel class);
    // rg_tail_encode(h, 0) keeps the two full passes; armed per call.
    bool tail_enc = false, tail_enc_off = false;
    int enc_helpers = 0;   // helper blocks per launch (rgk_step_enc_helpers); 0: none, the pass encodes every env
    bool step_generic = false;  // development library only: the pre-streaming launch stays on k_step_w32<false, true> (rgk_step generic_enc)
    int bound_steps = 0;   // k_step launches since the bound tensor was last written: its in-place pass works from the list of exactly ONE
    int stair_gen = 0;           // producers of the stair set launched so far (k_build, k_step, the debug descent; rg_state.h)
    float *obs_scratch = nullptr;  // rg_obs_host: device-side observation buffer, kept between calls
    size_t obs_scratch_cap = 0;
    std::vector<uint64_t> seed_lo, seed_hi;  // host copy of the seeds the next reset will use (reseed envs: the base of the per-build hash)
    std::vector<uint8_t> reseed;             // 0 = configured seed, 1 = fresh seed per build, 2 = fresh seed inside seed_range per build
    std::vector<uint64_t> range_lo, range_span;  // [2][n] low / high words; empty if no env has a seed_range
    unsigned long long *d_probe = nullptr;
    // ---- per-env configs that differ in more than the seed (python/src/lib.rs:270-294 takes one GameConfig per env): the handle is then a
    // PARENT over one sub-handle per distinct config ("group").  Every group is an ordinary homogeneous batch with its own state and
    // kernels; the parent owns the mirrors in the handle's env order (S.screen .. S.done, assembled from the groups') and routes the calls.
    std::vector<rg_handle *> sub;      // empty for an ordinary handle
    std::vector<int> g_of, l_of;       // env -> (group, index inside the group); groups keep the env order
    int32_t *d_ext = nullptr;          // (sub-handle) device copy of its local -> handle env index map
    std::vector<int32_t> ext;          // (sub-handle) the same on the host
    uint8_t *d_keys_sub = nullptr;     // (sub-handle) keys of its envs gathered from the handle's key vector
    int planes_sym = 0;                // one-hot depth of the handle's symbol image (= symbols of env 0's config, like ParallelGameState::symbols)
    bool screens_stale = true;         // (parent) S.screen / S.hist / S.flags need assembling
    bool mixed = false;                // (parent) the groups differ in width / height (python/src/lib.rs:270-294 takes ANY GameConfig per env): there is no
                                       // [n_env][H][W] tensor then -- screens travel as ragged host copies (rg_fetch_states), the tensor entry points refuse
    std::vector<size_t> ragged_off;    // (mixed parent) [n + 1] byte offset of env i's H_i * W_i screen in the ragged env-order layout
    size_t stat_rows = 0;        // workload counters: one row of 8 per k_step block (summed by rg_counters)
    RgState *d_SP = nullptr;     // device-resident copy of SP: k_step reads the spare's pointers from it on the rare take path (one kernel argument
                                 // instead of a second 60-pointer struct in SGPRs)
    ncclComm_t comm = nullptr;   // rg_comm_init: the RCCL communicator of the one collective of the sharded path (rg_allgather_compact)
    int comm_rank = 0, comm_world = 1;
    std::string err;
    // per-kernel HIP-event timing (rg_timing_*)
    bool timing = false;
    std::vector<hipEvent_t> ev[RG_TIMED_KERNELS];   // start/stop pairs
    size_t ev_used[RG_TIMED_KERNELS] = {0, 0, 0, 0, 0};
    uint64_t timing_seq[RG_TIMED_KERNELS] = {0, 0, 0, 0, 0};   // launches seen while timing is on (sampled or not)
    uint64_t timing_stride = 1;
    // state records (rg_state_save / rg_state_load; rg_state_io.h)
    uint64_t state_fp = 0;             // config fingerprint: FNV-1a 64 of the canonical config without seed / seed_range (create_homog)
    uint64_t *io_desc = nullptr;       // word descriptors of the record's SoA section (built on first use: the state's addresses never change)
    uint32_t *io_guard = nullptr;      // ... and per word its guard (rg_state_io.h RG_IO_GUARD_SHIFT)
    uint32_t io_words = 0;
    int32_t *ids_buf = nullptr; size_t ids_cap = 0;    // the host-side env ids of a save, a load or a cut, uploaded (env_ids_stage)
    uint8_t *io_ok = nullptr; size_t io_ok_cap = 0;    // per record of a load: its header fitted
    uint8_t *io_mark = nullptr;                        // [n] per env: restored by the load / rebuilt by the partial reset in flight (k_state_stairs clears it)
    // partial reset (rg_reset_envs / rg_reset_mask): the envs to rebuild, device-resident
    int32_t *reset_list = nullptr;                     // [n]
    uint32_t *reset_cnt = nullptr;                     // [1] entries of reset_list
    // episode accounting (rg_episode_*; rg_episode.h): off until rg_episode_enable, which allocates the arrays
    bool ep_on = false;
    RgEpisode ep = {};
    uint32_t ep_serial = 0;                            // update / cut calls since the enable
    // count-based novelty (rg_novelty_*; rg_novelty.h): off until rg_novelty_enable, which allocates the arrays and the tables
    bool nov_on = false;
    RgNovelty nov = {};
    uint64_t nov_calls = 0;                            // update / cut calls since the enable or the last clear
    // the cell archive (rg_archive_*; rg_archive.h): off until rg_archive_enable, which allocates the slot arrays and the records
    bool arc_on = false;
    RgArchive arc = {};
    uint32_t arc_serial = 0;                           // update calls since the enable or the last clear: the `when` of the records the next one writes, from 1
    uint8_t *arc_stage = nullptr; size_t arc_stage_cap = 0;   // rg_archive_restore: the gathered records (grown like ids_buf: the old buffer stays until rg_destroy)
    int32_t *arc_sid = nullptr; size_t arc_sid_cap = 0;       // ... and its host-side slot ids, uploaded
    // the tileset of the pixel passes (rg_tileset_set; rg_pixels.h): the font, then the ink table; allocated at the first call.  Config groups read the parent's
    uint8_t *tiles = nullptr; int tile_th = 0;
};

#define RG_TIMING_MAX 4096
struct TimedLaunch {  // times one kernel launch with an event pair when timing is on
    // Two forms.  bracket(): hipEventRecord before and after the launch -- the pair then also contains the marker packets' own processing and the
    // gap to the neighbouring kernels (~5-10 us around an 80 us kernel).  ext(): the pair is handed to the launch itself (rg_device.h rg_launch), which stamps it with the
    // dispatch's own begin / end -- the same clock rocprofv3 --kernel-trace reports; used for the two kernels of the step.
    rg_handle *h; int k; bool on, ext_;
    TimedLaunch(rg_handle *h_, int k_, bool ext = false) : h(h_), k(k_), on(false), ext_(ext) {
        // sampled: an event pair costs a few us of stream time, so only every `timing_stride`-th launch of a kernel is timed
        // (the sampled launch of every stride is its MIDDLE one, not its first: the first launch behind a synchronize runs on an idle, cold chip -- ~110 us
        // for a 65 us k_step -- and with 4 samples in the driver's 20-step window that one outlier made the reported average 80 us)
        if (h->timing && (h->timing_seq[k]++ % h->timing_stride) == h->timing_stride / 2 && h->ev_used[k] + 2 <= h->ev[k].size()) {
            on = true;
            if (!ext_) (void)hipEventRecord(h->ev[k][h->ev_used[k]], h->stream);
        }
    }
    hipEvent_t start_ev() const { return on && ext_ ? h->ev[k][h->ev_used[k]] : nullptr; }
    hipEvent_t stop_ev() const { return on && ext_ ? h->ev[k][h->ev_used[k] + 1] : nullptr; }
    void cancel() { on = false; }  // nothing was launched: leave the (unrecorded) pair unused
    void stop() { if (on) { if (!ext_) (void)hipEventRecord(h->ev[k][h->ev_used[k] + 1], h->stream); h->ev_used[k] += 2; on = false; } }
    ~TimedLaunch() { stop(); }
};

#define HIPCHK(h, call)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                \
            return 1;                                                                                    \
        }                                                                                                \
    } while (0)

template <typename T>
static bool dev_alloc(rg_handle *h, T **p, size_t count) {
    void *q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    if (hipMalloc(&q, bytes) != hipSuccess) { h->err = "hipMalloc failed (" + std::to_string(bytes) + " bytes)"; return false; }
    if (hipMemset(q, 0, bytes) != hipSuccess) { h->err = "hipMemset failed"; return false; }
    h->allocs.push_back(q);
    *p = (T *)q;
    return true;
}
#define SUBCHK(h, sh, call) do { if (call) { (h)->err = (sh)->err; return 1; } } while (0)

extern thread_local std::string g_create_err;  // behind rg_last_error(NULL): the refusals of the entry points without a handle (rg_api.cpp)

// (C linkage, like the entry points they are defined among)
extern "C" {
int flush_render(rg_handle *h);                          // rg_api.cpp: the pending k_render
int flush_mirrors(rg_handle *h);                         // ... or the assembly of a parent's mirrors
bool refuse_mixed(rg_handle *h, const char *what);
int symbols_check(rg_t *h, const std::string &w, const rg_handle *sh);
int obs_common(rg_t *h, uint32_t status_flag, int with_hist, int kind, float *out_dev);
int comm_release(rg_handle *h, bool teardown);           // rg_api_comm.cpp
int env_ids_stage(rg_handle *h, const char *what, const int32_t *env_ids, int k, int on_device, bool unique, const int32_t **out);  // rg_api_state.cpp
}
#pragma GCC visibility pop
