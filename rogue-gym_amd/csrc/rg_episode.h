// rg_episode.h -- episode accounting and the scout reward: THE statement of the rule (rg_episode_update / rg_episode_cut / rg_scout_host), on top of
// rg_route.h's notion of a known cell.  Host and device: k_episode (rg_episode.hip) and rg_scout_host (rg_readers_host.h) both call the pieces below.
//
// k_step rebuilds a finished env in the launch that ends its episode: afterwards only reward[e] and done[e] = 1 are left of the old game -- the status
// mirror shows level 1, the flag word has lost DEAD, the step counter is 0.  The lane state below is kept BESIDE the game state (it is not part of a state
// record or of the compact record) and is advanced once per step from the mirrors and the cells as the step left them.
//
// The engine has two terminal causes, the grave and the step limit, and after the rebuild the mirrors cannot tell them apart; the accounting's own step
// count can: an episode that ends with len >= max_steps ended by the limit, every other one by death.  A DEATH ON THE VERY LAST ALLOWED STEP IS THEREFORE
// REPORTED AS A TIME LIMIT.  That case is real (mini with enemies, max_steps 25: a handful per 8 000 env-steps of the random policy); a test pins it.
#pragma once
#include <cstdint>

#include "rg_route.h"

#define RG_EP_WHAT_ALL (RG_EP_STATS | RG_EP_SCOUT)
#define RG_EP_SLACK 64   // every per-env array is allocated with this many envs of slack behind the last one, which no launch writes (the tests fill and check it)

// bytes of one env's `seen` bitmap: bit b of byte j is cell 8 j + b in row-major order y * W + x; whole 16-byte pieces
static __host__ __device__ inline int rg_ep_seen_bytes(int hw) { return 16 * ((hw + 127) / 128); }

// The lane state.  ret / len / depth are public (rg_episode_arrays), level / scout_sum are the rule's own.
struct RgEpLane { float ret; int32_t len, depth, level, scout_sum; };
// a finished episode, as it goes to last_* and to the log
struct RgEpDone { float ret; int32_t len, depth; uint32_t cause; int32_t scout; };
// the arrays of a handle (device pointers; scout / seen / log NULL when off)
struct RgEpisode {
    float *ret; int32_t *len, *depth, *level, *scout_sum;
    uint8_t *died, *time_limit;
    float *last_return; int32_t *last_length, *last_depth; uint8_t *last_cause;
    float *scout; uint8_t *seen; int32_t seen_bytes;
    rg_episode_rec *log; uint32_t *log_cnt; int32_t log_cap;   // log_cnt[0]: records offered since the last read (those past log_cap were dropped)
};

// one step played: the reward mirror joins the return as ONE f32 add, in step order
static __host__ __device__ inline void rg_ep_account(RgEpLane &L, float reward) { L.ret = L.ret + reward; L.len += 1; }
// why an episode that the step kernel ended has ended (see the note on the last allowed step above)
static __host__ __device__ inline uint32_t rg_ep_cause(int32_t len, uint32_t max_steps) { return (uint32_t)len >= max_steps ? RG_EP_TIME_LIMIT : RG_EP_DIED; }
static __host__ __device__ inline RgEpDone rg_ep_finish(const RgEpLane &L, uint32_t cause) { return RgEpDone{L.ret, L.len, L.depth, cause, L.scout_sum}; }
// a new game stands in the lane (after a done, a cut, the enable): `level` its status mirror's dungeon_level, `len` the steps it has played already
static __host__ __device__ inline void rg_ep_rebase(RgEpLane &L, int32_t level, int32_t len) { L.ret = 0.f; L.len = len; L.depth = L.level = level; L.scout_sum = 0; }
// the running game reports `level`: true = it is another level than `seen` belongs to, whose bits are dropped
static __host__ __device__ inline bool rg_ep_new_level(RgEpLane &L, int32_t level) {
    if (level == L.level) return false;
    L.level = level;
    L.depth = level > L.depth ? level : L.depth;
    return true;
}

// Which of the cells 8 j .. 8 j + 7 can count at all: rows 1 .. H - 2 (the rows the screen draws tiles on), i.e. W <= index < H * W - W.
static __host__ __device__ inline uint32_t rg_ep_row_bits(int j, int hw, int W) {
    const int c0 = 8 * j, lo = W - c0, hi = hw - W - c0;
    const uint32_t from = lo <= 0 ? 0xffu : lo >= 8 ? 0u : (0xffu << lo) & 0xffu, below = hi <= 0 ? 0u : hi >= 8 ? 0xffu : (1u << hi) - 1u;
    return from & below;
}
// the known bit of one cell word (a cell of the player's map: drawn or in view)
static __host__ __device__ inline uint32_t rg_ep_known(uint32_t c) { return (uint32_t)rg_route_known(c, false); }
// byte j of the known bitmap of a grid given cell by cell
static __host__ __device__ inline uint32_t rg_ep_known_byte(const uint16_t *cells, int j, int hw, int W) {
    uint32_t b = 0;
    for (int t = 0; t < 8; t++)
        if (8 * j + t < hw) b |= rg_ep_known(cells[8 * j + t]) << t;
    return b & rg_ep_row_bits(j, hw, W);
}
// The bitmap step on any number of bits: `seen` as loaded (drop = the bits belong to another level or another game: start from nothing), `known` the
// level's known cells now.  Returns the bits seen for the first time; a cell that drops off the player's map stays in `seen` and is never paid twice.
static __host__ __device__ inline uint32_t rg_ep_fresh(uint32_t known, uint32_t &seen, bool drop) {
    const uint32_t old = drop ? 0u : seen, fresh = known & ~old;
    seen = old | fresh;
    return fresh;
}
