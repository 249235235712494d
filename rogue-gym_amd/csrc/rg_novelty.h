// rg_novelty.h -- count-based novelty: the hash of what an env shows and the visit tables that remember it (rg_novelty_*).  THE statement of the rule, as
// rg_episode.h is for the accounting.  Host and device, plain C++: k_nov_hash / k_nov_insert (rg_novelty.hip) and the host twins (rg_readers_host.h:
// rg_novelty_hash_host, rgh_nov_insert) both call the pieces below.
//
// KEY BYTES.  `what` selects the bytes B (length L) that are hashed for an env:
//   RG_NOV_POS    eight bytes: the player's x as u16 LE, y as u16 LE, four zero bytes.  Not privileged: '@' is on the screen.
//   RG_NOV_SCREEN rows 1 .. H-2 of the env's screen mirror (the rows the screen draws tiles on), L = (H-2) * W: what the policy sees, as of the last Redraw.
//   RG_NOV_CROP   the (2ry+1) x (2rx+1) window of the same rows around the player's cell, row-major; the window is rg_obs_crop's (window cell (j, i) is screen
//                 cell (py - ry + j, px - rx + i)), and a window cell outside rows 1 .. H-2 or outside the columns is ' '.
// HASH.  B is padded with zero bytes to a multiple of 8; w_i, i = 0 .. m-1, are its little-endian u64 words; mix is the splitmix64 finaliser;
//   acc  = sum_i mix(w_i ^ ((i + 1) * 0x9e3779b97f4a7c15))   mod 2^64
//   salt = what | dungeon_level << 8 | (u64)L << 32          (dungeon_level: the status mirror's)
//   hash = mix(acc + mix(salt)), and a result of 0 becomes 1 -- 0 marks an empty slot of the global table.
// THE SUM MAKES THE WORDS INDEPENDENT: every word's term depends on the word and its index alone, so a wave hashes one env's screen with one word per lane
// (or two: a 16-byte load) and reduces the terms with plain adds, in any order.
// EPISODIC TABLE.  cap slots per env (a power of two, 64 .. 65 536) of 16 bytes {u64 hash, u32 gen, u32 count}, read and written as ONE 16-byte access.  Each env
// has a generation gen[e]; a slot whose gen differs from it is EMPTY, so an episode end is gen[e] += 1 and costs nothing (clearing tables would be a spike at the
// mass timeouts a cohort of envs has at multiples of max_steps).  Insert: linear probing from hash & (cap - 1), step 1, at most cap probes; a current slot with
// this hash gets count += 1, the first empty slot becomes {hash, gen[e], 1}; with neither the visit is DROPPED: the count reported is 0 and it is counted
// (dropped_episode).  One lane owns an env's table: no atomics.  (gen is 32 bits: a slot written 2^32 episodes ago would read as current.)
// GLOBAL TABLE.  One per handle, gcap slots (a power of two, 1 024 .. 2^28) of the same 16 bytes (gen unused), shared by all envs, emptied by rg_novelty_clear
// only.  Insert: a 64-bit compare-and-swap of the hash word (0 -> hash) along the same probe sequence, then an atomic add on the slot's count; every probe
// claims, matches or moves on -- no loop waits for another lane -- at most min(gcap, RG_NOV_GPROBES) times; a visit that finds neither its hash nor an empty
// slot by then is dropped (count 0, dropped_global): the table is full.  RG_NOV_GPROBES = 1 024 is the smallest gcap, so a table of that size is probed end
// to end; a larger one counts as full once a run of 1 024 occupied slots stands behind a start slot (linear probing: about 98 % occupied) -- gcap probes of
// a 2^22-slot table for each of the tens of thousands of new states of a step would take minutes, in a launch that every later step waits for.  The count
// reported is the slot's count after EVERY env's visit of the call has been added (a launch of its own reads it back), so below capacity the result does not
// depend on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rogue_gym_hip.h"  // RG_NOV_*

#define RG_NOV_SLACK 64        // every per-env array is allocated with this many envs of slack behind the last one, which no launch writes
#define RG_NOV_CAP_MIN 64
#define RG_NOV_CAP_MAX 65536
#define RG_NOV_GCAP_MIN 1024
#define RG_NOV_GCAP_MAX (1 << 28)
#define RG_NOV_GPROBES 1024   // probes of a global insert at most (= RG_NOV_GCAP_MIN)
#define RG_NOV_GOLD 0x9e3779b97f4a7c15ull

struct alignas(16) RgNovSlot { uint64_t hash; uint32_t gen, count; };
// the arrays of a handle (device pointers; those of a scope that is off are NULL)
struct RgNovelty {
    uint64_t *hash; int32_t *count, *gcount;   // [N + slack] public (rg_novelty_arrays)
    uint32_t *gen;                             // [N] the env's generation
    int32_t *gslot;                            // [N] the global slot this call's visit went to, -1 = dropped: what the read-back launch reads
    RgNovSlot *tab, *gtab;                     // [N][cap] episodic, [gcap] global
    unsigned long long *stat;                  // [4] occupied_global, dropped_global, dropped_episode, (unused)
    int32_t what, ry, rx, cap, gcap;
};

static __host__ __device__ inline uint64_t rg_nov_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
// the term of word i (from 0) in acc
static __host__ __device__ inline uint64_t rg_nov_term(uint64_t w, uint32_t i) { return rg_nov_mix(w ^ ((uint64_t)(i + 1) * RG_NOV_GOLD)); }
static __host__ __device__ inline uint64_t rg_nov_salt(uint32_t what, int32_t level, uint32_t L) { return (uint64_t)what | ((uint64_t)(uint32_t)level << 8) | ((uint64_t)L << 32); }
// the finishing step
static __host__ __device__ inline uint64_t rg_nov_finish(uint64_t acc, uint64_t salt) {
    const uint64_t h = rg_nov_mix(acc + rg_nov_mix(salt));
    return h ? h : 1ull;
}
static __host__ __device__ inline uint32_t rg_nov_key_len(int what, int H, int W, int ry, int rx) {
    return what == RG_NOV_POS ? 8u : what == RG_NOV_SCREEN ? (uint32_t)((H - 2) * W) : (uint32_t)((2 * ry + 1) * (2 * rx + 1));
}
static __host__ __device__ inline uint64_t rg_nov_pos_word(int px, int py) { return (uint64_t)(uint32_t)(px & 0xffff) | ((uint64_t)(uint32_t)(py & 0xffff) << 16); }
// byte k < L of the key of RG_NOV_SCREEN / RG_NOV_CROP; `screen` = the env's mirror u8 [H][W]
static __host__ __device__ inline uint32_t rg_nov_key_byte(int what, const uint8_t *screen, int H, int W, int px, int py, int ry, int rx, uint32_t k) {
    if (what == RG_NOV_SCREEN) return screen[(uint32_t)W + k];
    const int wc = 2 * rx + 1, j = (int)k / wc, y = py - ry + j, x = px - rx + ((int)k - j * wc);
    return (y >= 1 && y <= H - 2 && x >= 0 && x < W) ? screen[y * W + x] : (uint32_t)' ';
}
// word i of the zero-padded key, byte by byte (the form for any geometry; the device reads aligned whole-screen keys 16 bytes at a time instead)
static __host__ __device__ inline uint64_t rg_nov_key_word(int what, const uint8_t *screen, int H, int W, int px, int py, int ry, int rx, uint32_t L, uint32_t i) {
    uint64_t w = 0;
    for (uint32_t b = 0; b < 8; b++) {
        const uint32_t k = 8 * i + b;
        if (k < L) w |= (uint64_t)rg_nov_key_byte(what, screen, H, W, px, py, ry, rx, k) << (8 * b);
    }
    return w;
}
// The episodic insert on one env's table: the visit's count, 0 = dropped.
static __host__ __device__ inline uint32_t rg_nov_insert(RgNovSlot *tab, uint32_t cap, uint32_t gen, uint64_t hash) {
    uint32_t at = (uint32_t)hash & (cap - 1);
    for (uint32_t p = 0; p < cap; p++, at = (at + 1) & (cap - 1)) {
        RgNovSlot s = tab[at];
        if (s.gen != gen) { s.hash = hash; s.gen = gen; s.count = 1; tab[at] = s; return 1; }
        if (s.hash == hash) { s.count += 1; tab[at] = s; return s.count; }
    }
    return 0;
}
static inline bool rg_nov_pow2_in(long long v, long long lo, long long hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }
