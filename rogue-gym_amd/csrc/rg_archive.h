// rg_archive.h -- the cell archive: per hashed state ("cell") the best state record any env has offered (rg_archive_*).  THE statement of the rule, as
// rg_novelty.h is for the visit counts.  Host and device, plain C++: the kernels (rg_archive.hip, librogue_gym_archive.so) and the host twin
// (rga_offer_host below, behind rg_archive_offer_host) both call the pieces below.
//
// OFFER.  (key, score, steps, env): key u64, offered as 1 where it is 0 (0 marks an empty slot; the novelty hash never is 0); score i32, larger is better;
// steps u32, the length of the env's running episode, shorter is better; env the env id.
// BEATS.  A beats B iff score_A > score_B, or the scores are equal and steps_A < steps_B.  Packed as bid = (score + 2^31) << 32 | ~steps (rg_arc_bid) that is
// bid_A > bid_B as u64.  Among the offers of ONE call with equal (score, steps) the lowest env id wins.
// TABLE.  One per handle, `cells` slots (a power of two, 1 024 .. 2^24), open addressing: linear probing from key & (cells - 1), step 1, at most
// min(cells, RG_ARC_PROBES) probes; every probe claims (a zero key, by one 64-bit compare-and-swap on the device), matches or moves on.  An offer that finds
// neither its key nor an empty slot by then is DROPPED: its slot is -1 and it is counted.  A slot holds key, the stored offer's score and steps, seen (the
// offers the key ever received), chosen (how often it was restored from), when (the serial of the update call that last wrote it, from 1; 0 = no record
// yet, which anything beats) and a state record of R bytes.
// UPDATE.  For every key offered in a call: seen grows by the number of offers; if the call's best offer beats the stored one STRICTLY (or there is none), that
// env's state record replaces the stored record and (score, steps, when) follow.  An equal (score, steps) from a later call replaces nothing.  slot[e] is the
// env's slot (-1: dropped, or masked out), stored[e] is 1 iff this env's record was written in this call.  Except for which slot a key lands in, the table
// after a call is a function of the offers alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#define RG_ARC_SLACK 64          // every per-env array is allocated with this many envs of slack behind the last one, which no launch writes
#define RG_ARC_CELLS_MIN 1024
#define RG_ARC_CELLS_MAX (1 << 24)
#define RG_ARC_PROBES 1024       // probes of an offer at most (= RG_ARC_CELLS_MIN)

// the arrays of a handle (device pointers)
struct RgArchive {
    uint64_t *key; int32_t *score; uint32_t *steps, *seen, *chosen, *when; uint8_t *records;   // [cells] public (rg_archive_arrays); records [cells][R]
    unsigned long long *bid, *win;   // [cells] the call's best bid (0 between calls) and (serial << 32 | ~env) of the env that takes the slot
    int32_t *slot; uint8_t *stored; int32_t *score_in; uint32_t *steps_in;   // [N + slack] public
    int32_t *list; uint32_t *cnt;    // [N] the envs whose record this call writes, [1] their number
    unsigned long long *stat;        // [4] occupied, dropped offers, records written, (unused)
    int32_t cells; uint32_t R;
};

// a slot of the HOST twin's table (rg_archive_offer_host): the device keeps the same words as arrays
struct RgArcSlot { uint64_t key; int32_t score; uint32_t steps, seen, chosen, when, zero; };

static __host__ __device__ inline uint64_t rg_arc_key(uint64_t key) { return key ? key : 1ull; }
static __host__ __device__ inline uint64_t rg_arc_bid(int32_t score, uint32_t steps) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(~steps);
}
static __host__ __device__ inline bool rg_arc_beats(int32_t score, uint32_t steps, uint32_t when_b, int32_t score_b, uint32_t steps_b) {
    return when_b == 0 || rg_arc_bid(score, steps) > rg_arc_bid(score_b, steps_b);
}
static __host__ __device__ inline uint32_t rg_arc_probes(uint32_t cells) { return cells < RG_ARC_PROBES ? cells : RG_ARC_PROBES; }
static inline bool rg_arc_pow2_in(long long v, long long lo, long long hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

// The host twin: ONE offer on a host table of `cells` slots.  *slot = the key's slot or -1 (dropped, nothing written); *stored = 1 iff the offer replaced
// the stored one.  (Offers of one call given in ascending env order: the strict rule keeps the lowest env id among equals.)
static inline int rga_offer_host(std::string &err, void *slots, int cells, uint64_t key, int32_t score, uint32_t steps, uint32_t serial, int32_t *slot, int32_t *stored) {
    const std::string w = "rg_archive_offer_host: ";
    if (!slots) { err = w + "slots is NULL"; return 1; }
    if ((uintptr_t)slots & 7u) { err = w + "slots must be 8-byte aligned"; return 1; }
    if (!rg_arc_pow2_in(cells, 1, RG_ARC_CELLS_MAX)) { err = w + "cells must be a power of two, 1 <= cells <= " + std::to_string(RG_ARC_CELLS_MAX) + ", got " + std::to_string(cells); return 1; }
    if (serial == 0) { err = w + "serial must not be 0 (0 marks a slot without a record)"; return 1; }
    if (!slot || !stored) { err = w + "slot and stored must not be NULL"; return 1; }
    RgArcSlot *tab = static_cast<RgArcSlot *>(slots);
    const uint32_t m = (uint32_t)cells - 1u, last = rg_arc_probes((uint32_t)cells);
    key = rg_arc_key(key);
    uint32_t at = (uint32_t)key & m;
    *slot = -1; *stored = 0;
    for (uint32_t p = 0; p < last; p++, at = (at + 1u) & m) {
        RgArcSlot &s = tab[at];
        if (s.key == 0) s.key = key;
        if (s.key != key) continue;
        *slot = (int32_t)at;
        s.seen += 1;
        if (rg_arc_beats(score, steps, s.when, s.score, s.steps)) { s.score = score; s.steps = steps; s.when = serial; *stored = 1; }
        break;
    }
    return 0;
}
