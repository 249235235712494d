// rg_action_mask.h -- which keys of KeyMap::ai do anything for an env right now: THE statement of the rule (rg_action_mask / rg_action_mask_host) and the
// stateless draw among the legal keys (rg_sample_index).  Host and device: k_action_mask (rg_action_mask.hip) and rg_action_mask_host (rg_readers_host.h) both
// call rg_key_legal's pieces, so the rule is written once.  file:line citations name the reference's sources.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rg_state.h"

// bits of rg_legal_bits: 0..7 the Direction enum order (dungeon/coord.rs:198-242: Up Down Left Right LeftUp RightUp LeftDown RightDown), then '>' and the
// keys that always act ('.' NoOp, 's' Search)
#define RG_LB_STAIR 8
#define RG_LB_ALWAYS 9
#define RG_LB_NONE 15   // not a key of KeyMap::ai

// the surface of a cell word can be stood on (Surface::can_walk, rogue/mod.rs:177-182)
static __host__ __device__ inline bool rg_walkable(uint32_t c) {
    const uint32_t s = c & C_SURF_MASK;
    return !(s == S_WALLX || s == S_WALLY || s == S_NONE);
}

// Floor::can_move_impl as the player (floor.rs:169-182): the target inside the grid, walkable, neither hidden nor locked; for a diagonal both orthogonal
// neighbours inside the grid and walkable -- their SURFACE only.  A monster on the target changes nothing (the move is an attack, actions.rs:168-231).
static __host__ __device__ inline bool rg_can_move(const uint16_t *cell, int H, int W, int px, int py, int dx, int dy) {
    const int x = px + dx, y = py + dy;
    if (x < 0 || y < 0 || x >= W || y >= H) return false;
    const uint32_t t = cell[y * W + x];
    bool ok = rg_walkable(t) && !(t & (C_HIDDEN | C_LOCKED));
    if (dx != 0 && dy != 0) ok = ok && rg_walkable(cell[py * W + x]) && rg_walkable(cell[y * W + px]);  // (inside the grid whenever the target is)
    return ok;
}

// Every answer for one env as bits (RG_LB_*).  An env in the Grave modal answers every key, '.' included, with IgnoredInput (core/src/lib.rs:301-315): 0.
static __host__ __device__ inline uint32_t rg_legal_bits(const uint16_t *cell, int H, int W, int px, int py, int dead) {
    uint32_t b = 1u << RG_LB_ALWAYS;
    b |= (uint32_t)rg_can_move(cell, H, W, px, py, 0, -1) << 0;
    b |= (uint32_t)rg_can_move(cell, H, W, px, py, 0, 1) << 1;
    b |= (uint32_t)rg_can_move(cell, H, W, px, py, -1, 0) << 2;
    b |= (uint32_t)rg_can_move(cell, H, W, px, py, 1, 0) << 3;
    b |= (uint32_t)rg_can_move(cell, H, W, px, py, -1, -1) << 4;
    b |= (uint32_t)rg_can_move(cell, H, W, px, py, 1, -1) << 5;
    b |= (uint32_t)rg_can_move(cell, H, W, px, py, -1, 1) << 6;
    b |= (uint32_t)rg_can_move(cell, H, W, px, py, 1, 1) << 7;
    b |= (uint32_t)((cell[py * W + px] & C_SURF_MASK) == S_STAIR) << RG_LB_STAIR;  // '>' asks for the surface under the player (actions.rs:16-65)
    return dead ? 0u : b;  // (a select at the end, not a branch at the top: the kernel's cell loads do not wait for its flag word)
}

// KeyMap::ai (input.rs:73-100; j is down, k is up): the bit of rg_legal_bits that answers `key`; a run key (MoveUntil) is judged by its first move
static __host__ __device__ inline uint32_t rg_key_bit(uint8_t key) {
    switch (key | 0x20) {  // (letters: the lower case; the three others are checked exactly below)
    case 'k': return 0; case 'j': return 1; case 'h': return 2; case 'l': return 3;
    case 'y': return 4; case 'u': return 5; case 'b': return 6; case 'n': return 7;
    default: break;
    }
    return key == '>' ? RG_LB_STAIR : (key == '.' || key == 's') ? RG_LB_ALWAYS : RG_LB_NONE;
}

// One key for one env: 0 = the reference would answer it with CantMove, with "no downstairs" or with IgnoredInput.  `cell` = u16 [H][W] cell words
// (surface in bits 0-2, CellAttr << 4: rg_state.h), (px, py) the player's cell, dead = RG_FLAG_DEAD.
static __host__ __device__ inline uint32_t rg_key_legal(const uint16_t *cell, int H, int W, int px, int py, int dead, uint8_t key) {
    return (rg_legal_bits(cell, H, W, px, py, dead) >> rg_key_bit(key)) & 1u;
}

// The draw among `count` legal keys of env `env` at the caller's counter `draw`: a splitmix64 finalizer over the three, all arithmetic mod 2^64, and the
// high word scaled to [0, count).  Stateless: the same arguments give the same index.
static __host__ __device__ inline uint32_t rg_sample_index_of(uint64_t seed, uint32_t env, uint64_t draw, uint32_t count) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)env + 1ull) + 0xD1B54A32D192ED03ull * draw;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return count ? (uint32_t)(((z >> 32) * (uint64_t)count) >> 32) : 0u;
}
