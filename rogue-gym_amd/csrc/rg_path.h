// rg_path.h -- shortest-path fields towards goal cells and the teacher key that follows them: THE statement of the rule (rg_path / rg_path_host).
// Host and device: k_path (rg_path.hip) and rg_path_host (rg_readers_host.h) both call the pieces below, and the move test itself is rg_action_mask.h's
// rg_walkable / rg_can_move (Floor::can_move_impl as the player), so nothing is stated twice.
//
// The field is PRIVILEGED: it sees stairs, gold and passages the player has not discovered.  It is a teacher, a shaping potential or a critic input,
// not an observation the reference's player has.
#pragma once
#include <cstdint>

#include "../../include/rogue_gym_hip.h"  // RG_GOAL_*, RG_PATH_UNREACHABLE
#include "rg_action_mask.h"

#define RG_PATH_GOALS_ALL (RG_GOAL_STAIRS | RG_GOAL_GOLD | RG_GOAL_CELL)
#define RG_PATH_INF RG_PATH_UNREACHABLE

// a cell a move may end on: what rg_can_move demands of its target
static __host__ __device__ inline bool rg_path_ok(uint32_t c) { return rg_walkable(c) && !(c & (C_HIDDEN | C_LOCKED)); }

// Is the cell a goal?  `own` = it is the player's cell (gold is taken by moving ONTO it, and the generator can put the player down on a gold cell),
// `given` = it is the caller's cell of RG_GOAL_CELL.  A goal has D = 0 whatever its own word; one that is not rg_path_ok is never expanded.
static __host__ __device__ inline bool rg_path_goal(uint32_t c, uint32_t goals, bool own, bool given) {
    return ((goals & RG_GOAL_STAIRS) && (c & C_SURF_MASK) == S_STAIR) || ((goals & RG_GOAL_GOLD) && (c & C_GOLD) && !own) ||
           ((goals & RG_GOAL_CELL) && given);
}

// Direction enum order (dungeon/coord.rs:198-242: Up Down Left Right LeftUp RightUp LeftDown RightDown) -- the bit order of rg_legal_bits -- as
// (dx, dy) and as keys of KeyMap::ai, packed into immediates
static __host__ __device__ inline int rg_path_dx(int d) { return (int)((0x20202011u >> (4 * d)) & 3u) - 1; }  // 0 0 -1 1 -1 1 -1 1
static __host__ __device__ inline int rg_path_dy(int d) { return (int)((0x22001120u >> (4 * d)) & 3u) - 1; }  // -1 1 0 0 -1 -1 1 1
static __host__ __device__ inline uint8_t rg_path_dir_key(int d) { return (uint8_t)(0x6E6275796C686A6Bull >> (8 * d)); }  // k j h l y u b n

// The teacher key.  dead = RG_FLAG_DEAD; d = D at the player's cell (RG_PATH_INF: unreachable); stairs_here = the surface under the player is the stairs
// and RG_GOAL_STAIRS is in the set; dirs = bit i set iff direction i satisfies rg_can_move from the player's cell and its target's D is d - 1 (consulted
// for 0 < d < RG_PATH_INF only; one bit is always set then, the guard is for a caller's defect).
static __host__ __device__ inline uint8_t rg_path_key(int dead, uint32_t d, bool stairs_here, uint32_t dirs) {
    if (dead) return (uint8_t)'.';
    if (d == 0) return (uint8_t)(stairs_here ? '>' : '.');
    if (d == RG_PATH_INF || !(dirs & 0xffu)) return (uint8_t)'s';  // Search is what reveals hidden cells
    return rg_path_dir_key(__builtin_ctz(dirs & 0xffu));
}
static __host__ __device__ inline int32_t rg_path_dist(uint32_t d) { return d == RG_PATH_INF ? -1 : (int32_t)d; }
