// rg_route.h -- search-aware and map-aware routes: THE statement of the rule (rg_route / rg_route_host), on top of rg_path.h and rg_action_mask.h.
// Host and device: k_route (rg_route.hip) and rg_route_host (rg_readers_host.h) both call the pieces below.
//
// rg_path's rule has one notion of "passable".  Here two orthogonal mode bits vary it: RG_ROUTE_SECRETS plans THROUGH hidden / locked cells and asks for
// 's' when the next cell is one (Search touches the eight cells around the player, floor.rs:349-370); RG_ROUTE_KNOWN plans on the player's own map only
// (C_DRAWN / C_VISIBLE, which the state keeps bit-exact with the reference), so its answers are NOT privileged.  With mode 0, no frontier goal and no
// fallback every answer equals rg_path's.
#pragma once
#include <cstdint>

#include "rg_path.h"

#define RG_ROUTE_GOALS_ALL (RG_PATH_GOALS_ALL | RG_GOAL_FRONTIER)
#define RG_ROUTE_MODE_ALL (RG_ROUTE_SECRETS | RG_ROUTE_KNOWN)
#define RG_ROUTE_NO_TIER 255u

static __host__ __device__ inline bool rg_route_secret(uint32_t c) { return (c & (C_HIDDEN | C_LOCKED)) != 0; }
// the cell is on the player's map: drawn or in view, or the player's own (`own`)
static __host__ __device__ inline bool rg_route_known(uint32_t c, bool own) { return (c & (C_DRAWN | C_VISIBLE)) != 0 || own; }
// K: the cell may be planned on at all
static __host__ __device__ inline bool rg_route_k(uint32_t c, uint32_t mode, bool own) { return !(mode & RG_ROUTE_KNOWN) || rg_route_known(c, own); }
// what the corner rule of a diagonal asks of the two orthogonal neighbours: the surface as it is NOW, which is what the engine's move test reads
static __host__ __device__ inline bool rg_route_corner(uint32_t c, uint32_t mode, bool own) { return rg_walkable(c) && rg_route_k(c, mode, own); }
// What a move of the search graph may end on.  A secret cell is a passage or door cell that was never drawn into the grid: it keeps the surface it was dug
// into -- a room's wall, bare rock -- until Search finds it (floor.rs:93-100, 359-366), so with RG_ROUTE_SECRETS its attr alone makes it a cell of the route.
static __host__ __device__ inline bool rg_route_pass(uint32_t c, uint32_t mode, bool own) {
    return rg_route_k(c, mode, own) && (rg_route_secret(c) ? (mode & RG_ROUTE_SECRETS) != 0 : rg_walkable(c));
}
// The goals a cell word decides alone: stairs and gold as rg_path_goal, but only where K; the caller's cell whatever its word.  The frontier needs the
// neighbours: rg_route_frontier.
static __host__ __device__ inline bool rg_route_goal(uint32_t c, uint32_t goals, uint32_t mode, bool own, bool given) {
    return (rg_route_k(c, mode, own) && rg_path_goal(c, goals & (RG_GOAL_STAIRS | RG_GOAL_GOLD), own, false)) || ((goals & RG_GOAL_CELL) && given);
}
// A frontier cell: pass, with an in-grid ORTHOGONAL neighbour that is not known.  Standing on a cell draws its four orthogonal neighbours unless they are
// hidden, so a frontier cell is resolved by stepping onto it, and a player standing on one stands next to a hidden cell.  unknown_beside = some in-grid
// orthogonal neighbour is not rg_route_known.
static __host__ __device__ inline bool rg_route_frontier(uint32_t c, uint32_t mode, bool own, bool unknown_beside) { return rg_route_pass(c, mode, own) && unknown_beside; }

// The key.  d, dirs as rg_path_key, with dirs bit i set iff direction i is a move of the search graph from the player's cell, its target's D is d - 1 AND
// its target is not secret -- so a move key is always legal by rg_can_move.  goals = the goal word of the tier that answers.  No such direction at a
// finite d > 0: the next cell is a secret one of the eight neighbours, which is exactly where Search works.
static __host__ __device__ inline uint8_t rg_route_key(int dead, uint32_t d, uint32_t goals, bool on_stairs, bool own_frontier, uint32_t dirs) {
    if (dead) return (uint8_t)'.';
    if (d == 0) return (uint8_t)(((goals & RG_GOAL_STAIRS) && on_stairs) ? '>' : ((goals & RG_GOAL_FRONTIER) && own_frontier) ? 's' : '.');
    return rg_path_key(0, d, false, dirs);
}
