// rg_objects.h -- the stairs, gold, doors and frontier cells of an env's level as an object table ordered by walking distance: THE statement of the rule
// (rg_objects / rg_objects_host), on top of rg_route.h.  Host and device: k_objects (rg_objects.hip) and rg_objects_host (rg_readers_host.h) both call the
// pieces below, so the rule is written once.
//
// mode is rg_route's: RG_ROUTE_SECRETS walks THROUGH hidden / locked cells, RG_ROUTE_KNOWN reads the player's own map only (C_DRAWN / C_VISIBLE) -- with
// it nothing in the answer is privileged; without it the table is PRIVILEGED in the sense of rg_path.h: it lists what the player has not discovered.
//
// A cell is ONE object.  Its kind word is the OR of the asked kinds it satisfies (rg_obj_kind): stairs and doors by the surface where K, gold where K and
// not under the player (rg_path's rule: gold is taken by moving onto it), the frontier by rg_route_frontier.  A hidden door keeps the wall surface it was
// dug into and is no door.
//
// walk of a cell = the number of moves from the player's cell to it in rg_route's search graph under `mode`: the target of a move is `pass`, both
// orthogonal neighbours of a diagonal are `corner`, the player's own cell starts the search whatever its word, monsters are ignored.  The graph is
// symmetric, so it is what rg_route answers as the distance when the cell is given as RG_GOAL_CELL under the same mode.  A qualifying cell the search
// does not reach is counted and not listed; the own cell is listed with walk 0 when it qualifies.
//
// The table holds the listed objects in ascending order of (walk, y, x), the first `cap` of them, as rows of RG_OBJ_COLS int16 (rg_obj_row); rows past
// the last listed object are all zero.  count[k] = the qualifying cells of kind bit k, reached or not, 0 for a kind that was not asked for.  An env in the
// Grave modal answers an all-zero table and zero counts.
#pragma once
#include <cstdint>

#include "rg_route.h"  // (and through it include/rogue_gym_hip.h: RG_OBJ_*)

#define RG_OBJ_KINDS_ALL (RG_OBJ_STAIRS | RG_OBJ_GOLD | RG_OBJ_DOOR | RG_OBJ_FRONTIER)

// the kinds a cell word decides alone; c = the cell word, own = it is the player's cell
static __host__ __device__ inline uint32_t rg_obj_kind_word(uint32_t c, uint32_t kinds, uint32_t mode, bool own) {
    if (!rg_route_k(c, mode, own)) return 0u;
    const uint32_t s = c & C_SURF_MASK;
    return kinds & ((s == S_STAIR ? RG_OBJ_STAIRS : 0u) | (((c & C_GOLD) && !own) ? RG_OBJ_GOLD : 0u) | (s == S_DOOR ? RG_OBJ_DOOR : 0u));
}
// ... and with the frontier, which needs the neighbours: unknown_beside as rg_route_frontier's
static __host__ __device__ inline uint32_t rg_obj_kind(uint32_t c, uint32_t kinds, uint32_t mode, bool own, bool unknown_beside) {
    return rg_obj_kind_word(c, kinds, mode, own) | (((kinds & RG_OBJ_FRONTIER) && rg_route_frontier(c, mode, own, unknown_beside)) ? RG_OBJ_FRONTIER : 0u);
}
// a row of the table as four words (eight int16): kind, dx | dy, walk | x, y | max(|dx|, |dy|), 0
static __host__ __device__ inline void rg_obj_row(uint32_t kind, int px, int py, int x, int y, uint32_t walk, uint32_t r[4]) {
    const int dx = x - px, dy = y - py, ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    r[0] = (kind & 0xffffu) | ((uint32_t)dx & 0xffffu) << 16;
    r[1] = ((uint32_t)dy & 0xffffu) | (walk & 0xffffu) << 16;
    r[2] = (uint32_t)x | (uint32_t)y << 16;
    r[3] = (uint32_t)(ax > ay ? ax : ay);
}
