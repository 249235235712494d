// rg_monsters.h -- the monsters of an env's level as an entity table, and the threat words: THE statement of the rule (rg_monsters / rg_monsters_host).
// Host and device: k_monsters (rg_monsters.hip) and rg_monsters_host (rg_readers_host.h) both call the pieces below, so the rule is written once.
// file:line citations name the reference's sources.
//
// A monster of the env's current level is ALIVE when its slot has MF_ALIVE.  It is SHOWN when a Redraw at this moment would put its letter on the screen --
// RunTime::draw_screen (core/src/lib.rs:264-285; rogue/mod.rs:278-300,398-404), which rg_obs.hip's k_render restates: its row is in 1 .. H-2, its cell word
// has C_VISIBLE or C_DRAWN, it is not the player's cell, the cell holds no gold (gold is drawn over a monster), and either dx*dx + dy*dy <= 2 or
// Floor::in_same_room (floor.rs:381-393) holds: same assigned area and, unless the room is Empty, both cells inside the room's rect or both outside it.
//
// RG_MON_SHOWN lists the shown monsters: nothing the screen cannot show.  RG_MON_ALL lists every alive monster of the level and is PRIVILEGED in the sense of
// rg_path.h: it sees monsters the player has not met, their hit points and whether they are awake.  A teacher, a shaping term or a critic input, not an
// observation the reference's player has.
//
// THE RULE READS THE GAME STATE, NOT THE SCREEN MIRROR.  The reference redraws its mirror only on a key that produces a Redraw.  Measured on the CPU engine
// (mini + enemies 0..11, 136 seeds x 120 random steps, 16 320 rows): 7 733 rows have a shown monster; in 811 of them the mirror does not carry the letter at
// the listed cell, and all 811 fall on steps whose key produced no Redraw, none on the 5 439 steps that redrew.  So the table equals the reference's own
// drawing whenever it draws, and between Redraws it is more current than the image.  tests/test_monsters_host.py pins both facts.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rogue_gym_hip.h"  // RG_MON_*
#include "rg_state.h"

#define RG_MON_EMPTY_KEY 0xffffffffffffffffull   // cheb <= 159: no monster has this key

// what the rule needs of an env besides its monsters: the player's cell, the assigned area the player stands in (ax1 <= ax0: none) and that room's rect
struct RgMonEnv {
    int px, py, H;
    int ax0, ay0, ax1, ay1;   // Room::assigned_area of the player's cell (rooms.rs:192-209), half-open
    int rx0, ry0, rx1, ry1;   // the room's rect, half-open
    bool empty, p_in;         // the room is Empty; the player's cell is inside the rect
};

// Floor::cd_to_room_id (floor.rs:194-200) by arithmetic -- the areas are disjoint: the id of the area that holds (x, y), -1 = none (row 0, the last row, the
// columns and rows past the last area); the area itself into E.  (Plain integer divisions: two per env.)
static __host__ __device__ inline int rg_mon_area(RgMonEnv &E, int x, int y, int W, int H, int rnx, int rny) {
    const int rsx = W / rnx, rsy = H / rny, cx = x / rsx, cy = y / rsy;
    E.ax0 = E.ay0 = E.ax1 = E.ay1 = 0;
    if (y < 1 || x < 0 || cx >= rnx || cy >= rny) return -1;
    if ((cy + 1) * rsy == H && y == H - 1) return -1;
    E.ax0 = cx * rsx; E.ax1 = E.ax0 + rsx;
    E.ay0 = cy == 0 ? 1 : cy * rsy; E.ay1 = (cy + 1) * rsy;
    if (E.ay1 == H) E.ay1 -= 1;
    return cy * rnx + cx;
}
// the room of the player's area: rect = x0 | y0<<8 | x1<<16 | y1<<24, meta = RM_* (rg_state.h)
static __host__ __device__ inline void rg_mon_room(RgMonEnv &E, uint32_t rect, uint32_t meta) {
    E.rx0 = (int)(rect & 0xff); E.ry0 = (int)((rect >> 8) & 0xff); E.rx1 = (int)((rect >> 16) & 0xff); E.ry1 = (int)(rect >> 24);
    E.empty = (meta & RM_KIND_MASK) == RK_EMPTY;
    E.p_in = E.px >= E.rx0 && E.px < E.rx1 && E.py >= E.ry0 && E.py < E.ry1;
}
// Floor::in_same_room(player, (x, y))
static __host__ __device__ inline bool rg_mon_same_room(const RgMonEnv &E, int x, int y) {
    if (!(x >= E.ax0 && x < E.ax1 && y >= E.ay0 && y < E.ay1)) return false;   // (an empty area holds nothing: the player stands in none)
    if (E.empty) return true;
    const bool in = x >= E.rx0 && x < E.rx1 && y >= E.ry0 && y < E.ry1;
    return in == E.p_in;
}
// c = the cell word under the monster at (x, y)
static __host__ __device__ inline bool rg_mon_shown(const RgMonEnv &E, uint32_t c, int x, int y) {
    if (y < 1 || y >= E.H - 1 || !(c & (C_VISIBLE | C_DRAWN)) || (c & C_GOLD) || (x == E.px && y == E.py)) return false;
    const int dx = x - E.px, dy = y - E.py;
    return dx * dx + dy * dy <= 2 || rg_mon_same_room(E, x, y);
}

// The order: ascending by (cheb, dx*dx + dy*dy, x<<8|y).  One 64-bit key: cheb in bits 56.., d2 (< 2^15) in 40.., the position word in 24.., and below it
// what does not take part in the order (positions are unique): shown in bit 23, the table slot (< 384) in bits 0..8.
static __host__ __device__ inline uint64_t rg_mon_key(int px, int py, int x, int y, bool shown, int slot) {
    const int dx = x - px, dy = y - py, ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, cheb = ax > ay ? ax : ay;
    return (uint64_t)cheb << 56 | (uint64_t)(dx * dx + dy * dy) << 40 | (uint64_t)((x << 8) | y) << 24 | (uint64_t)shown << 23 | (uint64_t)slot;
}
static __host__ __device__ inline int rg_mon_key_cheb(uint64_t k) { return (int)(k >> 56); }
// ... and beside it one word: the tile in bits 0..7, active in bit 8, min(hp, 32767) as an int16 in bits 16..31 (the stepper holds no alive monster with
// hp <= 0; a caller's negative value stays what it is, down to -32768)
static __host__ __device__ inline uint32_t rg_mon_pay(uint32_t tile, bool active, int32_t hp) {
    const int32_t h = hp > 32767 ? 32767 : hp < -32768 ? -32768 : hp;
    return (tile & 0xffu) | (uint32_t)active << 8 | ((uint32_t)h & 0xffffu) << 16;
}
// a row of the table as four words (eight int16): tile, dx, dy, cheb, shown | ALL only: active, hp, slot
static __host__ __device__ inline void rg_mon_row(uint64_t key, uint32_t pay, int px, int py, uint32_t mode, uint32_t r[4]) {
    if (key == RG_MON_EMPTY_KEY) { r[0] = r[1] = r[2] = r[3] = 0u; return; }
    const int x = (int)((key >> 32) & 0xff), y = (int)((key >> 24) & 0xff);
    const uint32_t dx = (uint32_t)(x - px) & 0xffffu, dy = (uint32_t)(y - py) & 0xffffu, shown = (uint32_t)(key >> 23) & 1u;
    const bool all = mode == RG_MON_ALL;
    r[0] = (pay & 0xffu) | dx << 16;
    r[1] = dy | (uint32_t)rg_mon_key_cheb(key) << 16;
    r[2] = shown | (all ? ((pay >> 8) & 1u) << 16 : 0u);
    r[3] = all ? (pay >> 16) | ((uint32_t)key & 0x1ffu) << 16 : 0u;
}
// The positional attack mask: the bit of the move key of RG_ACTION_KEYS[1 + i] (h j k l n b u y) that aims at (px + dx, py + dy), dx, dy in -1 .. 1; 0 for
// the own cell.  Positional only: it says nothing about the corner rule -- AND it with the action mask for legality.
static __host__ __device__ inline uint32_t rg_mon_attack_bit(int dx, int dy) {
    return (1u << ((0x415380627ull >> (4 * ((dy + 1) * 3 + dx + 1))) & 15u)) & 0xffu;   // y k u / h . l / b j n -> bits 7 2 6 / 0 - 3 / 5 1 4
}

// the threat words, always over the SHOWN monsters: [0] shown with cheb == 1, [1] the least cheb of a shown monster or -1, [2] the attack mask,
// [3] the monsters that qualify in the call's mode
struct RgMonThreat { int32_t adjacent, nearest, attack, count; };
static __host__ __device__ inline void rg_mon_threat_init(RgMonThreat &T) { T.adjacent = 0; T.nearest = -1; T.attack = 0; T.count = 0; }
static __host__ __device__ inline void rg_mon_threat_add(RgMonThreat &T, int px, int py, int x, int y, bool shown, bool qualifies) {
    T.count += (int32_t)qualifies;
    if (!shown) return;
    const int dx = x - px, dy = y - py, ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, cheb = ax > ay ? ax : ay;
    if (T.nearest < 0 || cheb < T.nearest) T.nearest = cheb;
    if (cheb == 1) { T.adjacent += 1; T.attack |= (int32_t)rg_mon_attack_bit(dx, dy); }
}
