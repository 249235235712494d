// rg_obs_dev.h -- the device code that the observation units share: rg_obs.hip (k_obs, k_obs_stream, k_obs_resid, k_redraw) and rg_obs_fix.hip (k_obs_fix,
// librogue_gym_obsfix.so).  The observation store, the observation record staged in LDS, phases A and B of a Redraw, and the Redraw service of one env by one
// wave (RG_OBS_REDRAW_ENV).  ONE text for every kernel that draws a Redraw, so that they cannot drift apart.  Device only; include after rg_device.h.
// file:line citations are relative to the reference's tree, as in rg_obs.hip.
#pragma once
#include "rg_device.h"

// The observation tensor is a write-once 134 MB stream per step (mini gray): non-temporal stores keep it from evicting the
// env state (tile grids, mirrors, tables) that the next k_step re-reads from L2 / Infinity Cache.
__device__ __forceinline__ void store_obs(float4 *p, float4 v) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    f4v nv = {v.x, v.y, v.z, v.w};
#ifdef RG_EXP_OBS_PLAIN_STORES
    *reinterpret_cast<f4v *>(p) = nv;  // (experiment build: profiles/r06_experiments.txt)
#else
    __builtin_nontemporal_store(nv, reinterpret_cast<f4v *>(p));
#endif
}
// Per-env overlay inputs staged in LDS, in the layout of the env's OBSERVATION RECORD (RgState::obs_rec, RG_OBS_REC_WORDS): words [0, nr) the monster
// words, [nr] the player's position, [nr + 1, 2 nr + 1) the room rects, then the room metas one byte each.  The record is what an ordinary Redraw reads --
// one 64-byte line per env, written by whoever writes the env's tables (k_step: monsters and player after every turn that redraws; the generator and the
// spare hand-off: the rooms) -- instead of the env's column of four
// [slot][env] tables: 16 lines of 64 bytes for 52 useful ones, 0.43 x 65 536 times per step (28 MB of the pass's 228; measured: 44.7 -> 40.3 us).
// The gold overlay needs no table at all: the tile word carries Floor::items' membership bit (C_GOLD).
struct ObsTabs { uint32_t w[RG_OBS_REC_WORDS(RG_OBS_MAX_ROOMS)]; };
#define OBS_ENV_BYTES(hw) ((((size_t)(hw) + sizeof(ObsTabs)) + 15) & ~(size_t)15)

// Phase A of a Redraw (RunTime::draw_screen, rogue/mod.rs:278-290): the 8 tile words of uint4 `i` of an env's grid (cells 8i .. 8i+7) -> 8 glyph bytes
// (bit 7: an object on the cell is drawn, draw_ranges) and 8 visited bytes of the history plane
__device__ __forceinline__ void draw_cells8(uint4 v, int i, int W, int HW, uint32_t g[2], uint32_t hb[2]) {
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
    g[0] = g[1] = hb[0] = hb[1] = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        uint32_t cw = (q[t >> 1] >> ((t & 1) * 16)) & 0xffff;
        int idx = i * 8 + t;
        bool inner = idx >= W && idx < HW - W;  // rows 1..H-2 only (rogue/mod.rs:278-290)
        uint32_t gl = ' ';
        if (inner && (cw & C_VISIBLE)) gl = glyph_of(cw);
        if (inner && (cw & (C_VISIBLE | C_DRAWN))) gl = ((cw & C_GOLD) ? (uint32_t)'*' : gl) | 0x80u;  // bit 7: an object on this cell is drawn (draw_ranges);
                                                                                                  // gold is drawn over a monster, under the player
        g[t >> 2] |= gl << ((t & 3) * 8);
        hb[t >> 2] |= ((cw & C_VISITED) ? 1u : 0u) << ((t & 3) * 8);
    }
}
// Phase B: whether the monster at (x, y) is drawn as seen from the player at (px, py) (core/src/lib.rs:271-283): adjacent, or in the same room
// (Floor::in_same_room, floor.rs:381-393) -- room rects and metas from the env's observation record staged in LDS
__device__ __forceinline__ bool monster_shown(const RgConfig &c, const ObsTabs *tb, int nrooms, int px, int py, int x, int y) {
    int dx = px - x, dy = py - y;
    bool show = dx * dx + dy * dy <= 2;
    if (!show) {
        int id = room_id_of(c, px, py);
        if (id >= 0 && room_id_of(c, x, y) == id) {
            if ((reinterpret_cast<const uint8_t *>(&tb->w[2 * nrooms + 1])[id] & RM_KIND_MASK) == RK_EMPTY) show = true;
            else {
                int x0, y0, x1, y1;
                unpack_rect(tb->w[nrooms + 1 + id], x0, y0, x1, y1);
                bool ina = px >= x0 && px < x1 && py >= y0 && py < y1, inb = x >= x0 && x < x1 && y >= y0 && y < y1;
                show = ina == inb;
            }
        }
    }
    return show;
}

// The Redraw service of k_obs_stream, k_obs_resid and k_obs_fix: one env with a pending Redraw, drawn from its tiles by the whole wave (the staged path of k_obs: LDS
// draw, overlays, mirror write-back, encode, flag word; the barriers are the wave's own).  ONE text for these kernels, so that they cannot drift apart -- a macro
// and not a function, like RG_STEP_BLOCK_BODY: k_obs_stream's registers are pinned (tests/test_obs_typed_resources.py), and as an inlined function the same
// statements cost it one more.  It reads the caller's S, c, out, lane, W, HW, Q4, Q8, nrooms, rec_words, gray4 and LDS arrays (scr, tb, mtile), and e, fle, v,
// t_rec: the env, its flag word, and its tile words and observation record, loaded ahead of time.
#define RG_OBS_REDRAW_ENV() \
    lds_barrier();  /* the previous Redraw's LDS reads done */                                                                                                           \
    if (lane < rec_words) tb.w[lane] = t_rec;                                                                                                                            \
    /* the history plane is rewritten only when the visited set changed since it was last written (k_step: HIST_DIRTY), never on a stale Redraw */                       \
    const bool upd_hist = !(fle & RG_FLAG_HIST_STALE) && (fle & RG_FLAG_HIST_DIRTY);                                                                                     \
    if (lane < Q8) {                                                                                                                                                     \
        uint32_t g[2], hb[2];                                                                                                                                            \
        draw_cells8(v, lane, W, HW, g, hb);                                                                                                                              \
        reinterpret_cast<uint2 *>(scr)[lane] = make_uint2(g[0], g[1]);                                                                                                   \
        if (upd_hist) reinterpret_cast<uint2 *>(S.hist + (size_t)e * HW)[lane] = make_uint2(hb[0], hb[1]);                                                               \
    }                                                                                                                                                                    \
    lds_barrier();                                                                                                                                                       \
    /* entity overlays; draw priority monster < gold < player (core/src/lib.rs:271-283), as in k_obs */                                                                  \
    const uint32_t ppos = tb.w[nrooms];                                                                                                                                  \
    const int px = POS_X(ppos), py = POS_Y(ppos);                                                                                                                        \
    if (lane < nrooms) {                                                                                                                                                 \
        const uint32_t mw = tb.w[lane];                                                                                                                                  \
        if ((mw >> 24) & MF_ALIVE) {                                                                                                                                     \
            const int x = POS_X(mw), y = POS_Y(mw);                                                                                                                      \
            const uint32_t under = scr[y * W + x];                                                                                                                       \
            if (monster_shown(c, &tb, nrooms, px, py, x, y) && (under & 0x80u) && under != (0x80u | '*')) scr[y * W + x] = (uint8_t)(0x80u | mtile[(mw >> 16) & 0xff]);  \
        }                                                                                                                                                                \
    }                                                                                                                                                                    \
    lds_barrier();                                                                                                                                                       \
    if (lane == 0 && (scr[py * W + px] & 0x80u)) scr[py * W + px] = (uint8_t)(0x80u | '@');                                                                              \
    lds_barrier();                                                                                                                                                       \
    uint32_t *m4 = reinterpret_cast<uint32_t *>(S.screen + (size_t)e * HW);                                                                                              \
    float4 *oe = reinterpret_cast<float4 *>(out) + (size_t)e * Q4;                                                                                                       \
    for (int q = lane; q < Q4; q += WAVE) {                                                                                                                              \
        const uint32_t g = reinterpret_cast<const uint32_t *>(scr)[q] & 0x7f7f7f7fu;                                                                                     \
        m4[q] = g;                                                                                                                                                       \
        store_obs(&oe[q], gray4(g));                                                                                                                                     \
    }                                                                                                                                                                    \
    if (lane == 0)  /* (rg_obs.hip k_obs: a stale Redraw leaves the history mirror one level behind) */                                                                  \
        S.flags[e] = (fle & ~(RG_FLAG_REDRAW | RG_FLAG_HIST_STALE | RG_FLAG_HIST_LAG | ((fle & RG_FLAG_HIST_STALE) ? 0u : RG_FLAG_HIST_DIRTY))) |                        \
                     ((fle & RG_FLAG_HIST_STALE) ? RG_FLAG_HIST_LAG : 0u);
