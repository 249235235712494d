// rg_route.hip -- search-aware and map-aware routes on the device: distance, key and answering tier per env (rg_route; gfx950).
//
//   k_route<WN, GS> : one wave per 64 / GS consecutive envs; lane y of a group of GS lanes owns grid row y of the group's env as bit masks
//
// Shaped like rg_path.hip's keys-only pass, as a translation unit of its own so that nothing here touches the code generation of the kernels whose
// register counts the resource tests pin.  The rule itself is rg_route.h's, shared with the host entry point; the bit rows and the choice of instance
// are rg_rows.h's, shared with rg_path.hip.
#include "rg_device.h"
#include "rg_route.h"

#include "rg_rows.h"

// the five row masks of the rule (rg_route.h): ps = pass, ck = corner, kn = known, g0 / g1 = the goals of the two tiers that a cell word decides
// alone (the frontier joins them once every row is in)
template <int WN> struct Masks { Row<WN> ps, ck, kn, g0, g1; };
struct Bits { uint32_t ps, ck, kn, g0, g1; };
// one cell word -> its bits, as a cell that is neither the player's nor the caller's: those two are judged again, on their own, once the row is in
static __device__ __forceinline__ void cell_bits(uint32_t c, uint32_t goals, uint32_t fallback, uint32_t mode, uint32_t sh, Bits &b) {
    b.ps |= (uint32_t)rg_route_pass(c, mode, false) << sh;
    b.ck |= (uint32_t)rg_route_corner(c, mode, false) << sh;
    b.kn |= (uint32_t)rg_route_known(c, false) << sh;
    b.g0 |= (uint32_t)rg_route_goal(c, goals, mode, false, false) << sh;
    b.g1 |= (uint32_t)rg_route_goal(c, fallback, mode, false, false) << sh;
}

// The group's lanes load their rows -- the env's grid, once -- into the masks above.  The frontier, pass & (unknown to the left | right | above | below), is
// computed once, outside every divergent branch (the row shifts read neighbour lanes), from `unk` = not known, limited to the grid's own bits and rows, and
// ORed into the goal masks of the tiers that ask for it.  One level of the search is k_path's with pass and corner in place of ok and walkable; no LDS
// traffic and no barrier inside the level loop, four levels per block, a hard bound of H * W levels.  The lane that owns the player's row notes the level
// at which the player's cell is reached and that level's eight direction terms, ANDed with `legal` = rg_legal_bits on the player's cell (computed once
// per env): a direction of the search graph that rg_can_move also allows is one whose target is not secret.
// Tiers: the level loop runs from the goal masks of `goals`; when some group of the wave was not reached and there is a fallback, it runs once more from
// the fallback's masks for those groups -- the grid masks stay in registers, the groups already answered inject nothing and stay empty.
// GROUPS (ext): env e's answers go to the handle's row ext[e], and its cell of RG_GOAL_CELL is row ext[e]'s.
template <int WN, int GS>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4))) k_route(const uint16_t *__restrict__ p_pos, const uint32_t *__restrict__ flags, const uint16_t *__restrict__ cell,
                                               const int32_t *__restrict__ ext, int n, int W, int H, uint32_t goals, uint32_t fallback, uint32_t mode,
                                               const int32_t *__restrict__ gcell, int32_t *__restrict__ dist, uint8_t *__restrict__ key, uint8_t *__restrict__ tier_out) {
    constexpr int G = WAVE / GS, LB = 4;
    constexpr bool ROW16 = GS == 16;
    const int lane = threadIdx.x, grp = lane / GS, row = lane % GS;
    const int e = blockIdx.x * G + grp, HW = W * H;
    const bool active = e < n, row_ok = active && row < H;
    uint32_t pos = 0, fl = 0, xe = 0;
    int cy = -1, cx = -1;
    if (active) {
        pos = p_pos[e];
        fl = flags[e];
        xe = ext ? (uint32_t)ext[e] : (uint32_t)e;
        if ((goals | fallback) & RG_GOAL_CELL) { cy = gcell[2 * (size_t)xe]; cx = gcell[2 * (size_t)xe + 1]; }
    }
    const int py = POS_Y(pos);
    const bool mine = row_ok && row == py;           // this lane owns the player's row
    const int pxo = mine ? POS_X(pos) : -1;          // the player's column in my row, the given cell's column in my row: -1 = not in this row
    const int cxo = (row_ok && row == cy && cx >= 0 && cx < W) ? cx : -1;
    Masks<WN> m = {r_zero<WN>(), r_zero<WN>(), r_zero<WN>(), r_zero<WN>(), r_zero<WN>()};
    const uint16_t *grid = cell + (size_t)(active ? e : 0) * (size_t)HW;
    if (row_ok) {
        const uint16_t *rowp = grid + row * W;
        if ((W & 7) == 0) {  // (then every row of every env starts on a multiple of 16 bytes)
            const u4v *r4 = reinterpret_cast<const u4v *>(rowp);
#pragma unroll
            for (int k = 0; k < WN; k++) {
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    const int j = k * 4 + jj;
                    if (j * 8 < W) {
                        const u4v v = r4[j];
                        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
                        Bits b = {0, 0, 0, 0, 0};
#pragma unroll
                        for (int t = 0; t < 8; t++) {
                            const uint32_t c = (t & 1) ? q[t >> 1] >> 16 : q[t >> 1] & 0xffffu;
                            cell_bits(c, goals, fallback, mode, (uint32_t)t, b);
                        }
                        m.ps.w[k] |= b.ps << (jj * 8);
                        m.ck.w[k] |= b.ck << (jj * 8);
                        m.kn.w[k] |= b.kn << (jj * 8);
                        m.g0.w[k] |= b.g0 << (jj * 8);
                        m.g1.w[k] |= b.g1 << (jj * 8);
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < WN; k++) {  // (word by word, so that no mask is ever indexed at run time)
                Bits b = {0, 0, 0, 0, 0};
#pragma unroll 1
                for (int j = 0; j < 32 && 32 * k + j < W; j++) cell_bits(rowp[32 * k + j], goals, fallback, mode, (uint32_t)j, b);
                m.ps.w[k] = b.ps;
                m.ck.w[k] = b.ck;
                m.kn.w[k] = b.kn;
                m.g0.w[k] = b.g0;
                m.g1.w[k] = b.g1;
            }
        }
    }
    uint32_t pc = S_NONE, legal = 0;  // the cell word under the player; the directions rg_can_move allows from it
    if (pxo >= 0) {  // the player's own cell: known whatever its word, and gold under the player is no goal
        pc = grid[row * W + pxo];
        legal = rg_legal_bits(grid, H, W, pxo, row, 0) & 0xffu;
        r_put<WN>(m.ps, pxo, rg_route_pass(pc, mode, true));
        r_put<WN>(m.ck, pxo, rg_route_corner(pc, mode, true));
        r_put<WN>(m.kn, pxo, true);
        r_put<WN>(m.g0, pxo, rg_route_goal(pc, goals, mode, true, pxo == cxo));
        r_put<WN>(m.g1, pxo, rg_route_goal(pc, fallback, mode, true, pxo == cxo));
    }
    if (cxo >= 0) {  // the caller's cell
        const uint32_t cc = grid[row * W + cxo];
        r_put<WN>(m.g0, cxo, rg_route_goal(cc, goals, mode, cxo == pxo, true));
        r_put<WN>(m.g1, cxo, rg_route_goal(cc, fallback, mode, cxo == pxo, true));
    }
    const Spot P = {pxo >= 0 ? pxo >> 5 : -1, pxo >= 0 ? 1u << (pxo & 31) : 0u};
    const bool up_ok = row > 0, dn_ok = row + 1 < H;
    bool own_front = false;
    {  // the frontier (every lane takes part: the shifts read neighbour lanes)
        Row<WN> unk;
#pragma unroll
        for (int k = 0; k < WN; k++) {
            const int left = W - 32 * k;  // the grid's bits of word k
            const uint32_t in = !row_ok || left <= 0 ? 0u : left >= 32 ? ~0u : (1u << (left & 31)) - 1u;
            unk.w[k] = ~m.kn.w[k] & in;
        }
        const Row<WN> ul = r_shl1<WN>(unk), ur = r_shr1<WN>(unk), uu = r_neighbour<WN, ROW16, true>(unk, up_ok), ud = r_neighbour<WN, ROW16, false>(unk, dn_ok);
        Row<WN> fm;
#pragma unroll
        for (int k = 0; k < WN; k++) {
            fm.w[k] = m.ps.w[k] & (ul.w[k] | ur.w[k] | uu.w[k] | ud.w[k]);
            m.g0.w[k] |= (goals & RG_GOAL_FRONTIER) ? fm.w[k] : 0u;
            m.g1.w[k] |= (fallback & RG_GOAL_FRONTIER) ? fm.w[k] : 0u;
        }
        own_front = r_at<WN>(fm, P);
    }
    constexpr bool KEEP_W = WN <= 3;  // the widest rows fetch the neighbours' corner masks anew in every level
    const Row<WN> wu0 = r_neighbour<WN, ROW16, true>(m.ck, up_ok), wd0 = r_neighbour<WN, ROW16, false>(m.ck, dn_ok);  // corner masks of rows y - 1, y + 1
    const uint64_t gmask = GS == 64 ? ~0ull : ((1ull << (GS & 63)) - 1ull) << (grp * GS);  // my group's lanes
    bool found = false;
    uint32_t dpl = RG_PATH_INF, dirs = 0, tr = RG_ROUTE_NO_TIER;  // (the player's lane) D at the player's cell, the direction bits of rg_route_key, the tier
    const uint32_t max_blk = (uint32_t)(HW / LB) + 1u;  // the hard bound: levels 0 .. H * W at the least
#pragma unroll 1
    for (uint32_t tier = 0; tier < 2u; tier++) {
        const bool answered = (__ballot(found) & gmask) != 0;  // my group has its answer from the tier before
        Row<WN> vis = r_zero<WN>(), fr = r_zero<WN>(), inject;
#pragma unroll
        for (int k = 0; k < WN; k++) inject.w[k] = answered ? 0u : tier ? m.g1.w[k] : m.g0.w[k];
#pragma unroll 1
        for (uint32_t blk = 0;; blk++) {  // levels LB * blk .. LB * blk + LB - 1
#pragma unroll
            for (int j = 0; j < LB; j++) {
                const Row<WN> wu = KEEP_W ? wu0 : r_neighbour<WN, ROW16, true>(m.ck, up_ok), wd = KEEP_W ? wd0 : r_neighbour<WN, ROW16, false>(m.ck, dn_ok);
                Row<WN> E;
#pragma unroll
                for (int k = 0; k < WN; k++) E.w[k] = fr.w[k] & m.ps.w[k];
                const Row<WN> fu = r_neighbour<WN, ROW16, true>(E, up_ok), fd = r_neighbour<WN, ROW16, false>(E, dn_ok);
                Row<WN> au, ad;  // E of the neighbour rows where the cell beside it in MY row is a corner cell: (x + dx, y) of the corner rule
#pragma unroll
                for (int k = 0; k < WN; k++) { au.w[k] = fu.w[k] & m.ck.w[k]; ad.w[k] = fd.w[k] & m.ck.w[k]; }
                const Row<WN> el = r_shl1<WN>(E), er = r_shr1<WN>(E), aul = r_shl1<WN>(au), aur = r_shr1<WN>(au), adl = r_shl1<WN>(ad), adr = r_shr1<WN>(ad);
                Row<WN> nw;
#pragma unroll
                for (int k = 0; k < WN; k++) {
                    const uint32_t tgt = el.w[k] | er.w[k] | fu.w[k] | fd.w[k] | ((aul.w[k] | aur.w[k]) & wu.w[k]) | ((adl.w[k] | adr.w[k]) & wd.w[k]);
                    nw.w[k] = (tgt & m.ps.w[k] & ~vis.w[k]) | inject.w[k];
                    inject.w[k] = 0u;
                    vis.w[k] |= nw.w[k];
                    fr.w[k] = nw.w[k];
                }
                if (!found && r_at<WN>(nw, P)) {  // (only ever true in the lane of the player's row)
                    found = true;
                    dpl = blk * LB + j;
                    tr = tier;
                    Row<WN> t;
                    dirs = (uint32_t)r_at<WN>(fu, P) | (uint32_t)r_at<WN>(fd, P) << 1 | (uint32_t)r_at<WN>(el, P) << 2 | (uint32_t)r_at<WN>(er, P) << 3;
#pragma unroll
                    for (int k = 0; k < WN; k++) t.w[k] = aul.w[k] & wu.w[k];
                    dirs |= (uint32_t)r_at<WN>(t, P) << 4;
#pragma unroll
                    for (int k = 0; k < WN; k++) t.w[k] = aur.w[k] & wu.w[k];
                    dirs |= (uint32_t)r_at<WN>(t, P) << 5;
#pragma unroll
                    for (int k = 0; k < WN; k++) t.w[k] = adl.w[k] & wd.w[k];
                    dirs |= (uint32_t)r_at<WN>(t, P) << 6;
#pragma unroll
                    for (int k = 0; k < WN; k++) t.w[k] = adr.w[k] & wd.w[k];
                    dirs |= (uint32_t)r_at<WN>(t, P) << 7;
                    dirs &= legal;  // "target not secret"
                }
            }
            uint32_t any_fr = 0;
#pragma unroll
            for (int k = 0; k < WN; k++) any_fr |= fr.w[k];
            const uint64_t live = __ballot(any_fr != 0), hit = __ballot(found);
            if (__all((hit & gmask) != 0 || (live & gmask) == 0)) break;
            if (blk >= max_blk) break;
        }
        if (!fallback || !__any(mine && !found)) break;  // (wave-uniform) nobody is left for the second tier
    }
    if (mine) {
        const uint32_t gw = tr == 1u ? fallback : goals;  // the goal word of the tier that answered
        if (dist) dist[xe] = rg_path_dist(dpl);
        if (key) key[xe] = rg_route_key((int)(fl & RG_FLAG_DEAD), dpl, gw, (pc & C_SURF_MASK) == S_STAIR, own_front, dirs);
        if (tier_out) tier_out[xe] = (uint8_t)tr;
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launcher: defined here against the prototype the host units call it by
// ---------------------------------------------------------------------------------------------
template <int WN, int GS>
static void launch_route(const RgState *S, const RgConfig *c, uint32_t goals, uint32_t fallback, uint32_t mode, const int32_t *gcell, int32_t *dist, uint8_t *key, uint8_t *tier,
                         hipStream_t st) {
    const int G = WAVE / GS, blocks = (S->n + G - 1) / G;
    hipLaunchKernelGGL((k_route<WN, GS>), dim3(blocks), dim3(WAVE), 0, st, S->p_pos, S->flags, S->cell, S->ext, S->n, (int)c->width, (int)c->height, goals, fallback, mode, gcell,
                       dist, key, tier);
}
extern "C" {
// goals / fallback / mode: checked by the caller (rg_route); gcell: needed iff either goal word has RG_GOAL_CELL; dist / key / tier: any may be NULL
void rgk_route(const RgState *S, const RgConfig *c, uint32_t goals, uint32_t fallback, uint32_t mode, const int32_t *gcell, int32_t *dist, uint8_t *key, uint8_t *tier,
               hipStream_t st) {
    if (S->n <= 0) return;
    rows_dispatch((int)c->width, (int)c->height, [&](auto wn, auto gs) {
        launch_route<decltype(wn)::value, decltype(gs)::value>(S, c, goals, fallback, mode, gcell, dist, key, tier, st);
    });
}
}
