// rg_path.hip -- shortest-path fields towards goal cells, the distance at the player's cell and the teacher key, on the device (rg_path; gfx950).
//
//   k_path<WN, GS, FIELD> : one wave per 64 / GS consecutive envs; lane y of a group of GS lanes owns grid row y of the group's env as bit masks
//
// A translation unit of its own, as rg_action_mask.hip is, so that the code generation of the step and observation kernels -- their register counts are
// pinned by the resource tests -- is not touched by anything here.  The rule itself is rg_path.h's, shared with the host entry point; the bit rows
// and the choice of instance are rg_rows.h's, shared with rg_route.hip.
// The field is PRIVILEGED (rg_path.h): it sees stairs, gold and passages the player has not discovered.
#include "rg_device.h"
#include "rg_path.h"

#include "rg_rows.h"

// one cell word -> its bits of the three row masks (rg_path.h: the rule), as a cell that is neither the player's nor the caller's: those two are
// judged again, on their own, once the row is in
static __device__ __forceinline__ void cell_bits(uint32_t c, uint32_t goals, uint32_t sh, uint32_t &ok, uint32_t &wk, uint32_t &goal) {
    ok |= (uint32_t)rg_path_ok(c) << sh;
    wk |= (uint32_t)rg_walkable(c) << sh;
    goal |= (uint32_t)rg_path_goal(c, goals, false, false) << sh;
}

// The group's lanes load their rows -- the env's grid, once -- into three masks each: ok (a move may end there), wk (walkable by surface: the corner rule)
// and the goal set.  One level of the search is then, per row: the expandable frontier E = frontier & ok shifted left / right, E of rows y -+ 1 by a
// one-lane DPP shift, for a diagonal ANDed with the two walkable masks the corner rule names -- (x + dx, y) in my row, (x, y + dy) in the neighbour's -- and
// the whole ANDed with ok & ~visited.  (The corner rule names the same two cells from either end of a move, so searching from the goals outwards gives the
// least number of moves TOWARDS them.)  No LDS traffic and no barrier inside the level loop; level 0 injects the goal cells, whatever their own words.
// The lane that owns the player's row notes the level at which the player's cell is reached: the frontier of the level before is exactly the set of cells
// at D - 1, so the eight direction tests of the teacher key are the eight terms of that level's step, ANDed with the player's bit.
// !FIELD: levels go four at a time, and the wave ends when every group has reached its player or emptied its frontier.  Per env: the grid, p_pos and the
//   flag word read, 5 bytes written.
// FIELD: every level runs, eight at a time; distances are kept as bit planes per row (three low planes by the level's position in its block, ten high ones
//   once per block: distances < H * W <= 7680 < 8192), expanded at the end into the group's image in LDS and copied out as 16-byte pieces.  The image
//   sits in LDS at the env's own misalignment, so aligned pieces of the output are aligned pieces of LDS; the ragged ends go out as u16.
// Both loops carry the hard bound of H * W levels beside their exits.
// GROUPS (ext): env e's distance and key go to the handle's row ext[e], and its cell of RG_GOAL_CELL is row ext[e]'s.
// (amdgpu_waves_per_eu(4): the 128-register budget as a bound the compiler keeps; no instance needs scratch to meet it)
template <int WN, int GS, bool FIELD>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4))) k_path(const uint16_t *__restrict__ p_pos, const uint32_t *__restrict__ flags, const uint16_t *__restrict__ cell,
                                              const int32_t *__restrict__ ext, int n, int W, int H, uint32_t goals, const int32_t *__restrict__ gcell,
                                              uint16_t *__restrict__ field, int32_t *__restrict__ dist, uint8_t *__restrict__ key) {
    extern __shared__ __align__(16) uint16_t image[];  // FIELD: [G][pitch16]
    constexpr int G = WAVE / GS, LB = FIELD ? 8 : 4, NHI = 10;
    constexpr bool ROW16 = GS == 16, HI_LDS = FIELD && WN > 3;  // the widest rows keep their ten high planes in LDS (50 registers otherwise), touched once per block
    const int lane = threadIdx.x, grp = lane / GS, row = lane % GS;
    const int e = blockIdx.x * G + grp, HW = W * H;
    const bool active = e < n, row_ok = active && row < H;
    uint32_t pos = 0, fl = 0, xe = 0;
    int cy = -1, cx = -1;
    if (active) {
        pos = p_pos[e];
        fl = flags[e];
        xe = ext ? (uint32_t)ext[e] : (uint32_t)e;
        if (goals & RG_GOAL_CELL) { cy = gcell[2 * (size_t)xe]; cx = gcell[2 * (size_t)xe + 1]; }
    }
    const int py = POS_Y(pos);
    const bool mine = row_ok && row == py;           // this lane owns the player's row
    const int pxo = mine ? POS_X(pos) : -1;          // the player's column in my row, the given cell's column in my row: -1 = not in this row
    const int cxo = (row_ok && row == cy && cx >= 0 && cx < W) ? cx : -1;
    Row<WN> ok = r_zero<WN>(), wk = r_zero<WN>(), goal = r_zero<WN>();
    uint32_t pc = S_NONE;  // the cell word under the player
    if (row_ok) {
        const uint16_t *rowp = cell + (size_t)e * (size_t)HW + row * W;
        if ((W & 7) == 0) {  // (then every row of every env starts on a multiple of 16 bytes)
            const u4v *r4 = reinterpret_cast<const u4v *>(rowp);
#pragma unroll
            for (int k = 0; k < WN; k++) {  // (fully unrolled: compile-time word indices; the guard is the only run-time part)
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    const int j = k * 4 + jj;
                    if (j * 8 < W) {
                        const u4v v = r4[j];
                        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
                        uint32_t o = 0, w = 0, g = 0;
#pragma unroll
                        for (int t = 0; t < 8; t++) {
                            const uint32_t c = (t & 1) ? q[t >> 1] >> 16 : q[t >> 1] & 0xffffu;
                            cell_bits(c, goals, (uint32_t)t, o, w, g);
                        }
                        ok.w[k] |= o << (jj * 8);
                        wk.w[k] |= w << (jj * 8);
                        goal.w[k] |= g << (jj * 8);
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < WN; k++) {  // (word by word, so that no mask is ever indexed at run time)
                uint32_t o = 0, w = 0, g = 0;
#pragma unroll 1
                for (int j = 0; j < 32 && 32 * k + j < W; j++) {
                    const uint32_t c = rowp[32 * k + j];
                    cell_bits(c, goals, (uint32_t)j, o, w, g);
                }
                ok.w[k] = o;
                wk.w[k] = w;
                goal.w[k] = g;
            }
        }
    }
    if (pxo >= 0) {  // the player's own cell: gold under the player is no goal
        pc = cell[(size_t)e * (size_t)HW + row * W + pxo];
        r_put<WN>(goal, pxo, rg_path_goal(pc, goals, true, pxo == cxo));
    }
    if (cxo >= 0) r_put<WN>(goal, cxo, rg_path_goal(cell[(size_t)e * (size_t)HW + row * W + cxo], goals, cxo == pxo, true));  // the caller's cell
    const Spot P = {pxo >= 0 ? pxo >> 5 : -1, pxo >= 0 ? 1u << (pxo & 31) : 0u};
    const bool up_ok = row > 0, dn_ok = row + 1 < H;
    constexpr bool KEEP_W = WN <= 3;  // the widest rows fetch the neighbours' walkable masks anew in every level: ten registers against ten DPP moves
    const Row<WN> wu0 = r_neighbour<WN, ROW16, true>(wk, up_ok), wd0 = r_neighbour<WN, ROW16, false>(wk, dn_ok);  // walkable masks of rows y - 1, y + 1
    Row<WN> vis = r_zero<WN>(), fr = r_zero<WN>(), inject = goal;
    Row<WN> p0 = r_zero<WN>(), p1 = r_zero<WN>(), p2 = r_zero<WN>(), ph[FIELD && !HI_LDS ? NHI : 1];
#pragma unroll
    for (int b = 0; b < (FIELD && !HI_LDS ? NHI : 1); b++) ph[b] = r_zero<WN>();
    const int pitch16 = (HW + 8 + 7) & ~7;  // FIELD: u16 per group of the image: the grid and its shift, a multiple of 16 bytes
    uint32_t *hil = reinterpret_cast<uint32_t *>(image + G * pitch16) + lane;  // HI_LDS: plane b, word k of my row at hil[(b * WN + k) * WAVE]
    if (HI_LDS) {
#pragma unroll
        for (int i = 0; i < NHI * WN; i++) hil[i * WAVE] = 0u;
    }
    const uint64_t gmask = GS == 64 ? ~0ull : ((1ull << (GS & 63)) - 1ull) << (grp * GS);  // my group's lanes
    bool found = false;
    uint32_t dpl = RG_PATH_INF, dirs = 0;  // (the player's lane) D at the player's cell and the direction bits of rg_path_key
    const uint32_t max_blk = (uint32_t)(HW / LB) + 1u;  // the hard bound: levels 0 .. H * W at the least
    uint32_t blk = 0;
    for (;; blk++) {  // levels LB * blk .. LB * blk + LB - 1
        Row<WN> acc = r_zero<WN>();
#pragma unroll
        for (int j = 0; j < LB; j++) {
            const Row<WN> wu = KEEP_W ? wu0 : r_neighbour<WN, ROW16, true>(wk, up_ok), wd = KEEP_W ? wd0 : r_neighbour<WN, ROW16, false>(wk, dn_ok);
            Row<WN> E;
#pragma unroll
            for (int k = 0; k < WN; k++) E.w[k] = fr.w[k] & ok.w[k];
            const Row<WN> fu = r_neighbour<WN, ROW16, true>(E, up_ok), fd = r_neighbour<WN, ROW16, false>(E, dn_ok);
            Row<WN> au, ad;  // E of the neighbour rows where the cell beside it in MY row is walkable: (x + dx, y) of the corner rule
#pragma unroll
            for (int k = 0; k < WN; k++) { au.w[k] = fu.w[k] & wk.w[k]; ad.w[k] = fd.w[k] & wk.w[k]; }
            const Row<WN> el = r_shl1<WN>(E), er = r_shr1<WN>(E), aul = r_shl1<WN>(au), aur = r_shr1<WN>(au), adl = r_shl1<WN>(ad), adr = r_shr1<WN>(ad);
            Row<WN> nw;
#pragma unroll
            for (int k = 0; k < WN; k++) {
                const uint32_t tgt = el.w[k] | er.w[k] | fu.w[k] | fd.w[k] | ((aul.w[k] | aur.w[k]) & wu.w[k]) | ((adl.w[k] | adr.w[k]) & wd.w[k]);
                nw.w[k] = (tgt & ok.w[k] & ~vis.w[k]) | inject.w[k];
                inject.w[k] = 0u;
                vis.w[k] |= nw.w[k];
                fr.w[k] = nw.w[k];
                if (FIELD) {
                    if (j & 1) p0.w[k] |= nw.w[k];
                    if (j & 2) p1.w[k] |= nw.w[k];
                    if (j & 4) p2.w[k] |= nw.w[k];
                    acc.w[k] |= nw.w[k];
                }
            }
            if (!FIELD && !found && r_at<WN>(nw, P)) {  // (only ever true in the lane of the player's row; FIELD reads its answers from the image)
                found = true;
                dpl = blk * LB + j;
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
            }
        }
        uint32_t any_fr = 0;
#pragma unroll
        for (int k = 0; k < WN; k++) any_fr |= fr.w[k];
        if (FIELD) {
#pragma unroll
            for (int b = 0; b < NHI; b++)
                if ((blk >> b) & 1u) {  // (wave-uniform)
#pragma unroll
                    for (int k = 0; k < WN; k++) {
                        if (HI_LDS) hil[(b * WN + k) * WAVE] |= acc.w[k];
                        else ph[HI_LDS ? 0 : b].w[k] |= acc.w[k];
                    }
                }
            if (!__any(any_fr != 0)) break;
        } else {
            const uint64_t live = __ballot(any_fr != 0), hit = __ballot(found);
            if (__all((hit & gmask) != 0 || (live & gmask) == 0)) break;
        }
        if (blk >= max_blk) break;
    }
    if (!FIELD && mine) {
        if (dist) dist[xe] = rg_path_dist(dpl);
        if (key) key[xe] = rg_path_key((int)(fl & RG_FLAG_DEAD), dpl, (goals & RG_GOAL_STAIRS) && (pc & C_SURF_MASK) == S_STAIR, dirs);
    }
    if (FIELD) {
        const size_t a16 = (size_t)e * (size_t)HW;       // the env's first u16 of the output
        const int m16 = (int)(a16 & 7);                  // ... and how far that is past a multiple of 16 bytes
        uint16_t *img = image + grp * pitch16;
        if (row_ok) {  // expand my row: cell x -> u16 distance, 0xFFFF where the cell was never reached
            const int nhi = 32 - __clz((int)blk);        // high planes in use (wave-uniform)
            const int li0 = m16 + row * W;
#pragma unroll
            for (int k = 0; k < WN; k++) {
                uint32_t hk[NHI];
#pragma unroll
                for (int b = 0; b < NHI; b++) hk[b] = HI_LDS ? (b < nhi ? hil[(b * WN + k) * WAVE] : 0u) : ph[HI_LDS ? 0 : b].w[k];
#pragma unroll 1
                for (int j = 0; j < 32; j += 2) {
                    const int x = 32 * k + j;
                    if (x >= W) break;
                    uint32_t lo = ((p0.w[k] >> j) & 1u) | (((p1.w[k] >> j) & 1u) << 1) | (((p2.w[k] >> j) & 1u) << 2);
                    uint32_t hi = ((p0.w[k] >> (j + 1)) & 1u) | (((p1.w[k] >> (j + 1)) & 1u) << 1) | (((p2.w[k] >> (j + 1)) & 1u) << 2);
#pragma unroll
                    for (int b = 0; b < NHI; b++)
                        if (b < nhi) {
                            lo |= ((hk[b] >> j) & 1u) << (3 + b);
                            hi |= ((hk[b] >> (j + 1)) & 1u) << (3 + b);
                        }
                    if (!((vis.w[k] >> j) & 1u)) lo = RG_PATH_INF;
                    if (!((vis.w[k] >> (j + 1)) & 1u)) hi = RG_PATH_INF;
                    const int li = li0 + x;
                    if (!(li & 1) && x + 1 < W) {
                        *reinterpret_cast<uint32_t *>(img + li) = lo | (hi << 16);
                    } else {
                        img[li] = (uint16_t)lo;
                        if (x + 1 < W) img[li + 1] = (uint16_t)hi;
                    }
                }
            }
        }
        __syncthreads();  // (the block is one wave)
        if (mine) {  // the distance and the key from the finished field, by the rule's own words
            const uint16_t *g = cell + (size_t)e * (size_t)HW, *D = img + m16;
            const int px = pxo;
            dpl = D[py * W + px];
            if (dpl != 0 && dpl != RG_PATH_INF) {
#pragma unroll 1
                for (int d = 0; d < 8; d++) {
                    const int dx = rg_path_dx(d), dy = rg_path_dy(d);
                    if (rg_can_move(g, H, W, px, py, dx, dy) && D[(py + dy) * W + px + dx] == dpl - 1u) dirs |= 1u << d;
                }
            }
            if (dist) dist[xe] = rg_path_dist(dpl);
            if (key) key[xe] = rg_path_key((int)(fl & RG_FLAG_DEAD), dpl, (goals & RG_GOAL_STAIRS) && (pc & C_SURF_MASK) == S_STAIR, dirs);
        }
        if (active) {
            uint16_t *o = field + (a16 - (size_t)m16);   // 16-byte aligned (rg_path checks field_dev); nothing before field + a16 is written
            const int end16 = m16 + HW;
            for (int p = row * 8; p < end16; p += GS * 8) {
                if (p >= m16 && p + 8 <= end16) {
                    *reinterpret_cast<u4v *>(o + p) = *reinterpret_cast<const u4v *>(img + p);
                } else {
                    const int q1 = p + 8 < end16 ? p + 8 : end16;
#pragma unroll 1
                    for (int q = p > m16 ? p : m16; q < q1; q++) o[q] = img[q];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launcher: defined here against the prototype the host units call it by
// ---------------------------------------------------------------------------------------------
template <int WN, int GS>
static void launch_path(const RgState *S, const RgConfig *c, uint32_t goals, const int32_t *gcell, uint16_t *field, int32_t *dist, uint8_t *key, hipStream_t st) {
    const int G = WAVE / GS, blocks = (S->n + G - 1) / G, W = (int)c->width, H = (int)c->height;
    if (field) {
        const size_t lds = (size_t)G * (size_t)((W * H + 8 + 7) & ~7) * sizeof(uint16_t) + (WN > 3 ? (size_t)10 * WN * WAVE * sizeof(uint32_t) : 0);  // image (+ high planes)
        hipLaunchKernelGGL((k_path<WN, GS, true>), dim3(blocks), dim3(WAVE), lds, st, S->p_pos, S->flags, S->cell, S->ext, S->n, W, H, goals, gcell, field, dist, key);
    } else {
        hipLaunchKernelGGL((k_path<WN, GS, false>), dim3(blocks), dim3(WAVE), 0, st, S->p_pos, S->flags, S->cell, S->ext, S->n, W, H, goals, gcell, field, dist, key);
    }
}
extern "C" {
// goals: a non-empty subset of RG_GOAL_*; gcell: needed iff RG_GOAL_CELL; field / dist / key: any may be NULL (checked by the caller)
void rgk_path(const RgState *S, const RgConfig *c, uint32_t goals, const int32_t *gcell, uint16_t *field, int32_t *dist, uint8_t *key, hipStream_t st) {
    if (S->n <= 0) return;
    rows_dispatch((int)c->width, (int)c->height, [&](auto wn, auto gs) { launch_path<decltype(wn)::value, decltype(gs)::value>(S, c, goals, gcell, field, dist, key, st); });
}
}
