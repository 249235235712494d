// rg_objects.hip -- the stairs, gold, doors and frontier cells of every env as a table ordered by walking distance, on the device (rg_objects; gfx950).
//
//   k_objects<WN, GS> : one wave per 64 / GS consecutive envs; lane y of a group of GS lanes owns grid row y of the group's env as bit masks
//
// The third user of rg_rows.h, shaped like rg_route.hip and a translation unit of its own, so that nothing here touches the code generation of the kernels
// whose register counts the resource tests pin.  The rule itself is rg_objects.h's, shared with the host entry point.
// Without RG_ROUTE_KNOWN the table is PRIVILEGED (rg_objects.h): it lists what the player has not discovered.
#include "rg_device.h"
#include "rg_objects.h"

#include "rg_rows.h"

// the row masks of the rule: ps = pass, ck = corner, kn = known (rg_route.h); st / gd / dr = the asked kinds a cell word decides alone (rg_objects.h)
struct OBits { uint32_t ps, ck, kn, st, gd, dr; };
// one cell word -> its bits, as a cell that is not the player's: that one is judged again, on its own, once the row is in
static __device__ __forceinline__ void obj_bits(uint32_t c, uint32_t kinds, uint32_t mode, uint32_t sh, OBits &b) {
    const uint32_t kw = rg_obj_kind_word(c, kinds, mode, false);
    b.ps |= (uint32_t)rg_route_pass(c, mode, false) << sh;
    b.ck |= (uint32_t)rg_route_corner(c, mode, false) << sh;
    b.kn |= (uint32_t)rg_route_known(c, false) << sh;
    b.st |= (kw & RG_OBJ_STAIRS ? 1u : 0u) << sh;
    b.gd |= (kw & RG_OBJ_GOLD ? 1u : 0u) << sh;
    b.dr |= (kw & RG_OBJ_DOOR ? 1u : 0u) << sh;
}
template <int WN> static __device__ __forceinline__ uint32_t r_pop(const Row<WN> &a) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < WN; k++) c += (uint32_t)__popc(a.w[k]);
    return c;
}
// the sum of v over the lanes of my group, in every lane of it (a butterfly of log2(GS) exchanges)
template <int GS> static __device__ __forceinline__ uint32_t group_sum(uint32_t v) {
#pragma unroll
    for (int d = 1; d < GS; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d, GS);
    return v;
}

// The cells of one level that are objects become rows.  `hit` = the level's newly reached cells & the object mask, almost always zero in every lane: one
// ballot skips the level.  Otherwise the lanes' row counts are prefix-summed over the group in lane (= grid row) order, which is the (y, x) order inside one
// walk, and each lane stores its rows at listed + prefix, bits in ascending x, one 16-byte store a row.  The kind word of a hit is judged again from its
// cell word (one cached load per listed object) and the frontier mask, so no per-kind mask stays in registers through the level loop.
// `listed` (the same in every lane of a group) grows by the group's total; a row at or past cap is not stored.
template <int WN, int GS>
static __device__ __forceinline__ void obj_extract(const Row<WN> &nw, const Row<WN> &obj, const Row<WN> &fm, uint32_t level, const uint16_t *__restrict__ rowp, int row, int pxo, int px,
                                                   int py, uint32_t kinds, uint32_t mode, int cap, u4v *__restrict__ rows, uint32_t &listed) {
    Row<WN> hit;
    uint32_t any_hit = 0;
#pragma unroll
    for (int k = 0; k < WN; k++) { hit.w[k] = nw.w[k] & obj.w[k]; any_hit |= hit.w[k]; }
    if (__ballot(any_hit != 0) == 0) return;  // (wave-uniform)
    const uint32_t cnt = r_pop<WN>(hit);
    uint32_t inc = cnt;
#pragma unroll
    for (int d = 1; d < GS; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, d, GS);
        if (row >= d) inc += v;
    }
    const uint32_t total = (uint32_t)__shfl((int)inc, GS - 1, GS);
    uint32_t slot = listed + inc - cnt;
    if (cnt != 0 && slot < (uint32_t)cap) {
#pragma unroll
        for (int k = 0; k < WN; k++) {
            uint32_t m = hit.w[k];
            while (m != 0 && slot < (uint32_t)cap) {
                const int b = __builtin_ctz(m), x = 32 * k + b;
                m &= m - 1u;
                const uint32_t kind = rg_obj_kind_word(rowp[x], kinds, mode, x == pxo) | ((fm.w[k] >> b) & 1u ? RG_OBJ_FRONTIER : 0u);
                uint32_t r[4];
                rg_obj_row(kind, px, py, x, row, level, r);
                rows[slot++] = u4v{r[0], r[1], r[2], r[3]};
            }
        }
    }
    listed += total;
}

// The group's lanes load their rows -- the env's grid, once -- into the masks above, by k_route's two loaders.  The frontier, pass & (unknown to the left |
// right | above | below), is computed once, outside every divergent branch (the row shifts read neighbour lanes).  The counts are pop-counts of the kind
// masks summed over the group; after them only pass, corner, the object mask (the OR of the asked kinds) and the frontier mask stay live.
// The search is k_route's level loop seeded with the player's bit: level 0 is the player's own cell, whatever its word; no LDS traffic and no barrier
// inside the loop, four levels per block, a hard bound of H * W levels.  A group is finished when cap rows are listed, when every object is listed or when
// a level reached nothing new; the wave ends when every group is.  The rows past the last listed one are zero-filled at the end, GS rows at a time.
// An env in the Grave modal loads nothing: empty masks, a zero table, zero counts.
// GROUPS (ext): env e's rows go to the handle's env index ext[e].
template <int WN, int GS>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4))) k_objects(const uint16_t *__restrict__ p_pos, const uint32_t *__restrict__ flags, const uint16_t *__restrict__ cell,
                                                 const int32_t *__restrict__ ext, int n, int W, int H, uint32_t kinds, uint32_t mode, int cap,
                                                 u4v *__restrict__ table, u4v *__restrict__ count) {
    constexpr int G = WAVE / GS, LB = 4;
    constexpr bool ROW16 = GS == 16;
    const int lane = threadIdx.x, grp = lane / GS, row = lane % GS;
    const int e = blockIdx.x * G + grp, HW = W * H;
    const bool active = e < n;
    uint32_t pos = 0, fl = RG_FLAG_DEAD, xe = 0;
    if (active) {
        pos = p_pos[e];
        fl = flags[e];
        xe = ext ? (uint32_t)ext[e] : (uint32_t)e;
    }
    const bool row_ok = active && !(fl & RG_FLAG_DEAD) && row < H;
    const int px = POS_X(pos), py = POS_Y(pos);
    const int pxo = (row_ok && row == py) ? px : -1;  // the player's column in my row: -1 = not in this row
    Row<WN> ps = r_zero<WN>(), ck = r_zero<WN>(), kn = r_zero<WN>(), st = r_zero<WN>(), gd = r_zero<WN>(), dr = r_zero<WN>();
    const uint16_t *rowp = cell + (size_t)(active ? e : 0) * (size_t)HW + (row_ok ? row * W : 0);
    if (row_ok) {
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
                        OBits b = {0, 0, 0, 0, 0, 0};
#pragma unroll
                        for (int t = 0; t < 8; t++) {
                            const uint32_t c = (t & 1) ? q[t >> 1] >> 16 : q[t >> 1] & 0xffffu;
                            obj_bits(c, kinds, mode, (uint32_t)t, b);
                        }
                        ps.w[k] |= b.ps << (jj * 8);
                        ck.w[k] |= b.ck << (jj * 8);
                        kn.w[k] |= b.kn << (jj * 8);
                        st.w[k] |= b.st << (jj * 8);
                        gd.w[k] |= b.gd << (jj * 8);
                        dr.w[k] |= b.dr << (jj * 8);
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < WN; k++) {  // (word by word, so that no mask is ever indexed at run time)
                OBits b = {0, 0, 0, 0, 0, 0};
#pragma unroll 1
                for (int j = 0; j < 32 && 32 * k + j < W; j++) obj_bits(rowp[32 * k + j], kinds, mode, (uint32_t)j, b);
                ps.w[k] = b.ps;
                ck.w[k] = b.ck;
                kn.w[k] = b.kn;
                st.w[k] = b.st;
                gd.w[k] = b.gd;
                dr.w[k] = b.dr;
            }
        }
    }
    if (pxo >= 0) {  // the player's own cell: known whatever its word, and gold under the player is no object
        const uint32_t pc = rowp[pxo], kw = rg_obj_kind_word(pc, kinds, mode, true);
        r_put<WN>(ps, pxo, rg_route_pass(pc, mode, true));
        r_put<WN>(ck, pxo, rg_route_corner(pc, mode, true));
        r_put<WN>(kn, pxo, true);
        r_put<WN>(st, pxo, (kw & RG_OBJ_STAIRS) != 0);
        r_put<WN>(gd, pxo, (kw & RG_OBJ_GOLD) != 0);
        r_put<WN>(dr, pxo, (kw & RG_OBJ_DOOR) != 0);
    }
    const Spot P = {pxo >= 0 ? pxo >> 5 : -1, pxo >= 0 ? 1u << (pxo & 31) : 0u};
    const bool up_ok = row > 0, dn_ok = row + 1 < H;
    Row<WN> fm, obj;
    {  // the frontier (every lane takes part: the shifts read neighbour lanes)
        Row<WN> unk;
#pragma unroll
        for (int k = 0; k < WN; k++) {
            const int left = W - 32 * k;  // the grid's bits of word k
            const uint32_t in = !row_ok || left <= 0 ? 0u : left >= 32 ? ~0u : (1u << (left & 31)) - 1u;
            unk.w[k] = ~kn.w[k] & in;
        }
        const Row<WN> ul = r_shl1<WN>(unk), ur = r_shr1<WN>(unk), uu = r_neighbour<WN, ROW16, true>(unk, up_ok), ud = r_neighbour<WN, ROW16, false>(unk, dn_ok);
#pragma unroll
        for (int k = 0; k < WN; k++) {
            fm.w[k] = (kinds & RG_OBJ_FRONTIER) ? ps.w[k] & (ul.w[k] | ur.w[k] | uu.w[k] | ud.w[k]) : 0u;
            obj.w[k] = st.w[k] | gd.w[k] | dr.w[k] | fm.w[k];
        }
    }
    // the counts, and the number of objects: two kinds to a word (a kind has at most H * W <= 7 680 cells)
    const uint32_t c01 = group_sum<GS>(r_pop<WN>(st) | r_pop<WN>(gd) << 16), c23 = group_sum<GS>(r_pop<WN>(dr) | r_pop<WN>(fm) << 16);
    const uint32_t n_obj = group_sum<GS>(r_pop<WN>(obj));
    if (count && active && row == 0) count[xe] = u4v{c01 & 0xffffu, c01 >> 16, c23 & 0xffffu, c23 >> 16};
    if (!table) return;  // (wave-uniform)
    u4v *rows = table + (size_t)xe * (size_t)cap;
    uint32_t listed = 0;
    if (pxo >= 0) r_put<WN>(ps, pxo, true);  // the own cell starts the search whatever its word (it is never a move's target: level 0 has visited it)
    Row<WN> vis, fr;
#pragma unroll
    for (int k = 0; k < WN; k++) vis.w[k] = fr.w[k] = P.pw == k ? P.pb : 0u;
    obj_extract<WN, GS>(fr, obj, fm, 0u, rowp, row, pxo, px, py, kinds, mode, cap, rows, listed);
    constexpr bool KEEP_W = WN <= 3;  // the widest rows fetch the neighbours' corner masks anew in every level
    const Row<WN> wu0 = r_neighbour<WN, ROW16, true>(ck, up_ok), wd0 = r_neighbour<WN, ROW16, false>(ck, dn_ok);  // corner masks of rows y - 1, y + 1
    const uint64_t gmask = GS == 64 ? ~0ull : ((1ull << (GS & 63)) - 1ull) << (grp * GS);  // my group's lanes
    const uint32_t max_blk = (uint32_t)(HW / LB) + 1u;  // the hard bound: levels 0 .. H * W at the least
#pragma unroll 1
    for (uint32_t blk = 0;; blk++) {  // levels 1 + LB * blk .. LB * blk + LB
        {  // (before the block: a group with nothing left to list, or nothing to expand, is finished)
            uint32_t any_fr = 0;
#pragma unroll
            for (int k = 0; k < WN; k++) any_fr |= fr.w[k];
            const uint64_t live = __ballot(any_fr != 0);
            if (__all(listed >= (uint32_t)cap || listed >= n_obj || (live & gmask) == 0)) break;
            if (blk >= max_blk) break;
        }
#pragma unroll
        for (int j = 0; j < LB; j++) {
            const Row<WN> wu = KEEP_W ? wu0 : r_neighbour<WN, ROW16, true>(ck, up_ok), wd = KEEP_W ? wd0 : r_neighbour<WN, ROW16, false>(ck, dn_ok);
            Row<WN> E;
#pragma unroll
            for (int k = 0; k < WN; k++) E.w[k] = fr.w[k] & ps.w[k];
            const Row<WN> fu = r_neighbour<WN, ROW16, true>(E, up_ok), fd = r_neighbour<WN, ROW16, false>(E, dn_ok);
            Row<WN> au, ad;  // E of the neighbour rows where the cell beside it in MY row is a corner cell: (x + dx, y) of the corner rule
#pragma unroll
            for (int k = 0; k < WN; k++) { au.w[k] = fu.w[k] & ck.w[k]; ad.w[k] = fd.w[k] & ck.w[k]; }
            const Row<WN> el = r_shl1<WN>(E), er = r_shr1<WN>(E), aul = r_shl1<WN>(au), aur = r_shr1<WN>(au), adl = r_shl1<WN>(ad), adr = r_shr1<WN>(ad);
#pragma unroll
            for (int k = 0; k < WN; k++) {
                const uint32_t tgt = el.w[k] | er.w[k] | fu.w[k] | fd.w[k] | ((aul.w[k] | aur.w[k]) & wu.w[k]) | ((adl.w[k] | adr.w[k]) & wd.w[k]);
                fr.w[k] = tgt & ps.w[k] & ~vis.w[k];
                vis.w[k] |= fr.w[k];
            }
            obj_extract<WN, GS>(fr, obj, fm, blk * LB + (uint32_t)j + 1u, rowp, row, pxo, px, py, kinds, mode, cap, rows, listed);
        }
    }
    if (active)
        for (uint32_t s = (uint32_t)row; s < (uint32_t)cap; s += GS)
            if (s >= listed) rows[s] = u4v{0u, 0u, 0u, 0u};
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launcher: defined here against the prototype the host units call it by
// ---------------------------------------------------------------------------------------------
template <int WN, int GS>
static void launch_objects(const RgState *S, const RgConfig *c, uint32_t kinds, uint32_t mode, int cap, int16_t *table, int32_t *count, hipStream_t st) {
    const int G = WAVE / GS, blocks = (S->n + G - 1) / G;
    hipLaunchKernelGGL((k_objects<WN, GS>), dim3(blocks), dim3(WAVE), 0, st, S->p_pos, S->flags, S->cell, S->ext, S->n, (int)c->width, (int)c->height, kinds, mode, table ? cap : 0,
                       reinterpret_cast<u4v *>(table), reinterpret_cast<u4v *>(count));
}
extern "C" {
// kinds / mode / cap: checked by the caller (rg_objects); table / count: 16-byte aligned, either may be NULL
void rgk_objects(const RgState *S, const RgConfig *c, uint32_t kinds, uint32_t mode, int cap, int16_t *table, int32_t *count, hipStream_t st) {
    if (S->n <= 0) return;
    rows_dispatch((int)c->width, (int)c->height, [&](auto wn, auto gs) {
        launch_objects<decltype(wn)::value, decltype(gs)::value>(S, c, kinds, mode, cap, table, count, st);
    });
}
}
