// rg_obs_fix.hip -- k_obs_fix: the fix-up pass behind a step launch that pre-streamed the gray images (rg_kernels.hip enc_helper; RgState::enc_rows), group-wise
// (gfx950).  Same bits and side effects as rg_obs.hip's k_obs_resid -- the image lines of every env's mask re-encoded from the final mirror, every env with a
// pending Redraw drawn from its tiles (mirror write-back, history plane, flag word) -- in another order of work.  A library of its own
// (librogue_gym_obsfix.so, which librogue_gym_hip.so links: units.sh), as the novelty pass and the cell archive are: the kernel set and register counts the
// resource tests pin in the other code objects stay what they are.
//
// One wave owns a GROUP of OBS_FIX_GROUP consecutive envs and is done after it: 8 192 one-wave blocks at 65 536 envs, no loop over groups and so no chain
// of groups.  k_obs_resid walks runs of 4 envs, 1.6 of them per wave, each a chain flags -> mirror words -> stores (-> tiles -> draw), of
// which its one-run-ahead prefetch hides the first link only (profiles/r11_experiments.txt).  Here a wave
//   1. loads the group's flag words and line masks with one coalesced load each (lane i: env i), the gray table and the glyph table beside them -- one round
//      trip for the five loads -- and fills the LDS tables;
//   2. ballots on RG_FLAG_REDRAW (such an env is drawn in full: its mask is ignored) and leaves if the group has neither a Redraw nor a masked line;
//   3. requests the first Redraw env's tiles and observation record, which nothing waits for before the draw;
//   4. packs the group's masked lines densely: a prefix sum of popc(mask) over the group's lanes, each lane writes its env's (env in group << 4 | line)
//      entries into an LDS list of at most 16 per env (128 for the group);
//   5. serves the list eight lines per wave instruction -- eight lanes per 128-byte image line, lane >> 3 the list entry, lane & 7 the float4 -- the mirror
//      words of OBS_FIX_AHEAD such passes requested before the first of their stores; a longer list loops (all 128 entries: four trips);
//   6. draws the group's Redraw envs one at a time (RG_OBS_REDRAW_ENV, rg_obs_dev.h: k_obs_resid's loop), the next one's tiles requested before each draw.
// So a wave holds one chain, flags -> {tiles, mirror words} -> stores -> draw.  One-wave blocks, because the barriers of the Redraw service are the wave's
// own (lds_barrier).  No flag, fence or spin between waves.  The comments at the loads below say what the built code looked like without each of them:
// profiles/r12_experiments.txt.
#include "rg_device.h"
#include "rg_obs_dev.h"

// Group and depth from the sweep of profiles/r12_experiments.txt, 65 536 mini envs on one MI355X: groups of 8 and 16 envs both beat k_obs_resid (pass 8.6 - 8.7
// and 8.9 - 9.0 us against 10.9), groups of 32 do not (10.1 - 10.4 us); 2 or 4 passes ahead give the same pass within 0.1 us.  Groups of 8 gave the best
// `value` (+2.0 to 2.6 % against +1.6 to 2.0 %) and are the only ones that are also faster than k_obs_resid on every smaller batch measured (4 096 to 49 152
// envs: n / 8 waves, where groups of 16 leave too few waves in flight and lose 0.6 to 0.9 us), so no batch size takes another path.
#ifndef OBS_FIX_GROUP
#define OBS_FIX_GROUP 8
#endif
#ifndef OBS_FIX_AHEAD
#define OBS_FIX_AHEAD 4
#endif
static_assert(OBS_FIX_GROUP >= 8 && OBS_FIX_GROUP <= WAVE && (OBS_FIX_GROUP & (OBS_FIX_GROUP - 1)) == 0, "a group is 8, 16, 32 or 64 envs: one lane per env");
static_assert(OBS_FIX_AHEAD >= 1 && OBS_FIX_AHEAD <= 8, "passes whose mirror words are in flight together");
#if OBS_FIX_GROUP <= 16
typedef uint8_t fix_entry_t;   // env in group << 4 | line
#else
typedef uint16_t fix_entry_t;
#endif

__global__ void __launch_bounds__(WAVE) k_obs_fix(RgState S, RgConfig c, float *__restrict__ out) {
    __shared__ float lutf[128];                              // glyph -> gray value
    __shared__ uint8_t mtile[RG_MAX_ENEMY_KINDS + 6];        // monster type -> glyph
    __shared__ __align__(16) uint8_t scr[512];               // the staged screen of a Redraw env (HW = 512: rgk_obs_tail_capable)
    __shared__ ObsTabs tb;                                   // its observation record
    __shared__ fix_entry_t list[OBS_FIX_GROUP * 16];         // the group's masked lines, packed
    // (a grid of exactly 512 cells, rgk_obs_tail_capable: the tile words of an env are one uint4 per lane, its image two float4 per lane, and a line mask
    // has 16 bits.  Compile-time here, so that no load of a Redraw's inputs sits under a lane mask with a select behind it.)
    constexpr int HW = 512, Q4 = HW >> 2, Q8 = HW >> 3;
    static_assert(Q8 == WAVE, "one uint4 of tile words per lane");
    const int lane = threadIdx.x, W = c.width, n = S.n;
    const int nrooms = c.room_num_x * c.room_num_y, rec_words = RG_OBS_REC_WORDS(nrooms);
    const int base = blockIdx.x * OBS_FIX_GROUP;
    // the group's flag words and line masks; a lane past the group or the batch holds zeros: nothing to serve
    const bool in = lane < OBS_FIX_GROUP && base + lane < n;
    const uint32_t fl = in ? S.flags[base + lane] : 0u;
    uint32_t rows = in ? (uint32_t)S.enc_rows[base + lane] : 0u;
    // the tables go out beside those loads and are written BEFORE the early exit: with their first use behind it the compiler sinks the loads there, a round
    // trip of their own for every group with work.  (gray_lut: the table the step launch's helpers encoded with -- the host's, the same single division
    // as k_obs_stream's)
    lutf[lane] = S.gray_lut[lane];
    lutf[lane + WAVE] = S.gray_lut[lane + WAVE];
    static_assert(((RG_MAX_ENEMY_KINDS + 6) & (RG_MAX_ENEMY_KINDS + 5)) == 0 && RG_MAX_ENEMY_KINDS + 6 <= WAVE, "the glyph table is filled without a lane mask");
    mtile[lane & (RG_MAX_ENEMY_KINDS + 5)] = c.mon[lane & (RG_MAX_ENEMY_KINDS + 5)].tile;  // (no lane mask: a load under one is issued behind the others' wait)
    uint64_t rmask = __ballot(fl & RG_FLAG_REDRAW);
    if (fl & RG_FLAG_REDRAW) rows = 0u;  // (drawn in full below)
    if (!(rmask | __ballot(rows != 0u))) return;
    // an env's tile words and observation record: plain loads, no select (a lane past the record reads its last word again and drops it: RG_OBS_REDRAW_ENV)
    const int rec_lane = lane < rec_words ? lane : rec_words - 1;
    auto load_tiles = [&](int e, uint4 &v, uint32_t &rec) {
        v = reinterpret_cast<const uint4 *>(S.cell + (size_t)e * HW)[lane];
        rec = S.obs_rec[(size_t)e * rec_words + rec_lane];
    };
    uint4 tv;       // (read only behind a load: the Redraw loop runs where rmask is not 0)
    uint32_t trec;
    if (rmask) load_tiles(base + __builtin_ctzll(rmask), tv, trec);  // in flight while the list is built and the masked lines are served
    // the line list: lane i's entries start at the number of lines of envs 0 .. i-1 (lanes past the group count 0)
    const int cnt = __popc(rows);
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < OBS_FIX_GROUP; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const int total = __shfl(incl, OBS_FIX_GROUP - 1);  // <= 16 OBS_FIX_GROUP: the list's size
    {
        int at = incl - cnt;
        for (uint32_t r = rows; r; r &= r - 1) list[at++] = (fix_entry_t)((lane << 4) | __builtin_ctz(r));
    }
    lds_barrier();  // the tables and the list are ready
    auto gray4 = [&](uint32_t w) {
        w &= 0x7f7f7f7fu;
        float4 v; v.x = lutf[w & 0xff]; v.y = lutf[(w >> 8) & 0xff]; v.z = lutf[(w >> 16) & 0xff]; v.w = lutf[w >> 24];
        return v;
    };
    {
        // image line b of an env = cells 32 b .. 32 b + 31 = mirror words 8 b .. 8 b + 7 = float4s 8 b .. 8 b + 7 of its image
        const uint32_t *m = reinterpret_cast<const uint32_t *>(S.screen) + (size_t)base * Q4;
        float4 *o = reinterpret_cast<float4 *>(out) + (size_t)base * Q4;
        const int slot = lane >> 3, sub = lane & 7;
        auto serve = [&](int p0) {  // passes p0 .. p0 + OBS_FIX_AHEAD - 1: every mirror word requested before the first store
            uint32_t w[OBS_FIX_AHEAD];
            int off[OBS_FIX_AHEAD];
#pragma unroll
            for (int k = 0; k < OBS_FIX_AHEAD; k++) {
                // (a lane past the list reads the list's last line again and stores nothing)
                const int idx = (p0 + k) * 8 + slot;
                const uint32_t ent = list[idx < total ? idx : total - 1];
                const int at = (int)(ent >> 4) * Q4 + (int)(ent & 15u) * 8 + sub;
                w[k] = m[at];
                off[k] = idx < total ? at : -1;
            }
#pragma unroll
            for (int k = 0; k < OBS_FIX_AHEAD; k++)
                if (off[k] >= 0) store_obs(&o[off[k]], gray4(w[k]));
        };
        // the first OBS_FIX_AHEAD passes are straight-line code (a group of ordinary play has about 12 lines): in front of a loop that loads, the compiler waits for
        // every load in flight -- the Redraw's tiles
        if (total > 0) serve(0);
        for (int p0 = OBS_FIX_AHEAD; p0 * 8 < total; p0 += OBS_FIX_AHEAD) serve(p0);
    }
    if (rmask) {  // k_obs_resid's Redraw service.  (The first env's inputs and the later ones' are different variables: as one loop-carried pair the compiler
                  // copied the first load's registers right behind the load, a wait for the tiles in front of everything else.)
        uint4 v = tv;
        uint32_t t_rec = trec;
        for (;;) {
            const int i = __builtin_ctzll(rmask);
            rmask &= rmask - 1;
            const int e = base + i;
            const uint32_t fle = __builtin_amdgcn_readlane(fl, i);
            uint4 nv;
            uint32_t nrec;
            if (rmask) load_tiles(base + __builtin_ctzll(rmask), nv, nrec);  // the next Redraw's, in flight behind this draw
            { RG_OBS_REDRAW_ENV(); }
            if (!rmask) break;
            v = nv;
            t_rec = nrec;
        }
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launchers: defined here against the prototypes the host units call them by
// ---------------------------------------------------------------------------------------------
#ifndef RG_BUILD_ID
#define RG_BUILD_ID "unstamped"
#endif
extern "C" {
// the build id of this library, readable from the file as librogue_gym_hip.so's is (rg_api.cpp rg_build_id)
const char *rgk_obs_fix_build_id(void) { static const char id[] = "RGBUILDID:" RG_BUILD_ID; return id + 10; }
// one one-wave block per group of OBS_FIX_GROUP envs; an empty batch still launches a (guarded) block
int rgk_obs_fix_blocks(int n) {
    const int blocks = (n + OBS_FIX_GROUP - 1) / OBS_FIX_GROUP;
    return blocks < 1 ? 1 : blocks;
}
// the same contract as rgk_obs_resid (rg_obs.hip): S->enc_rows is the last step launch's, the grid has 512 cells (rgk_obs_tail_capable)
void rgk_obs_fix(const RgState *S, const RgConfig *c, float *out, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    rg_launch(k_obs_fix, dim3(rgk_obs_fix_blocks(S->n)), dim3(WAVE), 0, st, ev0, ev1, *S, *c, out);
}
}
