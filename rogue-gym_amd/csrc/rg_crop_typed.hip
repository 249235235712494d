// rg_crop_typed.hip -- the player-centred crop: f32, f16 and bf16 images and a window of symbol ids (rg_obs_crop, rg_obs_crop_typed; gfx950).
//
//   k_crop_typed<KIND, DT> : KIND 0 gray / 1 one-hot with DT = RG_OBS_F32 / RG_OBS_F16 / RG_OBS_BF16, KIND 2 symbol ids with RG_OBS_U8
//
// Env e's window is [C][2ry+1][2rx+1], centred on its player cell, of the image the full encode would write, padded with the encoding of ' ' (gray 0, one-hot
// channel 0, history 0, status planes their constant value).  The mirrors are current (rg_api_obs.cpp flushes the pending render first): this pass only reads them.
// The scheme: a wave per run of envs on a persistent grid, the window's box of mirror cells staged in LDS, every plane expanded from LDS in the output's type
// (no value converted per cell) and stored as 16-byte pieces.  An f32 element is the value itself, a 16-bit one that value rounded to nearest even.
// Built with -Os like rg_obs.hip.  file:line citations name the reference's sources, as in rg_obs.hip.
#include <type_traits>
#include "rg_device.h"

// x / d for 0 <= x < 2^30 by a multiply and a shift (m = ceil(2^s / d), s = 30 + ceil(log2 d): exact on that range; computed on the host).  The five
// divisors' shifts share one word, 6 bits each (kernel arguments live in SGPRs, and the crop kernel has few to spare)
enum { CT_D_CA, CT_D_AREA, CT_D_WC, CT_D_BB, CT_D_BW };
static __device__ __forceinline__ uint32_t mdiv(uint32_t x, uint32_t m, uint32_t shifts, int which) {
    return (uint32_t)(((uint64_t)x * m) >> ((shifts >> (6 * which)) & 63));
}
struct CropTypedArgs {
    int ry, rx, hc, wc, area, ca;         // radii, window height and width, window cells, elements per env (C x area)
    int run, bh, bw, bb;                  // envs per wave, the staged box (rows, columns, cells: bh * bw)
    int planes, nst, with_hist, nplanes;  // glyph planes (1, or the handle's one-hot depth), status planes, history plane, C
    uint32_t sflag;
    uint32_t m[5], shifts;                // multipliers and shifts of x / ca, x / area, x / wc, x / bb, x / bw (CT_D_*)
};

// the element of type DT that holds the finite f32 `f`, as bits: f itself, or the 16-bit value nearest to it
template <int DT>
static __device__ __forceinline__ uint32_t crop_elem(float f) { return DT == RG_OBS_F32 ? __float_as_uint(f) : cvt16<DT>(f); }

#define CT_UNROLL 8
#define CT_WAVES 16384
// LDS, with `ts` the bytes of a table entry (4 for f32 elements, else 2): 128 entries glyph -> gray value, 128 bytes glyph -> symbol id, then per env of the
// run 16 bytes of geometry and 16 entries of status values, then the boxes
#define CT_LDS_FIXED(ts) (128 * (ts) + 128)
#define CT_LDS_PER_ENV(ts) (16 + 16 * (ts))

// One wave owns a RUN of a.run consecutive envs, on a persistent grid.  Each env's window is staged in LDS as the BOX of min(2ry+1, H) x min(2rx+1, W)
// mirror cells that holds every screen cell of the window: glyphs (gray) or symbol ids (one-hot, ids) and, with the history plane, visited bytes; a window
// cell outside the screen is ' ' / 0 without a read.  The run's images are one contiguous stretch of the tensor, which the lanes write as 16-byte PIECES
// of the tensor (EPL = 4, 8 or 16 consecutive elements): a lane decodes its piece's first element into (env, plane, window row, column) once, with the
// multiply-shift division, and steps from there.  An env's image is C x area x sizeof(T) bytes -- 9 for a 3x3 id window -- so a run neither starts nor ends
// on a piece boundary in general (an f32 run starts on one: the run length is a multiple of 4): the run's first and last piece are written element by
// element, only the elements that are the run's (the neighbouring run's wave writes the others), and every piece in between is one non-temporal 16-byte
// store.  This form serves every window with any run length, so the run is chosen by LDS and bytes in flight alone.
// GROUPS (ext: a config group of a handle with several): env e's image goes to the handle's env ext[e] -- element stores, one env's image apart from the next.
// InvalidTileError (one-hot and ids): raised for a glyph without a symbol INSIDE the window only; box cells outside it are not checked.
// (The kernel takes the few arrays it reads, not RgState / RgConfig by value, as k_obs_typed does: their kernel arguments cost the one-hot instances SGPR spills.)
template <int KIND, int DT>
__global__ void __launch_bounds__(WAVE) k_crop_typed(const uint16_t *__restrict__ p_pos, const int32_t *__restrict__ status, const uint8_t *__restrict__ screen,
                                                    const uint8_t *__restrict__ hist, uint32_t *__restrict__ flags, const int32_t *__restrict__ ext, int n, int W, int H,
                                                    int symbols, CropTypedArgs a, uint8_t *__restrict__ out, int32_t *__restrict__ centers,
                                                    uint32_t *__restrict__ err_any) {
    constexpr int ES = DT == RG_OBS_U8 ? 1 : DT == RG_OBS_F32 ? 4 : 2;  // bytes per element
    constexpr int EPL = 16 / ES;                  // elements per 16-byte piece
    constexpr int EPW = 4 / ES;                   // elements per 32-bit word
    constexpr uint32_t ONE = DT == RG_OBS_U8 ? 1u : DT == RG_OBS_F16 ? 0x3C00u : DT == RG_OBS_BF16 ? 0x3F80u : 0x3F800000u;  // 1.0 (history plane of the ids: 1)
    typedef typename std::conditional<DT == RG_OBS_F32, uint32_t, uint16_t>::type tab_t;  // a table entry: an element's bits
    constexpr int TS = sizeof(tab_t);
    extern __shared__ __align__(16) uint8_t smem[];
    tab_t *lutv = reinterpret_cast<tab_t *>(smem);             // glyph -> gray value, in the output's type (KIND 0)
    uint8_t *luts = smem + 128 * TS;                            // glyph -> symbol id
    int4 *geo = reinterpret_cast<int4 *>(smem + CT_LDS_FIXED(TS));  // [run] {player y, player x, box row 0, box column 0}
    tab_t *stv = reinterpret_cast<tab_t *>(smem + CT_LDS_FIXED(TS) + 16 * a.run);  // [run][16] status plane values, converted once per env
    uint8_t *box = smem + CT_LDS_FIXED(TS) + CT_LDS_PER_ENV(TS) * a.run;  // [run][bb] staged glyphs (gray) or symbol ids
    uint8_t *hbox = box + (size_t)a.run * a.bb;                 // [run][bb] staged visited bytes (with_hist)
    const int lane = threadIdx.x, HW = W * H, R = a.run;
    for (int g = lane; g < 128; g += WAVE) {
        const uint32_t sy = tile_to_sym((uint32_t)g);
        luts[g] = (uint8_t)sy;
        if (KIND == 0) lutv[g] = (tab_t)crop_elem<DT>((float)(uint8_t)sy / (float)(uint8_t)symbols);  // python/src/lib.rs:84 (the same single f32 division as k_obs)
    }
    const uint32_t smax = (uint32_t)symbols - 1;  // construct_symbol_map fills channels 0..symbols-2 (symbol.rs:51-71)
    const int nruns = (n + R - 1) / R;
    for (int run = blockIdx.x; run < nruns; run += gridDim.x) {
        const int base = run * R, cnt = n - base < R ? n - base : R;
        lds_barrier();  // the previous run's LDS reads done (and, the first time, the tables written)
        if (lane < cnt) {
            const int e = base + lane;
            const uint32_t pos = p_pos[e];
            const int cx = POS_X(pos), cy = POS_Y(pos);
            const int oy = min(max(cy - a.ry, 0), H - a.bh), ox = min(max(cx - a.rx, 0), W - a.bw);
            geo[lane] = make_int4(cy, cx, oy, ox);
            if (KIND != 2) {
                int p = 0;
                for (int b = 0; b < 9; b++)  // StatusFlagInner bit b -> index b + (b > 0) of Status::to_vec (rg_obs.hip kStatusIdx)
                    if (a.sflag & (1u << b)) stv[lane * 16 + p++] = (tab_t)crop_elem<DT>((float)status[(size_t)e * 10 + b + (b > 0)]);
            }
            if (centers) {
                const int xe = ext ? ext[e] : e;
                centers[2 * (size_t)xe] = cy;
                centers[2 * (size_t)xe + 1] = cx;
            }
        }
        lds_barrier();
        // ---- stage the boxes: CT_UNROLL independent byte loads per lane in flight, then the LDS writes (one-hot, ids: the symbol id, not the glyph) ----
        const int tot = cnt * a.bb;
        auto box_cell = [&](int k, int &r, int &y, int &x) {
            r = (int)mdiv((uint32_t)k, a.m[CT_D_BB], a.shifts, CT_D_BB);
            const int t = k - r * a.bb, j = (int)mdiv((uint32_t)t, a.m[CT_D_BW], a.shifts, CT_D_BW);
            const int4 gg = geo[r];
            y = gg.z + j; x = gg.w + (t - j * a.bw);
        };
        for (int k0 = 0; k0 < tot; k0 += WAVE * CT_UNROLL) {
            uint32_t gv[CT_UNROLL], hv[CT_UNROLL];
#pragma unroll
            for (int u = 0; u < CT_UNROLL; u++) {
                int r, y, x;
                box_cell(min(k0 + u * WAVE + lane, tot - 1), r, y, x);  // (past the end a repeat of the last cell, not a branch)
                const size_t off = (size_t)(base + r) * HW + y * W + x;
                gv[u] = screen[off];
                hv[u] = a.with_hist ? hist[off] : 0u;
            }
            uint32_t bad = 0;  // bit u: staged cell u is a glyph without a symbol inside its window (InvalidTileError, e.g. 'Z')
#pragma unroll
            for (int u = 0; u < CT_UNROLL; u++) {
                const int k = k0 + u * WAVE + lane;
                if (k >= tot) continue;
                const uint32_t g = gv[u] & 0x7f;
                box[k] = KIND ? luts[g] : (uint8_t)g;
                if (a.with_hist) hbox[k] = (uint8_t)hv[u];
                if (KIND != 0 && luts[g] >= smax) {
                    int r, y, x;
                    box_cell(k, r, y, x);
                    const int4 gg = geo[r];
                    bad |= (abs(y - gg.x) <= a.ry && abs(x - gg.y) <= a.rx) ? 1u << u : 0u;
                }
            }
            if (KIND != 0 && bad) {  // (rare: outside the loop, which then holds no atomics)
#pragma unroll 1
                for (int u = 0; u < CT_UNROLL; u++)
                    if ((bad >> u) & 1) {
                        int r, y, x;
                        box_cell(k0 + u * WAVE + lane, r, y, x);
                        atomicOr(&flags[base + r], RG_FLAG_ERR_TILE);
                    }
                atomicOr(err_any, RG_FLAG_ERR_TILE);
            }
        }
        lds_barrier();
        // ---- expand: every value from LDS, already in the output's type ----
        auto value = [&](int r, int p, int j, int i) -> uint32_t {
            const int4 gg = geo[r];
            const int y = gg.x - a.ry + j, x = gg.y - a.rx + i;
            const bool inside = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            const int bi = r * a.bb + (y - gg.z) * a.bw + (x - gg.w);
            if (p < a.planes) {
                if (KIND == 0) return lutv[inside ? box[bi] : (uint32_t)' '];
                const uint32_t sy = inside ? box[bi] : 0u;  // (' ' is symbol 0)
                if (KIND == 2) return sy;
                return (sy == (uint32_t)p && (uint32_t)p < smax) ? ONE : 0u;
            }
            if (KIND != 2 && p < a.planes + a.nst) return stv[r * 16 + (p - a.planes)];
            return (inside && hbox[bi]) ? ONE : 0u;
        };
        // the run's elements are [0, totf) of the stretch that starts at element base * ca of the tensor; `hs` elements of the piece that holds
        // its first one belong to the run before (GROUPS: every element is stored by itself, pieces are only the lanes' share of the work)
        const int totf = cnt * a.ca;
        const size_t first = (size_t)base * a.ca;
        const int hs = ext ? 0 : (int)(first & (size_t)(EPL - 1));
        uint8_t *o = out + (first - hs) * ES;  // 16-byte aligned (rg_obs_crop_typed checks `out`)
        const int npieces = (hs + totf + EPL - 1) / EPL;
        for (int k = lane; k < npieces; k += WAVE) {
            const int f0 = k * EPL - hs;  // the piece's first element, relative to the run: negative in the run's first piece only
            const int fs = max(f0, 0);
            int r = (int)mdiv((uint32_t)fs, a.m[CT_D_CA], a.shifts, CT_D_CA);
            const int rem = fs - r * a.ca;
            int p = (int)mdiv((uint32_t)rem, a.m[CT_D_AREA], a.shifts, CT_D_AREA);
            const int cell = rem - p * a.area;
            int j = (int)mdiv((uint32_t)cell, a.m[CT_D_WC], a.shifts, CT_D_WC), i = cell - j * a.wc;
            const bool whole = !ext && f0 >= 0 && f0 + EPL <= totf;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (whole) {
#pragma unroll
                for (int t = 0; t < EPL; t++) {
                    w[t / EPW] |= value(r, p, j, i) << ((t % EPW) * 8 * ES);
                    if (++i == a.wc) { i = 0; if (++j == a.hc) { j = 0; if (++p == a.nplanes) { p = 0; ++r; } } }
                }
                u4v v = {w[0], w[1], w[2], w[3]};
                __builtin_nontemporal_store(v, reinterpret_cast<u4v *>(o + (size_t)k * 16));
            } else {  // the run's first and last piece, and every piece of a config group: element stores, the run's own elements only
#pragma unroll 1
                for (int f = fs; f < min(f0 + EPL, totf); f++) {
                    const uint32_t v = value(r, p, j, i);
                    uint8_t *dst = ext ? out + ((size_t)ext[base + r] * a.ca + (size_t)(f - r * a.ca)) * ES : out + (first + (size_t)f) * ES;
                    if (ES == 1) __builtin_nontemporal_store((uint8_t)v, dst);
                    else if (ES == 2) __builtin_nontemporal_store((uint16_t)v, reinterpret_cast<uint16_t *>(dst));
                    else __builtin_nontemporal_store(v, reinterpret_cast<uint32_t *>(dst));
                    if (++i == a.wc) { i = 0; if (++j == a.hc) { j = 0; if (++p == a.nplanes) { p = 0; ++r; } } }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launcher: defined here against the prototype the host units call it by
// ---------------------------------------------------------------------------------------------
static void host_magic(CropTypedArgs &a, int which, uint32_t d) {  // (mdiv)
    uint32_t l = 0;
    while ((1u << l) < d) l++;
    const uint32_t s = 30 + l;
    a.m[which] = (uint32_t)(((1ull << s) + d - 1) / d);
    a.shifts |= s << (6 * which);
}
extern "C" {
// the player-centred crop (rg_obs_crop, rg_obs_crop_typed; kind / dtype combination, radii and arguments checked by the caller, mirrors drawn): one wave per run of
// envs, persistent grid.  Returns 0 if the window's size does not fit the kernel's index arithmetic or its LDS (cannot happen within the documented radii).
int rgk_crop_typed(const RgState *S, const RgConfig *c, int kind, int dtype, int ry, int rx, uint32_t sflag, int with_hist, int planes_sym, void *out, int32_t *centers,
                   uint32_t *err_any, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    CropTypedArgs a;
    const int hc = 2 * ry + 1, es = dtype == RG_OBS_U8 ? 1 : dtype == RG_OBS_F32 ? 4 : 2, ts = dtype == RG_OBS_F32 ? 4 : 2;
    a.ry = ry; a.rx = rx; a.hc = hc; a.wc = 2 * rx + 1; a.area = hc * a.wc;
    a.planes = kind == 1 ? planes_sym : 1; a.nst = kind == 2 ? 0 : __builtin_popcount(sflag); a.with_hist = with_hist ? 1 : 0; a.sflag = kind == 2 ? 0u : sflag;
    a.nplanes = a.planes + a.nst + a.with_hist;
    a.ca = a.nplanes * a.area;
    a.bh = hc < c->height ? hc : c->height; a.bw = a.wc < c->width ? a.wc : c->width; a.bb = a.bh * a.bw;
    // envs per wave: 4, doubled while a run writes under 4 KB and stages at most 16 KB of LDS; any run length is served (a multiple of 4 starts every f32 run
    // on a piece boundary), so the largest window -- the whole 160 x 48 screen staged twice, 15 KB per env -- keeps the run of 4: at most 62 400 bytes of LDS
    a.run = 4;
    const size_t stage = (size_t)a.bb * (1 + a.with_hist);
    while (a.run < 64 && (size_t)a.run * a.ca * es < 4096 && (size_t)a.run * 2 * stage <= 16384) a.run *= 2;
    const size_t smem = CT_LDS_FIXED(ts) + CT_LDS_PER_ENV(ts) * (size_t)a.run + (size_t)a.run * stage;
    if (smem > 65536 || (uint64_t)a.run * a.ca >= (1ull << 30) || (uint64_t)a.run * a.bb >= (1ull << 30)) return 0;
    a.shifts = 0;
    host_magic(a, CT_D_CA, (uint32_t)a.ca); host_magic(a, CT_D_AREA, (uint32_t)a.area); host_magic(a, CT_D_WC, (uint32_t)a.wc);
    host_magic(a, CT_D_BB, (uint32_t)a.bb); host_magic(a, CT_D_BW, (uint32_t)a.bw);
    const int nruns = (S->n + a.run - 1) / a.run;
    const int blocks = nruns < CT_WAVES ? nruns : CT_WAVES;
    auto launch = [&](auto kernel) {
        rg_launch(kernel, dim3(blocks), dim3(WAVE), smem, st, ev0, ev1, S->p_pos, S->status, S->screen, S->hist, S->flags, S->ext, S->n, (int)c->width, (int)c->height,
                  (int)c->symbols, a, static_cast<uint8_t *>(out), centers, err_any);
    };
    if (kind == 2) launch(k_crop_typed<2, RG_OBS_U8>);
    else if (kind == 0) { if (dtype == RG_OBS_F32) launch(k_crop_typed<0, RG_OBS_F32>); else if (dtype == RG_OBS_F16) launch(k_crop_typed<0, RG_OBS_F16>); else launch(k_crop_typed<0, RG_OBS_BF16>); }
    else if (dtype == RG_OBS_F32) launch(k_crop_typed<1, RG_OBS_F32>);
    else if (dtype == RG_OBS_F16) launch(k_crop_typed<1, RG_OBS_F16>);
    else launch(k_crop_typed<1, RG_OBS_BF16>);
    return 1;
}
}
