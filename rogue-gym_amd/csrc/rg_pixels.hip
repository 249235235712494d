// rg_pixels.hip -- screens and player-centred windows as pixels through a tileset (rg_obs_pixels / rg_obs_pixels_crop; gfx950).  The rule: rg_pixels.h.
//
//   k_pixels : one instance; channels, tile height, window and screen size are run-time arguments
//
// The child of k_crop_typed (rg_crop_typed.hip: a wave per run of envs on a persistent grid, the window's box of mirror cells staged in LDS, the run's images
// one contiguous stretch of the tensor written in 16-byte pieces, `ext` for config groups).  Built with -Os like the other observation passes.
#include "rg_device.h"
#include "rg_pixels.h"

// x / d for 0 <= x < 2^30 by a multiply and a shift (k_crop_typed's mdiv: m = ceil(2^s / d), s = 30 + l, l = ceil(log2 d), computed on the host; here the shift
// kept is l): floor(x m / 2^s) = floor(floor(4 x m / 2^32) / 2^l), and 4 x fits 32 bits -- one v_mul_hi_u32 and two shifts, no 64-bit product
enum { PX_D_UPE, PX_D_PU, PX_D_WC, PX_D_TH, PX_D_BB, PX_D_BW, PX_DIVS };
static __device__ __forceinline__ uint32_t mdiv(uint32_t x, uint32_t m, uint32_t l) { return __umulhi(x << 2, m) >> l; }
struct PixelArgs {
    int crop, ry, rx, hc, wc;       // a window around the player (else the whole screen: hc = H, wc = W), radii, window cells
    int th, channels;               // tile rows, 1 (gray) or 3 (RGB)
    int pu, upe;                    // 8-byte units (one cell's pixel row in one channel) per plane (hc * th * wc) and per env (channels * pu)
    int run, bh, bw, bb, staged;    // envs per wave, the staged box (rows, columns, cells: bh * bw); staged 0: the box does not fit the LDS, glyphs are read from memory
    uint32_t m[PX_DIVS];            // multipliers and shifts (l) of x / upe, x / pu, x / wc, x / th, x / bb, x / bw (PX_D_*)
    uint8_t s[PX_DIVS + 2];
};

typedef uint32_t u2v __attribute__((ext_vector_type(2)));

#define PX_UNROLL 8
#define PX_WAVES 4096     // 16 one-wave blocks on each of 256 CUs: every block resident, the tables staged once per wave
#define PX_LDS_MAX 10240  // 160 KB of LDS per CU / 16 blocks: four waves per SIMD
// LDS: the font [256][th] (padded to whole 16-byte pieces: it is one), the ink table's planes in use, then per env of the run 16 bytes of geometry, then the boxes
#define PX_LDS_GEO 16

// One wave owns a RUN of a.run consecutive envs.  The font, the channels' ink planes (entry 256 = the paper) and each env's box of glyph bytes are in LDS.  The
// output of a run is one contiguous stretch of 8-byte UNITS -- one cell's pixel row in one channel: a font row byte spread to eight mask bytes, ink selected
// over paper byte-wise (rg_px_row) -- which the lanes write as 16-byte PIECES of two units, consecutive lanes consecutive pieces of a pixel row.  An env's image
// is a multiple of 8 bytes and in general not of 16 (a window has an odd number of cells per row, th may be odd), so a run's first and last piece may be
// one unit, stored as 8 bytes; every piece in between is one non-temporal 16-byte store.  A lane decodes its piece's first unit into (env, channel, cell row,
// tile row, cell column) once with the multiply-shift division and steps to the second.
// GROUPS (ext: a config group of a handle with several): env e's image goes to the handle's env ext[e] -- every unit an 8-byte store.
__global__ void __launch_bounds__(WAVE) k_pixels(const uint16_t *__restrict__ p_pos, const uint8_t *__restrict__ screen, const int32_t *__restrict__ ext, int n, int W, int H,
                                                 const uint8_t *__restrict__ tiles, PixelArgs a, uint8_t *__restrict__ out, int32_t *__restrict__ centers) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int fbytes = 256 * a.th, tbytes = a.channels * RG_PX_TAB_STRIDE;
    const uint8_t *fontl = smem;                               // [256][th]
    const uint8_t *tabl = smem + fbytes;                       // [channels][RG_PX_TAB_STRIDE]
    int4 *geo = reinterpret_cast<int4 *>(smem + fbytes + tbytes);  // [run] {window row 0, window column 0, box row 0, box column 0} in screen coordinates
    uint8_t *box = smem + fbytes + tbytes + PX_LDS_GEO * a.run;    // [run][bb] staged glyph bytes
    const int lane = threadIdx.x, HW = W * H, R = a.run;
    {   // the tables, 16 bytes at a time: the font, then the luminance plane (gray) or the R, G, B planes
        const u4v *src = reinterpret_cast<const u4v *>(tiles);
        const u4v *tsrc = reinterpret_cast<const u4v *>(tiles + RG_PX_FONT_BYTES + (a.channels == 1 ? RG_PX_PLANE_LUM * RG_PX_TAB_STRIDE : 0));
        u4v *dst = reinterpret_cast<u4v *>(smem);
        for (int k = lane; k < fbytes / 16; k += WAVE) dst[k] = src[k];
        for (int k = lane; k < tbytes / 16; k += WAVE) dst[fbytes / 16 + k] = tsrc[k];
    }
    const int nruns = (n + R - 1) / R;
    for (int run = blockIdx.x; run < nruns; run += gridDim.x) {
        const int base = run * R, cnt = n - base < R ? n - base : R;
        lds_barrier();  // the previous run's LDS reads done (and, the first time, the tables written)
        if (lane < cnt) {
            const int e = base + lane;
            int cy = 0, cx = 0, oy = 0, ox = 0;
            if (a.crop) {
                const uint32_t pos = p_pos[e];
                cx = POS_X(pos); cy = POS_Y(pos);
                oy = min(max(cy - a.ry, 0), H - a.bh); ox = min(max(cx - a.rx, 0), W - a.bw);
                if (centers) {
                    const int xe = ext ? ext[e] : e;
                    centers[2 * (size_t)xe] = cy;
                    centers[2 * (size_t)xe + 1] = cx;
                }
            }
            geo[lane] = make_int4(cy - a.ry, cx - a.rx, oy, ox);  // (the whole screen: ry = rx = 0 and cy = cx = 0, the window starts at the screen's corner)
        }
        lds_barrier();
        // ---- stage the boxes: PX_UNROLL independent byte loads per lane in flight, then the LDS writes ----
        if (a.staged) {
            const int tot = cnt * a.bb;
            for (int k0 = 0; k0 < tot; k0 += WAVE * PX_UNROLL) {
                uint32_t gv[PX_UNROLL];
#pragma unroll
                for (int u = 0; u < PX_UNROLL; u++) {
                    const int k = min(k0 + u * WAVE + lane, tot - 1);  // (past the end a repeat of the last cell, not a branch)
                    const int r = (int)mdiv((uint32_t)k, a.m[PX_D_BB], a.s[PX_D_BB]);
                    const int t = k - r * a.bb, j = (int)mdiv((uint32_t)t, a.m[PX_D_BW], a.s[PX_D_BW]);
                    const int4 gg = geo[r];
                    gv[u] = screen[(size_t)(base + r) * HW + (gg.z + j) * W + gg.w + (t - j * a.bw)];
                }
#pragma unroll
                for (int u = 0; u < PX_UNROLL; u++) {
                    const int k = k0 + u * WAVE + lane;
                    if (k < tot) box[k] = (uint8_t)gv[u];
                }
            }
            lds_barrier();
        }
        // ---- expand ----
        auto unit = [&](int r, int c, int j, int py, int i) -> u2v {
            const int4 gg = geo[r];
            const int y = gg.x + j, x = gg.y + i;
            uint32_t g = ' ';
            if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
                g = a.staged ? box[r * a.bb + (y - gg.z) * a.bw + (x - gg.w)] : screen[(size_t)(base + r) * HW + y * W + x];
            const uint8_t *t = tabl + c * RG_PX_TAB_STRIDE;
            u2v v;
            uint32_t lo, hi;
            rg_px_row(fontl[g * a.th + py], t[g], t[256], lo, hi);
            v.x = lo; v.y = hi;
            return v;
        };
        // the run's units are [0, totu) of the stretch that starts at unit base * upe of the tensor; with `hs` the first unit of the piece that holds
        // its first one belongs to the run before (GROUPS: every unit is stored by itself, pieces are only the lanes' share of the work)
        const int totu = cnt * a.upe;
        const size_t first = (size_t)base * a.upe;
        const int hs = ext ? 0 : (int)(first & 1);
        uint8_t *o = out + (first - hs) * 8;  // 16-byte aligned (the entry points check `out`)
        const int npieces = (hs + totu + 1) >> 1;
        for (int k = lane; k < npieces; k += WAVE) {
            const int f0 = 2 * k - hs;  // the piece's first unit, relative to the run: -1 in the run's first piece only
            const int fs = max(f0, 0);
            int r = (int)mdiv((uint32_t)fs, a.m[PX_D_UPE], a.s[PX_D_UPE]);
            const int rem = fs - r * a.upe;
            int c = (int)mdiv((uint32_t)rem, a.m[PX_D_PU], a.s[PX_D_PU]);
            const int pr = rem - c * a.pu;
            const int row = (int)mdiv((uint32_t)pr, a.m[PX_D_WC], a.s[PX_D_WC]);
            int i = pr - row * a.wc, j = (int)mdiv((uint32_t)row, a.m[PX_D_TH], a.s[PX_D_TH]), py = row - j * a.th;
            auto next = [&]() { if (++i == a.wc) { i = 0; if (++py == a.th) { py = 0; if (++j == a.hc) { j = 0; if (++c == a.channels) { c = 0; ++r; } } } } };
            if (!ext && f0 >= 0 && f0 + 2 <= totu) {
                const u2v v0 = unit(r, c, j, py, i);
                next();
                const u2v v1 = unit(r, c, j, py, i);
                u4v v = {v0.x, v0.y, v1.x, v1.y};
                __builtin_nontemporal_store(v, reinterpret_cast<u4v *>(o + (size_t)k * 16));
            } else {  // the run's first and last piece where they are half the run's, and every piece of a config group: unit stores, the run's own units only
#pragma unroll 1
                for (int f = fs; f < min(f0 + 2, totu); f++) {
                    const u2v v = unit(r, c, j, py, i);
                    uint8_t *dst = ext ? out + ((size_t)ext[base + r] * a.upe + (size_t)(f - r * a.upe)) * 8 : out + (first + (size_t)f) * 8;
                    __builtin_nontemporal_store(v, reinterpret_cast<u2v *>(dst));
                    next();
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launchers: defined here against the prototypes the host units call them by
// ---------------------------------------------------------------------------------------------
static void host_magic(PixelArgs &a, int which, uint32_t d) {  // (mdiv)
    uint32_t l = 0;
    while ((1u << l) < d) l++;
    const uint32_t s = 30 + l;
    a.m[which] = (uint32_t)(((1ull << s) + d - 1) / d);
    a.s[which] = (uint8_t)l;
}
// the shape of a launch: everything the kernel's arguments hold but the pointers.  Returns the dynamic LDS of a block, 0 if the image does not fit the index arithmetic.
static size_t pixel_args(PixelArgs &a, int H, int W, int th, int channels, int ry, int rx) {
    a.crop = ry >= 0 ? 1 : 0;
    a.ry = a.crop ? ry : 0; a.rx = a.crop ? rx : 0;
    a.hc = a.crop ? 2 * ry + 1 : H; a.wc = a.crop ? 2 * rx + 1 : W;
    a.th = th; a.channels = channels;
    a.pu = a.hc * th * a.wc; a.upe = channels * a.pu;
    a.bh = a.hc < H ? a.hc : H; a.bw = a.wc < W ? a.wc : W; a.bb = a.bh * a.bw;
    // envs per wave: 1, doubled while a run writes at most 32 KB (the staging round trip and the last, partly filled round of pieces are paid once per run) and its boxes fit the LDS that lets 16 blocks reside on a CU.  A box that does not fit alone
    // (the whole screen from about 5 000 cells) is not staged: the glyph bytes then come from memory, th * channels reads of a cached byte each
    const size_t fixed = 256 * (size_t)th + (size_t)channels * RG_PX_TAB_STRIDE;
    a.staged = fixed + PX_LDS_GEO + (size_t)a.bb <= PX_LDS_MAX ? 1 : 0;
    a.run = 1;
    while (a.run < 64 && (size_t)a.run * 2 * a.upe * 8 <= 32768 && fixed + 2 * (size_t)a.run * (PX_LDS_GEO + (a.staged ? a.bb : 0)) <= PX_LDS_MAX) a.run *= 2;
    if ((uint64_t)a.run * a.upe >= (1ull << 30) || (uint64_t)a.run * a.bb >= (1ull << 30)) return 0;
    host_magic(a, PX_D_UPE, (uint32_t)a.upe); host_magic(a, PX_D_PU, (uint32_t)a.pu); host_magic(a, PX_D_WC, (uint32_t)a.wc); host_magic(a, PX_D_TH, (uint32_t)th);
    host_magic(a, PX_D_BB, (uint32_t)a.bb); host_magic(a, PX_D_BW, (uint32_t)a.bw);
    return fixed + (size_t)a.run * (PX_LDS_GEO + (a.staged ? a.bb : 0));
}
extern "C" {
// the dynamic LDS a launch of this shape asks for (ry < 0: the whole screen), *run and *staged as chosen; 0 = not served.  For the resource tests: no device.
int rgk_pixels_lds(int H, int W, int th, int channels, int ry, int rx, int *run, int *staged) {
    PixelArgs a;
    const size_t smem = pixel_args(a, H, W, th, channels, ry, rx);
    if (run) *run = a.run;
    if (staged) *staged = a.staged;
    return (int)smem;
}
// the pixel pass (arguments checked by the caller, mirrors drawn): `tiles` = the handle's tileset on the device, the font (RG_PX_FONT_BYTES, [256][th] at its
// start) then the ink table (RG_PX_TAB_BYTES).  ry < 0: the whole screen.  Returns 0 if the image does not fit the kernel's index arithmetic.
int rgk_pixels(const RgState *S, const RgConfig *c, const uint8_t *tiles, int th, int channels, int ry, int rx, uint8_t *out, int32_t *centers, hipStream_t st,
               hipEvent_t ev0, hipEvent_t ev1) {
    PixelArgs a;
    const size_t smem = pixel_args(a, (int)c->height, (int)c->width, th, channels, ry, rx);
    if (!smem || smem > PX_LDS_MAX) return 0;
    const int nruns = (S->n + a.run - 1) / a.run;
    const int blocks = nruns < PX_WAVES ? nruns : PX_WAVES;
    rg_launch(k_pixels, dim3(blocks), dim3(WAVE), smem, st, ev0, ev1, S->p_pos, S->screen, S->ext, S->n, (int)c->width, (int)c->height, tiles, a, out, centers);
    return 1;
}
}
