// rg_obs.hip -- render / observation-encode kernels of the batched Rogue-Gym stepper (gfx950).
//
//   k_obs<gray|symbol> : fused RunTime::draw_screen (mirror refresh of Redraw envs) + PlayerState::{gray,symbol}_image
//   k_obs_stream       : the same for the plain gray image of grids of at most 512 cells, streamed in runs of envs
//   k_redraw + k_obs_typed : the same images in f16 / bf16 elements, and the screen as a u8 plane of symbol ids (rg_obs_typed)
//   k_render, k_gray, k_symbol, k_encode_scalar : unfused fallbacks
//
// Built as its own translation unit with -Os: these kernels are bandwidth/latency-bound and measurably faster with less
// unrolling (k_obs 83 -> 67-70 us at 65 536 mini envs), while the issue-bound step kernel wants -O3.
// file:line citations are relative to /root/reference.
#include <cstdlib>
#include "rg_device.h"
#include "rg_obs_dev.h"

// ---------------------------------------------------------------------------------------------
// k_render: RunTime::draw_screen (core/src/lib.rs:264-285; rogue/mod.rs:278-300,398-404) into the
// PlayerState mirrors, only for envs whose last key produced Reaction::Redraw
// ---------------------------------------------------------------------------------------------
#define RENDER_THREADS 256
__device__ __forceinline__ bool in_same_room(const RgState &S, const RgConfig &c, int e, int ax, int ay, int bx, int by) {
    int id = room_id_of(c, ax, ay);  // Floor::in_same_room (floor.rs:381-393)
    if (id < 0 || room_id_of(c, bx, by) != id) return false;
    uint8_t meta = S.room_meta[id * S.n + e];
    if ((meta & RM_KIND_MASK) == RK_EMPTY) return true;
    int x0, y0, x1, y1;
    unpack_rect(S.room_rect[id * S.n + e], x0, y0, x1, y1);
    bool ina = ax >= x0 && ax < x1 && ay >= y0 && ay < y1, inb = bx >= x0 && bx < x1 && by >= y0 && by < y1;
    return ina == inb;
}

__global__ void __launch_bounds__(RENDER_THREADS) k_render(RgState S, RgConfig c) {
    __shared__ uint8_t s_scr[RG_MAX_W * RG_MAX_H];
    const int tid = threadIdx.x, W = c.width, H = c.height, HW = W * H, n = S.n;
    const int nrooms = c.room_num_x * c.room_num_y;
    for (int e = blockIdx.x; e < n; e += gridDim.x) {
        const uint32_t fl = S.flags[e];
        if (!(fl & RG_FLAG_REDRAW)) continue;
        const uint16_t *cell = S.cell + (size_t)e * HW;
        const bool upd_hist = !(fl & RG_FLAG_HIST_STALE);
        uint8_t *hist = S.hist + (size_t)e * HW;
        for (int i = tid; i < HW; i += RENDER_THREADS) {
            uint32_t v = cell[i];
            int y = i / W;
            uint8_t g = ' ';
            if (y >= 1 && y < H - 1 && (v & C_VISIBLE)) g = glyph_of(v);
            s_scr[i] = g;
            if (upd_hist) hist[i] = (v & C_VISITED) ? 1 : 0;
        }
        __syncthreads();
        const uint32_t ppos = S.p_pos[e];
        const int px = POS_X(ppos), py = POS_Y(ppos);
        // draw priority: player > gold > monster (core/src/lib.rs:271-283): lowest priority first
        for (int r = tid; r < nrooms; r += RENDER_THREADS) {  // (a grid may have more rooms than the block has threads)
            uint32_t w = S.mon_w0[r * n + e];
            if ((w >> 24) & MF_ALIVE) {
                int x = POS_X(w), y = POS_Y(w);
                uint32_t v = cell[y * W + x];
                int dx = px - x, dy = py - y;
                if ((v & (C_VISIBLE | C_DRAWN)) && y >= 1 && y < H - 1 && (dx * dx + dy * dy <= 2 || in_same_room(S, c, e, px, py, x, y)))
                    s_scr[y * W + x] = c.mon[(w >> 16) & 0xff].tile;
            }
        }
        __syncthreads();
        for (int r = tid; r < nrooms; r += RENDER_THREADS) {
            uint32_t g = S.gold_pos[r * n + e];
            if (g & 0x10000u) {
                int x = POS_X(g), y = POS_Y(g);
                if ((cell[y * W + x] & (C_VISIBLE | C_DRAWN)) && y >= 1 && y < H - 1) s_scr[y * W + x] = '*';
            }
        }
        __syncthreads();
        if (tid == 0 && (cell[py * W + px] & (C_VISIBLE | C_DRAWN)) && py >= 1 && py < H - 1) s_scr[py * W + px] = '@';
        __syncthreads();
        uint8_t *scr = S.screen + (size_t)e * HW;
        if ((HW & 3) == 0) {
            uint32_t *d4 = reinterpret_cast<uint32_t *>(scr);
            const uint32_t *s4 = reinterpret_cast<const uint32_t *>(s_scr);
            for (int i = tid; i < HW / 4; i += RENDER_THREADS) d4[i] = s4[i];
        } else
            for (int i = tid; i < HW; i += RENDER_THREADS) scr[i] = s_scr[i];
        if (tid == 0)  // the history plane was written unless this Redraw was stale
            S.flags[e] = (fl & ~(RG_FLAG_REDRAW | RG_FLAG_HIST_STALE | RG_FLAG_HIST_LAG | (upd_hist ? RG_FLAG_HIST_DIRTY : 0u))) | ((fl & RG_FLAG_HIST_STALE) ? RG_FLAG_HIST_LAG : 0u);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// k_gray / k_symbol: observation encode (python/src/lib.rs:72-111,162-205; flags.rs:88-115)
// one thread = 4 consecutive cells of one env, all planes; float4 (16-byte) stores
// ---------------------------------------------------------------------------------------------
// StatusFlagInner bit b -> index into Status::to_vec
__device__ __constant__ uint8_t kStatusIdx[9] = {0, 2, 3, 4, 5, 6, 7, 8, 9};

// rs / rst: distance between two envs' records in bytes (screen, hist) and in i32 words (status): hw and 10 for the mirrors, the record size for
// a packed compact batch (rg_pack_compact)
__global__ void __launch_bounds__(256) k_gray(const uint8_t *__restrict__ screen, const uint8_t *__restrict__ hist, const int32_t *__restrict__ status,
                                              int n, int hw, size_t rs, size_t rst, int symbols, uint32_t sflag, int with_hist, float *__restrict__ out,
                                              const int32_t *__restrict__ ext) {
    const int q = hw >> 2;  // quads per env (hw % 4 == 0 checked on the host)
    const size_t total = (size_t)n * q;
    const int nplanes = 1 + __popc(sflag) + (with_hist ? 1 : 0);
    const float fsym = (float)(uint8_t)symbols;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        int e = (int)(g / q), i = (int)(g - (size_t)e * q);
        uint32_t s4 = reinterpret_cast<const uint32_t *>(screen + (size_t)e * rs)[i];
        float4 v;
        v.x = (float)(uint8_t)tile_to_sym(s4 & 0xff) / fsym;
        v.y = (float)(uint8_t)tile_to_sym((s4 >> 8) & 0xff) / fsym;
        v.z = (float)(uint8_t)tile_to_sym((s4 >> 16) & 0xff) / fsym;
        v.w = (float)(uint8_t)tile_to_sym(s4 >> 24) / fsym;
        float4 *o = reinterpret_cast<float4 *>(out + (size_t)(ext ? ext[e] : e) * nplanes * hw) + i;
        o[0] = v;
        int p = 1;
        for (int b = 0; b < 9; b++)
            if (sflag & (1u << b)) {
                float f = (float)status[(size_t)e * rst + kStatusIdx[b]];
                float4 sv; sv.x = sv.y = sv.z = sv.w = f;
                o[(size_t)p * q] = sv;
                p++;
            }
        if (with_hist) {
            uint32_t h4 = reinterpret_cast<const uint32_t *>(hist + (size_t)e * rs)[i];
            float4 hv;
            hv.x = (h4 & 0xff) ? 1.f : 0.f; hv.y = (h4 & 0xff00) ? 1.f : 0.f; hv.z = (h4 & 0xff0000) ? 1.f : 0.f; hv.w = (h4 >> 24) ? 1.f : 0.f;
            o[(size_t)p * q] = hv;
        }
    }
}

__global__ void __launch_bounds__(256) k_symbol(const uint8_t *__restrict__ screen, const uint8_t *__restrict__ hist, const int32_t *__restrict__ status,
                                                uint32_t *__restrict__ flags, uint32_t *__restrict__ err_any,
                                                int n, int hw, size_t rs, size_t rst, int symbols, int planes_sym, uint32_t sflag, int with_hist, float *__restrict__ out,
                                                const int32_t *__restrict__ ext) {
    const int q = hw >> 2;
    const size_t total = (size_t)n * q;
    const int nplanes = planes_sym + __popc(sflag) + (with_hist ? 1 : 0);  // planes_sym >= symbols: the handle's one-hot depth (groups of a handle may differ)
    const uint32_t symbol_max = (uint32_t)symbols - 1;  // construct_symbol_map fills channels 0..symbols-2 (symbol.rs:51-71)
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        int e = (int)(g / q), i = (int)(g - (size_t)e * q);
        uint32_t s4 = reinterpret_cast<const uint32_t *>(screen + (size_t)e * rs)[i];
        uint32_t a = tile_to_sym(s4 & 0xff), b = tile_to_sym((s4 >> 8) & 0xff), cc = tile_to_sym((s4 >> 16) & 0xff), d = tile_to_sym(s4 >> 24);
        if (a >= symbol_max || b >= symbol_max || cc >= symbol_max || d >= symbol_max) {  // InvalidTileError (e.g. 'Z')
            if (flags) atomicOr(&flags[e], RG_FLAG_ERR_TILE);
            atomicOr(err_any, RG_FLAG_ERR_TILE);
        }
        float4 *o = reinterpret_cast<float4 *>(out + (size_t)(ext ? ext[e] : e) * nplanes * hw) + i;
        for (uint32_t ch = 0; ch < (uint32_t)planes_sym; ch++) {
            float4 v;
            v.x = a == ch ? 1.f : 0.f; v.y = b == ch ? 1.f : 0.f; v.z = cc == ch ? 1.f : 0.f; v.w = d == ch ? 1.f : 0.f;
            if (ch >= symbol_max) v.x = v.y = v.z = v.w = 0.f;
            o[(size_t)ch * q] = v;
        }
        int p = planes_sym;
        for (int bb = 0; bb < 9; bb++)
            if (sflag & (1u << bb)) {
                float f = (float)status[(size_t)e * rst + kStatusIdx[bb]];
                float4 sv; sv.x = sv.y = sv.z = sv.w = f;
                o[(size_t)p * q] = sv;
                p++;
            }
        if (with_hist) {
            uint32_t h4 = reinterpret_cast<const uint32_t *>(hist + (size_t)e * rs)[i];
            float4 hv;
            hv.x = (h4 & 0xff) ? 1.f : 0.f; hv.y = (h4 & 0xff00) ? 1.f : 0.f; hv.z = (h4 & 0xff0000) ? 1.f : 0.f; hv.w = (h4 >> 24) ? 1.f : 0.f;
            o[(size_t)p * q] = hv;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_obs: fused mirror refresh + observation encode (the steady-state path: one pass per step)
// ---------------------------------------------------------------------------------------------
// For every env: if the last key produced a Redraw, draw the screen from the tile words (+ entity
// overlays) and refresh the screen / history mirrors; otherwise re-read the 1-byte-per-cell mirror.  The
// screen is staged in LDS, then encoded straight into the caller's f32 tensor with float4 stores.
// HBM traffic per env-step (mini gray): 1 KB tiles (Redraw envs) or 0.5 KB mirror read, 0.5 KB mirror
// write (Redraw envs), 2 KB observation write.  A block of 256 threads serves `epb` envs, `tpe` threads each;
// a thread owns 8 consecutive cells (one 16-byte tile load, two float4 stores per plane).
#define OBS_THREADS 256
// (store_obs, ObsTabs, draw_cells8, monster_shown: rg_obs_dev.h, shared with rg_obs_fix.hip)

// GROUPS: the batch is one config group of a handle with several (RgState::ext maps its envs to the handle's env order, and the one-hot depth is the
// handle's): compiled separately so that the ordinary kernel carries none of it (its 72 registers = 7 waves per SIMD are what its bandwidth rests on)
// BOUND (rg_obs_bind): `out` is the handle's bound observation tensor and its contents are current up to the last k_step: only the envs that k_step listed
// (RgState::obs_list: final flag word with REDRAW or SCR_CHANGED) are encoded -- work item i is env list[i] -- and their SCR_CHANGED bit is cleared; every other
// env's image is already what a full encode would write.  A separate instance: the ordinary kernel carries none of it.
template <int KIND, bool GROUPS, bool BOUND = false>
__global__ void __launch_bounds__(OBS_THREADS) k_obs(RgState S, RgConfig c, uint32_t sflag, int with_hist, float *__restrict__ out,
                                                    uint32_t *__restrict__ err_any, int tpe, int epb, int planes_sym, int hi_prio) {
    // Wide grids: above the background generator's waves (k_regen, priority 0), which otherwise take issue slots from this bandwidth-bound pass for as long
    // as the two overlap (80x24: 79.9 -> 75.2 us, 222 -> 229 M).  Not where the step kernel is the capped two-waves-per-SIMD instance (W <= 32): generator waves
    // held back here are still resident when the next k_step starts, and there a resident generator wave keeps a step block waiting for its registers
    // (mini: k_obs 46.7 -> 45.6 us but k_step 55.7 -> 60.3 us; profiles/r04_experiments.txt).
    if (hi_prio) __builtin_amdgcn_s_setprio(3);
    extern __shared__ __align__(16) uint8_t smem[];
    float *lutf = reinterpret_cast<float *>(smem);        // glyph -> gray value (KIND 0)
    uint8_t *luts = smem + 512;                            // glyph -> symbol id
    uint8_t *mtile = smem + 512 + 128;                     // monster type -> glyph (RgConfig::mon[].tile: indexed per lane, so not from the kernarg segment)
    uint8_t *envs = smem + 512 + 128 + 64;                 // epb x {HW staged screen bytes, ObsTabs}
    const int tid = threadIdx.x, W = c.width, H = c.height, HW = W * H, Q8 = HW >> 3;
    // (BOUND: the work items are the entries of the last k_step's list)
    const int32_t *list = BOUND ? S.obs_list + (size_t)S.obs_par * S.n : nullptr;
    const int n = BOUND ? (int)S.obs_cnt[S.obs_par] : S.n;
    const int nrooms = c.room_num_x * c.room_num_y;
    const int symbols = c.symbols;
    for (int g = tid; g < 128; g += blockDim.x) {
        uint32_t sy = tile_to_sym((uint32_t)g);
        luts[g] = (uint8_t)sy;
        lutf[g] = (float)(uint8_t)sy / (float)(uint8_t)symbols;  // python/src/lib.rs:84 (same single division)
    }
    for (int g = tid; g < RG_MAX_ENEMY_KINDS + 6; g += blockDim.x) mtile[g] = c.mon[g].tile;
    const int le = tid / tpe, lt = tid - le * tpe;
    const int base_planes = KIND ? (GROUPS ? planes_sym : symbols) : 1;  // planes_sym >= symbols: the handle's one-hot depth (config groups of one handle may differ)
    const int nplanes = base_planes + __popc(sflag) + (with_hist ? 1 : 0);
    uint8_t *scr = envs + (size_t)le * OBS_ENV_BYTES(HW);
    ObsTabs *tb = reinterpret_cast<ObsTabs *>(scr + HW);
    // Persistent blocks, software-pipelined two envs deep: the flag word of the env after next and -- now that its flag word is known -- the
    // inputs of the next env (tile quad + entity tables if it redraws, its screen mirror if not) are requested before the current env is
    // encoded, so an env costs no exposed round trip and nothing is fetched that is not used.
    struct Pre { uint4 v0; uint32_t rec; };  // (`rec`: the lane's word of the env's observation record)
    const int rec_words = RG_OBS_REC_WORDS(nrooms);
    const uint32_t *rec_all = S.obs_rec;  // (rgk_obs: rec_words <= tpe, one word per thread)
    const int stride = gridDim.x * epb;
    // An env WITHOUT a pending Redraw -- nine in ten since the turn keeps the mirror itself -- is a plain stream: mirror word -> table -> float4.  With one env per
    // block (always) and at most two words per thread, such an env takes no LDS staging and none of the four barriers of the Redraw path: its words go from
    // the prefetch registers straight to the stores (round 6: the pass was latency-bound per block -- LDS round trips and barriers between the load and the
    // store of every env -- at 5.0 TB/s where a plain fill of the same 134 MB runs at 6.5).
    const int Q4 = HW >> 2;
    // Up to four words per thread: on the 32x16 grid a thread carries 16 cells and ONE wave serves TWO envs per iteration (tpe = 32, epb = 2: rgk_obs) -- twice the
    // bytes in flight per wave of a pass whose blocks are latency-bound (one env per memory round trip).  Two envs per block only where the block is a single wave:
    // its halves then take the two paths under lane masks and the staged path's barriers are the wave's own.
    const bool one_wave = blockDim.x == WAVE;
    const bool fast_ok = (epb == 1 || one_wave) && Q4 <= 4 * tpe && sflag == 0 && !with_hist;  // (status / history planes: the general path)
    // item -> env: the identity, or (BOUND) the list entry -- one more dependent load, fetched one iteration earlier than the flag word
    auto load_env = [&](int base) -> int {
        const int i = base + le;
        if (!BOUND) return i;
        return (le < epb && i < n) ? list[i] : 0;
    };
    auto load_flag = [&](int base, int e) -> uint32_t {
        return (le < epb && base + le < n) ? S.flags[e] : 0u;
    };
    auto prefetch = [&](int base, int e, uint32_t fl) {
        Pre p; p.v0 = make_uint4(0, 0, 0, 0); p.rec = 0;
        if (le < epb && base + le < n) {
            if (fl & RG_FLAG_REDRAW) {
                if (lt < Q8) p.v0 = reinterpret_cast<const uint4 *>(S.cell + (size_t)e * HW)[lt];
                if (lt < rec_words) p.rec = rec_all[(size_t)e * rec_words + lt];
            } else if (fast_ok) {  // the words this thread ENCODES (phase C's layout: words lt, lt + tpe, ...), see the fast path below
                const uint32_t *m4 = reinterpret_cast<const uint32_t *>(S.screen + (size_t)e * HW);
                if (lt < Q4) p.v0.x = m4[lt];
                if (lt + tpe < Q4) p.v0.y = m4[lt + tpe];
                if (lt + 2 * tpe < Q4) p.v0.z = m4[lt + 2 * tpe];
                if (lt + 3 * tpe < Q4) p.v0.w = m4[lt + 3 * tpe];
            } else if (lt < Q8) {
                const uint2 m = reinterpret_cast<const uint2 *>(S.screen + (size_t)e * HW)[lt];
                p.v0.x = m.x; p.v0.y = m.y;
            }
        }
        return p;
    };
    const uint32_t smax = (uint32_t)symbols - 1;  // construct_symbol_map fills channels 0..symbols-2 (symbol.rs:51-71)
    // one word (4 cells) of an env's image(s): glyph planes, status planes, history plane -- whole-line float4 stores (lanes contiguous in q)
    auto emit_glyphs = [&](float4 *o, int q, uint32_t g, bool &bad) {
        const int q4 = Q4;
        const uint32_t b0 = g & 0x7f, b1 = (g >> 8) & 0x7f, b2 = (g >> 16) & 0x7f, b3 = g >> 24;
        if (KIND == 0) {
            float4 v; v.x = lutf[b0]; v.y = lutf[b1]; v.z = lutf[b2]; v.w = lutf[b3];
            store_obs(&o[q], v);
        } else {
            const uint32_t s0 = luts[b0], s1 = luts[b1], s2 = luts[b2], s3 = luts[b3];
            bad = bad || s0 >= smax || s1 >= smax || s2 >= smax || s3 >= smax;
            for (uint32_t ch = 0; ch < smax; ch++) {
                float4 v;
                v.x = s0 == ch ? 1.f : 0.f; v.y = s1 == ch ? 1.f : 0.f; v.z = s2 == ch ? 1.f : 0.f; v.w = s3 == ch ? 1.f : 0.f;
                store_obs(&o[(size_t)ch * q4 + q], v);
            }
            float4 z; z.x = z.y = z.z = z.w = 0.f;
            for (uint32_t ch = smax; ch < (uint32_t)base_planes; ch++) store_obs(&o[(size_t)ch * q4 + q], z);  // the last channel is never set
        }
    };
    auto emit = [&](float4 *o, int q, uint32_t g, const float *stf, int nst, const uint32_t *hist4, bool &bad) {
        const int q4 = Q4;
        emit_glyphs(o, q, g, bad);
        int p = base_planes;
        for (int b = 0; b < nst; b++, p++) {
            float4 sv; sv.x = sv.y = sv.z = sv.w = stf[b];
            store_obs(&o[(size_t)p * q4 + q], sv);
        }
        if (with_hist) {
            const uint32_t h4 = hist4[q];  // (a redrawn env: written in phase A by this block, barrier in between)
            float4 a;
            a.x = (h4 & 0xff) ? 1.f : 0.f; a.y = (h4 & 0xff00) ? 1.f : 0.f; a.z = (h4 & 0xff0000) ? 1.f : 0.f; a.w = (h4 >> 24) ? 1.f : 0.f;
            store_obs(&o[(size_t)p * q4 + q], a);
        }
    };
    lds_barrier();  // the tables are ready (the fast path below has no barrier of its own)
    const int base0 = blockIdx.x * epb;
    int e_cur = load_env(base0), e_nxt = load_env(base0 + stride), e_nn = load_env(base0 + 2 * stride);
    uint32_t fl_cur = load_flag(base0, e_cur), fl_nxt = load_flag(base0 + stride, e_nxt);
    Pre nxt = prefetch(base0, e_cur, fl_cur);
    for (int base = base0; base < n; base += stride) {
        const int e = e_cur;
        const bool valid = le < epb && base + le < n;
        const Pre cur = nxt;
        const uint32_t fl = fl_cur;
        e_cur = e_nxt; e_nxt = e_nn;
        fl_cur = fl_nxt;
        fl_nxt = load_flag(base + 2 * stride, e_nxt);
        e_nn = load_env(base + 3 * stride);
        if (base + stride < n) nxt = prefetch(base + stride, e_cur, fl_cur);
        const uint4 *cell4 = reinterpret_cast<const uint4 *>(S.cell + (size_t)e * HW);
        const uint4 v0 = cur.v0;
        const uint32_t t_rec = cur.rec;
        // the register-to-store path of an env without a pending Redraw (a half-wave of a one-wave block, else the whole block: one env per block there)
        const bool my_fast = fast_ok && valid && !(fl & RG_FLAG_REDRAW);
        if (my_fast) {
            const int xe = GROUPS ? __builtin_amdgcn_readfirstlane(S.ext[e]) : e;
            float4 *o = reinterpret_cast<float4 *>(out + (size_t)xe * nplanes * HW);
            bool bad = false;
            if (lt < Q4) emit_glyphs(o, lt, v0.x & 0x7f7f7f7fu, bad);
            if (lt + tpe < Q4) emit_glyphs(o, lt + tpe, v0.y & 0x7f7f7f7fu, bad);
            if (lt + 2 * tpe < Q4) emit_glyphs(o, lt + 2 * tpe, v0.z & 0x7f7f7f7fu, bad);
            if (lt + 3 * tpe < Q4) emit_glyphs(o, lt + 3 * tpe, v0.w & 0x7f7f7f7fu, bad);
            if (KIND == 1 && bad) { atomicOr(&S.flags[e], RG_FLAG_ERR_TILE); atomicOr(err_any, RG_FLAG_ERR_TILE); }
            if (BOUND && lt == 0) atomicAnd(&S.flags[e], ~RG_FLAG_SCR_CHANGED);
        }
        const bool staged = valid && !my_fast;  // the lanes that take the staged path below
        if (fast_ok && !(one_wave ? __any(staged) : staged)) continue;  // (block-uniform: a one-wave block votes; several waves serve ONE env)
        const bool redraw = staged && (fl & RG_FLAG_REDRAW);
        lds_barrier();  // previous iteration's LDS reads done
        if (staged) {
            if (redraw) {
                if (lt < rec_words) tb->w[lt] = t_rec;
                // the history plane is rewritten only when the visited set changed since it was last written (k_step: HIST_DIRTY), never on a
                // stale Redraw
                const bool upd_hist = !(fl & RG_FLAG_HIST_STALE) && (fl & RG_FLAG_HIST_DIRTY);
                uint2 *hist8 = reinterpret_cast<uint2 *>(S.hist + (size_t)e * HW);
                for (int i = lt; i < Q8; i += tpe) {
                    uint4 v = i == lt ? v0 : cell4[i];
                    uint32_t g[2], hb[2];
                    draw_cells8(v, i, W, HW, g, hb);
                    reinterpret_cast<uint2 *>(scr)[i] = make_uint2(g[0], g[1]);
                    if (upd_hist) hist8[i] = make_uint2(hb[0], hb[1]);
                }
            } else {
                const uint2 *m8 = reinterpret_cast<const uint2 *>(S.screen + (size_t)e * HW);
                for (int i = lt; i < Q8; i += tpe) reinterpret_cast<uint2 *>(scr)[i] = i == lt ? make_uint2(v0.x, v0.y) : m8[i];
            }
        }
        lds_barrier();
        // ---- phase B: entity overlays from LDS only; draw priority monster < gold < player (core/src/lib.rs:271-283): a monster never replaces the
        //      '*' the decode put there (no other glyph is '*'), the player replaces anything ----
        const uint32_t ppos = redraw ? tb->w[nrooms] : 0;
        const int px = POS_X(ppos), py = POS_Y(ppos);
        if (redraw && lt < nrooms) {
            uint32_t w = tb->w[lt];
            if ((w >> 24) & MF_ALIVE) {
                int x = POS_X(w), y = POS_Y(w);
                const bool show = monster_shown(c, tb, nrooms, px, py, x, y);
                const uint32_t under = scr[y * W + x];
                if (show && (under & 0x80u) && under != (0x80u | '*')) scr[y * W + x] = (uint8_t)(0x80u | mtile[(w >> 16) & 0xff]);
            }
        }
        lds_barrier();
        if (redraw && lt == 0 && (scr[py * W + px] & 0x80u)) scr[py * W + px] = (uint8_t)(0x80u | '@');
        lds_barrier();
        if (with_hist) __syncthreads();  // the history plane is re-read from global memory below (written in phase A by other lanes)
        // ---- phase C: mirror write-back + encode.  One float4 (4 cells) per lane per plane, lanes contiguous: every wave-level store
        //      covers whole 128-byte lines (1 KB per instruction) ----
        if (staged) {
            uint32_t *m4 = reinterpret_cast<uint32_t *>(S.screen + (size_t)e * HW);
            const uint32_t *scr4 = reinterpret_cast<const uint32_t *>(scr);
            const uint32_t *hist4 = reinterpret_cast<const uint32_t *>(S.hist + (size_t)e * HW);
            const int xe = GROUPS ? __builtin_amdgcn_readfirstlane(S.ext[e]) : e;  // config-group handles write at the handle's env index (one env per block: uniform)
            float4 *o = reinterpret_cast<float4 *>(out + (size_t)xe * nplanes * HW);
            float stf[9];
            int nst = 0;
            for (int b = 0; b < 9; b++)
                if (sflag & (1u << b)) stf[nst++] = (float)S.status[(size_t)e * 10 + kStatusIdx[b]];
            bool bad = false;
            for (int q = lt; q < Q4; q += tpe) {
                const uint32_t g = scr4[q] & 0x7f7f7f7fu;
                if (redraw) m4[q] = g;
                emit(o, q, g, stf, nst, hist4, bad);
            }
            if (KIND == 1 && bad) { atomicOr(&S.flags[e], RG_FLAG_ERR_TILE); atomicOr(err_any, RG_FLAG_ERR_TILE); }
            const uint32_t seen = BOUND ? RG_FLAG_SCR_CHANGED : 0u;  // (the bound tensor now shows this env's screen)
            if (redraw && lt == 0) {  // a stale Redraw leaves the history mirror one level behind (k_step refreshes it before the next descent)
                const uint32_t clr = seen | RG_FLAG_REDRAW | RG_FLAG_HIST_STALE | RG_FLAG_HIST_LAG | ((fl & RG_FLAG_HIST_STALE) ? 0u : RG_FLAG_HIST_DIRTY);
                const uint32_t set = (fl & RG_FLAG_HIST_STALE) ? RG_FLAG_HIST_LAG : 0u;
                if (KIND == 1) {  // atomic: the other lanes OR their ERR_TILE into the same word (a plain store of this lane's view dropped theirs)
                    atomicAnd(&S.flags[e], ~clr);
                    if (set) atomicOr(&S.flags[e], set);
                } else S.flags[e] = (fl & ~clr) | set;
            } else if (BOUND && !redraw && lt == 0) atomicAnd(&S.flags[e], ~RG_FLAG_SCR_CHANGED);  // (atomic: the one-hot kind ORs its error bit into the same word)
        }
    }
}

// (RG_OBS_REDRAW_ENV, the Redraw service of k_obs_stream and k_obs_resid: rg_obs_dev.h, shared with k_obs_fix)

// ---------------------------------------------------------------------------------------------
// k_obs_stream: the gray image without status / history planes, no config groups, not bound, on grids of at most 512 cells (the headline workload:
// 65 536 mini envs).  Same bits, flags and mirrors as k_obs<0, false>.
// ---------------------------------------------------------------------------------------------
// One wave owns a RUN of OBS_RUN consecutive envs (4: 16 384 waves at 65 536 envs, eight per SIMD; runs of 8 and 16 and smaller grids measured slower,
// profiles/r07_experiments.txt), whose mirrors are one contiguous stretch of the screen array and whose images are one contiguous stretch
// of the tensor.  It issues the run's flag words (one coalesced load) and every mirror word of the run at once -- nothing of the stream waits on a flag --
// ballots on RG_FLAG_REDRAW, and streams each env without a pending Redraw (98 % of them) mirror word -> glyph table -> one whole-line float4 store per
// 64 words.  The run's Redraw envs are drawn afterwards from the tiles, one at a time, by the whole wave (the staged path of k_obs: LDS draw, overlays,
// mirror write-back, encode, flag word); the tile loads of the first are issued before the stream's stores, so its latency hides behind them, and the
// barriers are the wave's own.  k_obs instead walks its envs as a chain per block -- flag word -> mirror or tiles -> stores -- one env per round trip.
#ifndef OBS_RUN
#define OBS_RUN 4
#endif
#ifndef OBS_STREAM_WAVES
#define OBS_STREAM_WAVES 16384
#endif
__global__ void __launch_bounds__(WAVE) k_obs_stream(RgState S, RgConfig c, float *__restrict__ out, int hi_prio) {
    if (hi_prio) __builtin_amdgcn_s_setprio(3);
    __shared__ float lutf[128];                              // glyph -> gray value
    __shared__ uint8_t mtile[RG_MAX_ENEMY_KINDS + 6];        // monster type -> glyph
    __shared__ __align__(16) uint8_t scr[512];               // the staged screen of a Redraw env (HW <= 512: rgk_obs)
    __shared__ ObsTabs tb;                                   // its observation record
    const int lane = threadIdx.x, W = c.width, HW = W * c.height, Q4 = HW >> 2, Q8 = HW >> 3, n = S.n;
    const int nrooms = c.room_num_x * c.room_num_y, rec_words = RG_OBS_REC_WORDS(nrooms);
    for (int g = lane; g < 128; g += WAVE) lutf[g] = (float)(uint8_t)tile_to_sym((uint32_t)g) / (float)(uint8_t)c.symbols;  // python/src/lib.rs:84 (same single division)
    for (int g = lane; g < RG_MAX_ENEMY_KINDS + 6; g += WAVE) mtile[g] = c.mon[g].tile;
    lds_barrier();
    auto gray4 = [&](uint32_t w) {
        w &= 0x7f7f7f7fu;
        float4 v; v.x = lutf[w & 0xff]; v.y = lutf[(w >> 8) & 0xff]; v.z = lutf[(w >> 16) & 0xff]; v.w = lutf[w >> 24];
        return v;
    };
    // a run's flag words (lane i: env i) and mirror words (words lane and lane + 64 of each env: Q4 <= 128); zeros past the batch
    struct Run { uint32_t fl, w0[OBS_RUN], w1[OBS_RUN]; };
    auto load_run = [&](int r, Run &R) {
        const int base = r * OBS_RUN, cnt = n - base;
        R.fl = lane < cnt && lane < OBS_RUN ? S.flags[base + lane] : 0u;
        const uint32_t *m = reinterpret_cast<const uint32_t *>(S.screen) + (size_t)base * Q4;
#pragma unroll
        for (int i = 0; i < OBS_RUN; i++) {
            R.w0[i] = i < cnt && lane < Q4 ? m[i * Q4 + lane] : 0u;
            R.w1[i] = i < cnt && lane + WAVE < Q4 ? m[i * Q4 + lane + WAVE] : 0u;
        }
    };
    // Persistent waves, one run ahead: the next run's loads are issued before this run's stores, so a wave's loads and stores overlap and
    // the waves of the grid drift out of step (a wave with ONE run loads everything, then stores everything, all waves in the same phase)
    const int nruns = (n + OBS_RUN - 1) / OBS_RUN;
    Run cur;
    load_run(blockIdx.x, cur);
    for (int r = blockIdx.x; r < nruns; r += gridDim.x) {
        const int base = r * OBS_RUN, cnt = n - base < OBS_RUN ? n - base : OBS_RUN;
        Run nxt;
        load_run(r + gridDim.x, nxt);
        const uint32_t fl = cur.fl;
#ifdef RG_EXP_OBS_STREAM_BOUND
        uint64_t rmask = 0;  // (experiment build: every env streamed from its mirror, Redraws NOT drawn -- the bound of the stream, profiles/r07_experiments.txt)
#else
        uint64_t rmask = __ballot(fl & RG_FLAG_REDRAW);
#endif
        // the first Redraw env's tile words and observation record: in flight while the stream's stores issue
        auto load_tiles = [&](int e, uint4 &v, uint32_t &rec) {
            v = lane < Q8 ? reinterpret_cast<const uint4 *>(S.cell + (size_t)e * HW)[lane] : make_uint4(0, 0, 0, 0);
            rec = lane < rec_words ? S.obs_rec[(size_t)e * rec_words + lane] : 0u;
        };
        uint4 tv = make_uint4(0, 0, 0, 0);
        uint32_t trec = 0;
        if (rmask) load_tiles(base + __builtin_ctzll(rmask), tv, trec);
        float4 *o = reinterpret_cast<float4 *>(out) + (size_t)base * Q4;
#pragma unroll
        for (int i = 0; i < OBS_RUN; i++) {
            if (i >= cnt || ((rmask >> i) & 1)) continue;  // (run-uniform)
            if (lane < Q4) store_obs(&o[i * Q4 + lane], gray4(cur.w0[i]));
            if (lane + WAVE < Q4) store_obs(&o[i * Q4 + lane + WAVE], gray4(cur.w1[i]));
        }
        while (rmask) {
            const int i = __builtin_ctzll(rmask);
            rmask &= rmask - 1;
            const int e = base + i;
            const uint32_t fle = __builtin_amdgcn_readlane(fl, i);
            const uint4 v = tv;
            const uint32_t t_rec = trec;
            if (rmask) load_tiles(base + __builtin_ctzll(rmask), tv, trec);
            RG_OBS_REDRAW_ENV();
        }
        cur = nxt;
    }
}

// ---------------------------------------------------------------------------------------------
// k_obs_resid: the run-wise fix-up pass, the predecessor of k_obs_fix (rg_obs_fix.hip, librogue_gym_obsfix.so), which rg_step_obs_gray launches in its place.
// It stays compiled: its name and register count are pinned with this unit's (tests/test_pixels_resources.py), the development library launches it where
// RG_OBS_RESID_BLOCKS is set (rg_api.cpp; tests/test_gpu_resid_grid.py), and it is the statement k_obs_fix is compared with.
// The fix-up pass behind a step launch whose helper blocks pre-streamed every env's gray image from the screen mirror as they found it
// (rg_kernels.hip enc_helper; RgState::enc_rows).  An env with a pending Redraw is drawn from the tiles exactly as k_obs_stream draws it (mirror write-back,
// history plane, flag word).  Any other env whose turn wrote mirror bytes has the image lines of its mask -- bit b: cells 32 b .. 32 b + 31, one 128-byte line
// -- re-encoded from the final mirror: whole lines, the lanes of the other lines idle.  An env with mask 0 costs its share of one coalesced load of flag
// words and masks.  Same bits as k_obs_stream.
// ---------------------------------------------------------------------------------------------
// One wave owns a run of OBS_RESID_RUN consecutive envs, persistent and one run ahead with the flag words and masks (lane i: env i of the run).  The mirror
// words of the run's masked lines are requested together once those are known, then stored; then the run's Redraw envs, one at a time.
// OBS_RESID_WAVES caps the grid (rgk_obs_resid_blocks).  54 VGPRs and 104 SGPRs: seven waves per SIMD as the compiler reports it, 7 168 resident one-wave
// blocks on the chip.  The cap comes from the grid sweep of profiles/r11_experiments.txt, 65 536 envs, one MI355X only: the pass is flat between 6 144 and
// 16 384 waves (11.1 - 11.7 us) and a latency chain below (about 1 us more for every further run a wave walks); 10 240 waves -- 1.6 runs per wave, 1.4
// residency rounds -- gave the best `value`, +0.7 % against a wave per run (16 384).
#ifndef OBS_RESID_RUN
#define OBS_RESID_RUN 4
#endif
#ifndef OBS_RESID_WAVES
#define OBS_RESID_WAVES 10240
#endif
__global__ void __launch_bounds__(WAVE) k_obs_resid(RgState S, RgConfig c, float *__restrict__ out) {
    __shared__ float lutf[128];                              // glyph -> gray value
    __shared__ uint8_t mtile[RG_MAX_ENEMY_KINDS + 6];        // monster type -> glyph
    __shared__ __align__(16) uint8_t scr[512];               // the staged screen of a Redraw env (HW = 512: rgk_obs_tail_capable)
    __shared__ ObsTabs tb;                                   // its observation record
    const int lane = threadIdx.x, W = c.width, HW = W * c.height, Q4 = HW >> 2, Q8 = HW >> 3, n = S.n;
    const int nrooms = c.room_num_x * c.room_num_y, rec_words = RG_OBS_REC_WORDS(nrooms);
    const int nruns = (n + OBS_RESID_RUN - 1) / OBS_RESID_RUN;
    // a run's flag words and line masks; a lane past the run or the batch holds zeros: nothing to serve
    auto load_run = [&](int r, uint32_t &fl, uint32_t &rows) {
        const int base = r * OBS_RESID_RUN;
        const bool in = r < nruns && lane < OBS_RESID_RUN && base + lane < n;
        fl = in ? S.flags[base + lane] : 0u;
        rows = in ? (uint32_t)S.enc_rows[base + lane] : 0u;
    };
    uint32_t fl_cur, rw_cur;
    load_run(blockIdx.x, fl_cur, rw_cur);
    // the table the step launch's helpers encoded with (RgState::gray_lut: the host's, the same single division as k_obs_stream's)
    lutf[lane] = S.gray_lut[lane];
    lutf[lane + WAVE] = S.gray_lut[lane + WAVE];
    for (int g = lane; g < RG_MAX_ENEMY_KINDS + 6; g += WAVE) mtile[g] = c.mon[g].tile;
    lds_barrier();
    auto gray4 = [&](uint32_t w) {
        w &= 0x7f7f7f7fu;
        float4 v; v.x = lutf[w & 0xff]; v.y = lutf[(w >> 8) & 0xff]; v.z = lutf[(w >> 16) & 0xff]; v.w = lutf[w >> 24];
        return v;
    };
    auto load_tiles = [&](int e, uint4 &v, uint32_t &rec) {
        v = lane < Q8 ? reinterpret_cast<const uint4 *>(S.cell + (size_t)e * HW)[lane] : make_uint4(0, 0, 0, 0);
        rec = lane < rec_words ? S.obs_rec[(size_t)e * rec_words + lane] : 0u;
    };
    const int band = lane >> 3;  // mirror word `lane` lies in image line lane >> 3, word lane + 64 in line 8 + (lane >> 3)
    for (int r = blockIdx.x; r < nruns; r += gridDim.x) {
        const int base = r * OBS_RESID_RUN;
        const uint32_t fl = fl_cur, rows = rw_cur;
        load_run(r + gridDim.x, fl_cur, rw_cur);
        uint64_t rmask = __ballot(fl & RG_FLAG_REDRAW);
        const uint64_t smask = __ballot(!(fl & RG_FLAG_REDRAW) && rows != 0u);
        if (!(rmask | smask)) continue;
        uint4 tv = make_uint4(0, 0, 0, 0);
        uint32_t trec = 0;
        if (rmask) load_tiles(base + __builtin_ctzll(rmask), tv, trec);  // in flight while the masked lines are served
        const uint32_t *m = reinterpret_cast<const uint32_t *>(S.screen) + (size_t)base * Q4;
        float4 *o = reinterpret_cast<float4 *>(out) + (size_t)base * Q4;
        uint32_t w0[OBS_RESID_RUN], w1[OBS_RESID_RUN];
#pragma unroll
        for (int i = 0; i < OBS_RESID_RUN; i++) {  // (run-uniform branches; the line's eight lanes inside)
            w0[i] = w1[i] = 0u;
            if ((smask >> i) & 1) {
                const uint32_t ri = __builtin_amdgcn_readlane(rows, i);
                if ((ri >> band) & 1u) w0[i] = m[i * Q4 + lane];
                if ((ri >> (8 + band)) & 1u) w1[i] = m[i * Q4 + lane + WAVE];
            }
        }
#pragma unroll
        for (int i = 0; i < OBS_RESID_RUN; i++) {
            if (!((smask >> i) & 1)) continue;
            const uint32_t ri = __builtin_amdgcn_readlane(rows, i);
            if ((ri >> band) & 1u) store_obs(&o[i * Q4 + lane], gray4(w0[i]));
            if ((ri >> (8 + band)) & 1u) store_obs(&o[i * Q4 + lane + WAVE], gray4(w1[i]));
        }
        while (rmask) {  // (k_obs_stream's Redraw service)
            const int i = __builtin_ctzll(rmask);
            rmask &= rmask - 1;
            const int e = base + i;
            const uint32_t fle = __builtin_amdgcn_readlane(fl, i);
            const uint4 v = tv;
            const uint32_t t_rec = trec;
            if (rmask) load_tiles(base + __builtin_ctzll(rmask), tv, trec);
            RG_OBS_REDRAW_ENV();
        }
    }
}

// one 4-byte word of the compact record per thread (hw % 4 == 0: every record section is word-aligned).  Record = {screen u8[hw], status i32[10],
// reward f32, flags u32 (the public bits: terminal, dead, message flags, error bits -- not the mirror bookkeeping), hist u8[hw] if with_hist}:
// everything ThreadConductor::step hands back per env in one reply (state AND terminal flag, python/src/thread_impls.rs:61-81; parallel.py:59-64
// derives reward and done from exactly that), so the one collective of the sharded path carries the learner's whole step
#define RG_PUBLIC_FLAGS (RG_FLAG_TERMINAL | RG_FLAG_DEAD | RG_FLAG_MSG_MASK | RG_FLAG_ERR_MASK)
__global__ void __launch_bounds__(256) k_pack(const uint8_t *__restrict__ screen, const uint8_t *__restrict__ hist, const int32_t *__restrict__ status,
                                              const float *__restrict__ reward, const uint32_t *__restrict__ flags, int n, int hw, int with_hist, uint32_t *__restrict__ out) {
    const int qs = hw >> 2, qr = qs + 12 + (with_hist ? qs : 0);
    const size_t total = (size_t)n * qr;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(g / qr), i = (int)(g - (size_t)e * qr);
        uint32_t v;
        if (i < qs) v = reinterpret_cast<const uint32_t *>(screen + (size_t)e * hw)[i];
        else if (i < qs + 10) v = (uint32_t)status[(size_t)e * 10 + (i - qs)];
        else if (i == qs + 10) v = __float_as_uint(reward[e]);
        else if (i == qs + 11) v = flags[e] & RG_PUBLIC_FLAGS;
        else v = reinterpret_cast<const uint32_t *>(hist + (size_t)e * hw)[i - qs - 12];
        out[g] = v;
    }
}

// rg_step_fetch: everything ParallelGameState::step hands back, written by ONE launch to wherever the caller wants it -- pinned host memory (the kernel's
// stores cross PCIe themselves: no copy engine, no staging) or a device snapshot for the screens.  4-byte words, grid-stride: [screen][hist][status][flags],
// and the error word (read and cleared: what rg_sync does with a 4-byte copy and a memset).
__global__ void __launch_bounds__(256) k_export(const uint32_t *__restrict__ screen, const uint32_t *__restrict__ hist, const uint32_t *__restrict__ status,
                                                const uint32_t *__restrict__ flags, uint32_t *__restrict__ err_any, size_t w_scr, size_t w_status, size_t w_flags,
                                                uint32_t *__restrict__ o_screen, uint32_t *__restrict__ o_hist, uint32_t *__restrict__ o_status,
                                                uint32_t *__restrict__ o_flags, uint32_t *__restrict__ o_err) {
    const size_t total = (o_screen ? 2 * w_scr : 0) + w_status + w_flags;
    const size_t base = o_screen ? 2 * w_scr : 0;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        if (g < base) { if (g < w_scr) o_screen[g] = screen[g]; else o_hist[g - w_scr] = hist[g - w_scr]; }
        else if (g < base + w_status) o_status[g - base] = status[g - base];
        else o_flags[g - base - w_status] = flags[g - base - w_status];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // (an exchange: the background producers OR their error bits into this word while this kernel runs, and a bit raised between a read and a clear
        // would never be reported)
        const uint32_t e = atomicExch(err_any, 0u);
        *o_err = e;
    }
}
__global__ void __launch_bounds__(256) k_scatter_rows(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int32_t *__restrict__ ext, int n, int row_bytes) {
    if ((row_bytes & 3) == 0) {
        const int rw = row_bytes >> 2;
        const size_t total = (size_t)n * rw;
        for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
            const int e = (int)(g / rw), i = (int)(g - (size_t)e * rw);
            reinterpret_cast<uint32_t *>(dst)[(size_t)ext[e] * rw + i] = reinterpret_cast<const uint32_t *>(src)[g];
        }
    } else {
        const size_t total = (size_t)n * row_bytes;
        for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
            const int e = (int)(g / row_bytes), i = (int)(g - (size_t)e * row_bytes);
            dst[(size_t)ext[e] * row_bytes + i] = src[g];
        }
    }
}
__global__ void __launch_bounds__(256) k_gather_keys(const uint8_t *__restrict__ keys, const int32_t *__restrict__ ext, uint8_t *__restrict__ dst, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = keys[ext[e]];
}

__global__ void k_probe_clock(unsigned long long *out, int spin) {
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    uint32_t x = threadIdx.x + 1u;
    for (int i = 0; i < spin; i++) x = x * 1664525u + 1013904223u;  // dependent VALU chain: 2 instructions per iteration
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; out[2] = x; out[3] = (unsigned long long)spin; }
}

// scalar fallbacks for H*W not divisible by 4 (never the case for the benchmark sizes)
__global__ void __launch_bounds__(256) k_encode_scalar(const uint8_t *__restrict__ screen, const uint8_t *__restrict__ hist, const int32_t *__restrict__ status,
                                                       uint32_t *__restrict__ flags, uint32_t *__restrict__ err_any, int n, int hw, size_t rs, size_t rst, int symbols,
                                                       int planes_sym, uint32_t sflag, int with_hist, int kind, float *__restrict__ out, const int32_t *__restrict__ ext) {
    const size_t total = (size_t)n * hw;
    const int base = kind ? planes_sym : 1;
    const int nplanes = base + __popc(sflag) + (with_hist ? 1 : 0);
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        int e = (int)(g / hw), i = (int)(g - (size_t)e * hw);
        uint32_t sym = tile_to_sym(screen[(size_t)e * rs + i]);
        float *o = out + (size_t)(ext ? ext[e] : e) * nplanes * hw + i;
        if (!kind) o[0] = (float)(uint8_t)sym / (float)(uint8_t)symbols;
        else {
            if (sym >= (uint32_t)symbols - 1) { if (flags) atomicOr(&flags[e], RG_FLAG_ERR_TILE); atomicOr(err_any, RG_FLAG_ERR_TILE); }
            for (int ch = 0; ch < planes_sym; ch++) o[(size_t)ch * hw] = (sym == (uint32_t)ch && ch < symbols - 1) ? 1.f : 0.f;
        }
        int p = base;
        for (int b = 0; b < 9; b++)
            if (sflag & (1u << b)) { o[(size_t)p * hw] = (float)status[(size_t)e * rst + kStatusIdx[b]]; p++; }
        if (with_hist) o[(size_t)p * hw] = hist[(size_t)e * rs + i] ? 1.f : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// k_redraw: RunTime::draw_screen of the envs with a pending Redraw into the screen / history mirrors, and nothing else -- the staged path of k_obs without
// its encode, for the typed pass below (which then streams every env from its mirror).  Same mirrors, history rule and flag words as k_obs leaves.
// ---------------------------------------------------------------------------------------------
// A block owns REDRAW_RUN consecutive envs per iteration: one coalesced load of their flag words (the next run's is requested before this run is drawn), a
// ballot, and the few envs with the flag set (2 % of a random policy's step: k_step keeps the mirror itself on an ordinary turn) are drawn one at a time by the
// whole block.  k_render walks one env per block iteration and serves every caller and grid; this pass costs a flag sweep where nothing is pending.
#define REDRAW_RUN 8
__global__ void __launch_bounds__(OBS_THREADS) k_redraw(RgState S, RgConfig c) {
    extern __shared__ __align__(16) uint8_t scr[];      // the staged screen [HW]
    __shared__ uint8_t mtile[RG_MAX_ENEMY_KINDS + 6];    // monster type -> glyph
    __shared__ ObsTabs tb;                               // the env's observation record
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), B = blockDim.x, W = c.width, HW = W * c.height, n = S.n;
    const int nrooms = c.room_num_x * c.room_num_y, rec_words = RG_OBS_REC_WORDS(nrooms);
    for (int g = tid; g < RG_MAX_ENEMY_KINDS + 6; g += B) mtile[g] = c.mon[g].tile;
    const int nruns = (n + REDRAW_RUN - 1) / REDRAW_RUN;
    auto load_flags = [&](int r) -> uint32_t {  // lane i of every wave: env i of the run
        const int e = r * REDRAW_RUN + lane;
        return lane < REDRAW_RUN && e < n ? S.flags[e] : 0u;
    };
    uint32_t fl = load_flags(blockIdx.x);
    for (int r = blockIdx.x; r < nruns; r += gridDim.x) {
        const uint32_t fl_nxt = load_flags(r + gridDim.x);
        uint64_t rmask = __ballot(fl & RG_FLAG_REDRAW);  // (the same in every wave of the block)
        while (rmask) {
            const int i = __builtin_ctzll(rmask);
            rmask &= rmask - 1;
            const int e = r * REDRAW_RUN + i;
            const uint32_t fle = __builtin_amdgcn_readlane(fl, i);
            // the history plane is rewritten only when the visited set changed since it was last written (k_step: HIST_DIRTY), never on a stale Redraw
            const bool upd_hist = !(fle & RG_FLAG_HIST_STALE) && (fle & RG_FLAG_HIST_DIRTY);
            lds_barrier();  // the previous env's LDS reads done (and, the first time, the glyph table written)
            for (int j = tid; j < rec_words; j += B) tb.w[j] = S.obs_rec[(size_t)e * rec_words + j];
            const uint4 *cell4 = reinterpret_cast<const uint4 *>(S.cell + (size_t)e * HW);
            uint2 *hist8 = reinterpret_cast<uint2 *>(S.hist + (size_t)e * HW);
            for (int j = tid; j < (HW >> 3); j += B) {
                uint32_t g[2], hb[2];
                draw_cells8(cell4[j], j, W, HW, g, hb);
                reinterpret_cast<uint2 *>(scr)[j] = make_uint2(g[0], g[1]);
                if (upd_hist) hist8[j] = make_uint2(hb[0], hb[1]);
            }
            lds_barrier();
            // entity overlays; draw priority monster < gold < player (core/src/lib.rs:271-283), as in k_obs
            const uint32_t ppos = tb.w[nrooms];
            const int px = POS_X(ppos), py = POS_Y(ppos);
            for (int rm = tid; rm < nrooms; rm += B) {
                const uint32_t mw = tb.w[rm];
                if ((mw >> 24) & MF_ALIVE) {
                    const int x = POS_X(mw), y = POS_Y(mw);
                    const uint32_t under = scr[y * W + x];
                    if (monster_shown(c, &tb, nrooms, px, py, x, y) && (under & 0x80u) && under != (0x80u | '*')) scr[y * W + x] = (uint8_t)(0x80u | mtile[(mw >> 16) & 0xff]);
                }
            }
            lds_barrier();
            if (tid == 0 && (scr[py * W + px] & 0x80u)) scr[py * W + px] = (uint8_t)(0x80u | '@');
            lds_barrier();
            uint2 *m8 = reinterpret_cast<uint2 *>(S.screen + (size_t)e * HW);
            for (int j = tid; j < (HW >> 3); j += B) {
                const uint2 g = reinterpret_cast<const uint2 *>(scr)[j];
                m8[j] = make_uint2(g.x & 0x7f7f7f7fu, g.y & 0x7f7f7f7fu);
            }
            if (tid == 0)  // (k_obs: a stale Redraw leaves the history mirror one level behind; k_step refreshes it before the next descent)
                S.flags[e] = (fle & ~(RG_FLAG_REDRAW | RG_FLAG_HIST_STALE | RG_FLAG_HIST_LAG | ((fle & RG_FLAG_HIST_STALE) ? 0u : RG_FLAG_HIST_DIRTY))) |
                             ((fle & RG_FLAG_HIST_STALE) ? RG_FLAG_HIST_LAG : 0u);
        }
        fl = fl_nxt;
    }
}

// ---------------------------------------------------------------------------------------------
// k_obs_typed: the whole-screen images in 16-bit elements, and the screen as a plane of symbol ids (rg_obs_typed).  KIND 0 gray / 1 one-hot with
// DT = RG_OBS_F16 / RG_OBS_BF16: every element is the f32 element of k_obs rounded to T (round to nearest even).  KIND 2 with RG_OBS_U8: Symbol::from_tile
// of every glyph (+ the 0 / 1 history plane).  The mirrors are current (k_redraw, or k_render, ran first on the stream): this pass only reads them.
// ---------------------------------------------------------------------------------------------
// A lane's ITEM is one 16-byte piece of every plane of one env: 8 consecutive cells of a 16-bit type (one uint2 of mirror in), 16 cells of u8 (one uint4 in);
// an env is Q = H*W / cells items.  A block of `B` threads owns a RUN of `run` consecutive envs per iteration -- their mirrors are one contiguous stretch of the
// screen array, so item j of the run is simply mirror piece j -- with up to OBS_T_ITEMS items per thread (host: run * Q <= OBS_T_ITEMS * B): four envs per wave
// on the 32x16 grid, four envs per 256-thread block on 80x24.  Lanes are contiguous in j, so every wave-level store covers whole lines of a plane.  Persistent
// blocks, one run ahead: the next run's mirror pieces are requested before this run's stores issue (k_obs_stream's scheme).  Status planes need the env to be
// block-uniform: the host gives such a launch run = 1, and the nine values are then scalar loads, converted once per item.
// No value is converted per cell: gray goes through a 128-entry LDS table of already rounded 16-bit values (one f32 division and one rounding per glyph and
// block), one-hot and history planes select between the two constants 1.0 / 0 of the type, packed two per register.
// (The kernel takes the few arrays it reads, not RgState / RgConfig by value, and draws nothing: with the Redraw path of k_obs fused in, every instance
// spilled 36 to 60 SGPRs.)
#define OBS_T_ITEMS 4
__device__ __forceinline__ void store_obs16(u4v *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    u4v v = {a, b, c, d};
    __builtin_nontemporal_store(v, p);
}
// bytes of `w` that are not zero -> 1
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) { return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; }

template <int KIND, int DT>
__global__ void __launch_bounds__(OBS_THREADS) k_obs_typed(const uint8_t *__restrict__ screen, const uint8_t *__restrict__ hist, const int32_t *__restrict__ status,
                                                          uint32_t *__restrict__ flags, uint32_t *__restrict__ err_any, int n, int hw, int symbols, int planes,
                                                          uint32_t sflag, int with_hist, int run, u4v *__restrict__ out) {
    constexpr int CW = DT == RG_OBS_U8 ? 4 : 2;  // mirror words per item
    typedef uint32_t wv __attribute__((ext_vector_type(CW)));
    constexpr uint32_t ONE = DT == RG_OBS_F16 ? 0x3C00u : 0x3F80u;  // 1.0
    __shared__ uint16_t lut16[128];  // glyph -> gray value, rounded (KIND 0)
    __shared__ uint8_t luts[128];    // glyph -> symbol id
    const int tid = threadIdx.x, B = blockDim.x, Q = hw / (4 * CW);
    for (int g = tid; g < 128; g += B) {
        const uint32_t sy = tile_to_sym((uint32_t)g);
        luts[g] = (uint8_t)sy;
        if (KIND == 0) lut16[g] = (uint16_t)cvt16<DT>((float)(uint8_t)sy / (float)(uint8_t)symbols);  // python/src/lib.rs:84 (the same single f32 division), then rounded
    }
    const int nplanes = planes + __popc(sflag) + (with_hist ? 1 : 0);
    const uint32_t smax = (uint32_t)symbols - 1;  // construct_symbol_map fills channels 0..symbols-2 (symbol.rs:51-71)
    // item k of this thread: piece j = tid + k B of the run = piece ql[k] of the run's env el[k] (the same in every run: divided once)
    const int per_run = run * Q;
    int el[OBS_T_ITEMS], ql[OBS_T_ITEMS];
#pragma unroll
    for (int k = 0; k < OBS_T_ITEMS; k++) {
        const int j = tid + k * B;
        el[k] = j < per_run ? j / Q : -1;
        ql[k] = el[k] < 0 ? 0 : j - el[k] * Q;
    }
    struct Run { wv w[OBS_T_ITEMS], h[OBS_T_ITEMS]; };
    auto load_run = [&](int r, Run &R) {  // zeros past the run and past the batch
        const int base = r * run;
        const wv *m = reinterpret_cast<const wv *>(screen + (size_t)base * hw), *hm = reinterpret_cast<const wv *>(hist + (size_t)base * hw);
#pragma unroll
        for (int k = 0; k < OBS_T_ITEMS; k++) {
            const bool ok = el[k] >= 0 && base + el[k] < n;
            R.w[k] = ok ? m[tid + k * B] : (wv)0u;
            R.h[k] = ok && with_hist ? hm[tid + k * B] : (wv)0u;
        }
    };
    auto gray2 = [&](uint32_t w, int hi) -> uint32_t {  // cells 2 hi, 2 hi + 1 of a mirror word
        return (uint32_t)lut16[(w >> (16 * hi)) & 0x7f] | ((uint32_t)lut16[(w >> (16 * hi + 8)) & 0x7f] << 16);
    };
    auto one2 = [&](bool a, bool b) -> uint32_t { return (a ? ONE : 0u) | (b ? ONE << 16 : 0u); };
    lds_barrier();  // the tables are ready
    const int nruns = (n + run - 1) / run;
    Run cur;
    load_run(blockIdx.x, cur);
    for (int r = blockIdx.x; r < nruns; r += gridDim.x) {
        Run nxt;
        load_run(r + gridDim.x, nxt);
        const int base = r * run;
#pragma unroll
        for (int k = 0; k < OBS_T_ITEMS; k++) {
            const int e = base + el[k];
            if (el[k] < 0 || e >= n) continue;
            u4v *o = out + (size_t)e * nplanes * Q + ql[k];
            uint32_t w[CW], h[CW];
#pragma unroll
            for (int t = 0; t < CW; t++) { w[t] = cur.w[k][t]; h[t] = cur.h[k][t]; }
            bool bad = false;  // a glyph without a symbol (InvalidTileError, e.g. 'Z')
            if (KIND == 0) {
                store_obs16(o, gray2(w[0], 0), gray2(w[0], 1), gray2(w[1], 0), gray2(w[1], 1));
            } else if (KIND == 1) {
                uint32_t s[8];
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    s[t] = luts[(w[t >> 2] >> ((t & 3) * 8)) & 0x7f];
                    bad = bad || s[t] >= smax;
                }
                for (uint32_t ch = 0; ch < smax; ch++)
                    store_obs16(o + (size_t)ch * Q, one2(s[0] == ch, s[1] == ch), one2(s[2] == ch, s[3] == ch), one2(s[4] == ch, s[5] == ch), one2(s[6] == ch, s[7] == ch));
                for (uint32_t ch = smax; ch < (uint32_t)planes; ch++) store_obs16(o + (size_t)ch * Q, 0u, 0u, 0u, 0u);  // the last channel is never set
            } else {
                uint32_t id[CW];
#pragma unroll
                for (int t = 0; t < CW; t++) {
                    const uint32_t a = luts[w[t] & 0x7f], b = luts[(w[t] >> 8) & 0x7f], c = luts[(w[t] >> 16) & 0x7f], d = luts[(w[t] >> 24) & 0x7f];
                    bad = bad || a >= smax || b >= smax || c >= smax || d >= smax;
                    id[t] = a | (b << 8) | (c << 16) | (d << 24);
                }
                store_obs16(o, id[0], id[1], id[CW - 2], id[CW - 1]);  // (CW = 4 here: the u8 type is the only one of this kind)
            }
            int p = planes;
            if (KIND != 2 && sflag) {
                const int eu = __builtin_amdgcn_readfirstlane(e);  // (run = 1 with status planes: the block's one env)
                for (int b = 0; b < 9; b++)
                    if (sflag & (1u << b)) {
                        const uint32_t v = cvt16<DT>((float)status[(size_t)eu * 10 + kStatusIdx[b]]) * 0x10001u;
                        store_obs16(o + (size_t)p * Q, v, v, v, v);
                        p++;
                    }
            }
            if (with_hist) {
                if (KIND == 2) store_obs16(o + (size_t)p * Q, nonzero_bytes(h[0]), nonzero_bytes(h[1]), nonzero_bytes(h[CW - 2]), nonzero_bytes(h[CW - 1]));
                else
                    store_obs16(o + (size_t)p * Q, one2(h[0] & 0xffu, h[0] & 0xff00u), one2(h[0] & 0xff0000u, h[0] >> 24), one2(h[1] & 0xffu, h[1] & 0xff00u),
                                one2(h[1] & 0xff0000u, h[1] >> 24));
            }
            // (atomic, as k_obs<1>: the lanes of an env share its flag word)
            if (KIND != 0 && bad) { atomicOr(&flags[e], RG_FLAG_ERR_TILE); atomicOr(err_any, RG_FLAG_ERR_TILE); }
        }
        cur = nxt;
    }
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launchers: defined here against the prototypes the host units call them by
// ---------------------------------------------------------------------------------------------
extern "C" {
void rgk_render(const RgState *S, const RgConfig *c, hipStream_t st) {
    int blocks = S->n < 8192 ? S->n : 8192;
    hipLaunchKernelGGL(k_render, dim3(blocks), dim3(RENDER_THREADS), 0, st, *S, *c);
}
// fused mirror refresh + encode; returns 0 if the geometry is not supported (caller falls back to k_render + encode)
int rgk_obs(const RgState *S, const RgConfig *c, uint32_t sflag, int with_hist, int kind, float *out, uint32_t *err_any, int planes_sym, int bound, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    int hw = c->width * c->height;
    if (hw & 7) return 0;
    if (c->room_num_x * c->room_num_y > RG_OBS_MAX_ROOMS || !S->obs_rec) return 0;  // the fused kernel's LDS overlay tables hold 64 rooms (one thread per room + the player): unfused path
    int q8 = hw / 8;
    int tpe = q8 >= OBS_THREADS ? OBS_THREADS : ((q8 + 63) / 64) * 64;  // threads per env: a whole number of waves
    if (tpe > OBS_THREADS) tpe = OBS_THREADS;
    if (RG_OBS_REC_WORDS(c->room_num_x * c->room_num_y) > tpe) return 0;  // the env's observation record is fetched one word per thread (a <= 512-cell grid with more than 28 rooms: unfused path)
    const int bthreads = tpe, epb = 1;  // one env per block: no cross-env barrier coupling (4 envs per 256-thread block measured 10-20 % slower; two envs per one-wave
                                        // block on the 32x16 grid -- half a wave and four words per thread each, which k_obs supports -- 30.0 against 28.9 us: round 6)
    const bool groups = S->ext != nullptr;
    size_t smem = 512 + 128 + 64 + (size_t)epb * OBS_ENV_BYTES(hw);
    int blocks = (S->n + epb - 1) / epb;
    // persistent grid: launching one tiny workgroup per env is dispatch-rate bound (65 536 one-wave blocks: 71 us; 16 384 looping blocks: 51 us)
    {
        int cap = bthreads <= 64 ? 16384 : 8192;
#ifdef RG_DEV_KNOBS
        if (const char *ev = getenv("RG_OBS_BLOCKS")) cap = atoi(ev);
#endif
        if (blocks > cap) blocks = cap;
    }
    const int hi_prio = !(c->width <= 32 && c->room_num_x * c->room_num_y <= 32);  // (rg_kernels.hip rgk_step: those configs step with k_step_w32)
    // gray, no status / history planes, no config groups, not bound, one wave per env (<= 512 cells): the run-streaming kernel
    bool stream = !kind && !groups && !bound && sflag == 0 && !with_hist && tpe == WAVE;
#ifdef RG_DEV_KNOBS
    if (const char *ev = getenv("RG_OBS_STREAM")) stream = stream && atoi(ev) != 0;  // (RG_OBS_STREAM=0: k_obs<0, false> -- tests/test_gpu_obs_stream.py)
#endif
    if (stream) {
        int sblocks = (S->n + OBS_RUN - 1) / OBS_RUN, cap = OBS_STREAM_WAVES;  // persistent waves, each looping over runs
#ifdef RG_DEV_KNOBS
        if (const char *ev = getenv("RG_OBS_BLOCKS")) if (atoi(ev) > 0) cap = atoi(ev);
#endif
        if (sblocks > cap) sblocks = cap;
        rg_launch(k_obs_stream, dim3(sblocks), dim3(WAVE), 0, st, ev0, ev1, *S, *c, out, hi_prio);
        return 1;
    }
    auto launch = [&](auto kernel) { rg_launch(kernel, dim3(blocks), dim3(bthreads), smem, st, ev0, ev1, *S, *c, sflag, with_hist, out, err_any, tpe, epb, planes_sym, hi_prio); };
    if (bound && !groups && !kind) launch(k_obs<0, false, true>);       // (rg_obs_bind: the in-place pass over the last k_step's list)
    else if (bound && !groups) launch(k_obs<1, false, true>);
    else if (!kind && !groups) launch(k_obs<0, false>);
    else if (!kind) launch(k_obs<0, true>);
    else if (!groups) launch(k_obs<1, false>);
    else launch(k_obs<1, true>);
    return 1;
}
// whether rgk_obs serves this handle's plain gray image (no status planes, no history plane, not bound) with k_obs_stream -- of the conditions under which
// rg_step_obs_gray arms the pre-streamed encode, the ones that are this file's -- on a grid of exactly 512 cells (two mirror words per lane)
int rgk_obs_tail_capable(const RgState *S, const RgConfig *c) {
    const int hw = c->width * c->height, nr = c->room_num_x * c->room_num_y;
    if (hw != 512 || nr > RG_OBS_MAX_ROOMS || !S->obs_rec || !S->ovl || S->ext) return 0;
    if (RG_OBS_REC_WORDS(nr) > WAVE) return 0;
#ifdef RG_DEV_KNOBS
    if (const char *ev = getenv("RG_OBS_STREAM")) if (atoi(ev) == 0) return 0;
#endif
    return 1;
}
// the fix-up pass behind a step launch that pre-streamed the images (S->enc_rows is that launch's): its Redraw envs and the image lines its turns touched
// its grid: one-wave blocks, never more than there are runs, at most OBS_RESID_WAVES of them (each then loops over runs gridDim.x apart, one run ahead
// with the flag words).  Development builds: RG_OBS_RESID_BLOCKS > 0 takes the cap's place, read at every launch (the grid sweep, and the tests that let
// one wave walk every run).
int rgk_obs_resid_blocks(int n) {
    const int nruns = (n + OBS_RESID_RUN - 1) / OBS_RESID_RUN;
    int cap = OBS_RESID_WAVES;
#ifdef RG_DEV_KNOBS
    if (const char *ev = getenv("RG_OBS_RESID_BLOCKS")) if (atoi(ev) > 0) cap = atoi(ev);
#endif
    const int blocks = nruns < cap ? nruns : cap;
    return blocks < 1 ? 1 : blocks;
}
void rgk_obs_resid(const RgState *S, const RgConfig *c, float *out, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    rg_launch(k_obs_resid, dim3(rgk_obs_resid_blocks(S->n)), dim3(WAVE), 0, st, ev0, ev1, *S, *c, out);
}
void rgk_encode(const uint8_t *screen, const uint8_t *hist, const int32_t *status, uint32_t *flags, uint32_t *err_any, int n, int hw, size_t rs, size_t rst,
                int symbols, int planes_sym, uint32_t sflag, int with_hist, int kind, float *out, const int32_t *ext, hipStream_t st) {
    if ((hw & 3) == 0 && (rs & 3) == 0) {
        size_t total = (size_t)n * (hw >> 2);
        int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
        if (blocks < 1) blocks = 1;
        if (!kind) hipLaunchKernelGGL(k_gray, dim3(blocks), dim3(256), 0, st, screen, hist, status, n, hw, rs, rst, symbols, sflag, with_hist, out, ext);
        else hipLaunchKernelGGL(k_symbol, dim3(blocks), dim3(256), 0, st, screen, hist, status, flags, err_any, n, hw, rs, rst, symbols, planes_sym, sflag, with_hist, out, ext);
    } else {
        size_t total = (size_t)n * hw;
        int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
        hipLaunchKernelGGL(k_encode_scalar, dim3(blocks), dim3(256), 0, st, screen, hist, status, flags, err_any, n, hw, rs, rst, symbols, planes_sym, sflag, with_hist, kind, out, ext);
    }
}
void rgk_export(const RgState *S, uint32_t *err_any, void *o_screen, void *o_hist, void *o_status, void *o_flags, uint32_t *o_err, hipStream_t st) {
    const size_t n = (size_t)S->n, w_scr = n * (size_t)S->hw / 4, w_status = n * 10, w_flags = n;
    const size_t total = (o_screen ? 2 * w_scr : 0) + w_status + w_flags;
    int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_export, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(S->screen), reinterpret_cast<const uint32_t *>(S->hist),
                       reinterpret_cast<const uint32_t *>(S->status), S->flags, err_any, w_scr, w_status, w_flags, static_cast<uint32_t *>(o_screen), static_cast<uint32_t *>(o_hist),
                       static_cast<uint32_t *>(o_status), static_cast<uint32_t *>(o_flags), o_err);
}
// compact record of every env: {screen u8[hw], status i32[10], reward f32, flags u32, hist u8[hw] (optional)}, back to back -- the payload of the ONE
// all-gather per step of the multi-GPU path; expanded on the consumer by rgk_encode with rs = record size
void rgk_pack(const RgState *S, int with_hist, uint8_t *out, hipStream_t st) {
    const int hw = S->hw;
    const size_t rec = (size_t)hw + RG_COMPACT_FIXED_BYTES + (with_hist ? hw : 0);
    const size_t total = (size_t)S->n * (rec / 4);
    int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_pack, dim3(blocks), dim3(256), 0, st, S->screen, S->hist, S->status, S->reward, S->flags, S->n, hw, with_hist, reinterpret_cast<uint32_t *>(out));
}
// handle with several config groups: rows of a group's array -> the handle's array at the group's env indices (row_words 4-byte words per env)
void rgk_scatter_rows(const void *src, void *dst, const int32_t *ext, int n, int row_bytes, hipStream_t st) {
    const size_t total = (size_t)n * row_bytes;
    int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_scatter_rows, dim3(blocks), dim3(256), 0, st, (const uint8_t *)src, (uint8_t *)dst, ext, n, row_bytes);
}
void rgk_gather_keys(const uint8_t *keys, const int32_t *ext, uint8_t *dst, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_gather_keys, dim3((n + 255) / 256), dim3(256), 0, st, keys, ext, dst, n);
}
// the Redraw sweep in front of the typed pass (k_redraw): returns 0 where it does not apply (more rooms than the LDS overlay tables hold: the caller runs k_render)
int rgk_redraw(const RgState *S, const RgConfig *c, hipStream_t st) {
    const int hw = c->width * c->height;
    if ((hw & 7) || c->room_num_x * c->room_num_y > RG_OBS_MAX_ROOMS || !S->obs_rec) return 0;
    int B = ((hw / 8 + WAVE - 1) / WAVE) * WAVE;
    if (B > OBS_THREADS) B = OBS_THREADS;
    const int nruns = (S->n + REDRAW_RUN - 1) / REDRAW_RUN;
    hipLaunchKernelGGL(k_redraw, dim3(nruns < 8192 ? nruns : 8192), dim3(B), (size_t)hw, st, *S, *c);
    return 1;
}
// the typed whole-screen pass (rg_obs_typed; kind / dtype combination and arguments checked by the caller, mirrors drawn).  Returns 0 if the grid is not
// a whole number of 16-byte pieces per plane (there is no fallback kernel).
int rgk_obs_typed(const RgState *S, const RgConfig *c, int kind, int dtype, uint32_t sflag, int with_hist, int planes_sym, void *out, uint32_t *err_any,
                  hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    const int hw = c->width * c->height, cells = dtype == RG_OBS_U8 ? 16 : 8;
    if (hw % cells) return 0;
    const int Q = hw / cells;
    int B = ((Q + WAVE - 1) / WAVE) * WAVE;  // threads per block: an env's items, in whole waves
    if (B > OBS_THREADS) B = OBS_THREADS;
    if (Q > OBS_T_ITEMS * B) return 0;  // (cannot happen: RG_MAX_W x RG_MAX_H is 960 items)
    // envs per block and iteration: as many as its threads hold items for; one (block-uniform) where status planes are written
    int run = sflag ? 1 : OBS_T_ITEMS * B / Q;
    if (run < 1) run = 1;
    const int nruns = (S->n + run - 1) / run, cap = B <= WAVE ? OBS_STREAM_WAVES : 4096;  // persistent grid
    const int blocks = nruns < cap ? nruns : cap;
    const int planes = kind == 1 ? planes_sym : 1;
    auto launch = [&](auto kernel) {
        rg_launch(kernel, dim3(blocks), dim3(B), 0, st, ev0, ev1, S->screen, S->hist, S->status, S->flags, err_any, S->n, hw, (int)c->symbols, planes, sflag, with_hist, run,
                  static_cast<u4v *>(out));
    };
    if (kind == 2) launch(k_obs_typed<2, RG_OBS_U8>);
    else if (kind == 0 && dtype == RG_OBS_F16) launch(k_obs_typed<0, RG_OBS_F16>);
    else if (kind == 0) launch(k_obs_typed<0, RG_OBS_BF16>);
    else if (dtype == RG_OBS_F16) launch(k_obs_typed<1, RG_OBS_F16>);
    else launch(k_obs_typed<1, RG_OBS_BF16>);
    return 1;
}
// shader-clock probe: one wave spins for `spin` iterations and reports {s_memtime ticks (shader clock), s_memrealtime ticks (constant 100 MHz)}
void rgk_probe_clock(unsigned long long *out, int spin, hipStream_t st) { hipLaunchKernelGGL(k_probe_clock, dim3(1), dim3(64), 0, st, out, spin); }
}
