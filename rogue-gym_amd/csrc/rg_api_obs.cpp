// rg_api_obs.cpp -- the typed observations, the player-centred crops, the tileset and the pixel passes behind the C-ABI (the f32 observation: rg_api.cpp obs_common).
#include <cstring>

#include "rg_handle.h"
#include "rg_launch.h"
#include "rg_pixels.h"

extern "C" {
// Typed observations (f16 / bf16 images, u8 symbol ids).  typed_check: every refusal, before anything is launched (or stepped); kind_dtype_check: those the typed crops share.
int rg_obs_dtype_bytes(int dtype) { return dtype == RG_OBS_F32 ? 4 : (dtype == RG_OBS_F16 || dtype == RG_OBS_BF16) ? 2 : dtype == RG_OBS_U8 ? 1 : -1; }
static int kind_dtype_check(rg_t *h, const std::string &w, int kind, int dtype, uint32_t status_flag) {
    if (kind < 0 || kind > 2) { h->err = w + "kind must be 0 (gray), 1 (symbol) or 2 (symbol ids), got " + std::to_string(kind); return 1; }
    if (rg_obs_dtype_bytes(dtype) < 0) { h->err = w + "dtype must be RG_OBS_F32 (0), RG_OBS_F16 (1), RG_OBS_BF16 (2) or RG_OBS_U8 (3), got " + std::to_string(dtype); return 1; }
    if (kind == 2 && dtype != RG_OBS_U8) { h->err = w + "kind 2 (symbol ids) takes dtype RG_OBS_U8 only, got dtype " + std::to_string(dtype); return 1; }
    if (kind != 2 && dtype == RG_OBS_U8) { h->err = w + "dtype RG_OBS_U8 is for kind 2 (symbol ids) only, got kind " + std::to_string(kind); return 1; }
    if (kind == 2 && (status_flag & 0x1ffu)) { h->err = w + "status_flag must be 0 for kind 2 (status values do not fit a byte; read the status mirror)"; return 1; }
    return 0;
}
static int typed_check(rg_t *h, const char *what, int kind, int dtype, uint32_t status_flag, const void *out_dev) {
    const std::string w = std::string(what) + ": ";
    if (kind_dtype_check(h, w, kind, dtype, status_flag)) return 1;
    if (!out_dev || ((uintptr_t)out_dev & 15)) { h->err = w + "out_dev must be a non-null, 16-byte aligned device pointer"; return 1; }
    if (dtype == RG_OBS_F32) return 0;  // (the f32 call: its own rules)
    if (!h->sub.empty() || h->mixed) { h->err = w + "not for a handle with config groups or mixed sizes"; return 1; }
    const int cells = dtype == RG_OBS_U8 ? 16 : 8;
    if (h->S.hw % cells) {
        h->err = w + "H*W must be a multiple of " + std::to_string(cells) + " for this dtype (a lane writes whole 16-byte pieces of a plane), got " + std::to_string(h->cfg.height) +
                 " x " + std::to_string(h->cfg.width);
        return 1;
    }
    return 0;
}
static int obs_typed_checked(rg_t *h, int kind, int dtype, uint32_t status_flag, int with_hist, void *out_dev) {
    if (dtype == RG_OBS_F32) return obs_common(h, status_flag, with_hist, kind, static_cast<float *>(out_dev));
    HIPCHK(h, hipSetDevice(h->device));
    // pending Redraws: drawn first by the Redraw sweep (k_redraw: the staged path of the f32 pass without its encode), by k_render where that does not apply
    if (h->render_pending) {
        bool swept;
        { TimedLaunch t(h, 1); swept = rgk_redraw(&h->S, &h->cfg, h->stream) != 0; if (!swept) t.cancel(); }
        if (swept) {
            HIPCHK(h, hipGetLastError());
            h->render_pending = false;
            h->bound_valid = false;  // (Redraw flags were consumed without the bound observation tensor being written: its next call encodes every env)
        } else if (flush_render(h)) return 1;
    }
    {
        TimedLaunch t(h, 2, true);
        if (!rgk_obs_typed(&h->S, &h->cfg, kind, dtype, status_flag & 0x1ffu, with_hist ? 1 : 0, h->planes_sym, out_dev, h->d_err, h->stream, t.start_ev(), t.stop_ev())) {
            t.cancel();
            h->err = "rg_obs_typed: grid not supported";
            return 1;
        }
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}
int rg_obs_typed(rg_t *h, int kind, int dtype, uint32_t status_flag, int with_hist, void *out_dev) {
    return typed_check(h, "rg_obs_typed", kind, dtype, status_flag, out_dev) ? 1 : obs_typed_checked(h, kind, dtype, status_flag, with_hist, out_dev);
}
int rg_step_obs_typed(rg_t *h, const uint8_t *keys, int keys_on_device, int kind, int dtype, uint32_t status_flag, int with_hist, void *out_dev) {
    if (typed_check(h, "rg_step_obs_typed", kind, dtype, status_flag, out_dev)) return 1;
    return rg_step_prefix(h, keys, h->S.n, keys_on_device) ? 1 : obs_typed_checked(h, kind, dtype, status_flag, with_hist, out_dev);
}
// The window passes: player-centred crops (rg_crop_typed.hip) and pixels (rg_pixels.hip).  window_check: the refusals they share, `w` being the entry
// point's name and a colon; crop = false: the whole screen, no radii.
static int window_check(rg_t *h, const std::string &w, bool crop, int radius_y, int radius_x, const void *out_dev) {
    if (crop && (radius_y < 0 || radius_y > RG_MAX_H - 1 || radius_x < 0 || radius_x > RG_MAX_W - 1)) {
        h->err = w + "radius_y, radius_x must satisfy 0 <= radius_y <= " + std::to_string(RG_MAX_H - 1) + " and 0 <= radius_x <= " + std::to_string(RG_MAX_W - 1) + ", got (" +
                 std::to_string(radius_y) + ", " + std::to_string(radius_x) + ")";
        return 1;
    }
    if (!out_dev || ((uintptr_t)out_dev & 15)) { h->err = w + "out_dev must be a non-null, 16-byte aligned device pointer"; return 1; }
    return 0;
}
// window_launch(leaf): leaf enqueues one kernel on a handle without groups and returns 0, or sets that handle's error and returns 1; on a handle with config
// groups every group writes its envs straight into the handle's tensor (RgState::ext): the window has one size for every env, so a mixed-size batch is served too.
// The mirrors are made current first (pending Redraws drawn by k_render: a bound observation tensor is then re-encoded in full by its next call).
extern "C++" template <class Leaf> static int window_launch(rg_t *h, Leaf leaf) {
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->sub.empty()) {
        for (rg_handle *sh : h->sub) SUBCHK(h, sh, window_launch(sh, leaf));
        return 0;
    }
    if (flush_render(h) || leaf(h)) return 1;
    HIPCHK(h, hipGetLastError());
    return 0;
}
// The crops.  crop_check: every refusal, before anything is launched (or stepped).
static int crop_check(rg_t *h, const char *what, int kind, int dtype, int radius_y, int radius_x, uint32_t status_flag, const void *out_dev) {
    const std::string w = std::string(what) + ": ";
    if (kind_dtype_check(h, w, kind, dtype, status_flag)) return 1;
    if (window_check(h, w, true, radius_y, radius_x, out_dev)) return 1;
    if (kind == 1)  // (kind 2 has no channel count: each env is judged by its own group's symbols)
        for (rg_handle *sh : h->sub)
            if (symbols_check(h, w, sh)) return 1;
    return 0;
}
static int crop_checked(rg_t *h, const char *what, int kind, int dtype, int radius_y, int radius_x, uint32_t status_flag, int with_hist, void *out_dev, int32_t *centers_dev) {
    const int planes_sym = h->planes_sym;  // (the handle's one-hot depth, for every group)
    return window_launch(h, [=](rg_t *l) {
        if (rgk_crop_typed(&l->S, &l->cfg, kind, dtype, radius_y, radius_x, status_flag & 0x1ffu, with_hist ? 1 : 0, planes_sym, out_dev, centers_dev, l->d_err, l->stream, nullptr,
                           nullptr))
            return 0;
        l->err = std::string(what) + ": window too large";
        return 1;
    });
}
int rg_obs_crop(rg_t *h, int kind, int radius_y, int radius_x, uint32_t status_flag, int with_hist, float *out_dev, int32_t *centers_dev) {
    if (kind != 0 && kind != 1) { h->err = "rg_obs_crop: kind must be 0 (gray) or 1 (symbol), got " + std::to_string(kind); return 1; }
    if (crop_check(h, "rg_obs_crop", kind, RG_OBS_F32, radius_y, radius_x, status_flag, out_dev)) return 1;
    return crop_checked(h, "rg_obs_crop", kind, RG_OBS_F32, radius_y, radius_x, status_flag, with_hist, out_dev, centers_dev);
}
int rg_obs_crop_typed(rg_t *h, int kind, int dtype, int radius_y, int radius_x, uint32_t status_flag, int with_hist, void *out_dev, int32_t *centers_dev) {
    if (crop_check(h, "rg_obs_crop_typed", kind, dtype, radius_y, radius_x, status_flag, out_dev)) return 1;
    return crop_checked(h, "rg_obs_crop_typed", kind, dtype, radius_y, radius_x, status_flag, with_hist, out_dev, centers_dev);
}
int rg_step_obs_crop_typed(rg_t *h, const uint8_t *keys, int keys_on_device, int kind, int dtype, int radius_y, int radius_x, uint32_t status_flag, int with_hist,
                           void *out_dev, int32_t *centers_dev) {
    if (crop_check(h, "rg_step_obs_crop_typed", kind, dtype, radius_y, radius_x, status_flag, out_dev)) return 1;
    if (rg_step_prefix(h, keys, h->S.n, keys_on_device)) return 1;
    return crop_checked(h, "rg_step_obs_crop_typed", kind, dtype, radius_y, radius_x, status_flag, with_hist, out_dev, centers_dev);
}
// Pixels (rg_pixels.hip; the rule: rg_pixels.h).  pixels_check: every refusal, before anything is launched (or stepped); radius_y < 0 = the whole screen.
int rg_tileset_default(int *th, uint8_t *font, uint8_t *palette) { rg_px_default(th, font, palette); return 0; }
int rg_tileset_set(rg_t *h, int th, const uint8_t *font_host, const uint8_t *palette_host) {
    std::vector<uint8_t> blob(RG_PX_FONT_BYTES + RG_PX_TAB_BYTES, 0), dfont(RG_PX_FONT_BYTES), dpal(257 * 3);
    int dth;
    rg_px_default(&dth, dfont.data(), dpal.data());
    if (!font_host) { font_host = dfont.data(); th = dth; }
    if (!palette_host) palette_host = dpal.data();
    if (th < RG_TILE_MIN_H || th > RG_TILE_MAX_H) {
        h->err = "rg_tileset_set: th must satisfy " + std::to_string(RG_TILE_MIN_H) + " <= th <= " + std::to_string(RG_TILE_MAX_H) + ", got " + std::to_string(th);
        return 1;
    }
    memcpy(blob.data(), font_host, 256 * (size_t)th);
    rg_px_tables(palette_host, blob.data() + RG_PX_FONT_BYTES);
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->tiles && !dev_alloc(h, &h->tiles, blob.size())) return 1;
    // a pass in flight may still read the old tables (the groups' passes on their own streams too): wait, then copy before returning
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (rg_handle *sh : h->sub) HIPCHK(h, hipStreamSynchronize(sh->stream));
    HIPCHK(h, hipMemcpy(h->tiles, blob.data(), blob.size(), hipMemcpyHostToDevice));
    h->tile_th = th;
    return 0;
}
static int pixels_check(rg_t *h, const char *what, bool crop, int channels, int radius_y, int radius_x, const void *out_dev) {
    const std::string w = std::string(what) + ": ";
    if (channels != 1 && channels != 3) { h->err = w + "channels must be 1 (gray) or 3 (RGB), got " + std::to_string(channels); return 1; }
    if (window_check(h, w, crop, radius_y, radius_x, out_dev)) return 1;
    if (!crop && (!h->sub.empty() || h->mixed)) { h->err = w + "not for a handle with config groups or mixed sizes (rg_obs_pixels_crop serves them)"; return 1; }
    return 0;
}
static int pixels_checked(rg_t *h, int channels, int radius_y, int radius_x, uint8_t *out_dev, int32_t *centers_dev) {
    if (!h->tiles && rg_tileset_set(h, 0, nullptr, nullptr)) return 1;  // (no rg_tileset_set so far: the built-in)
    const uint8_t *tiles = h->tiles;  // (the handle's tileset, for every group)
    const int th = h->tile_th;
    return window_launch(h, [=](rg_t *l) {
        TimedLaunch t(l, 2, true);
        if (rgk_pixels(&l->S, &l->cfg, tiles, th, channels, radius_y, radius_x, out_dev, centers_dev, l->stream, t.start_ev(), t.stop_ev())) return 0;
        t.cancel();
        l->err = "rg_obs_pixels: image too large";
        return 1;
    });
}
int rg_obs_pixels(rg_t *h, int channels, uint8_t *out_dev) {
    return pixels_check(h, "rg_obs_pixels", false, channels, -1, 0, out_dev) ? 1 : pixels_checked(h, channels, -1, 0, out_dev, nullptr);
}
int rg_obs_pixels_crop(rg_t *h, int channels, int radius_y, int radius_x, uint8_t *out_dev, int32_t *centers_dev) {
    return pixels_check(h, "rg_obs_pixels_crop", true, channels, radius_y, radius_x, out_dev) ? 1 : pixels_checked(h, channels, radius_y, radius_x, out_dev, centers_dev);
}
int rg_step_obs_pixels(rg_t *h, const uint8_t *keys, int keys_on_device, int channels, uint8_t *out_dev) {
    if (pixels_check(h, "rg_step_obs_pixels", false, channels, -1, 0, out_dev)) return 1;
    return rg_step_prefix(h, keys, h->S.n, keys_on_device) ? 1 : pixels_checked(h, channels, -1, 0, out_dev, nullptr);
}
int rg_step_obs_pixels_crop(rg_t *h, const uint8_t *keys, int keys_on_device, int channels, int radius_y, int radius_x, uint8_t *out_dev, int32_t *centers_dev) {
    if (pixels_check(h, "rg_step_obs_pixels_crop", true, channels, radius_y, radius_x, out_dev)) return 1;
    return rg_step_prefix(h, keys, h->S.n, keys_on_device) ? 1 : pixels_checked(h, channels, radius_y, radius_x, out_dev, centers_dev);
}
int rg_pixels_host(int th, const uint8_t *font, const uint8_t *palette, int channels, int H, int W, const uint8_t *screen, int cy, int cx, int radius_y, int radius_x,
                   uint8_t *out) {
    return rg_px_host(g_create_err, th, font, palette, channels, H, W, screen, cy, cx, radius_y, radius_x, out);
}
}  // extern "C"
