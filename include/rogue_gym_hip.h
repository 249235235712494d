/*
 * rogue_gym_hip.h -- C ABI of the MI355X-native batched Rogue-Gym stepper (librogue_gym_hip.so).
 *
 * This is the drop-in boundary: the entry points are what the reference's FFI crate
 * (`rogue_gym_python._rogue_gym`, /root/reference/python/src/lib.rs) would bind in place of
 * its per-env `GameStateImpl` + one-OS-thread-per-env `ThreadConductor`.  Plain pointers and
 * sizes only -- no torch / PyO3 types.  All buffers named "dev" live in HBM on the handle's
 * device; observations are written into caller-owned device buffers (e.g. torch tensors) and
 * never leave HBM.
 *
 * Conventions: every function returns 0 on success, non-zero on failure; the message is
 * available from rg_last_error() (the Python shim raises
 * RuntimeError("Error in rogue-gym: " + msg), mirroring python/src/lib.rs:20-26).
 * A handle is not thread-safe; distinct handles are independent.  Calls are asynchronous on the
 * handle's HIP stream unless stated otherwise.
 *
 * file:line citations are relative to /root/reference.
 */
#ifndef ROGUE_GYM_HIP_H
#define ROGUE_GYM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rg_handle rg_t;

/* bits of the per-env flag word returned by rg_flags()/rg_fetch_states() */
#define RG_FLAG_TERMINAL   0x00000001u  /* PlayerState.is_terminal (state_impls.rs:77) */
#define RG_FLAG_DEAD       0x00000002u  /* engine is in the Grave modal (core/src/lib.rs:301-315) */
#define RG_FLAG_REDRAW     0x00000004u  /* internal: screen mirror refresh pending */
#define RG_FLAG_HIST_STALE 0x00000008u  /* internal: this Redraw keeps the old level's history */
#define RG_FLAG_HIST_LAG   0x00000010u  /* internal: the history mirror still shows the level before the current one */
#define RG_FLAG_HIST_DIRTY 0x00000020u  /* internal: the visited set changed since the history mirror was last written */
#define RG_FLAG_SCR_CHANGED 0x00000040u /* internal: the turn itself changed bytes of the screen mirror since the bound observation tensor was last written (rg_obs_bind) */
#define RG_FLAG_MSG_SHIFT  8            /* bits 8..14: MessageFlagInner (python/src/flags.rs:6-39) */
#define RG_FLAG_MSG_MASK   0x00007f00u
#define RG_FLAG_ERR_KEY    0x00010000u  /* ErrorKind::InvalidInput: key not in KeyMap::ai (input.rs:73-100) */
#define RG_FLAG_ERR_DEAD   0x00020000u  /* ErrorKind::IgnoredInput: action key while dead */
#define RG_FLAG_ERR_TILE   0x00040000u  /* symbol image: glyph with symbol >= symbols-1 (python/src/lib.rs:96-102) */
#define RG_FLAG_ERR_INTERNAL 0x00080000u /* a capacity guard of the stepper tripped (each is proven unreachable; see rg_kernels.hip) */
#define RG_FLAG_ERR_STATE  0x00100000u  /* a loaded record did not fit this env (magic / version / fingerprint / geometry): the env is unchanged (rg_state_load) */
#define RG_FLAG_ERR_MASK   0x00ff0000u

/* Replaces GameState::__new__ / ParallelGameState::new (python/src/lib.rs:217-225,270-294) and
 * ThreadConductor::new (thread_impls.rs:14-34): parses one GameConfig JSON per env
 * (core/src/lib.rs:42-86).  Envs may differ in anything: envs with equal configs (seeds aside) form a group that is
 * stepped as one homogeneous batch, and the handle presents all groups in the caller's env order.  When the groups differ in width / height
 * there is no [n_env][H][W] tensor: rg_screen / rg_hist / rg_obs_* / rg_pack_compact / rg_expand_compact / rg_obs_host then fail with a message
 * that says so, and rg_fetch_states delivers the screens in a ragged layout (rg_env_dims); everything else works unchanged.  Allocates the SoA
 * state for n_env environments on HIP device `device`, generates every level-1 dungeon and
 * draws the first screens.  auto_reset != 0 selects ThreadConductor::step semantics (terminal
 * envs are rebuilt inside rg_step and report the post-reset state with is_terminal forced
 * true, thread_impls.rs:69-79); 0 selects single GameState semantics.
 * cfg_json[i] may be NULL (= GameConfig::default()). */
int rg_create(const char *const *cfg_json, int n_env, uint64_t max_steps, int device, int auto_reset, rg_t **out);
void rg_destroy(rg_t *h);
/* error text of the last failed call on `h` (h == NULL: last failed rg_create on this thread) */
const char *rg_last_error(const rg_t *h);

/* Build id: the first 16 hex digits of the sha256 over the library's sources (the csrc files and this header), so that a test can tell whether the library
 * that is loaded was built from the sources that are checked out. */
const char *rg_build_id(void);

/* GameState::screen_size / symbols (python/src/lib.rs:226-228,255-257,295-300) */
int rg_dims(const rg_t *h, int *height, int *width, int *symbols, int *n_env);
/* Height and width of every env's own config (host arrays of n_env i32; either may be NULL).  Equal for all envs unless the batch mixes sizes. */
int rg_env_dims(const rg_t *h, int32_t *heights, int32_t *widths);
/* `symbols` of every env's own config (GameStateImpl::new computes it per env, state_impls.rs:21-25; PlayerState.symbols): out_host = i32 [n_env].
 * rg_dims reports env 0's, like ParallelGameState::symbols (python/src/lib.rs:281-285,298-300). */
int rg_env_symbols(const rg_t *h, int32_t *out_host);
/* Run all later work of this handle on `hip_stream` (a hipStream_t; NULL = default stream). */
int rg_set_stream(rg_t *h, void *hip_stream);

/* GameState::set_seed / ParallelGameState::seed (python/src/lib.rs:229-232,301-307;
 * thread_impls.rs:45-50,125-128): u128 seeds as (lo, hi) words, used at the next reset. n may be
 * smaller than n_env (zip semantics). Host pointers. */
int rg_seed(rg_t *h, const uint64_t *seed_lo, const uint64_t *seed_hi, int n);
/* GameState::reset / ParallelGameState::reset: rebuild every env from its config (+ seed). */
int rg_reset(rg_t *h);
/* Reset the envs the caller picks (Isaac Gym's reset_idx, EnvPool's reset(env_ids), Gymnasium's reset_mask).  Each chosen env is rebuilt exactly as rg_reset
 * rebuilds it: GameConfig::build from its seed (a `seed: None` env draws a fresh build ticket), level 1, steps 0, reward 0, done 0, flags REDRAW | HIST_DIRTY,
 * an empty dist cache, its next-level structure dropped, its key log rolled (the cut-off episode becomes the "previous" one).  Every other env keeps every
 * byte of its state.  The spares are not consulted and stay valid: a fixed-seed env's spare was built from the same seed, a reseeding env's ticket is its own.
 * rg_reset_envs: k env ids, host (range-checked, duplicates refused, nothing launched on a refusal) or device i32 (ids_on_device != 0: the caller's
 *   responsibility; an id out of range is skipped and raises RG_FLAG_ERR_INTERNAL at the next rg_sync).  env_ids NULL = every env (k is ignored).
 * rg_reset_mask: mask_dev = u8 [n_env] on the device, non-zero = rebuild.  The mask is compacted into a list on the device: no host round trip.
 * Both are asynchronous on the handle's stream; an empty list / all-zero mask is a valid no-op.  Mirrors are redrawn at the next read, and a bound
 * observation tensor (rg_obs_bind) encodes every env at its next call.  Not for handles with config groups.
 * rg_seed_envs: rg_seed for chosen envs (host pointers; seed_hi may be NULL): the seeds are used at those envs' next reset of any kind, rg_dump_config
 *   reports them, and exactly those envs' spares are dropped and regenerated. */
int rg_reset_envs(rg_t *h, const int32_t *env_ids, int k, int ids_on_device);
int rg_reset_mask(rg_t *h, const uint8_t *mask_dev);
int rg_seed_envs(rg_t *h, const int32_t *env_ids, const uint64_t *seed_lo, const uint64_t *seed_hi, int k);
/* GameState::react / ParallelGameState::step (python/src/lib.rs:241-243,315-321 ->
 * state_impls.rs:51-79, thread_impls.rs:61-81): one key byte per env.  `keys` is a device pointer
 * when keys_on_device != 0, else a host pointer (copied H2D on the stream). */
int rg_step(rg_t *h, const uint8_t *keys, int keys_on_device);
/* ThreadConductor::step zips the key vector with the envs (thread_impls.rs:62-64): with n_keys < n_env only the first n_keys envs receive a
 * key; surplus keys are dropped.  (The reference then blocks forever on the reply of the envs that got no instruction; here they simply keep
 * their state, reward 0.)  rg_step == rg_step_prefix with n_keys = n_env. */
int rg_step_prefix(rg_t *h, const uint8_t *keys, int n_keys, int keys_on_device);
/* rg_step followed by rg_obs_gray(status_flag, with_hist, out_dev) as ONE call -- what a learner's loop does every step (GameState::react then
 * PlayerState::gray_image, python/src/lib.rs:72-87,251-256): one trip through the binding instead of two.  (A step kernel whose waves also drew and
 * encoded their own envs was built and measured in round 5: 196 us against 52 + 44 us for the two launches -- profiles/r05_experiments.txt.) */
int rg_step_obs_gray(rg_t *h, const uint8_t *keys, int keys_on_device, uint32_t status_flag, int with_hist, float *out_dev);
/* A BOUND observation tensor (opt-in): `out_dev` becomes the handle's standing observation batch for exactly this image setting (kind 0 gray / 1 symbol,
 * no status planes, no history plane) -- what the reference's learner rebuilds from the PlayerState values after every step (parallel.py:44-66 ->
 * ImageSetting.expand -> PlayerState::gray_image / symbol_image, python/src/lib.rs:72-205).  While bound, every rg_step_obs_gray / rg_obs_gray / rg_obs_symbol
 * call with the same arguments keeps the tensor CURRENT IN PLACE: it rewrites the images of the envs whose screen changed since the last such call (a Redraw
 * drawn from the tiles, or bytes the turn wrote into the screen mirror itself) and leaves the others -- whose f32 image is already what a full encode would
 * write -- untouched; the contents after the call are bit-identical to the unbound call's.  The caller must not write to the tensor.  The first call after
 * binding, and the first after anything else drew the mirrors (rg_fetch_states, an observation call with other arguments, rg_screen ...), encodes every env.
 * out_dev = NULL unbinds.  Not for handles with config groups.  (65 536 mini envs: 57 % of the envs of a step of the random policy change nothing on screen.) */
int rg_obs_bind(rg_t *h, int kind, uint32_t status_flag, int with_hist, float *out_dev);
/* Wait for the stream; returns non-zero (and sets the error text) if any env raised an error flag
 * since the last call (invalid key / action while dead), like the PyRuntimeError of lib.rs:20-26. */
int rg_sync(rg_t *h);

/* Device-resident mirrors (PlayerState, python/src/lib.rs:29-38), valid until rg_destroy:
 *   screen  u8  [n_env][H][W]   glyph bytes, refreshed only on Reaction::Redraw
 *   hist    u8  [n_env][H][W]   0/1 visited-history plane (copy_hist, lib.rs:105-111)
 *   status  i32 [n_env][10]     Status::to_vec order (player.rs:418-430), refreshed on StatusUpdated
 *   flags   u32 [n_env]         RG_FLAG_* bits
 *   reward  f32 [n_env]         max(0, gold_after - gold_before) of the last rg_step (parallel.py:60-63)
 *   done    u8  [n_env]         is_terminal of the state returned by the last rg_step (parallel.py:64)
 * Reading them (rg_screen/rg_hist/rg_obs_*) flushes the pending screen render first. */
int rg_screen(rg_t *h, uint8_t **dev);
int rg_hist(rg_t *h, uint8_t **dev);
int rg_status(rg_t *h, int32_t **dev);
int rg_flags(rg_t *h, uint32_t **dev);
int rg_reward(rg_t *h, float **dev);
int rg_done(rg_t *h, uint8_t **dev);

/* StairRewardParallel (python/rogue_gym/envs/wrappers.py:45-64) fused into the step kernel: from the next rg_step on, `bonus` is added to
 * reward[e] whenever the dungeon level env e reports after the key is above the level it reported one step earlier (the comparison level
 * follows the reported one, so it is back at 1 after an auto-reset: a descent that ends the episode pays nothing, exactly as the wrapper).
 * The bonus is part of the reward mirror and of the compact record (rg_pack_compact / rg_allgather_compact).  0 (the default) = off.
 * A call that puts an env on another level without a key -- rg_reset, rg_reset_envs / rg_reset_mask, rg_state_load, rg_archive_restore, rg_debug_descend --
 * pays nothing and moves the comparison level with it: the first rg_step behind it compares with the level the env reported after that call, so a
 * level-3 record loaded over a level-1 game earns no bonus, and its next descent earns one. */
int rg_set_stair_reward(rg_t *h, float bonus);

/* rg_step_obs_gray on the plain f32 gray image of a 512-cell grid stepped by the capped W <= 32 kernel (no status planes, no history plane, no config
 * groups, no bound tensor) streams every env's image from the screen mirror in helper blocks of the step launch, beside the turns, and a fix-up pass
 * behind it re-encodes the image lines the turns touched and draws the Redraw envs (the pre-streamed encode).  on = 0: the step
 * kernel and the full observation pass one after the other, as on every other handle -- the same bits either way (A/B
 * runs, twin-handle tests).  Default: on.  The Python binding calls it with 0 for a handle created while ROGUE_GYM_HIP_NO_TAIL_ENCODE=1 is set. */
int rg_tail_encode(rg_t *h, int on);

/* PlayerState::gray_image[_with_hist] / symbol_image[_with_hist] for the whole batch
 * (python/src/lib.rs:72-111,162-205; flags.rs:88-115; symbol.rs:17-71), written straight into
 * out_dev = f32 [n_env][C][H][W] with C = 1 (gray) or `symbols` (one-hot) + popcount(status_flag)
 * (+1 with hist).  Bit layout of status_flag: StatusFlagInner (flags.rs:45-55). */
int rg_obs_gray(rg_t *h, uint32_t status_flag, int with_hist, float *out_dev);
int rg_obs_symbol(rg_t *h, uint32_t status_flag, int with_hist, float *out_dev);
int rg_obs_channels(const rg_t *h, int symbol, uint32_t status_flag, int with_hist);

/* Player-centred crop of the same image: out_dev = f32 [n_env][C][2*radius_y+1][2*radius_x+1] (16-byte aligned), C and plane order those of
 * rg_obs_channels(h, kind, status_flag, with_hist), kind 0 = gray, 1 = one-hot symbol.  With P the image rg_obs_gray / rg_obs_symbol would write
 * for env e now, padded on every side with the encoding of a blank cell ' ' (gray 0; one-hot: channel 0 = 1, as for every ' ' on the screen;
 * history 0; status planes their constant value):  out[e][c][j][i] = P_padded[c][cy - radius_y + j][cx - radius_x + i], (cx, cy) the player's
 * cell in screen coordinates -- bit-identical to slicing the padded full image.  The window has one size for every env, so this call also serves
 * handles with config groups and mixed-size batches (the rg_obs_* calls refuse those); a config group with more symbols than env 0's is refused
 * as by rg_obs_symbol.  Pending Redraws are drawn first (history stale / lag rules unchanged); a bound observation tensor (rg_obs_bind) is left
 * as it is and its next call encodes every env.  centers_dev (nullable) = i32 [n_env][2]: (cy, cx) of each window's centre.
 * InvalidTileError (a glyph without a symbol, e.g. 'Z', in the one-hot kind): raised, as by rg_obs_symbol, at the next rg_sync -- but only for
 * such a glyph INSIDE the window; cells outside it are not read.  0 <= radius_y <= RG_MAX_H - 1 (47) and 0 <= radius_x <= RG_MAX_W - 1 (159):
 * a window that size holds the whole screen from any player cell.  Other radii, another kind or a null out_dev: non-zero, with a message. */
int rg_obs_crop(rg_t *h, int kind, int radius_y, int radius_x, uint32_t status_flag, int with_hist, float *out_dev, int32_t *centers_dev);

/* TYPED observations: the same whole-screen images in the element type a learner consumes, and the screen as a plane of symbol ids.
 *   kind 0 = gray, 1 = one-hot symbol, dtype RG_OBS_F16 / RG_OBS_BF16: out_dev = T [n_env][C][H][W], C and plane order those of rg_obs_channels.
 *     Every element is the element rg_obs_gray / rg_obs_symbol would write for the same state, rounded to T by round-to-nearest-even (overflow to
 *     infinity in F16: a status plane such as gold can exceed 65 504) -- bit-identical to f32_image.to(T).  The gray value keeps its single f32 division
 *     (python/src/lib.rs:84) and is rounded afterwards.  dtype RG_OBS_F32 with kinds 0 / 1 is accepted and is exactly the rg_obs_gray / rg_obs_symbol call.
 *   kind 2 = symbol ids, dtype RG_OBS_U8 only: out_dev = u8 [n_env][1 + with_hist][H][W].  Plane 0 is Symbol::from_tile of each screen glyph
 *     (core/src/symbol.rs:17-40; 255 for a glyph without a symbol): wherever the one-hot image is valid it equals onehot.argmax(1), and ' ' is 0 --
 *     what an embedding layer indexes with.  The history plane, if asked for, is 0 / 1.  InvalidTileError as rg_obs_symbol: an id >= symbols - 1 sets
 *     RG_FLAG_ERR_TILE on the env and is reported by the next rg_sync; the byte written is still the id.  status_flag must be 0 (status values do not
 *     fit a byte; the `status` mirror is a device tensor already).
 * Side effects are those of the f32 call: pending Redraws are drawn at this call (screen and history mirrors, history stale / lag rules unchanged),
 * so a handle that only makes typed calls has the same mirrors and flag words, step for step, as one that only makes f32 calls.  A bound
 * observation tensor (rg_obs_bind) is left as it is and its next call encodes every env.  The pass is timing kernel 2 (rg_timing_*), like the f32 pass.
 * Refused, non-zero with a message naming the argument: out_dev null or not 16-byte aligned; an unknown kind or dtype; kind 2 with another dtype,
 * RG_OBS_U8 with kinds 0 / 1; status planes with kind 2; H*W not a multiple of 8 (16 for RG_OBS_U8: a lane writes whole 16-byte pieces of a plane,
 * and there are NO fallback kernels for other grids); handles with config groups or mixed sizes (as rg_obs_bind).  A refused call launches nothing.
 * rg_step_obs_typed = rg_step + rg_obs_typed in one trip through the binding (what rg_step_obs_gray is for f32); a refused call does not step.
 * rg_obs_dtype_bytes: the element size, 4 / 2 / 2 / 1, or -1 for anything else; stateless, needs no device.
 * The typed crop is rg_obs_crop_typed below.  Not typed (f32 only): the bound tensor (rg_obs_bind), rg_expand_compact, rg_obs_host, rg_encode_host[_batch]. */
#define RG_OBS_F32  0
#define RG_OBS_F16  1   /* IEEE binary16 */
#define RG_OBS_BF16 2
#define RG_OBS_U8   3   /* kind 2 only */
int rg_obs_dtype_bytes(int dtype);
int rg_obs_typed(rg_t *h, int kind, int dtype, uint32_t status_flag, int with_hist, void *out_dev);
int rg_step_obs_typed(rg_t *h, const uint8_t *keys, int keys_on_device, int kind, int dtype, uint32_t status_flag, int with_hist, void *out_dev);

/* TYPED player-centred crop: the window of rg_obs_crop in the element types of rg_obs_typed, and NLE's `chars_crop` -- the window as symbol ids.
 *   kind 0 / 1, dtype RG_OBS_F16 / RG_OBS_BF16: out_dev = T [n_env][C][2*radius_y+1][2*radius_x+1], every element the one rg_obs_crop would write,
 *     rounded to nearest even (F16 overflows to infinity): bit-identical to f32_crop.to(T).  dtype RG_OBS_F32 is exactly the rg_obs_crop call.
 *   kind 2, dtype RG_OBS_U8 only: out_dev = u8 [n_env][1 + with_hist][2*radius_y+1][2*radius_x+1].  Plane 0 is Symbol::from_tile of each window cell on
 *     the screen (255 for a glyph without a symbol) and 0, the id of ' ', outside it; the history plane is 0 / 1, and 0 outside the screen.  status_flag
 *     must be 0.  An 11 x 11 window is 121 bytes per env.
 * centers_dev (nullable) as rg_obs_crop.  InvalidTileError by rg_obs_crop's rule -- raised at the next rg_sync, only for a cell inside the window; kind 2:
 * an id >= symbols - 1, the byte written is still the id.  Handles with config groups and mixed-size batches are served for every kind: kind 1 refuses a
 * group with more symbols than env 0's, as rg_obs_crop does; kind 2 has no channel count and judges each env by its own group's `symbols`.  There is no
 * condition on H*W (the crop stages cells).  Side effects are those of rg_obs_crop: pending Redraws are drawn first, history stale / lag rules unchanged,
 * a bound tensor is re-encoded in full by its next call -- a handle that makes only these calls has the same mirrors and flag words, step for step, as
 * one that makes only rg_obs_crop calls.
 * Refused, non-zero with a message naming the entry point and the argument, nothing launched: an unknown kind or dtype; kind 2 with another dtype;
 * RG_OBS_U8 with kinds 0 / 1; status planes with kind 2; radii outside rg_obs_crop's range; out_dev null or not 16-byte aligned.
 * rg_step_obs_crop_typed = rg_step + rg_obs_crop_typed in one trip through the binding; a refused call does not step. */
int rg_obs_crop_typed(rg_t *h, int kind, int dtype, int radius_y, int radius_x, uint32_t status_flag, int with_hist, void *out_dev, int32_t *centers_dev);
int rg_step_obs_crop_typed(rg_t *h, const uint8_t *keys, int keys_on_device, int kind, int dtype, int radius_y, int radius_x, uint32_t status_flag, int with_hist,
                           void *out_dev, int32_t *centers_dev);

/* PIXELS: the screen, or the player-centred window, rendered through a tileset -- NLE's `pixel`, MiniHack's `pixel_crop`, Gym's rgb_array frame.
 * A tileset is two tables: a monochrome bitmap font u8 [256][th] (glyphs 8 pixels wide and th rows high, RG_TILE_MIN_H <= th <= RG_TILE_MAX_H; bit 7 of
 * a row byte is the leftmost pixel) and a palette u8 [257][3], the RGB ink of glyph byte g, entry 256 the paper.  With g the glyph of cell (y, x) and
 * ink = (font[g][py] >> (7 - px)) & 1:
 *   channels 3 (RGB):  out[e][c][y*th + py][x*8 + px] = ink ? palette[g][c] : palette[256][c]
 *   channels 1 (gray): the same with lum(r, g, b) = (77 r + 150 g + 29 b + 128) >> 8 in place of the three values (integer: host and device agree to the bit).
 * The glyph is the screen mirror byte of the cell after pending Redraws are drawn -- the byte rg_obs_typed kind 2 maps to a symbol id.  The output is u8,
 * planar.  There is no float form (a learner does .float() / 255 in its first layer), no tile wider than 8 pixels and no full-colour tile image: a
 * caller who wants another look passes another font and palette.
 *   rg_tileset_default (stateless, needs no device): the built-in tileset -- th = 8, an 8 x 8 font for 0x21 .. 0x7E with every other byte blank (font is
 *     filled as [256][8] and zero up to 256 * 16 bytes), and a palette that tells walls, doors, passages, floor, gold, stairs, the player and monsters apart
 *     on a dark paper.  Any of the three pointers may be NULL.
 *   rg_tileset_set: uploads a tileset to handle-owned device memory (allocated at the first call; the call waits for the handle's stream).  NULL font_host /
 *     palette_host mean the built-in's (th is then taken from the built-in font).  th outside 8 .. 16 is refused.  A handle with config groups shares one
 *     tileset.  Without a call, the first pixel call sets the built-in.
 *   rg_obs_pixels: out_dev = u8 [n_env][channels][H*th][W*8], the whole screen.  Refuses handles with config groups or mixed sizes, as rg_obs_typed does.
 *   rg_obs_pixels_crop: out_dev = u8 [n_env][channels][(2*radius_y+1)*th][(2*radius_x+1)*8], rg_obs_crop's window (the same radius range, the same
 *     centers_dev).  A window cell outside the screen is the glyph ' ' THROUGH the tileset (a font that gives ' ' ink shows it in the padding): the crop is
 *     bit-identical to slicing the full pixel image padded with ' ' cells.  Serves config groups and mixed sizes, as rg_obs_crop_typed does.  An 11 x 11
 *     window of 8 x 8 tiles is 88 x 88 pixels, 7 744 bytes per env in gray.
 * Side effects are those of rg_obs_crop_typed: pending Redraws are drawn first, history stale / lag rules unchanged, a bound tensor (rg_obs_bind) is left as
 * it is and encoded in full by its next call -- a handle that makes only pixel calls has the same mirrors and flag words, step for step, as one that
 * makes only rg_obs_crop calls.  The pass is timing kernel 2 (rg_timing_*), like the other observation passes.
 * Refused, non-zero with a message naming the entry point and the argument, before anything is launched or stepped: channels not 1 or 3; radii outside
 * rg_obs_crop's range; out_dev null or not 16-byte aligned.
 * rg_step_obs_pixels / rg_step_obs_pixels_crop = rg_step + the pass in one trip through the binding; a refused call does not step.
 * rg_pixels_host (stateless, needs no device): the rule on the CPU for ONE screen u8 [H][W] of arbitrary bytes, 1 <= H <= 48, 1 <= W <= 160; out as above
 *   with n_env = 1.  radius_y < 0: the whole screen (cy, cx, radius_x unused); else the window around (cy, cx), which must be a cell of the screen.  NULL
 *   font / palette: the built-in's.  A refused call writes nothing. */
#define RG_TILE_MIN_H 8
#define RG_TILE_MAX_H 16
int rg_tileset_default(int *th, uint8_t *font /*[256][16]*/, uint8_t *palette /*[257][3]*/);
int rg_tileset_set(rg_t *h, int th, const uint8_t *font_host, const uint8_t *palette_host);
int rg_obs_pixels(rg_t *h, int channels, uint8_t *out_dev);
int rg_obs_pixels_crop(rg_t *h, int channels, int radius_y, int radius_x, uint8_t *out_dev, int32_t *centers_dev);
int rg_step_obs_pixels(rg_t *h, const uint8_t *keys, int keys_on_device, int channels, uint8_t *out_dev);
int rg_step_obs_pixels_crop(rg_t *h, const uint8_t *keys, int keys_on_device, int channels, int radius_y, int radius_x, uint8_t *out_dev, int32_t *centers_dev);
int rg_pixels_host(int th, const uint8_t *font, const uint8_t *palette, int channels, int H, int W, const uint8_t *screen, int cy, int cx, int radius_y, int radius_x,
                   uint8_t *out);

/* LEGAL-ACTION MASKS: which keys would do anything for each env right now, and one key per env drawn uniformly among those, on the device.
 * The rule is the reference's own test, which neither its Python surface nor the screen mirror gives away: Dungeon::can_move_player
 * (core/src/dungeon/mod.rs:79) -> Floor::can_move_impl as the player (floor.rs:169-182), which move_player asks before anything else (actions.rs:168-231).
 *   '.' and 's': 1.
 *   h j k l y u b n (KeyMap::ai, input.rs:73-100: j is down, k is up) and the run keys H J K L Y U B N, judged by their first move: 1 iff the target cell is
 *     inside the grid, its surface can be walked on (not wall-x, wall-y or none), its attr has neither HIDDEN nor LOCKED, and -- for a diagonal -- both
 *     orthogonal neighbours (x+dx, y) and (x, y+dy) are inside the grid and walkable (surface only: their HIDDEN / LOCKED bits are not consulted, as in the
 *     reference).  A monster on the target changes nothing: the move is an attack and is legal.
 *   '>': 1 iff the surface of the player's own cell is the stairs (actions.rs:16-65).
 *   An env in the Grave modal (RG_FLAG_DEAD; handles without auto-reset only): every key 0 -- the reference answers every key, '.' included, with IgnoredInput.
 * So 0 means exactly: the reference would answer the key with CantMove, with "no downstairs" or with IgnoredInput.
 * rg_action_mask: `keys` = host list of n_keys key bytes, duplicates allowed; NULL = the 11 of RG_ACTION_KEYS (n_keys is then ignored).  mask_dev (nullable)
 *   = u8 [n_env][n_keys], 0 / 1, in the handle's env order.  sample_dev (nullable) = u8 [n_env]: for env e with `count` legal keys the key at the position of
 *   the (rg_sample_index(seed, e, draw, count) + 1)-th set entry of its row, keys[0] when count == 0 -- a key byte for rg_step.  The call is stateless: the
 *   caller varies `draw` (a step counter) between calls, and the same arguments on the same states give the same bytes.  Asynchronous on the handle's stream.
 *   It reads game state only (the player's cell, the flag word, the cell grid): the pending render is not flushed, the mirrors, every flag bit and a bound
 *   observation tensor are left alone.  Config groups and mixed-size batches are served (a row has one size for every env; each group writes its envs' rows).
 *   Refused, non-zero with a message naming the argument, nothing launched: n_keys < 1 or > RG_MASK_MAX_KEYS; a key outside KeyMap::ai (the message names
 *   the byte and its position); both outputs NULL; mask_dev not 16-byte aligned.
 * rg_sample_index (stateless, needs no device), all arithmetic mod 2^64:
 *     z = seed + 0x9E3779B97F4A7C15 * (env + 1) + 0xD1B54A32D192ED03 * draw
 *     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *     return count ? (uint32_t)(((z >> 32) * count) >> 32) : 0
 * rg_action_mask_host (stateless, needs no device): the same rule for ONE env given as a host grid `cells` = u16 [height][width] in rg_debug_fetch's layout,
 *   the player's cell (px, py) and the dead bit; out = u8 [n_keys].  Key rules and refusals as rg_action_mask; the message is read through
 *   rg_last_error(NULL). */
#define RG_ACTION_KEYS ".hjklnbuy>s"   /* RogueEnv.ACTIONS in index order */
#define RG_MASK_MAX_KEYS 32
int rg_action_mask(rg_t *h, const uint8_t *keys, int n_keys, uint8_t *mask_dev, uint8_t *sample_dev, uint64_t seed, uint64_t draw);
int rg_action_mask_host(const uint16_t *cells, int height, int width, int px, int py, int dead,
                        const uint8_t *keys, int n_keys, uint8_t *out);
uint32_t rg_sample_index(uint64_t seed, uint32_t env, uint64_t draw, uint32_t count);

/* MASKED CATEGORICAL ACTIONS FROM POLICY LOGITS: for each env one key drawn from the softmax of its row of logits over the keys that are legal now (the
 * rule of the action mask above), with the behaviour log-probability and the entropy, on the device -- what stands between a policy network and rg_step.
 * The rule, its random word and the bit fields of that word are stated once, in rogue-gym_amd/csrc/rg_policy.h; the kernel and the host twin agree bit for
 * bit on every output, floats included (integer operations, f32 add / multiply / fma and one division only; fixed polynomials for exp2 and ln).
 *   Logits: [n_env][n_keys] of dtype RG_OBS_F32 / RG_OBS_F16 / RG_OBS_BF16, row e for env e of the handle, 16-bit values widened exactly, multiplied by
 *     inv_temp.  NaN and -inf weigh 0, +inf is the largest finite value.  pi = the softmax over the LEGAL keys of the list; an illegal key has probability 0.
 *     A weight below 2^-125 of the largest is 0.  No legal key weighs: pi is uniform over the legal keys and the source is 1.
 *   mode RG_ACT_SAMPLE: one draw from pi -- t = u * S against the running sum of the weights in list order, the first legal key whose sum exceeds t.  With
 *     probability beta the env plays teacher_dev[e] instead, if that key is in the list and legal now (otherwise the policy's draw stands); with probability
 *     epsilon a uniform draw among the legal keys.  RG_ACT_GREEDY: the legal key with the largest logit, ties to the lowest index.  RG_ACT_GIVEN: no draw;
 *     given_dev[e] is the action whose log-probability is wanted (out of range or illegal: -inf).
 *   Outputs, each [n_env], every one but key_dev nullable: key u8, the byte rg_step takes; action i32, its index in the list; logp f32 = ln pi(action), ALWAYS
 *     under the pure masked softmax, also when epsilon or the teacher chose (-inf where pi gives 0); entropy f32 of pi in nats; source u8 0 policy, 1 uniform,
 *     2 teacher, 3 none.  mask_dev (nullable) = u8 [n_env][n_keys], exactly what the action-mask call writes.  An env with no legal key (the Grave modal)
 *     answers keys[0], action 0, logp 0, entropy 0, source 3.  In RG_ACT_GIVEN key_dev may be NULL too.
 *   The draw is a stateless function of (opts.seed, env index of the handle, opts.draw) with a stream constant of its own: equal seed and draw in the
 *     action-mask sample and here are unrelated.  The same arguments on the same states give the same bytes.
 *   Asynchronous on the handle's stream; reads game state only, as the action mask does; config groups and mixed sizes are served.  A handle that never calls
 *   it allocates and launches nothing for it.
 *   Refused, non-zero with a message naming the argument, nothing launched: n_keys or a key as for the action mask; an unknown dtype or mode; logits_dev NULL
 *   or not 16-byte aligned, mask_dev not 16-byte aligned; opts NULL; inv_temp not finite or not > 0; epsilon or beta outside [0, 1] or epsilon + beta > 1;
 *   beta > 0 without teacher_dev; RG_ACT_GIVEN without given_dev; key_dev NULL in a mode that draws.
 * rg_act_host (stateless, needs no device): the same rule for ONE env given as a host grid, as the action-mask host entry takes it; `logits` = n_keys
 *   elements of dtype; env = the env index of the draw; teacher_key = a key byte or -1; given = the action of RG_ACT_GIVEN.  Outputs nullable. */
#define RG_ACT_SAMPLE 0u
#define RG_ACT_GREEDY 1u
#define RG_ACT_GIVEN  2u
typedef struct rg_act_opts { float inv_temp, epsilon, beta; uint32_t mode; uint64_t seed, draw; } rg_act_opts;
int rg_act(rg_t *h, const uint8_t *keys, int n_keys, const void *logits_dev, int dtype, const rg_act_opts *opts,
           const uint8_t *teacher_dev, const int32_t *given_dev,
           uint8_t *key_dev, int32_t *action_dev, float *logp_dev, float *entropy_dev, uint8_t *source_dev, uint8_t *mask_dev);
int rg_act_host(const uint16_t *cells, int height, int width, int px, int py, int dead, const uint8_t *keys, int n_keys,
                const void *logits, int dtype, const rg_act_opts *opts, uint32_t env, int teacher_key, int given,
                uint8_t *key, int32_t *action, float *logp, float *entropy, uint8_t *source);

/* THE LEARNER'S SIDE OF THAT RULE: the log-probability of STORED actions and the entropy under STORED masks for any number of rows of logits, and the gradient
 * of both with respect to the logits -- what a PPO / A2C update evaluates for its T x N rows.  Stateless: no handle, a learner process may own no env.  The
 * rule is stated once, in rogue-gym_amd/csrc/rg_policy_grad.h; kernels (k_pg_eval, k_pg_grad in librogue_gym_learn.so) and host twins agree bit for bit.
 *   Rows: logits [n_rows][n_keys] of dtype RG_OBS_F32 / RG_OBS_F16 / RG_OBS_BF16, contiguous; mask u8 [n_rows][n_keys], a byte != 0 = the key is legal
 *     (what the action-mask call and rg_act's mask_dev write), NULL = every key; action i32 [n_rows], an index into the row, any value.
 *   rg_policy_eval: logp f32 [n_rows] and entropy f32 [n_rows], each nullable -- exactly what rg_act answers for that row in RG_ACT_GIVEN mode, so for the
 *     logits, mask and action of an rg_act call they equal its logp and entropy bit for bit (no legal key: 0 and 0; action out of range or illegal: -inf).
 *   rg_policy_grad: dlogits [n_rows][n_keys] of dtype = the gradient of sum_r g_logp[r] * logp[r] + g_entropy[r] * entropy[r]; either upstream array may be
 *     NULL and then counts as 0.  For a legal key that weighs: inv_temp * (g_logp * ([k == a] - pi_k) - g_entropy * pi_k * (logp_k + H)); +0.0 for every
 *     other key, for a row where no legal key weighs and a row with no legal key.  An action that is out of range, illegal or weightless (logp = -inf)
 *     makes the g_logp term 0 for the whole row; the entropy term still flows.  A NaN is the canonical quiet NaN; 16-bit results are the f32 result
 *     rounded to nearest even.
 *   Asynchronous on hip_stream (NULL = the null stream), on the caller's current device; nothing is read or written past row n_rows - 1; no alignment is
 *   asked for (a stretch of 64 rows that starts on a multiple of 16 bytes moves as 16-byte pieces, any other lane by lane).  n_rows == 0 is a valid no-op.
 *   Refused, non-zero with a message (rg_last_error(NULL)) naming the argument, nothing launched, outputs untouched: n_keys outside 1..32; an unknown dtype;
 *   NULL logits, actions or dlogits; inv_temp not finite or not > 0; n_rows < 0.
 * The *_host twins: the same rule over host pointers, no stream, no device. */
int rg_policy_eval(void *hip_stream, int64_t n_rows, int n_keys, const void *logits_dev, int dtype, const uint8_t *mask_dev,
                   const int32_t *action_dev, float inv_temp, float *logp_dev, float *entropy_dev);
int rg_policy_grad(void *hip_stream, int64_t n_rows, int n_keys, const void *logits_dev, int dtype, const uint8_t *mask_dev, const int32_t *action_dev, float inv_temp,
                   const float *g_logp_dev, const float *g_entropy_dev, void *dlogits_dev);
int rg_policy_eval_host(int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp,
                        float *logp, float *entropy);
int rg_policy_grad_host(int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp,
                        const float *g_logp, const float *g_entropy, void *dlogits);

/* RETURNS AND ADVANTAGES OF A ROLLOUT: GAE(lambda), discounted reward-to-go and V-trace for a whole [n_steps, n_envs] rollout in ONE launch -- what stands between
 * the stored reward / done / value rows and a PPO / A2C / IMPALA loss.  Stateless: no handle.  The rule is stated once, in rogue-gym_amd/csrc/rg_returns.h;
 * kernels (k_gae, k_vtrace in librogue_gym_returns.so) and host twins agree bit for bit.
 *   Arrays: time-major and contiguous, row t = n_envs consecutive elements, f32 except done and trunc (u8, any byte != 0 counts); last_value f32 [n_envs].
 *     Nullable: value (rg_gae only: +0.0), last_value (+0.0), done, trunc (never), trunc_value, and one of the two outputs.
 *   Each column is scanned from t = n_steps - 1 down to 0.  rg_gae, from adv_next = +0.0 and v_next = last_value[n]:
 *       end = done[t] || trunc[t];   boot = trunc[t] ? (trunc_value ? trunc_value[t] : value[t]) : (done[t] ? +0.0 : v_next)
 *       delta = fma(gamma, boot, reward[t]) - value[t];   adv[t] = fma(gamma * lam, end ? +0.0 : adv_next, delta);   ret[t] = value[t] + adv[t]
 *     value == NULL with lam = 1 is the discounted reward-to-go (in ret and adv alike), bootstrapped from last_value.  trunc marks a time-limit end, which
 *     bootstraps from the caller's trunc_value[t] (the value of the state that the rebuild replaced) and without it from value[t] itself, the partial-episode
 *     approximation.  The carry across an end is selected, not multiplied by 0: a NaN or an infinity stays inside its episode.
 *   rg_vtrace (Espeholt et al. 2018, lambda as in rlax): with ratio(bar) = min(bar, exp(logp_target[t] - logp_behaviour[t])), rho = ratio(rho_bar),
 *     c = lam * ratio(c_bar), rho_pg = ratio(pg_rho_bar), from acc = +0.0 and v_next = vs_next = last_value[n]:
 *       delta = rho * (fma(gamma, boot, reward[t]) - value[t]);   acc = fma(gamma * c, end ? +0.0 : acc, delta);   vs[t] = value[t] + acc
 *       pg_adv[t] = rho_pg * (fma(gamma, end ? boot : vs_next, reward[t]) - value[t])
 *     With logp_target == logp_behaviour and rho_bar == c_bar == 1, vs equals rg_gae's ret for the same lam bit for bit.
 *   A NaN is the canonical quiet NaN.  Asynchronous on hip_stream (NULL = the null stream), on the caller's current device; nothing is read or written past
 *   column n_envs - 1 or outside rows 0 .. n_steps - 1.  n_steps == 0 or n_envs == 0 is a valid no-op.  An output may be EXACTLY one of the [n_steps, n_envs]
 *   f32 inputs (adv == reward, ret == value) or the other output (the second one then stands).
 *   Refused, non-zero with a message (rg_last_error(NULL)) naming the argument, nothing launched, outputs untouched: n_steps or n_envs < 0; NULL reward; NULL
 *   value, logp_behaviour or logp_target for rg_vtrace; both outputs NULL; gamma or lam outside [0, 1] or not finite; a bar not finite or <= 0; trunc_value
 *   without trunc; an output that overlaps an input or the other output in any other way than exactly.
 * The *_host twins: the same rule over host pointers, no stream, no device. */
int rg_gae(void *hip_stream, int64_t n_steps, int64_t n_envs, const float *reward, const float *value, const float *last_value, const uint8_t *done, const uint8_t *trunc,
           const float *trunc_value, float gamma, float lam, float *adv, float *ret);
int rg_vtrace(void *hip_stream, int64_t n_steps, int64_t n_envs, const float *logp_behaviour, const float *logp_target, const float *reward, const float *value,
              const float *last_value, const uint8_t *done, const uint8_t *trunc, const float *trunc_value, float gamma, float lam, float rho_bar, float c_bar, float pg_rho_bar,
              float *vs, float *pg_adv);
int rg_gae_host(int64_t n_steps, int64_t n_envs, const float *reward, const float *value, const float *last_value, const uint8_t *done, const uint8_t *trunc,
                const float *trunc_value, float gamma, float lam, float *adv, float *ret);
int rg_vtrace_host(int64_t n_steps, int64_t n_envs, const float *logp_behaviour, const float *logp_target, const float *reward, const float *value, const float *last_value,
                   const uint8_t *done, const uint8_t *trunc, const float *trunc_value, float gamma, float lam, float rho_bar, float c_bar, float pg_rho_bar, float *vs,
                   float *pg_adv);

/* SHORTEST-PATH FIELDS AND TEACHER KEYS: for each env the number of moves from every cell to the nearest goal cell, that number at the player's cell, and the
 * key that takes the player one move closer, on the device.  The moves are the engine's own: rg_action_mask's move test (Floor::can_move_impl as the player).
 * The field is PRIVILEGED: it sees stairs, gold and passages the player has not discovered.  It is a teacher (imitation, DAgger), a shaping potential
 * (distance to the stairs) or a critic input, not an observation the reference's player has.
 *   Goals, the OR of: RG_GOAL_STAIRS every cell whose surface is the stairs; RG_GOAL_GOLD every cell that holds gold EXCEPT the player's own cell (gold is
 *     taken by moving onto it, and the generator can put the player down on a gold cell); RG_GOAL_CELL one caller-given cell (y, x) per env -- a cell outside
 *     the grid contributes nothing.
 *   A cell is `ok` iff its surface can be walked on and its attr has neither HIDDEN nor LOCKED: what the move test demands of a target.
 *   The field D = u16 [H][W]: 0 on every goal cell, whatever its own word.  For every other ok cell a, the least number of moves a -> ... -> goal, each move
 *     legal from its source: the target inside the grid and ok; for a diagonal both orthogonal neighbours walkable by SURFACE only.  RG_PATH_UNREACHABLE
 *     everywhere else: walls, bare cells, hidden / locked cells that are not goals, ok cells with no such path.  A goal cell that is not ok is not expanded
 *     (nobody can step onto it).  Monsters are ignored: a move into one is an attack.
 *   Distance i32: D at the player's cell, -1 for unreachable.
 *   Teacher key u8, a key byte for rg_step: '.' for an env in the Grave modal (RG_FLAG_DEAD).  Else, D[player] == 0: '>' when the surface under the player is
 *     the stairs and RG_GOAL_STAIRS is in the set, otherwise '.'.  Else, D[player] finite: the key of the FIRST direction in Direction-enum order (Up Down Left
 *     Right LeftUp RightUp LeftDown RightDown = k j h l y u b n) whose move is legal and whose target has D[player] - 1; one always exists.  Else 's': Search
 *     is what reveals hidden cells, and the caller mixes in exploration.
 * rg_path: cells_dev = i32 [n_env][2] (y, x), read iff goals & RG_GOAL_CELL; field_dev (nullable) = u16 [n_env][H][W], 16-byte aligned; dist_dev (nullable)
 *   = i32 [n_env]; key_dev (nullable) = u8 [n_env]; all in the handle's env order.  Without field_dev an env's search ends when it reaches the player's cell.
 *   Asynchronous on the handle's stream.  It reads game state only (the player's cell, the flag word, the cell grid): the pending render is not flushed, the
 *   mirrors, every flag bit, a bound observation tensor and the RNG streams are left alone.  Config groups and mixed-size batches are served for dist_dev /
 *   key_dev / cells_dev; field_dev on such a handle is refused (there is no [n_env][H][W] tensor).  Refused, non-zero with a message naming the argument,
 *   nothing launched: goals zero or with unknown bits; RG_GOAL_CELL without cells_dev; all outputs NULL; field_dev not 16-byte aligned.
 * rg_path_host (stateless, needs no device): the same rule for ONE env given as a host grid `cells` = u16 [height][width] in rg_debug_fetch's layout, the
 *   player's cell (px, py), the dead bit and the cell (cell_y, cell_x) of RG_GOAL_CELL; field_out = u16 [height][width], dist_out and key_out one value each,
 *   any of them NULL but not all.  Refused, non-zero, nothing written, the message read through rg_last_error(NULL): goals as above; all outputs NULL;
 *   cells NULL; the sizes or (px, py) out of range. */
#define RG_GOAL_STAIRS 1u
#define RG_GOAL_GOLD   2u
#define RG_GOAL_CELL   4u
#define RG_PATH_UNREACHABLE 0xFFFFu
int rg_path(rg_t *h, uint32_t goals, const int32_t *cells_dev, uint16_t *field_dev, int32_t *dist_dev, uint8_t *key_dev);
int rg_path_host(const uint16_t *cells, int height, int width, int px, int py, int dead, uint32_t goals, int cell_y, int cell_x,
                 uint16_t *field_out, int32_t *dist_out, uint8_t *key_out);

/* ROUTES THAT FINISH A LEVEL: rg_path's rule with two orthogonal mode bits, one more goal kind and a fallback goal set.  rg_path stops at the first secret (a
 * hidden or locked cell is never a move's target) and all of its answers are privileged; rg_route plans through secrets and / or on the player's own map.
 *   mode, the OR of: RG_ROUTE_SECRETS plan THROUGH hidden / locked cells and ask for 's' when the next cell is one (Search touches the eight cells around
 *     the player, floor.rs:349-370); RG_ROUTE_KNOWN plan on the player's own map only -- with it nothing is privileged.
 *   Per cell word c: walk = the surface can be walked on; secret = HIDDEN or LOCKED; known = DRAWN or VISIBLE, or the cell is the player's own;
 *     K = not RG_ROUTE_KNOWN, or known; pass = K and (secret ? RG_ROUTE_SECRETS : walk): what a move of the search graph may end on -- a secret cell keeps the
 *     surface it was dug into (a room's wall, bare rock) until Search finds it (floor.rs:93-100, 359-366), so its attr alone makes it a cell of the route;
 *     corner = walk and K: what the corner rule of a diagonal asks of the two orthogonal neighbours, by the surface as it is now.
 *   Goals: RG_GOAL_STAIRS and RG_GOAL_GOLD as in rg_path, but only where K; RG_GOAL_CELL as in rg_path, whatever the cell's own word; RG_GOAL_FRONTIER
 *     (legal only together with RG_ROUTE_KNOWN) every pass cell that has an in-grid ORTHOGONAL neighbour which is not known.  Standing on a cell draws its
 *     four orthogonal neighbours unless they are hidden, so a frontier cell is resolved by stepping onto it, and a player standing on one is next to a
 *     hidden cell.
 *   The field D and the distance are rg_path's with pass and corner in place of ok and walkable; a goal that is not pass is never expanded.
 *   Tiers: an env whose player is not reached from `goals` (tier 0) is answered from `fallback_goals` (tier 1; 0 = none).  tier u8 = 0, 1, or 255 when
 *     neither reached it (distance -1 then).
 *   Key u8: '.' for an env in the Grave modal.  Else, D[player] == 0: '>' on the stairs when RG_GOAL_STAIRS is among the answering tier's goals; otherwise 's'
 *     when RG_GOAL_FRONTIER is among them and the own cell is a frontier cell; otherwise '.'.  Else, D[player] finite: the key of the FIRST direction in
 *     Direction-enum order whose move is legal in the search graph, whose target has D[player] - 1 AND whose target is not secret; if there is none, 's':
 *     the next cell is a secret one of the eight neighbours.  Else 's'.  A move key is always legal by rg_action_mask's move test.
 *   With mode 0, no RG_GOAL_FRONTIER and no fallback every byte equals rg_path's.
 * rg_route: cells_dev, dist_dev, key_dev as rg_path's; tier_dev (nullable) = u8 [n_env].  There is no device field.  Asynchronous on the handle's stream.  It
 *   reads game state only: the pending render is not flushed, the mirrors, every flag bit, a bound observation tensor and the RNG streams are left alone.
 *   Config groups and mixed-size batches are served.  Refused, non-zero with a message naming the argument, nothing launched or written: unknown bits in goals,
 *   fallback_goals or mode; goals zero; RG_GOAL_FRONTIER (in either word) without RG_ROUTE_KNOWN; RG_GOAL_CELL (in either word) without cells_dev; all
 *   outputs NULL.
 * rg_route_host (stateless, needs no device): the same rule for ONE env, arguments as rg_path_host's; field_out = the field of the tier that answered (of
 *   the last tier searched when neither did).  Refusals as rg_route's, and cells NULL, the sizes or (px, py) out of range; the message is read through
 *   rg_last_error(NULL). */
#define RG_GOAL_FRONTIER  8u   /* accepted by rg_route only; rg_path keeps refusing it */
#define RG_ROUTE_SECRETS  1u
#define RG_ROUTE_KNOWN    2u
int rg_route(rg_t *h, uint32_t goals, uint32_t fallback_goals, uint32_t mode, const int32_t *cells_dev,
             int32_t *dist_dev, uint8_t *key_dev, uint8_t *tier_dev);
int rg_route_host(const uint16_t *cells, int height, int width, int px, int py, int dead, uint32_t goals, uint32_t fallback_goals,
                  uint32_t mode, int cell_y, int cell_x, uint16_t *field_out, int32_t *dist_out, uint8_t *key_out, uint8_t *tier_out);

/* EPISODE ACCOUNTING AND THE SCOUT REWARD: returns, lengths, depths and end causes of the episodes the stepper ends by itself, and one point per map cell
 * seen for the first time on a level (NLE's "scout" task), kept on the device beside the stepper.  rg_step rebuilds a finished env in the launch that ends
 * its episode; afterwards only reward and done = 1 are left of the old game.  This is a pass of its own behind the step (Gymnasium's
 * RecordEpisodeStatistics, EnvPool's info["episode"]): a handle that does not enable it launches and allocates nothing more.
 *   Per env: ret f32, len i32, depth i32 (the deepest level the running episode has reported), and -- with RG_EP_SCOUT -- `seen`, a bitmap of
 *     SB = 16 * ceil(H*W / 128) bytes: bit b of byte j is cell 8 j + b in row-major order y * W + x; bits of cells outside rows 1 .. H-2 (the rows the
 *     screen draws tiles on) and bits at or past H*W are always 0.  None of it is part of a state record (rg_state_save) or of the compact record.
 *   A KNOWN cell is one in rows 1 .. H-2 whose word has C_VISIBLE or C_DRAWN: the player's own map, which the state keeps bit-exact with the reference.
 *   rg_episode_update, once after a step, for the envs that step played (all, or the first n_keys of rg_step_prefix), on the mirrors and the cells as the
 *     step left them:  ret = ret + reward[e] as one f32 add (the reward mirror: a stair bonus of rg_set_stair_reward is included), len += 1.
 *     done[e] != 0 (the env has been rebuilt already): time_limit = len >= max_steps, died = !time_limit -- the engine has only these two terminal causes,
 *       and A DEATH ON THE VERY LAST ALLOWED STEP IS REPORTED AS A TIME LIMIT (after the rebuild the mirrors cannot tell the two apart).  The finished
 *       episode {ret, len, depth, cause, scout sum} goes to last_return / last_length / last_depth / last_cause and to the log; then ret = 0, len = 0,
 *       depth = the status mirror's dungeon_level (the new game's), seen = the known cells of the new level, scout[e] = 0: the first view of a new game
 *       is not something the old episode earned.
 *     else: a dungeon_level other than the one `seen` belongs to empties `seen` and raises depth; then scout[e] = the number of known cells not in
 *       `seen`, which join it.  Arriving on a new level pays for what is in view there; a cell that drops off the player's map (leaving a dark room)
 *       stays in `seen` and is never paid twice.
 *     It does not guard against being called twice for one step: a second call accounts the mirrors again.
 *   rg_episode_cut, after the caller rebuilt or overwrote envs (rg_reset, rg_reset_envs, rg_reset_mask, rg_state_load), for those envs: with record != 0
 *     and len > 0 the running episode is finished as above with cause RG_EP_CUT; in every case the lane is rebased as after a done, except that len is
 *     taken from the env's step counter (0 after a reset, the saved game's count after a load).  env_ids / k / ids_on_device as rg_reset_envs (host ids
 *     are range-checked and duplicates refused), or mask_dev as rg_reset_mask; both NULL = every env; both non-NULL is refused.
 *   rg_episode_enable: what = RG_EP_STATS or RG_EP_STATS | RG_EP_SCOUT; log_cap records of 32 bytes (0 = no log).  Allocates, and rebases every lane
 *     as a cut without record does.  Refused with a message: a handle created without auto-reset, a handle with config groups, a second enable, another
 *     `what`, a negative log_cap.
 *   rg_episode_arrays: device pointers valid until rg_destroy -- ret f32 [N], len / depth i32 [N], died / time_limit u8 [N] (rewritten by every update,
 *     0 where done is 0), last_return f32 [N], last_length / last_depth i32 [N], last_cause u8 [N] (0 = no episode yet), scout f32 [N] and seen
 *     u8 [N][SB] (both NULL without RG_EP_SCOUT), seen_bytes = SB.  Every array has 64 envs of slack behind env N-1 that no launch writes.
 *   The log: a wave that holds finished episodes takes ONE returning atomic for its slots, so the records of one call are contiguous in the buffer, in
 *     no particular order there; a record that finds the buffer full is dropped and counted.  rg_episode_log_read waits for the stream, copies the
 *     records appended since the last read to out_host (cap >= log_cap entries, else it is refused and the log stays), sorted by (serial, env), stores
 *     their number in *n and the number dropped since the last read in *dropped (nullable), and empties the log.  serial = the ordinal of the update
 *     or cut call since the enable, from 1.
 *   rg_scout_host (stateless, needs no device): the bitmap rule on ONE grid, `cells` = u16 [height][width] in rg_debug_fetch's layout, seen_inout =
 *     u8 [SB]: *fresh_out (nullable) = the known cells not in seen_inout, which join it; pad bits are written 0.  Refused, the message read through
 *     rg_last_error(NULL): cells or seen_inout NULL, sizes out of range.
 * Update, cut and enable are asynchronous on the handle's stream; they read game state and mirrors only and flush nothing. */
#define RG_EP_STATS 1u
#define RG_EP_SCOUT 2u
#define RG_EP_DIED       1u
#define RG_EP_TIME_LIMIT 2u
#define RG_EP_CUT        3u
typedef struct rg_episode_rec { uint32_t serial; int32_t env; float ret; int32_t length; int32_t depth; uint32_t cause; int32_t scout; uint32_t zero; } rg_episode_rec;
typedef struct rg_episode_arrays_t {
    float *ret; int32_t *len; int32_t *depth; uint8_t *died; uint8_t *time_limit;
    float *last_return; int32_t *last_length; int32_t *last_depth; uint8_t *last_cause;
    float *scout; uint8_t *seen; int32_t seen_bytes;
} rg_episode_arrays_t;
int rg_episode_enable(rg_t *h, uint32_t what, int log_cap);
int rg_episode_update(rg_t *h);
int rg_episode_cut(rg_t *h, const int32_t *env_ids, int k, int ids_on_device, const uint8_t *mask_dev, int record);
int rg_episode_arrays(rg_t *h, rg_episode_arrays_t *out);
int rg_episode_log_read(rg_t *h, rg_episode_rec *out_host, int cap, int *n, uint64_t *dropped);
int rg_scout_host(const uint16_t *cells, int height, int width, uint8_t *seen_inout, int32_t *fresh_out);

/* COUNT-BASED NOVELTY: a hash of what each env shows and visit counts of the hashed states, kept on the device beside the stepper -- the episodic count of
 * RIDE, the `count == 1` gate of NovelD / BeBold, #Exploration's lifetime count.  A pass of its own behind the step: a handle that does not enable it
 * launches and allocates nothing more.  The bonus itself (rsqrt of the count, the gate) is one tensor op of the learner's.  The rule -- key bytes, hash,
 * tables -- is stated once in csrc/rg_novelty.h.
 *   what: RG_NOV_POS hashes the player's cell (x, y as u16 LE, four zero bytes), RG_NOV_SCREEN rows 1 .. H-2 of the screen mirror as rg_screen returns it,
 *     RG_NOV_CROP the (2 radius_y + 1) x (2 radius_x + 1) window of those rows around the player (rg_obs_crop's window; cells outside the rows or the columns
 *     are ' ').  The dungeon level of the status mirror, `what` and the key length are hashed in; the hash is never 0.
 *   scope: RG_NOV_EPISODE -- a table of `cap` slots per env (a power of two, 64 .. 65 536; 16 bytes each) that an episode end empties by raising the env's
 *     generation: count[e] is how often env e has shown this state in its running episode, this visit included.  RG_NOV_GLOBAL -- one table of `gcap` slots
 *     (a power of two, 1 024 .. 2^28) for the handle, shared by all envs and emptied by rg_novelty_clear only: gcount[e] is the state's count after EVERY
 *     env's visit of the call has been added, so below capacity it does not depend on scheduling.  A visit that finds its table full (cap probes, or
 *     min(gcap, 1 024) probes of the global table -- about 98 % occupied for a large one -- without a match or an empty slot) is DROPPED: its count is 0
 *     and dropped_episode / dropped_global goes up.  Nothing waits for another lane.  A full global table makes every new state cost those 1 024 probes:
 *     size gcap by the distinct states expected (N x a few hundred for RG_NOV_SCREEN on procedurally generated levels), read rg_novelty_stats.
 *   rg_novelty_enable allocates (16 B x cap x N and 16 B x gcap), then counts every env's present state as a first visit.  Refused with a message that names
 *     the argument, nothing allocated: a handle created without auto-reset, a handle with config groups, a second enable, an unknown what or scope, radii
 *     outside rg_obs_crop's range with RG_NOV_CROP or non-zero otherwise, a cap or gcap that is not a power of two in range (the cap of a scope that is off
 *     is not looked at).
 *   rg_novelty_update, once after a step, for the envs that step played (all, or the first n_keys of rg_step_prefix): done[e] != 0 raises the env's
 *     generation first; then the state now standing in the lane is hashed and counted in each enabled table.
 *   rg_novelty_cut, after rg_reset, rg_reset_envs, rg_reset_mask or rg_state_load (the tables are not part of a state record), for the listed envs: the
 *     generation is raised, then the present state is counted.  env_ids / k / ids_on_device / mask_dev and their refusals as rg_episode_cut.
 *   rg_novelty_arrays: device pointers valid until rg_destroy -- hash u64 [N], count i32 [N] (NULL without RG_NOV_EPISODE), gcount i32 [N] (NULL without
 *     RG_NOV_GLOBAL).  Every array has 64 envs of slack behind env N-1 that no launch writes.
 *   rg_novelty_stats (waits for the stream): out[0] occupied_global, the slots of the global table in use; [1] dropped_global; [2] dropped_episode;
 *     [3] calls, the update and cut calls since the enable or the last clear.
 *   rg_novelty_table_read (waits for the stream): the occupied global slots, sorted by hash, into hashes_host / counts_host of `cap` entries each; *n = their
 *     number.  With hashes_host and counts_host NULL only *n is stored; a cap below *n is refused.  A learner's visitation histogram; the sum of the counts
 *     plus dropped_global is the number of visits offered.
 *   rg_novelty_clear empties the global table and zeroes the four counters.  The episodic tables stay.
 *   rg_novelty_hash_host (stateless, needs no device): the rule on ONE screen u8 [height][width] with the player at (px, py) on dungeon level `level`.
 *     Refused, the message read through rg_last_error(NULL): screen or hash NULL, sizes out of range, the player outside the grid, an unknown what, radii as
 *     above.  rg_novelty_finish_host is the hash's last step alone, mix(acc + mix(salt)) with 0 -> 1.  rg_novelty_insert_host is the episodic insert on a
 *     host table: slots = `cap` slots of {u64 hash, u32 gen, u32 count}, 16-byte aligned; *count = the visit's count, 0 = dropped.
 * Enable, update and cut are asynchronous on the handle's stream.  They read mirrors and game state as the step left them and flush the pending render first,
 * exactly as rg_screen does: behind an observation call the mirrors are drawn already. */
#define RG_NOV_POS    1
#define RG_NOV_SCREEN 2
#define RG_NOV_CROP   3
#define RG_NOV_EPISODE 1u
#define RG_NOV_GLOBAL  2u
typedef struct rg_novelty_arrays_t { uint64_t *hash; int32_t *count; int32_t *gcount; } rg_novelty_arrays_t;
int rg_novelty_enable(rg_t *h, int what, uint32_t scope, int radius_y, int radius_x, int cap, int gcap);
int rg_novelty_update(rg_t *h);
int rg_novelty_cut(rg_t *h, const int32_t *env_ids, int k, int ids_on_device, const uint8_t *mask_dev);
int rg_novelty_arrays(rg_t *h, rg_novelty_arrays_t *out);
int rg_novelty_stats(rg_t *h, uint64_t *out);
int rg_novelty_table_read(rg_t *h, uint64_t *hashes_host, uint32_t *counts_host, int cap, int *n);
int rg_novelty_clear(rg_t *h);
int rg_novelty_hash_host(int what, int level, int height, int width, const uint8_t *screen, int px, int py, int radius_y, int radius_x, uint64_t *hash);
uint64_t rg_novelty_finish_host(uint64_t acc, uint64_t salt);
int rg_novelty_insert_host(void *slots, int cap, uint32_t gen, uint64_t hash, uint32_t *count);

/* CELL ARCHIVE: per hashed state ("cell", Go-Explore's word) the best state record any env has offered, kept on the device, and the way back into it -- the
 * join of rg_state_save / rg_state_load and the novelty hash.  A pass of its own behind the step: a handle that does not enable it launches and allocates
 * nothing more.  The rule -- offers, who beats whom, the table -- is stated once in csrc/rg_archive.h.
 *   An OFFER is (key u64, score i32, steps u32, env).  A key of 0 is offered as 1.  A beats B iff score_A > score_B, or the scores are equal and
 *     steps_A < steps_B; among offers of ONE call with equal (score, steps) the lowest env id wins.
 *   rg_archive_enable(h, cells): one open-addressed table of `cells` slots (a power of two, 1 024 .. 2^24) and cells x R record bytes, R =
 *     rg_state_record_bytes(h) -- 192 MB at 2^14 cells of the mini config.  Refused with a message that names the argument, nothing allocated: a handle with
 *     config groups, a second enable, cells not a power of two in range, an allocation that fails.
 *   rg_archive_update(h, key_dev, score_dev, mask_dev), asynchronous on the handle's stream, flushes the pending render first as rg_state_save does.  Every env
 *     offers (mask_dev u8 [N] given: the envs with a non-zero byte).  key_dev NULL: the novelty hash (refused unless rg_novelty_enable was called); score_dev
 *     NULL: the env's pack gold; steps is always the env's steps word.  For every key offered: seen grows by the number of offers; if the best offer of the
 *     call beats the stored one strictly (an empty slot is beaten by anything; an equal (score, steps) from a later call replaces nothing) that env's state
 *     record -- byte for byte what rg_state_save would write at this moment -- replaces the stored one and (score, steps, when) follow, when = the serial of
 *     this call counted from 1.  slot[e] = the slot of env e's key, -1 if the probe found neither the key nor an empty slot within min(cells, 1 024)
 *     probes (the offer is DROPPED and counted) or the env was masked out; stored[e] = 1 iff env e's record was written by this call.  Except for which slot
 *     a key lands in, the table after a call does not depend on scheduling.
 *   rg_archive_arrays: device pointers valid until rg_destroy.  Per slot [cells]: key u64 (0 = empty), score i32, steps u32, seen u32, chosen u32, when u32,
 *     records u8 [cells][R].  Per env [N]: slot i32, stored u8, score_in i32 / steps_in u32 (what the last update read); these have 64 envs of slack
 *     behind env N-1 that no launch writes.
 *   rg_archive_restore(h, slot_ids, env_ids, k, ids_on_device): the records of slot_ids[0 .. k) are gathered into a staging buffer and loaded into env_ids
 *     (NULL: envs 0 .. k-1 with k = N) by rg_state_load, whose rules and refusals hold; chosen of each slot whose record was taken grows by 1.  An empty
 *     slot's all-zero record (or a device-side slot id out of range) is refused by the load's header check: the env is untouched, RG_FLAG_ERR_STATE is
 *     raised, chosen stays.  Host slot ids out of range are refused before anything is launched.  A slot may be named more than once.  Behind it the caller
 *     does what follows an rg_state_load (rg_novelty_cut, rg_episode_cut).
 *   rg_archive_stats (waits for the stream): out[0] occupied slots, [1] dropped offers, [2] records written, [3] update calls since the enable or the last
 *     clear.  rg_archive_clear empties the table, the records and the counters.
 *   rg_archive_offer_host (stateless, needs no device): the probe and the beats rule for ONE offer on a host table of `cells` (a power of two, 1 .. 2^24)
 *     slots of 32 bytes {u64 key, i32 score, u32 steps, u32 seen, u32 chosen, u32 when, u32 zero}, 8-byte aligned; serial != 0.  *slot = the key's slot or
 *     -1 (dropped: nothing written); *stored = 1 iff the offer replaced the stored one.  Refusals are read through rg_last_error(NULL). */
typedef struct rg_archive_arrays_t {
    uint64_t *key; int32_t *score; uint32_t *steps; uint32_t *seen; uint32_t *chosen; uint32_t *when; uint8_t *records;
    int32_t *slot; uint8_t *stored; int32_t *score_in; uint32_t *steps_in;
} rg_archive_arrays_t;
int rg_archive_enable(rg_t *h, int cells);
int rg_archive_update(rg_t *h, const uint64_t *key_dev, const int32_t *score_dev, const uint8_t *mask_dev);
int rg_archive_arrays(rg_t *h, rg_archive_arrays_t *out);
int rg_archive_restore(rg_t *h, const int32_t *slot_ids, const int32_t *env_ids, int k, int ids_on_device);
int rg_archive_stats(rg_t *h, uint64_t *out);
int rg_archive_clear(rg_t *h);
int rg_archive_offer_host(void *slots, int cells, uint64_t key, int32_t score, uint32_t steps, uint32_t serial, int32_t *slot, int32_t *stored);

/* MONSTER TABLES AND THREAT WORDS: the nearest monsters of every env as an entity list, and four words that say how close they are.  The monster tables are
 * device-resident and bit-exact with the reference; this is one small pass behind the step that hands them out in a form a policy, a shaping term or a
 * teacher can use, without parsing the image.  The rule is stated once in csrc/rg_monsters.h.
 *   A monster of the env's current level is ALIVE when its slot holds one.  It is SHOWN when a Redraw at this moment would put its letter on the screen
 *     (RunTime::draw_screen): its row is in 1 .. H-2, its cell is visible or drawn, it is not the player's cell, the cell holds no gold (gold is drawn
 *     over a monster), and either dx*dx + dy*dy <= 2 or Floor::in_same_room holds (same assigned area and, unless the room is Empty, both cells inside
 *     the room's rect or both outside it), with dx = x - px, dy = y - py.
 *   RG_MON_SHOWN lists the shown monsters: what the screen can show.  RG_MON_ALL lists every alive monster of the level and is PRIVILEGED in the same sense
 *     as rg_path: positions, hit points and wakefulness of monsters the player has not met.
 *   Order: ascending by (cheb = max(|dx|, |dy|), dx*dx + dy*dy, x<<8|y).  The nearest `cap` (1 .. RG_MON_MAX_CAP) are written as rows of RG_MON_COLS int16,
 *     16 bytes each: [0] the tile byte the screen shows for the monster's kind ('A'..'Z'; 0 marks an empty row), [1] dx, [2] dy, [3] cheb, [4] 1 if shown
 *     (always 1 in SHOWN mode), and in ALL mode [5] 1 if the monster is active (awake), [6] min(hp, 32767), [7] the monster's table slot; [5..7] are 0 in
 *     SHOWN mode.  Rows past the last listed monster are all zero, and every row of every env is written by every call.
 *   threat i32 [4], always over the SHOWN monsters whatever the mode: [0] how many have cheb == 1; [1] the cheb of the nearest, -1 = none; [2] a positional
 *     attack mask, bit i set when the cell the move key RG_ACTION_KEYS[1 + i] (h j k l n b u y) aims at holds a shown monster -- positional only, it says
 *     nothing about the corner rule: AND it with rg_action_mask's answer for legality; [3] the number of monsters that qualify in the call's mode (it may
 *     exceed cap).
 *   An env in the Grave modal (RG_FLAG_DEAD) answers an all-zero table and threat {0, -1, 0, 0}.
 *   The rule reads the GAME STATE, not the screen mirror: it equals the reference's own drawing whenever the reference draws, and between Redraws (a key
 *     that produced none) it is more current than the image.
 * rg_monsters: table_dev (nullable) = i16 [n_env][cap][RG_MON_COLS], threat_dev (nullable) = i32 [n_env][4], both 16-byte aligned.  Asynchronous on the
 *   handle's stream; it reads game state only and flushes nothing.  Config groups and mixed sizes are served, every env's rows at the handle's env index.
 *   Refused with a message, nothing launched or written: an unknown mode; cap outside 1 .. RG_MON_MAX_CAP while table_dev is given; both outputs NULL; an
 *   output that is not 16-byte aligned.
 * rg_monsters_host (stateless, needs no device): the same rule for ONE env on host arrays -- cells u16 [height][width], the player's cell, the dead bit, the
 *   n_mon monsters and the room_num_x * room_num_y rooms in rg_debug_state's layout (mon_type = tile - 'A'; room_rect packed, room_meta bits 0-1 the kind),
 *   so that an rg_debug_fetch result feeds it directly.  mon_alive (nullable) = i32 [n_mon], 0 = the entry is skipped; NULL = every entry is alive.  A row's
 *   slot column is the monster's index in the arrays given.  table_out = i16 [cap][RG_MON_COLS], threat_out = i32 [4], either NULL but not both.  Refusals as
 *   rg_monsters' (alignment aside), and NULL arrays, sizes, the player's cell or a monster's cell out of range; the message is read through
 *   rg_last_error(NULL). */
#define RG_MON_SHOWN   0u
#define RG_MON_ALL     1u
#define RG_MON_MAX_CAP 16
#define RG_MON_COLS    8
int rg_monsters(rg_t *h, uint32_t mode, int cap, int16_t *table_dev, int32_t *threat_dev);
int rg_monsters_host(const uint16_t *cells, int height, int width, int px, int py, int dead, int n_mon, const int32_t *mon_x, const int32_t *mon_y,
                     const int32_t *mon_type, const int32_t *mon_active, const int32_t *mon_hp, const int32_t *mon_alive, int room_num_x, int room_num_y,
                     const uint32_t *room_rect, const int32_t *room_meta, uint32_t mode, int cap, int16_t *table_out, int32_t *threat_out);

/* OBJECT TABLES BY WALKING DISTANCE: the stairs, gold, doors and frontier cells of every env's level as an entity list, nearest first by the number of moves
 * it takes to reach them -- what an object-centric policy, a feature-vector policy or an option policy that picks a target for rg_route needs beside
 * rg_monsters.  One search from the player's cell over rg_route's graph visits the objects in that order.  The rule is stated once in csrc/rg_objects.h.
 *   mode, the OR of RG_ROUTE_SECRETS and RG_ROUTE_KNOWN with rg_route's meaning; K, pass, corner and known are rg_route's predicates, the player's own cell
 *     judged as its own.  With RG_ROUTE_KNOWN nothing in the answer is privileged: it is the player's own map (DRAWN / VISIBLE).  Without it the table is
 *     PRIVILEGED in the sense of rg_path.
 *   kinds, the OR of: RG_OBJ_STAIRS a cell that is K and whose surface is the stairs; RG_OBJ_GOLD a cell that is K and holds gold, EXCEPT the player's own
 *     cell (gold is taken by moving onto it); RG_OBJ_DOOR a cell that is K and whose surface is a door, the '+' of the screen -- a hidden door keeps its wall
 *     surface and is none; RG_OBJ_FRONTIER (legal only together with RG_ROUTE_KNOWN) rg_route's frontier cells.  A cell is ONE object; its kind column is
 *     the OR of the asked kinds it satisfies (a door that is a frontier cell reads 12).
 *   walk of a cell = the number of moves from the player's cell to it in rg_route's search graph under mode (a move's target is pass, a diagonal's two
 *     orthogonal neighbours are corner, the own cell starts the search whatever its word, monsters are ignored): the distance rg_route answers when the cell
 *     is given as RG_GOAL_CELL under the same mode.  A qualifying cell the search does not reach is not listed; the own cell is listed with walk 0 when it
 *     qualifies.
 *   The table: the listed objects in ascending order of (walk, y, x), the first `cap` (1 .. RG_OBJ_MAX_CAP) of them, as rows of RG_OBJ_COLS int16, 16 bytes
 *     each: [0] the kind bits (0 marks an empty row), [1] dx = x - px, [2] dy = y - py, [3] walk (at most H*W <= 7 680), [4] x, [5] y, [6] max(|dx|, |dy|),
 *     [7] 0.  Rows past the last listed object are all zero, and every row of every env is written by every call.
 *   count i32 [4]: per kind bit the number of qualifying cells, reached or not; 0 for a kind that was not asked for.  It tells that more exists than the
 *     table holds or the search reached.
 *   An env in the Grave modal (RG_FLAG_DEAD) answers an all-zero table and zero counts.  Gold amounts and a first-move key per object are not part of it:
 *     the key to a chosen object is rg_route with that cell.
 * rg_objects: table_dev (nullable) = i16 [n_env][cap][RG_OBJ_COLS], count_dev (nullable) = i32 [n_env][4], both 16-byte aligned.  Asynchronous on the
 *   handle's stream; it reads game state only and flushes nothing.  Config groups and mixed sizes are served, every env's rows at the handle's env index.
 *   Refused with a message naming the argument, nothing launched or written: kinds zero or with unknown bits; unknown bits in mode; RG_OBJ_FRONTIER without
 *   RG_ROUTE_KNOWN; cap outside 1 .. RG_OBJ_MAX_CAP while table_dev is given; both outputs NULL; an output that is not 16-byte aligned.
 * rg_objects_host (stateless, needs no device): the same rule for ONE env by a plain queue search -- cells u16 [height][width] in rg_debug_fetch's layout,
 *   the player's cell and the dead bit; table_out = i16 [cap][RG_OBJ_COLS], count_out = i32 [4], either NULL but not both.  Refusals as rg_objects'
 *   (alignment aside), and cells NULL, the sizes or (px, py) out of range; the message is read through rg_last_error(NULL). */
#define RG_OBJ_STAIRS   1u
#define RG_OBJ_GOLD     2u
#define RG_OBJ_DOOR     4u
#define RG_OBJ_FRONTIER 8u
#define RG_OBJ_MAX_CAP  32
#define RG_OBJ_COLS     8
int rg_objects(rg_t *h, uint32_t kinds, uint32_t mode, int cap, int16_t *table_dev, int32_t *count_dev);
int rg_objects_host(const uint16_t *cells, int height, int width, int px, int py, int dead, uint32_t kinds, uint32_t mode, int cap,
                    int16_t *table_out, int32_t *count_out);

/* PlayerState::status_vec (python/src/lib.rs:158-161, flags.rs:67-87) for the whole batch: out_host = i32 [n_env][popcount(flag)].  Synchronous. */
int rg_status_vec(rg_t *h, uint32_t status_flag, int32_t *out_host);

/* Host copies for the value-object API (ParallelGameState::states/step return Vec<PlayerState>):
 * synchronous D2H of the mirrors; any pointer may be NULL.  screen / hist: u8 [n_env][H][W]; for a batch that mixes sizes the envs follow
 * each other in env order, env i taking H_i * W_i bytes (rg_env_dims). */
int rg_fetch_states(rg_t *h, uint8_t *screen, uint8_t *hist, int32_t *status, uint32_t *flags);
/* ParallelGameState::step (python/src/lib.rs:315-321) in one call and ONE stream wait, for small batches: keys from host memory (zipped with the envs like
 * rg_step_prefix), then the mirror refresh, then one kernel writes status i32 [n][10], flags u32 [n] -- and, if given, screen / hist u8 [n][H*W] -- straight to
 * their destinations, which must be device-visible (pinned host memory from rg_host_alloc, or device memory).  Errors as rg_sync.  Not for config groups. */
int rg_step_fetch(rg_t *h, const uint8_t *keys_host, int n_keys, uint8_t *screen, uint8_t *hist, int32_t *status, uint32_t *flags);

/* Device-side snapshots of the two big mirrors, for value-object callers that read mostly status / flags (parallel.py:59-64 uses gold and
 * is_terminal of every state, nothing else): rg_snapshot_take flushes the pending render and copies screen + hist device-to-device into
 * `dev` = u8 [2][n_env][H][W] (screen first; allocate with rg_dev_alloc), asynchronously on the handle's stream; rg_dev_read is a synchronous
 * D2H copy of any part of it (or of any device buffer of the handle) made when a PlayerState's screen is first looked at.  Not for batches that
 * mix sizes. */
int rg_dev_alloc(int device, size_t bytes, void **out);
void rg_dev_free(int device, void *p);
int rg_snapshot_take(rg_t *h, void *dev);
int rg_dev_read(rg_t *h, const void *dev_src, void *host_dst, size_t bytes);
/* the same for `rows` pieces of row_bytes that lie src_pitch apart on the device (screen and history of ONE env of a snapshot: one copy) */
int rg_dev_read_rows(rg_t *h, const void *dev_src, size_t src_pitch, void *host_dst, size_t row_bytes, int rows);

/* Stateless encode of ONE host-side PlayerState snapshot on the GPU (PlayerState.gray_image &c.
 * called on a cloned value object): uploads, runs the same encode kernel, downloads.
 * kind 0 = gray, 1 = symbol.  Returns non-zero on the symbol-image tile error. */
int rg_encode_host(int device, const uint8_t *screen, const uint8_t *hist, const int32_t *status, int height, int width,
                   int symbols, uint32_t status_flag, int with_hist, int kind, float *out_host);

/* The same for n snapshots at once (screen / hist u8 [n][H][W], status i32 [n][10], out f32 [n][C][H][W]); the device scratch is cached per
 * device, so repeated calls allocate nothing. */
int rg_encode_host_batch(int device, int n, const uint8_t *screen, const uint8_t *hist, const int32_t *status, int height, int width,
                         int symbols, uint32_t status_flag, int with_hist, int kind, float *out_host);
/* PlayerState images of the handle's CURRENT states for the whole batch, into host memory: fused mirror refresh + encode on the device
 * (scratch kept by the handle), one D2H copy.  Synchronous.  out_host = f32 [n_env][C][H][W], ideally pinned (rg_host_alloc). */
int rg_obs_host(rg_t *h, int kind, uint32_t status_flag, int with_hist, float *out_host);
/* Pinned (page-locked) host memory for rg_fetch_states / rg_obs_host destinations (D2H at full PCIe rate). */
int rg_host_alloc(size_t bytes, void **out);
void rg_host_free(void *p);

/* Multi-GPU: the ONE per-step collective gathers a compact record per env instead of the f32 observation.
 * rg_pack_compact writes u8 [n_env][rg_compact_record_bytes] = {screen u8[H*W], status i32[10], reward f32, flags u32, hist u8[H*W] if
 * with_hist} into out_dev (flushes the pending render first) -- everything ThreadConductor::step returns per env in one reply, state AND
 * terminal flag (python/src/thread_impls.rs:61-81; parallel.py:59-64 derives reward and done from it): `reward` is the step's gold delta,
 * `flags` the public RG_FLAG_* bits (TERMINAL = done, DEAD, message bits 8..14, error bits; the mirror bookkeeping bits are masked out).
 * After the all-gather, the consumer expands any number of records with rg_expand_compact into out_dev = f32 [n][C][H][W] --
 * PlayerState::{gray,symbol}_image[_with_hist] (python/src/lib.rs:72-111; symbol.rs:51-71) from the packed bytes -- and reads reward / flags
 * at RG_COMPACT_REWARD_OFFSET(H*W) / RG_COMPACT_FLAGS_OFFSET(H*W) of every record.  H*W must be divisible by 4. */
#define RG_COMPACT_FIXED_BYTES 48                       /* status i32[10] + reward f32 + flags u32 */
#define RG_COMPACT_STATUS_OFFSET(hw) (hw)
#define RG_COMPACT_REWARD_OFFSET(hw) ((hw) + 40)
#define RG_COMPACT_FLAGS_OFFSET(hw) ((hw) + 44)
#define RG_COMPACT_HIST_OFFSET(hw) ((hw) + RG_COMPACT_FIXED_BYTES)
int rg_compact_record_bytes(const rg_t *h, int with_hist);
int rg_pack_compact(rg_t *h, int with_hist, uint8_t *out_dev);
/* The collective itself ("exactly one per step: ncclAllGather (RCCL over xGMI) of the obs slice, in place into rank-ordered
 * slices"), for hosts that do not bring their own (the reference has none: its workers are threads, python/src/thread_impls.rs:14-34).
 * rg_comm_unique_id: ncclGetUniqueId on one rank, handed to the others by the caller (any channel; 128 bytes).  rg_comm_init: ncclCommInitRank
 * for the handle's device; every rank's handle must hold the same n_env.  rg_allgather_compact: packs this rank's records into slice `rank` of
 * out_dev = u8 [world * n_env][record] and all-gathers in place on the handle's stream (asynchronous like every launch; expand with
 * rg_expand_compact).  librccl is bound at run time: only these four calls need it. */
int rg_comm_unique_id(uint8_t id[128]);
int rg_comm_init(rg_t *h, const uint8_t id[128], int rank, int world);
int rg_comm_destroy(rg_t *h);
/* What the communicator reports about itself (ncclCommCount / ncclCommUserRank) -- not what rg_comm_init was told. */
int rg_comm_count(rg_t *h, int *count, int *rank);
int rg_allgather_compact(rg_t *h, int with_hist, uint8_t *out_dev);
int rg_expand_compact(rg_t *h, const uint8_t *packed_dev, int n, int packed_has_hist, int kind, uint32_t status_flag, int with_hist, float *out_dev);

/* Action-history log (RunTime::saved_inputs, core/src/lib.rs:288; GameState::dump_history, python/src/lib.rs:245-250).  Off by default;
 * rg_history_enable allocates a device-side key log of cap_per_env keys for the running and for the previous episode of every env (an
 * episode = one RunTime: it ends at rg_reset or at the auto-reset).  Every key that is in KeyMap::ai is logged when it is received (also
 * the ones rejected with IgnoredInput while dead), as the reference does.
 * rg_history_keys: raw key bytes; which = 0 running episode, 1 previous episode; *len = keys received (returns 2 if that exceeds the
 * capacity, i.e. the log is truncated).  rg_dump_history: the same as serde_json::to_string_pretty(Vec<InputCode>), the format of
 * data/learned/ddqn-minidungeon/best-actions.json; *needed = bytes incl. NUL (buf may be NULL to query). */
int rg_history_enable(rg_t *h, int cap_per_env);
int rg_history_keys(rg_t *h, int env, int which, uint8_t *keys, size_t cap, uint32_t *len);
int rg_dump_history(rg_t *h, int env, int which, char *buf, size_t cap, size_t *needed);

/* Workload counters accumulated by rg_step since the last reset of the counters: out[0] auto-resets, [1] descents, [2] dist maps built (BFS),
 * [3] levels generated inline by the step kernel (descents, and resets that found no spare), [4] spare levels taken, [5] Redraw reactions, [6] keys processed, [7] partial dist maps continued over the walkable mask saved with them (a map
 * begun before a descent or an opening search, grids of 33..96 columns; counted in [2] as well).  Synchronous. */
int rg_counters(rg_t *h, uint64_t out[8], int reset);
/* ... and the counters beyond the first eight (n_out <= 16): [8] descents whose level came from its next-level structure -- the first two thirds of
 * Dungeon::new_level (rogue/mod.rs:434-481: rooms, passages, gold, stairs) generated ahead of the descent by the background generator, the monsters and
 * the player's placement inside the turn; counted in [3] as well.  [9..15] reserved (0). */
int rg_counters_ex(rg_t *h, uint64_t *out, int n_out, int reset);
/* Effective shader clock right now: a one-wave spin kernel on the handle's stream compares s_memtime (shader-clock ticks) with
 * s_memrealtime (constant 100 MHz).  Synchronous; bench.py's evidence for the clock state of a run. */
int rg_probe_sclk(rg_t *h, double *mhz);

/* Per-kernel timing with HIP events recorded on the handle's stream (bench.py's roofline leg).
 * While enabled, every rg_step / render flush / rg_obs_* launch is bracketed by an event pair (up to
 * 4096 launches per kernel between reads).  rg_timing_read synchronises, returns the summed elapsed
 * milliseconds and launch counts per kernel {0: k_step, 1: k_render, 2: k_gray|k_symbol, 3: k_build}
 * and clears the accumulators.  on = N > 1 brackets only every N-th launch of each kernel (an event pair costs a few
 * microseconds of stream time). */
int rg_timing_enable(rg_t *h, int on);
int rg_timing_read(rg_t *h, double ms[4], uint64_t launches[4]);
/* The same for the first n <= 5 kernels {.., 4: k_regen -- the background generator, stamped on its own low-priority stream}: summed milliseconds and
 * number of SAMPLED launches per kernel, and (launches != NULL) how many launches of the kernel there were in all since the last read / enable. */
int rg_timing_read_all(rg_t *h, int n, double *ms, uint64_t *sampled, uint64_t *launches);
/* The individual samples behind those sums, for latency percentiles (bench.py `step_us`): the duration in ms of every sampled launch of `kernel`
 * (rg_timing_read_all's order) since rg_timing_enable, oldest first, at most `cap` of them, *n = how many.  kernel = -1: one value per STEP -- from the
 * begin of its k_step to the end of its observation pass (kernel 2), for the steps in which both were sampled (rg_timing_enable(h, 1): all).  Call it
 * before rg_timing_read / rg_timing_read_all, which reset the samples.  Not for handles with config groups. */
int rg_timing_read_samples(rg_t *h, int kernel, float *ms, int cap, int *n);

/* GameState::dump_config (python/src/lib.rs:252-254): canonical JSON of env i's effective config. */
int rg_dump_config(const rg_t *h, int env, char *buf, size_t cap);

/* Stateless: parse one GameConfig JSON (GameConfig::from_json, core/src/lib.rs:144-149) and write its canonical
 * re-serialisation (GameConfig::to_json with the reference's skip-if-default rules) into buf.  Needs no device.
 * Returns non-zero and sets rg_last_error(NULL) on a parse / validation error. */
int rg_config_canonical(const char *cfg_json, char *buf, size_t cap);

/* Stateless: what the stepper resolved from the item tables and the player's pack of one GameConfig (Player::init_items, player.rs:136-153;
 * InitItem::initialize, item/mod.rs:181-221) -- JSON {"weapon": {"times", "max", "hit_plus", "dam_plus"} (the wielded dice, fight.rs:21-33),
 * "armor_def" (Player::arm), "init_gold", "can_pickup", "init_draws": [[lo, hi] ...] (the item-stream draws of the build, weapon.rs:159),
 * "symbols", "n_enemies"}.  Needs no device; errors as rg_config_canonical. */
int rg_config_resolved(const char *cfg_json, char *buf, size_t cap);

/* The config surface, key by key: a JSON array of {"path", "status": "honoured" | "inert", "why"} for every key the reference's serde structs
 * know (core/src/lib.rs:42-86, rogue/mod.rs:23-66, item/{mod,gold,weapon,armor}.rs, player.rs:17-32, enemies.rs:18-121).  "inert" = serde reads
 * it and the engine never does; such keys are accepted, type-checked and written back by rg_dump_config.  Needs no device.  *needed = bytes incl.
 * NUL (buf may be NULL to query). */
int rg_config_schema(char *buf, size_t cap, size_t *needed);

/* Batched save and restore of env game states (ALE's cloneState / restoreState, for every env of the batch at once).
 * A STATE RECORD is one env's running game as a fixed-size, position-independent byte string of R = rg_state_record_bytes(h) bytes: no pointers, nothing
 * that depends on n_env.  R depends only on the config's geometry and room grid and on the handle's key-log capacity.  Layout (rogue-gym_amd/csrc/
 * rg_state_io.h; every section 16-byte aligned, padding zero):
 *   header (64 B): u32 magic "RGST", RG_STATE_VERSION, R, H | W << 16, rooms, sections, a 64-bit config fingerprint (FNV-1a of rg_config_canonical's text
 *                  without seed / seed_range), key-log capacity, key-log length
 *   cell u16 [H*W], screen u8 [H*W], hist u8 [H*W], dist maps u16 [9][H*W] (configs with enemies), their saved walkable masks (the grid class with
 *   partial maps), status i32 [10], the env's observation-overlay record, then one u32 per word of the SoA state: player, hunger, gold, level, steps,
 *   flags, reward, done, the three RNG streams, monster counts, the dist-cache ring (keys, head, length, partial / saved bits), and per room the room,
 *   monster and gold tables and the overlay positions; last the running episode's key log (the saving handle's capacity; 0 bytes when logging is off).
 * What a record does NOT carry, deliberately: what decides the env's FUTURE episodes -- seed, seed range, build counter, the pre-generated spare levels and
 * the previous episode's key log -- belongs to the destination slot.  A restored env plays out the saved episode; when that episode ends it resets from
 * its OWN seed, as rg_reset would.  Nor the generator's scratch (corridor records, maze stack: dead once a level is complete) and the handle-local flag bits
 * (RG_FLAG_SCR_CHANGED, the error bits: cleared in the record).  Records are canonical: padding, the key log past its length, the words of
 * empty slots (a dead monster's hp / exp, an absent gold's amount) and the dist-cache slots outside the cache's ring (maps, keys, saved masks: what an
 * earlier episode left behind) are zero, so equal states give equal bytes -- a rebuilt env's record equals that of a newly created one.
 * rg_state_save: flushes the pending render (records hold drawn mirrors), then writes k records to out_dev = u8 [k][R] (16-byte aligned), env_ids[i]'s
 *   state in record i; env_ids NULL = all n_env envs in order (k is then ignored).
 * rg_state_load: k records of rec_bytes each (R of the SAVING handle: it may differ from this handle's only in the key-log section; as many logged keys are
 *   loaded as fit) into envs env_ids[i] (NULL = all n_env in order).  Every header is checked on the device against this handle's fingerprint and layout:
 *   a record that does not fit leaves its env untouched, sets RG_FLAG_ERR_STATE in its flags and is reported by the next rg_sync.  The bound observation
 *   tensor (rg_obs_bind) is re-encoded in full at its next call.  A key log that the record did not hold completely is reported as truncated.
 * Both are asynchronous on the handle's stream.  The background generators neither read nor write what a load writes, so stream order suffices: nothing
 * is drained.  Host-side ids are range-checked and a load refuses duplicates; device-side ids (ids_on_device != 0, i32) are the caller's responsibility
 * (an id out of range is skipped and raises RG_FLAG_ERR_STATE).  Not for handles with config groups; rg_state_record_bytes returns -1 for them. */
int rg_state_record_bytes(const rg_t *h);
int rg_state_save(rg_t *h, const int32_t *env_ids, int k, int ids_on_device, uint8_t *out_dev);
int rg_state_load(rg_t *h, const uint8_t *rec_dev, size_t rec_bytes, const int32_t *env_ids, int k, int ids_on_device);

/* Parity/debug: synchronous copy of env i's internal state to the host. */
typedef struct rg_debug_state {
    int32_t px, py, dungeon_level, hp, hp_max, player_level, n_monsters, n_gold;
    uint32_t exp, food_left, quiet, pack_gold, steps;
    uint32_t rng[12];        /* dungeon, item, enemy streams x {x,y,z,w} */
    int32_t mon_x[384], mon_y[384], mon_type[384], mon_active[384], mon_hp[384];   /* one slot per room; 160 x 48 holds at most 40 x 9 = 360 rooms */
    uint32_t mon_exp[384];
    int32_t gold_x[384], gold_y[384], gold_amount[384];
    int32_t n_rooms;          /* room_num_x * room_num_y, row-major room ids */
    uint32_t room_rect[384];  /* x0 | y0<<8 | x1<<16 | y1<<24, half-open (Empty room: x0, y0 = its anchor cell) */
    int32_t room_meta[384];   /* bits 0-1 kind (0 Normal, 1 Maze, 2 Empty; rooms.rs:11-19), 4 dark, 8 visited, 16 has gold */
} rg_debug_state;
/* cells: u16 [H][W] = surface (bits 0-2, rogue/mod.rs:137-147) | door<<3 | CellAttr<<4 (field.rs:107-124) */
int rg_debug_fetch(rg_t *h, int env, rg_debug_state *out, uint16_t *cells);
/* Parity/debug: every env generates its next dungeon level and places the player there (Dungeon::new_level, rogue/mod.rs:434-481 +
 * actions::new_level, actions.rs:121-138) as on a successful '>' but without the turn around it (no hunger tick, no monster move,
 * no step count).  Lets tests reach levels 2..30 of thousands of seeds directly.  Mirrors are redrawn at the next read. */
int rg_debug_descend(rg_t *h);

#ifdef __cplusplus
}
#endif
#endif
