// rg_launch.h -- the host-callable launchers (rgk_*) of the .hip units, declared ONCE: every unit that defines one and every host unit that calls one includes
// this file, so a definition whose parameter list differs from what a caller sees is a compile error ("conflicting types"), not a launch with garbage arguments.
// Declarations only: no inline code, no macro.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rogue_gym_hip.h"  // rg_act_opts
#include "rg_state.h"

struct RgIoLayout;  // rg_state_io.h
struct RgEpisode;   // rg_episode.h
struct RgNovelty;   // rg_novelty.h
struct RgArchive;   // rg_archive.h

extern "C" {
// rg_kernels.hip
void rgk_build(const RgState *S, const RgConfig *c, hipStream_t st);
void rgk_reset_compact(const uint8_t *mask, int n, int32_t *list, uint32_t *cnt, hipStream_t st);
void rgk_build_list(const RgState *S, const RgConfig *c, const int32_t *list, const uint32_t *cnt, uint8_t *mark, hipStream_t st);
int rgk_step_epw(int n, int slots_per_simd);
size_t rgk_step_lds_per_cu(const RgConfig *c);
int rgk_step_bound_capable(const RgConfig *c);
int rgk_step_tail_capable(const RgConfig *c);
int rgk_step_enc_helpers(int n, int want);
int rgk_step(const RgState *S, const RgState *SP_dev, const RgConfig *c, const uint8_t *keys, int use_spares, int parity, int generic_enc, hipStream_t st, hipEvent_t ev0,
             hipEvent_t ev1);
void rgk_debug_descend(const RgState *S, const RgConfig *c, hipStream_t st);
void rgk_regen_gate(const uint32_t *mark, uint32_t target, uint32_t *err_any, hipStream_t st);
void rgk_regen(const RgState *SP, const RgConfig *c, int bulk, int spares, const uint32_t *mark, uint32_t target, uint32_t *err_any, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// rg_regen_lanes.hip
int rgk_regen_lanes_supported(const RgConfig *c, int maze_cap);
int rgk_regen_lanes(const RgState *SP, const RgConfig *c, uint32_t *q, int32_t *list, int bulk, int waves, int slots, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// rg_obs.hip
void rgk_render(const RgState *S, const RgConfig *c, hipStream_t st);
int rgk_obs(const RgState *S, const RgConfig *c, uint32_t sflag, int with_hist, int kind, float *out, uint32_t *err_any, int planes_sym, int bound, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
int rgk_obs_tail_capable(const RgState *S, const RgConfig *c);
int rgk_obs_resid_blocks(int n);
void rgk_obs_resid(const RgState *S, const RgConfig *c, float *out, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
void rgk_encode(const uint8_t *screen, const uint8_t *hist, const int32_t *status, uint32_t *flags, uint32_t *err_any, int n, int hw, size_t rs, size_t rst,
                int symbols, int planes_sym, uint32_t sflag, int with_hist, int kind, float *out, const int32_t *ext, hipStream_t st);
void rgk_export(const RgState *S, uint32_t *err_any, void *o_screen, void *o_hist, void *o_status, void *o_flags, uint32_t *o_err, hipStream_t st);
void rgk_pack(const RgState *S, int with_hist, uint8_t *out, hipStream_t st);
void rgk_scatter_rows(const void *src, void *dst, const int32_t *ext, int n, int row_bytes, hipStream_t st);
void rgk_gather_keys(const uint8_t *keys, const int32_t *ext, uint8_t *dst, int n, hipStream_t st);
int rgk_redraw(const RgState *S, const RgConfig *c, hipStream_t st);
int rgk_obs_typed(const RgState *S, const RgConfig *c, int kind, int dtype, uint32_t sflag, int with_hist, int planes_sym, void *out, uint32_t *err_any, hipStream_t st, hipEvent_t ev0,
                  hipEvent_t ev1);
void rgk_probe_clock(unsigned long long *out, int spin, hipStream_t st);
// rg_crop_typed.hip, rg_pixels.hip
int rgk_crop_typed(const RgState *S, const RgConfig *c, int kind, int dtype, int ry, int rx, uint32_t sflag, int with_hist, int planes_sym, void *out, int32_t *centers,
                   uint32_t *err_any, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
int rgk_pixels_lds(int H, int W, int th, int channels, int ry, int rx, int *run, int *staged);
int rgk_pixels(const RgState *S, const RgConfig *c, const uint8_t *tiles, int th, int channels, int ry, int rx, uint8_t *out, int32_t *centers, hipStream_t st, hipEvent_t ev0,
               hipEvent_t ev1);
// the readers of game state: rg_action_mask.hip, rg_path.hip, rg_route.hip, rg_monsters.hip, rg_objects.hip
void rgk_action_mask(const RgState *S, const RgConfig *c, const uint8_t *keys, int n_keys, uint8_t *mask, uint8_t *sample, uint64_t seed, uint64_t draw, hipStream_t st,
                     hipEvent_t ev0, hipEvent_t ev1);
// ... and rg_policy.hip (librogue_gym_policy.so)
void rgk_act(const RgState *S, const RgConfig *c, const uint8_t *keys, int n_keys, const void *logits, int dtype, const rg_act_opts *opts, const uint8_t *teacher,
             const int32_t *given, uint8_t *key, int32_t *action, float *logp, float *entropy, uint8_t *source, uint8_t *mask, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
const char *rgk_act_build_id(void);
// ... and rg_policy_grad.hip (librogue_gym_learn.so): stateless, no handle
void rgk_pg_eval(int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp, float *logp, float *entropy,
                 hipStream_t st);
void rgk_pg_grad(int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp, const float *g_lp, const float *g_ent,
                 void *dlogits, hipStream_t st);
const char *rgk_learn_build_id(void);
// ... and rg_returns.hip (librogue_gym_returns.so): stateless.  WEAK: a build of the host units that is linked without that library (tests/rule_mutants.py's
// fixed list) still loads, and the device entries, which test the address first, refuse with a message.
__attribute__((weak)) void rgk_gae(int64_t n_steps, int64_t n_envs, const float *reward, const float *value, const float *last_value, const uint8_t *done, const uint8_t *trunc,
                                   const float *trunc_value, float gamma, float gl, float *adv, float *ret, hipStream_t st);
__attribute__((weak)) void rgk_vtrace(int64_t n_steps, int64_t n_envs, const float *logp_behaviour, const float *logp_target, const float *reward, const float *value,
                                      const float *last_value, const uint8_t *done, const uint8_t *trunc, const float *trunc_value, float gamma, float lam, const float *bars,
                                      float *vs, float *pg_adv, hipStream_t st);
__attribute__((weak)) const char *rgk_returns_build_id(void);
void rgk_path(const RgState *S, const RgConfig *c, uint32_t goals, const int32_t *gcell, uint16_t *field, int32_t *dist, uint8_t *key, hipStream_t st);
void rgk_route(const RgState *S, const RgConfig *c, uint32_t goals, uint32_t fallback, uint32_t mode, const int32_t *gcell, int32_t *dist, uint8_t *key, uint8_t *tier,
               hipStream_t st);
void rgk_monsters(const RgState *S, const RgConfig *c, uint32_t mode, int cap, int16_t *table, int32_t *threat, hipStream_t st);
void rgk_objects(const RgState *S, const RgConfig *c, uint32_t kinds, uint32_t mode, int cap, int16_t *table, int32_t *count, hipStream_t st);
// rg_episode.hip, rg_novelty.hip (librogue_gym_novelty.so)
void rgk_episode(const RgState *S, const RgConfig *c, const RgEpisode *A, int slots, const int32_t *ids, const uint8_t *mask, int cut, int record, uint32_t serial,
                 hipStream_t st);
void rgk_novelty(const RgState *S, const RgConfig *c, const RgNovelty *A, int slots, const int32_t *ids, const uint8_t *mask, int cut, hipStream_t st);
const char *rgk_novelty_build_id(void);
// rg_state_io.hip
void rgk_state_save(const RgState *S, const RgIoLayout *L, const uint64_t *desc, const uint32_t *guard, const int32_t *ids, int k, uint8_t *out, hipStream_t st);
void rgk_state_load(const RgState *S, const RgIoLayout *L, const uint64_t *desc, const uint32_t *guard, const int32_t *ids, int k, const uint8_t *recs, uint32_t rec_bytes, uint8_t *ok,
                    uint8_t *mark, hipStream_t st);
void rgk_state_stairs(const RgState *S, const RgIoLayout *L, uint8_t *mark, hipStream_t st);
// rg_archive.hip (librogue_gym_archive.so)
void rgk_archive_update(const RgState *S, const RgIoLayout *L, const uint64_t *desc, const uint32_t *guard, const RgArchive *A, const uint64_t *key, const int32_t *score,
                        const uint8_t *mask, uint32_t serial, hipStream_t st);
void rgk_archive_gather(const RgArchive *A, const int32_t *sid, int k, uint8_t *out, hipStream_t st);
void rgk_archive_chosen(const RgArchive *A, const int32_t *sid, int k, const uint8_t *ok, hipStream_t st);
const char *rgk_archive_build_id(void);
// rg_obs_fix.hip (librogue_gym_obsfix.so)
int rgk_obs_fix_blocks(int n);
void rgk_obs_fix(const RgState *S, const RgConfig *c, float *out, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
const char *rgk_obs_fix_build_id(void);
// rg_step_enc.hip (librogue_gym_stepenc.so)
int rgk_step_enc_capable(const RgConfig *c);
int rgk_step_enc_takes(const RgState *S, int use_spares, int parity);
void rgk_step_enc(const RgState *S, const RgState *SP_dev, const RgConfig *c, const uint8_t *keys, int use_spares, int stage_off, int epw, int parity, int blocks, size_t smem,
                  hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
const char *rgk_step_enc_build_id(void);
}
