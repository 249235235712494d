// rg_api_readers.cpp -- the five readers of game state behind the C-ABI, and every CPU twin's one-line delegation.
#include "rg_handle.h"
#include "rg_launch.h"
#include "rg_readers_host.h"  // the rule headers of the readers of game state, their argument checks and their CPU twins

extern "C" {
// The readers of game state (rg_action_mask, rg_path, rg_route, rg_monsters, rg_objects: the kernel in the .hip unit and the rule in the header of that name, the
// argument checks and the CPU twins rg_*_host in rg_readers_host.h).  launch(leaf) enqueues one kernel on a handle without groups; on a handle with config groups
// every group writes its envs' rows straight into the handle's tensors (RgState::ext), as the crops do.
// Game state only: the pending render is not flushed, mirrors, flag words, a bound observation tensor and the RNG streams stay as they are.
extern "C++" template <class Launch> static int reader_launch(rg_t *h, Launch launch) {
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->sub.empty()) {
        for (rg_handle *sh : h->sub) SUBCHK(h, sh, reader_launch(sh, launch));
        return 0;
    }
    launch(h);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int rg_action_mask(rg_t *h, const uint8_t *keys, int n_keys, uint8_t *mask_dev, uint8_t *sample_dev, uint64_t seed, uint64_t draw) {
    uint8_t list[RG_MASK_MAX_KEYS];
    if (mask_keys_check(h->err, "rg_action_mask", keys, n_keys, list)) return 1;
    if (!mask_dev && !sample_dev) { h->err = "rg_action_mask: mask_dev and sample_dev are both NULL"; return 1; }
    if ((uintptr_t)mask_dev & 15) { h->err = "rg_action_mask: mask_dev must be a 16-byte aligned device pointer"; return 1; }
    return reader_launch(h, [=](rg_t *l) { rgk_action_mask(&l->S, &l->cfg, list, n_keys, mask_dev, sample_dev, seed, draw, l->stream, nullptr, nullptr); });
}
int rg_action_mask_host(const uint16_t *cells, int height, int width, int px, int py, int dead, const uint8_t *keys, int n_keys, uint8_t *out) {
    return rgh_action_mask(g_create_err, cells, height, width, px, py, dead, keys, n_keys, out);
}
uint32_t rg_sample_index(uint64_t seed, uint32_t env, uint64_t draw, uint32_t count) { return rg_sample_index_of(seed, env, draw, count); }
int rg_act(rg_t *h, const uint8_t *keys, int n_keys, const void *logits_dev, int dtype, const rg_act_opts *opts, const uint8_t *teacher_dev, const int32_t *given_dev,
           uint8_t *key_dev, int32_t *action_dev, float *logp_dev, float *entropy_dev, uint8_t *source_dev, uint8_t *mask_dev) {
    uint8_t list[RG_MASK_MAX_KEYS];
    if (mask_keys_check(h->err, "rg_act", keys, n_keys, list)) return 1;
    if (act_opts_check(h->err, "rg_act", opts, dtype, teacher_dev != nullptr, given_dev != nullptr, key_dev != nullptr, "teacher_dev", "given_dev", "key_dev")) return 1;
    if (!logits_dev || ((uintptr_t)logits_dev & 15)) { h->err = "rg_act: logits_dev must be a 16-byte aligned device pointer"; return 1; }
    if ((uintptr_t)mask_dev & 15) { h->err = "rg_act: mask_dev must be a 16-byte aligned device pointer"; return 1; }
    const rg_act_opts o = *opts;
    return reader_launch(h, [=](rg_t *l) {
        rgk_act(&l->S, &l->cfg, list, n_keys, logits_dev, dtype, &o, teacher_dev, given_dev, key_dev, action_dev, logp_dev, entropy_dev, source_dev, mask_dev, l->stream, nullptr, nullptr);
    });
}
int rg_act_host(const uint16_t *cells, int height, int width, int px, int py, int dead, const uint8_t *keys, int n_keys, const void *logits, int dtype, const rg_act_opts *opts,
                uint32_t env, int teacher_key, int given, uint8_t *key, int32_t *action, float *logp, float *entropy, uint8_t *source) {
    return rgh_act(g_create_err, cells, height, width, px, py, dead, keys, n_keys, logits, dtype, opts, env, teacher_key, given, key, action, logp, entropy, source);
}
int rg_path(rg_t *h, uint32_t goals, const int32_t *cells_dev, uint16_t *field_dev, int32_t *dist_dev, uint8_t *key_dev) {
    if (path_goals_check(h->err, "rg_path", goals)) return 1;
    if ((goals & RG_GOAL_CELL) && !cells_dev) { h->err = "rg_path: cells_dev is NULL and goals has RG_GOAL_CELL"; return 1; }
    if (!field_dev && !dist_dev && !key_dev) { h->err = "rg_path: field_dev, dist_dev and key_dev are all NULL"; return 1; }
    if ((uintptr_t)field_dev & 15) { h->err = "rg_path: field_dev must be a 16-byte aligned device pointer"; return 1; }
    if (field_dev && !h->sub.empty()) { h->err = "rg_path: field_dev is refused on a handle with config groups (there is no [n_env][H][W] tensor); dist_dev and key_dev are served"; return 1; }
    return reader_launch(h, [=](rg_t *l) { rgk_path(&l->S, &l->cfg, goals, cells_dev, field_dev, dist_dev, key_dev, l->stream); });
}
int rg_path_host(const uint16_t *cells, int height, int width, int px, int py, int dead, uint32_t goals, int cell_y, int cell_x, uint16_t *field_out, int32_t *dist_out,
                 uint8_t *key_out) {
    return rgh_path(g_create_err, cells, height, width, px, py, dead, goals, cell_y, cell_x, field_out, dist_out, key_out);
}
int rg_route(rg_t *h, uint32_t goals, uint32_t fallback_goals, uint32_t mode, const int32_t *cells_dev, int32_t *dist_dev, uint8_t *key_dev, uint8_t *tier_dev) {
    if (route_args_check(h->err, "rg_route", goals, fallback_goals, mode, cells_dev != nullptr, "cells_dev")) return 1;
    if (!dist_dev && !key_dev && !tier_dev) { h->err = "rg_route: dist_dev, key_dev and tier_dev are all NULL"; return 1; }
    return reader_launch(h, [=](rg_t *l) { rgk_route(&l->S, &l->cfg, goals, fallback_goals, mode, cells_dev, dist_dev, key_dev, tier_dev, l->stream); });
}
int rg_route_host(const uint16_t *cells, int height, int width, int px, int py, int dead, uint32_t goals, uint32_t fallback_goals, uint32_t mode, int cell_y, int cell_x,
                  uint16_t *field_out, int32_t *dist_out, uint8_t *key_out, uint8_t *tier_out) {
    return rgh_route(g_create_err, cells, height, width, px, py, dead, goals, fallback_goals, mode, cell_y, cell_x, field_out, dist_out, key_out, tier_out);
}
int rg_monsters(rg_t *h, uint32_t mode, int cap, int16_t *table_dev, int32_t *threat_dev) {
    if (mon_args_check(h->err, "rg_monsters", mode, cap, table_dev != nullptr, threat_dev != nullptr, "table_dev", "threat_dev")) return 1;
    if (((uintptr_t)table_dev | (uintptr_t)threat_dev) & 15) { h->err = "rg_monsters: table_dev and threat_dev must be 16-byte aligned device pointers"; return 1; }
    return reader_launch(h, [=](rg_t *l) { rgk_monsters(&l->S, &l->cfg, mode, cap, table_dev, threat_dev, l->stream); });
}
int rg_monsters_host(const uint16_t *cells, int height, int width, int px, int py, int dead, int n_mon, const int32_t *mon_x, const int32_t *mon_y, const int32_t *mon_type,
                     const int32_t *mon_active, const int32_t *mon_hp, const int32_t *mon_alive, int room_num_x, int room_num_y, const uint32_t *room_rect,
                     const int32_t *room_meta, uint32_t mode, int cap, int16_t *table_out, int32_t *threat_out) {
    return rgh_monsters(g_create_err, cells, height, width, px, py, dead, n_mon, mon_x, mon_y, mon_type, mon_active, mon_hp, mon_alive, room_num_x, room_num_y, room_rect, room_meta, mode,
                        cap, table_out, threat_out);
}
int rg_objects(rg_t *h, uint32_t kinds, uint32_t mode, int cap, int16_t *table_dev, int32_t *count_dev) {
    if (obj_args_check(h->err, "rg_objects", kinds, mode, cap, table_dev != nullptr, count_dev != nullptr, "table_dev", "count_dev")) return 1;
    if (((uintptr_t)table_dev | (uintptr_t)count_dev) & 15) { h->err = "rg_objects: table_dev and count_dev must be 16-byte aligned device pointers"; return 1; }
    return reader_launch(h, [=](rg_t *l) { rgk_objects(&l->S, &l->cfg, kinds, mode, cap, table_dev, count_dev, l->stream); });
}
int rg_objects_host(const uint16_t *cells, int height, int width, int px, int py, int dead, uint32_t kinds, uint32_t mode, int cap, int16_t *table_out, int32_t *count_out) {
    return rgh_objects(g_create_err, cells, height, width, px, py, dead, kinds, mode, cap, table_out, count_out);
}
int rg_scout_host(const uint16_t *cells, int height, int width, uint8_t *seen_inout, int32_t *fresh_out) {
    return rgh_scout(g_create_err, cells, height, width, seen_inout, fresh_out);
}
int rg_novelty_hash_host(int what, int level, int height, int width, const uint8_t *screen, int px, int py, int radius_y, int radius_x, uint64_t *hash) {
    return rgh_nov_hash(g_create_err, what, level, height, width, screen, px, py, radius_y, radius_x, hash);
}
uint64_t rg_novelty_finish_host(uint64_t acc, uint64_t salt) { return rg_nov_finish(acc, salt); }
int rg_novelty_insert_host(void *slots, int cap, uint32_t gen, uint64_t hash, uint32_t *count) { return rgh_nov_insert(g_create_err, slots, cap, gen, hash, count); }
}  // extern "C"
