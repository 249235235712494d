// rg_readers_host.h -- the readers of game state on the CPU: the argument checks that the device entry points (rg_api_*.cpp) share with the *_host twins, and the
// twins themselves (rgh_*; rg_action_mask_host, rg_act_host, rg_policy_eval_host, rg_policy_grad_host, rg_path_host, rg_route_host, rg_monsters_host, rg_objects_host, rg_scout_host, rg_novelty_hash_host and
// rg_novelty_insert_host are one-line delegations in rg_api_readers.cpp).  Host only and header only: plain C++ over a u16 grid and the rule headers' pieces -- no handle, no stream, no HIP call -- so a stand-alone program
// (tests/readers_host_main.cpp) runs this source under sanitizers.  Every refusal goes into `err`, the entry's name its prefix, before anything is written.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rg_action_mask.h"
#include "rg_path.h"
#include "rg_route.h"
#include "rg_objects.h"
#include "rg_monsters.h"
#include "rg_episode.h"
#include "rg_novelty.h"
#include "rg_policy.h"  // (last: it switches floating-point contraction off for what follows)
#include "rg_policy_grad.h"
#include "rg_returns.h"

// ---- the argument checks: `what` is the entry's name ----
static inline int grid_check(std::string &err, const char *what, const uint16_t *cells, int height, int width) {
    const std::string w = std::string(what) + ": ";
    if (!cells) { err = w + "cells must not be NULL"; return 1; }
    if (height < 1 || width < 1 || height > RG_MAX_H || width > RG_MAX_W) {
        err = w + "height, width must satisfy 1 <= height <= " + std::to_string(RG_MAX_H) + " and 1 <= width <= " + std::to_string(RG_MAX_W) + ", got (" + std::to_string(height) +
              ", " + std::to_string(width) + ")";
        return 1;
    }
    return 0;
}
static inline int player_check(std::string &err, const char *what, int px, int py, int height, int width) {
    if (px < 0 || py < 0 || px >= width || py >= height) {
        err = std::string(what) + ": the player's cell (px, py) = (" + std::to_string(px) + ", " + std::to_string(py) + ") is outside the " + std::to_string(width) + " x " +
              std::to_string(height) + " grid";
        return 1;
    }
    return 0;
}
// the key list of a mask call; on success `list` holds the n_keys keys the call judges (NULL keys: RG_ACTION_KEYS)
static inline int mask_keys_check(std::string &err, const char *what, const uint8_t *keys, int &n_keys, uint8_t list[RG_MASK_MAX_KEYS]) {
    const std::string w = std::string(what) + ": ";
    if (!keys) { keys = reinterpret_cast<const uint8_t *>(RG_ACTION_KEYS); n_keys = (int)(sizeof(RG_ACTION_KEYS) - 1); }
    if (n_keys < 1 || n_keys > RG_MASK_MAX_KEYS) { err = w + "n_keys must satisfy 1 <= n_keys <= " + std::to_string(RG_MASK_MAX_KEYS) + ", got " + std::to_string(n_keys); return 1; }
    for (int k = 0; k < n_keys; k++) {
        if (rg_key_bit(keys[k]) == RG_LB_NONE) {
            char hex[8];
            snprintf(hex, sizeof hex, "0x%02x", keys[k]);
            err = w + "keys[" + std::to_string(k) + "] = " + hex + (keys[k] >= 0x20 && keys[k] < 0x7f ? " ('" + std::string(1, (char)keys[k]) + "')" : std::string()) +
                  " is not a key of KeyMap::ai (input.rs:73-100)";
            return 1;
        }
        list[k] = keys[k];
    }
    return 0;
}
static inline int path_goals_check(std::string &err, const char *what, uint32_t goals) {
    if (goals == 0 || (goals & ~RG_PATH_GOALS_ALL)) {
        err = std::string(what) + ": goals must be a non-empty OR of RG_GOAL_STAIRS (1), RG_GOAL_GOLD (2) and RG_GOAL_CELL (4), got " + std::to_string(goals);
        return 1;
    }
    return 0;
}
static inline int route_args_check(std::string &err, const char *what, uint32_t goals, uint32_t fallback, uint32_t mode, bool have_cells, const char *cells_name) {
    const std::string w = std::string(what) + ": ";
    if (goals == 0 || (goals & ~RG_ROUTE_GOALS_ALL)) {
        err = w + "goals must be a non-empty OR of RG_GOAL_STAIRS (1), RG_GOAL_GOLD (2), RG_GOAL_CELL (4) and RG_GOAL_FRONTIER (8), got " + std::to_string(goals);
        return 1;
    }
    if (fallback & ~RG_ROUTE_GOALS_ALL) {
        err = w + "fallback_goals must be 0 or an OR of RG_GOAL_STAIRS (1), RG_GOAL_GOLD (2), RG_GOAL_CELL (4) and RG_GOAL_FRONTIER (8), got " + std::to_string(fallback);
        return 1;
    }
    if (mode & ~RG_ROUTE_MODE_ALL) { err = w + "mode must be an OR of RG_ROUTE_SECRETS (1) and RG_ROUTE_KNOWN (2), got " + std::to_string(mode); return 1; }
    if (((goals | fallback) & RG_GOAL_FRONTIER) && !(mode & RG_ROUTE_KNOWN)) {
        err = w + "RG_GOAL_FRONTIER in " + ((goals & RG_GOAL_FRONTIER) ? "goals" : "fallback_goals") + " needs RG_ROUTE_KNOWN in mode (the frontier is of the player's own map), got mode " +
              std::to_string(mode);
        return 1;
    }
    if (((goals | fallback) & RG_GOAL_CELL) && !have_cells) {
        err = w + cells_name + " is NULL and " + ((goals & RG_GOAL_CELL) ? "goals" : "fallback_goals") + " has RG_GOAL_CELL";
        return 1;
    }
    return 0;
}
static inline int mon_args_check(std::string &err, const char *what, uint32_t mode, int cap, bool have_table, bool have_threat, const char *table_name, const char *threat_name) {
    const std::string w = std::string(what) + ": ";
    if (mode != RG_MON_SHOWN && mode != RG_MON_ALL) { err = w + "mode must be RG_MON_SHOWN (0) or RG_MON_ALL (1), got " + std::to_string(mode); return 1; }
    if (!have_table && !have_threat) { err = w + table_name + " and " + threat_name + " are both NULL"; return 1; }
    if (have_table && (cap < 1 || cap > RG_MON_MAX_CAP)) { err = w + "cap must satisfy 1 <= cap <= " + std::to_string(RG_MON_MAX_CAP) + ", got " + std::to_string(cap); return 1; }
    return 0;
}
static inline int obj_args_check(std::string &err, const char *what, uint32_t kinds, uint32_t mode, int cap, bool have_table, bool have_count, const char *table_name, const char *count_name) {
    const std::string w = std::string(what) + ": ";
    if (kinds == 0 || (kinds & ~RG_OBJ_KINDS_ALL)) {
        err = w + "kinds must be a non-empty OR of RG_OBJ_STAIRS (1), RG_OBJ_GOLD (2), RG_OBJ_DOOR (4) and RG_OBJ_FRONTIER (8), got " + std::to_string(kinds);
        return 1;
    }
    if (mode & ~RG_ROUTE_MODE_ALL) { err = w + "mode must be an OR of RG_ROUTE_SECRETS (1) and RG_ROUTE_KNOWN (2), got " + std::to_string(mode); return 1; }
    if ((kinds & RG_OBJ_FRONTIER) && !(mode & RG_ROUTE_KNOWN)) {
        err = w + "RG_OBJ_FRONTIER in kinds needs RG_ROUTE_KNOWN in mode (the frontier is of the player's own map), got mode " + std::to_string(mode);
        return 1;
    }
    if (!have_table && !have_count) { err = w + table_name + " and " + count_name + " are both NULL"; return 1; }
    if (have_table && (cap < 1 || cap > RG_OBJ_MAX_CAP)) { err = w + "cap must satisfy 1 <= cap <= " + std::to_string(RG_OBJ_MAX_CAP) + ", got " + std::to_string(cap); return 1; }
    return 0;
}
// the env-id list of a cut, a partial reset, a save / load or rg_seed_envs: k ids of [0, n); unique: none of them twice, so k <= n.  ids == NULL (the list lives on
// the device): only k is judged
static inline int rgh_env_ids_check(std::string &err, const char *what, const int32_t *ids, int k, int n, bool unique) {
    const std::string w = std::string(what) + ": ";
    if (k < 0 || (unique && k > n)) { err = w + "k = " + std::to_string(k) + " env_ids for " + std::to_string(n) + " envs"; return 1; }
    if (!ids) return 0;
    std::vector<uint8_t> seen(unique ? (size_t)n : 0, 0);
    for (int i = 0; i < k; i++) {
        const int32_t e = ids[i];
        if (e < 0 || e >= n) { err = w + "env_ids[" + std::to_string(i) + "] = " + std::to_string(e) + " out of range [0, " + std::to_string(n) + ")"; return 1; }
        if (!unique) continue;
        if (seen[e]) { err = w + "env_ids holds " + std::to_string(e) + " twice"; return 1; }
        seen[e] = 1;
    }
    return 0;
}

// ---- the grid search of the path, route and objects twins ----
// A plain FIFO search over the eight moves of rg_path_dx / rg_path_dy: on return D[i] is the number of moves between cell i and the nearest cell that
// source(i) names, RG_PATH_INF where there is none.  The step from the popped cell b in direction d reaches a = b - d; the corner rule of a diagonal names the
// same two cells, (ay, bx) and (by, ax), from either end of the move, so one loop searches towards the sources (path, route) and away from them (objects).
// visit(b): called as a cell is popped, false ends the search; expand(b): the popped cell may be stepped from (a source is in the queue whatever its word);
// enter(a): a neighbour without a distance may get one; corner(i): what a diagonal asks of each of its two corner cells.
template <class Source, class Expand, class Enter, class Corner, class Visit>
static inline void rg_grid_search(int H, int W, std::vector<uint16_t> &D, Source source, Expand expand, Enter enter, Corner corner, Visit visit) {
    std::vector<int> fifo;
    fifo.reserve((size_t)H * W);
    D.assign((size_t)H * W, (uint16_t)RG_PATH_INF);
    for (int i = 0; i < H * W; i++)
        if (source(i)) { D[i] = 0; fifo.push_back(i); }
    for (size_t head = 0; head < fifo.size(); head++) {
        const int b = fifo[head], bx = b % W, by = b / W;
        if (!visit(b)) return;
        if (!expand(b)) continue;
        for (int d = 0; d < 8; d++) {
            const int dx = rg_path_dx(d), dy = rg_path_dy(d), ax = bx - dx, ay = by - dy;
            if (ax < 0 || ay < 0 || ax >= W || ay >= H) continue;
            const int a = ay * W + ax;
            if (D[a] != RG_PATH_INF || !enter(a)) continue;
            if (dx != 0 && dy != 0 && !(corner(ay * W + bx) && corner(by * W + ax))) continue;
            D[a] = (uint16_t)(D[b] + 1);
            fifo.push_back(a);
        }
    }
}
// rg_route_frontier's unknown_beside for cell i: some in-grid orthogonal neighbour is not on the player's map; pi = the player's cell
static inline bool rg_unknown_beside(const uint16_t *cells, int H, int W, int pi, int i) {
    const int x = i % W, y = i / W;
    auto unknown_at = [&](int x, int y) { return x >= 0 && y >= 0 && x < W && y < H && !rg_route_known(cells[y * W + x], y * W + x == pi); };
    return unknown_at(x - 1, y) || unknown_at(x + 1, y) || unknown_at(x, y - 1) || unknown_at(x, y + 1);
}

// ---- the twins ----
static inline int rgh_action_mask(std::string &err, const uint16_t *cells, int height, int width, int px, int py, int dead, const uint8_t *keys, int n_keys, uint8_t *out) {
    uint8_t list[RG_MASK_MAX_KEYS];
    if (mask_keys_check(err, "rg_action_mask_host", keys, n_keys, list)) return 1;
    if (!cells || !out) { err = "rg_action_mask_host: cells and out must not be NULL"; return 1; }
    if (player_check(err, "rg_action_mask_host", px, py, height, width)) return 1;  // (an empty grid has no cell inside it: the same refusal)
    for (int k = 0; k < n_keys; k++) out[k] = (uint8_t)rg_key_legal(cells, height, width, px, py, dead, list[k]);
    return 0;
}
// the options of an act call (rg_policy.h), shared by rg_act and rg_act_host
static inline int act_opts_check(std::string &err, const char *what, const rg_act_opts *o, int dtype, bool have_teacher, bool have_given, bool have_key, const char *teacher_name,
                                 const char *given_name, const char *key_name) {
    const std::string w = std::string(what) + ": ";
    if (dtype != RG_OBS_F32 && dtype != RG_OBS_F16 && dtype != RG_OBS_BF16) {
        err = w + "dtype must be RG_OBS_F32 (0), RG_OBS_F16 (1) or RG_OBS_BF16 (2), got " + std::to_string(dtype);
        return 1;
    }
    if (!o) { err = w + "opts must not be NULL"; return 1; }
    if (o->mode > RG_ACT_GIVEN) { err = w + "opts.mode must be RG_ACT_SAMPLE (0), RG_ACT_GREEDY (1) or RG_ACT_GIVEN (2), got " + std::to_string(o->mode); return 1; }
    if (!(o->inv_temp > 0.0f) || !(o->inv_temp <= 3.4028234663852886e38f)) { err = w + "opts.inv_temp must be finite and > 0, got " + std::to_string(o->inv_temp); return 1; }
    if (!(o->epsilon >= 0.0f && o->epsilon <= 1.0f)) { err = w + "opts.epsilon must lie in [0, 1], got " + std::to_string(o->epsilon); return 1; }
    if (!(o->beta >= 0.0f && o->beta <= 1.0f)) { err = w + "opts.beta must lie in [0, 1], got " + std::to_string(o->beta); return 1; }
    if (o->epsilon + o->beta > 1.0f) { err = w + "opts.epsilon + opts.beta must not exceed 1, got " + std::to_string(o->epsilon) + " + " + std::to_string(o->beta); return 1; }
    if (o->beta > 0.0f && !have_teacher) { err = w + "opts.beta > 0 needs a teacher: " + teacher_name + " is not given"; return 1; }
    if (o->mode == RG_ACT_GIVEN && !have_given) { err = w + "RG_ACT_GIVEN needs " + given_name; return 1; }
    if (o->mode != RG_ACT_GIVEN && !have_key) { err = w + key_name + " must not be NULL in a mode that draws"; return 1; }
    return 0;
}
// teacher_key / given: < 0 = none.  Every output may be NULL except `key` in a mode that draws.
static inline int rgh_act(std::string &err, const uint16_t *cells, int height, int width, int px, int py, int dead, const uint8_t *keys, int n_keys, const void *logits, int dtype,
                          const rg_act_opts *opts, uint32_t env, int teacher_key, int given, uint8_t *key, int32_t *action, float *logp, float *entropy, uint8_t *source) {
    uint8_t list[RG_MASK_MAX_KEYS];
    if (mask_keys_check(err, "rg_act_host", keys, n_keys, list)) return 1;
    if (act_opts_check(err, "rg_act_host", opts, dtype, teacher_key >= 0, opts && opts->mode == RG_ACT_GIVEN, key != nullptr, "teacher_key", "given", "key")) return 1;
    if (!cells || !logits) { err = "rg_act_host: cells and logits must not be NULL"; return 1; }
    if (player_check(err, "rg_act_host", px, py, height, width)) return 1;
    const uint32_t bits = rg_legal_bits(cells, height, width, px, py, dead);
    uint32_t row = 0;
    int teacher = -1;
    for (int k = n_keys - 1; k >= 0; k--) {
        row |= ((bits >> rg_key_bit(list[k])) & 1u) << k;
        if ((int)list[k] == teacher_key) teacher = k;  // (its first position)
    }
    const RgActOut r = rg_act_rule(row, n_keys, [=](int k) { return rg_pol_load(logits, k, dtype); }, *opts, env, teacher, given);
    if (key) *key = list[r.action >= 0 && r.action < n_keys ? r.action : 0];
    if (action) *action = r.action;
    if (logp) *logp = r.logp;
    if (entropy) *entropy = r.entropy;
    if (source) *source = (uint8_t)r.source;
    return 0;
}
// the arguments of the learner's entries (rg_policy_grad.h), shared by rg_policy_eval / rg_policy_grad and their host twins; sfx: "_dev" or ""
static inline int pg_args_check(std::string &err, const char *what, const char *sfx, int64_t n_rows, int n_keys, const void *logits, int dtype, const int32_t *action, float inv_temp,
                                bool wants_dlogits, const void *dlogits) {
    const std::string w = std::string(what) + ": ";
    if (n_rows < 0) { err = w + "n_rows must not be negative, got " + std::to_string(n_rows); return 1; }
    if (n_rows > (int64_t)0x7fffffff * 64) { err = w + "n_rows must not exceed 2^37 - 64, got " + std::to_string(n_rows); return 1; }
    if (n_keys < 1 || n_keys > RG_MASK_MAX_KEYS) { err = w + "n_keys must lie in 1.." + std::to_string(RG_MASK_MAX_KEYS) + ", got " + std::to_string(n_keys); return 1; }
    if (dtype != RG_OBS_F32 && dtype != RG_OBS_F16 && dtype != RG_OBS_BF16) {
        err = w + "dtype must be RG_OBS_F32 (0), RG_OBS_F16 (1) or RG_OBS_BF16 (2), got " + std::to_string(dtype);
        return 1;
    }
    if (!(inv_temp > 0.0f) || !(inv_temp <= 3.4028234663852886e38f)) { err = w + "inv_temp must be finite and > 0, got " + std::to_string(inv_temp); return 1; }
    if (!logits) { err = w + "logits" + sfx + " must not be NULL"; return 1; }
    if (!action) { err = w + "action" + sfx + " must not be NULL"; return 1; }
    if (wants_dlogits && !dlogits) { err = w + "dlogits" + sfx + " must not be NULL"; return 1; }
    return 0;
}
// the legal word of row r: a mask byte counts as != 0; no mask = every key
static inline uint32_t pg_host_row(const uint8_t *mask, int64_t r, int n_keys) {
    if (!mask) return rg_pg_all(n_keys);
    uint32_t row = 0;
    for (int k = 0; k < n_keys; k++) row |= (mask[r * n_keys + k] != 0 ? 1u : 0u) << k;
    return row;
}
static inline int rgh_policy_eval(std::string &err, int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp,
                                  float *logp, float *entropy) {
    if (pg_args_check(err, "rg_policy_eval_host", "", n_rows, n_keys, logits, dtype, action, inv_temp, false, nullptr)) return 1;
    const size_t esz = dtype == RG_OBS_F32 ? 4 : 2;
    for (int64_t r = 0; r < n_rows; r++) {
        const void *x = static_cast<const uint8_t *>(logits) + (size_t)r * n_keys * esz;
        const RgPgOut o = rg_pg_eval_rule(pg_host_row(mask, r, n_keys), n_keys, [=](int k) { return rg_pol_load(x, k, dtype); }, inv_temp, action[r]);
        if (logp) logp[r] = o.logp;
        if (entropy) entropy[r] = o.entropy;
    }
    return 0;
}
static inline int rgh_policy_grad(std::string &err, int64_t n_rows, int n_keys, const void *logits, int dtype, const uint8_t *mask, const int32_t *action, float inv_temp,
                                  const float *g_logp, const float *g_entropy, void *dlogits) {
    if (pg_args_check(err, "rg_policy_grad_host", "", n_rows, n_keys, logits, dtype, action, inv_temp, true, dlogits)) return 1;
    const size_t esz = dtype == RG_OBS_F32 ? 4 : 2;
    for (int64_t r = 0; r < n_rows; r++) {
        const void *x = static_cast<const uint8_t *>(logits) + (size_t)r * n_keys * esz;
        void *out = static_cast<uint8_t *>(dlogits) + (size_t)r * n_keys * esz;
        rg_pg_grad_rule(pg_host_row(mask, r, n_keys), n_keys, [=](int k) { return rg_pol_load(x, k, dtype); }, inv_temp, action[r], g_logp != nullptr, g_logp ? g_logp[r] : 0.0f,
                        g_entropy != nullptr, g_entropy ? g_entropy[r] : 0.0f, [=](int k, float v) {
                            if (dtype == RG_OBS_F32) static_cast<float *>(out)[k] = v;
                            else static_cast<uint16_t *>(out)[k] = (uint16_t)rg_pol_narrow(v, dtype);
                        });
    }
    return 0;
}
// the arguments of the returns entries (rg_returns.h), shared by rg_gae / rg_vtrace and their host twins.  vt: the V-trace entry (value and the two
// log-probability rows required, bars = rho_bar, c_bar, pg_rho_bar; outputs vs and pg_adv); else GAE (outputs adv and ret).
static inline int ret_args_check(std::string &err, const char *what, bool vt, int64_t n_steps, int64_t n_envs, const float *lb, const float *lt, const float *reward,
                                 const float *value, const float *last_value, const uint8_t *done, const uint8_t *trunc, const float *trunc_value, float gamma, float lam,
                                 const float *bars, const float *out_a, const float *out_b) {
    const std::string w = std::string(what) + ": ";
    const char *na = vt ? "vs" : "adv", *nb = vt ? "pg_adv" : "ret";
    const float fmax = 3.4028234663852886e38f;
    if (n_steps < 0) { err = w + "n_steps must not be negative, got " + std::to_string(n_steps); return 1; }
    if (n_envs < 0) { err = w + "n_envs must not be negative, got " + std::to_string(n_envs); return 1; }
    if (n_envs > (int64_t)0x7fffffff * 64) { err = w + "n_envs must not exceed 2^37 - 64, got " + std::to_string(n_envs); return 1; }
    if (n_envs > 0 && n_steps > ((int64_t)1 << 60) / n_envs) { err = w + "n_steps * n_envs must not exceed 2^60, got n_steps " + std::to_string(n_steps); return 1; }
    if (!reward) { err = w + "reward must not be NULL"; return 1; }
    if (vt && !value) { err = w + "value must not be NULL"; return 1; }
    if (vt && !lb) { err = w + "logp_behaviour must not be NULL"; return 1; }
    if (vt && !lt) { err = w + "logp_target must not be NULL"; return 1; }
    if (!out_a && !out_b) { err = w + na + " and " + nb + " are both NULL"; return 1; }
    if (!(gamma >= 0.0f && gamma <= 1.0f)) { err = w + "gamma must lie in [0, 1], got " + std::to_string(gamma); return 1; }
    if (!(lam >= 0.0f && lam <= 1.0f)) { err = w + "lam must lie in [0, 1], got " + std::to_string(lam); return 1; }
    if (vt) {
        const char *bn[3] = {"rho_bar", "c_bar", "pg_rho_bar"};
        for (int i = 0; i < 3; i++)
            if (!(bars[i] > 0.0f && bars[i] <= fmax)) { err = w + bn[i] + " must be finite and > 0, got " + std::to_string(bars[i]); return 1; }
    }
    if (trunc_value && !trunc) { err = w + "trunc_value without trunc"; return 1; }
    // an output may be exactly one of the [T, N] float arrays, and overlap nothing in any other way
    const uint64_t cells = (uint64_t)n_steps * (uint64_t)n_envs;
    struct Span { const char *name; const void *p; uint64_t bytes; };
    const Span in[] = {{"reward", reward, cells * 4}, {"value", value, cells * 4}, {"last_value", last_value, (uint64_t)n_envs * 4}, {"done", done, cells},
                       {"trunc", trunc, cells}, {"trunc_value", trunc_value, cells * 4}, {"logp_behaviour", vt ? lb : nullptr, cells * 4},
                       {"logp_target", vt ? lt : nullptr, cells * 4}, {na, out_a, cells * 4}};
    const Span out[] = {{na, out_a, cells * 4}, {nb, out_b, cells * 4}};
    for (int o = 0; o < 2; o++)
        for (const Span &i : in) {
            if (!out[o].p || !i.p) continue;
            if (o == 0 && &i == &in[8]) continue;                              // (the first output against itself)
            if (i.p == out[o].p && i.bytes == out[o].bytes) continue;          // the exact alias
            const uintptr_t a0 = (uintptr_t)out[o].p, b0 = (uintptr_t)i.p;
            if (a0 < b0 + i.bytes && b0 < a0 + out[o].bytes) {
                err = w + out[o].name + " overlaps " + i.name + " (an output may be exactly one of the [n_steps, n_envs] float arrays, nothing else)";
                return 1;
            }
        }
    return 0;
}
static inline float ret_gl(float gamma, float lam) { return gamma * lam; }
// the three bars and ln_bar = (float)log((double)bar) of each, as the launcher and the twin take them
static inline void ret_bars(float rho_bar, float c_bar, float pg_rho_bar, float out[6]) {
    out[0] = rho_bar; out[1] = c_bar; out[2] = pg_rho_bar;
    for (int i = 0; i < 3; i++) out[3 + i] = (float)std::log((double)out[i]);
}
static inline RgRetRow ret_host_row(int64_t at, const float *reward, const float *value, const uint8_t *done, const uint8_t *trunc, const float *trunc_value) {
    const bool tv = trunc && trunc_value;
    return {reward[at], value ? value[at] : 0.0f, tv ? trunc_value[at] : 0.0f, done && done[at] != 0, trunc && trunc[at] != 0, tv};
}
static inline int rgh_gae(std::string &err, int64_t n_steps, int64_t n_envs, const float *reward, const float *value, const float *last_value, const uint8_t *done,
                          const uint8_t *trunc, const float *trunc_value, float gamma, float lam, float *adv, float *ret) {
    if (ret_args_check(err, "rg_gae_host", false, n_steps, n_envs, nullptr, nullptr, reward, value, last_value, done, trunc, trunc_value, gamma, lam, nullptr, adv, ret)) return 1;
    const float gl = ret_gl(gamma, lam);
    for (int64_t n = 0; n < n_envs; n++) {
        RgGaeState s = {0.0f, last_value ? last_value[n] : 0.0f};
        for (int64_t t = n_steps - 1; t >= 0; t--) {
            const int64_t at = t * n_envs + n;
            const RgRetPair o = rg_gae_step(s, ret_host_row(at, reward, value, done, trunc, trunc_value), gamma, gl);   // (the row is read before anything is written)
            if (adv) adv[at] = o.a;
            if (ret) ret[at] = o.b;
        }
    }
    return 0;
}
static inline int rgh_vtrace(std::string &err, int64_t n_steps, int64_t n_envs, const float *logp_behaviour, const float *logp_target, const float *reward, const float *value,
                             const float *last_value, const uint8_t *done, const uint8_t *trunc, const float *trunc_value, float gamma, float lam, float rho_bar, float c_bar,
                             float pg_rho_bar, float *vs, float *pg_adv) {
    const float raw[3] = {rho_bar, c_bar, pg_rho_bar};
    if (ret_args_check(err, "rg_vtrace_host", true, n_steps, n_envs, logp_behaviour, logp_target, reward, value, last_value, done, trunc, trunc_value, gamma, lam, raw, vs, pg_adv))
        return 1;
    float b[6];
    ret_bars(rho_bar, c_bar, pg_rho_bar, b);
    const RgVtBars bars = {b[0], b[1], b[2], b[3], b[4], b[5]};
    for (int64_t n = 0; n < n_envs; n++) {
        const float lv = last_value ? last_value[n] : 0.0f;
        RgVtState s = {0.0f, lv, lv};
        for (int64_t t = n_steps - 1; t >= 0; t--) {
            const int64_t at = t * n_envs + n;
            const float lb = logp_behaviour[at], lt = logp_target[at];
            const RgRetPair o = rg_vtrace_step(s, ret_host_row(at, reward, value, done, trunc, trunc_value), lb, lt, gamma, lam, bars);
            if (vs) vs[at] = o.a;
            if (pg_adv) pg_adv[at] = o.b;
        }
    }
    return 0;
}
// The search runs from the goal cells over rg_path.h's pieces: rg_can_move(a -> b) taken apart into its target (expand), its start (enter) and its corners.
static inline int rgh_path(std::string &err, const uint16_t *cells, int height, int width, int px, int py, int dead, uint32_t goals, int cell_y, int cell_x, uint16_t *field_out,
                           int32_t *dist_out, uint8_t *key_out) {
    if (path_goals_check(err, "rg_path_host", goals)) return 1;
    if (!field_out && !dist_out && !key_out) { err = "rg_path_host: field_out, dist_out and key_out are all NULL"; return 1; }
    if (grid_check(err, "rg_path_host", cells, height, width) || player_check(err, "rg_path_host", px, py, height, width)) return 1;
    const int hw = height * width;
    std::vector<uint16_t> D;
    auto goal = [&](int i) { return rg_path_goal(cells[i], goals, i == py * width + px, i % width == cell_x && i / width == cell_y); };
    auto ok = [&](int i) { return rg_path_ok(cells[i]); };  // (a goal nobody can step onto is not expanded)
    rg_grid_search(height, width, D, goal, ok, ok, [&](int i) { return rg_walkable(cells[i]); }, [](int) { return true; });
    const uint32_t dp = D[py * width + px];
    uint32_t dirs = 0;
    if (dp != 0 && dp != RG_PATH_INF)
        for (int d = 0; d < 8; d++) {
            const int dx = rg_path_dx(d), dy = rg_path_dy(d);
            if (rg_can_move(cells, height, width, px, py, dx, dy) && D[(py + dy) * width + px + dx] == dp - 1) dirs |= 1u << d;
        }
    if (field_out) memcpy(field_out, D.data(), (size_t)hw * sizeof(uint16_t));
    if (dist_out) *dist_out = rg_path_dist(dp);
    if (key_out) *key_out = rg_path_key(dead, dp, (goals & RG_GOAL_STAIRS) && (cells[py * width + px] & C_SURF_MASK) == S_STAIR, dirs);
    return 0;
}
// One search per tier over rg_route.h's pieces, from the tier's goal cells.
static inline int rgh_route(std::string &err, const uint16_t *cells, int height, int width, int px, int py, int dead, uint32_t goals, uint32_t fallback_goals, uint32_t mode,
                            int cell_y, int cell_x, uint16_t *field_out, int32_t *dist_out, uint8_t *key_out, uint8_t *tier_out) {
    if (route_args_check(err, "rg_route_host", goals, fallback_goals, mode, true, "cells")) return 1;
    if (!field_out && !dist_out && !key_out && !tier_out) { err = "rg_route_host: field_out, dist_out, key_out and tier_out are all NULL"; return 1; }
    if (grid_check(err, "rg_route_host", cells, height, width) || player_check(err, "rg_route_host", px, py, height, width)) return 1;
    const int hw = height * width, pi = py * width + px;
    auto frontier_at = [&](int i) { return rg_route_frontier(cells[i], mode, i == pi, rg_unknown_beside(cells, height, width, pi, i)); };
    auto pass = [&](int i) { return rg_route_pass(cells[i], mode, i == pi); };  // (a goal nobody can step onto is not expanded)
    auto corner = [&](int i) { return rg_route_corner(cells[i], mode, i == pi); };
    std::vector<uint16_t> D;
    uint32_t dp = RG_PATH_INF, tier = RG_ROUTE_NO_TIER, gw = goals;
    for (uint32_t t = 0; t < 2 && tier == RG_ROUTE_NO_TIER; t++) {
        if (t && !fallback_goals) break;
        gw = t ? fallback_goals : goals;
        auto goal = [&](int i) {
            return rg_route_goal(cells[i], gw, mode, i == pi, i % width == cell_x && i / width == cell_y) || ((gw & RG_GOAL_FRONTIER) && frontier_at(i));
        };
        // (without field_out the search ends once the player's cell has its distance: every cell one move closer has its own by then)
        rg_grid_search(height, width, D, goal, pass, pass, corner, [&](int) { return field_out || D[pi] == RG_PATH_INF; });
        dp = D[pi];
        if (dp != RG_PATH_INF) tier = t;
    }
    uint32_t dirs = 0;
    if (dp != 0 && dp != RG_PATH_INF)
        for (int d = 0; d < 8; d++) {
            const int dx = rg_path_dx(d), dy = rg_path_dy(d), x = px + dx, y = py + dy;
            if (x < 0 || y < 0 || x >= width || y >= height) continue;
            const uint32_t t = cells[y * width + x];
            bool ok = rg_route_pass(t, mode, false) && !rg_route_secret(t) && D[y * width + x] == dp - 1;
            if (dx != 0 && dy != 0) ok = ok && rg_route_corner(cells[py * width + x], mode, false) && rg_route_corner(cells[y * width + px], mode, false);
            dirs |= (uint32_t)ok << d;
        }
    if (field_out) memcpy(field_out, D.data(), (size_t)hw * sizeof(uint16_t));
    if (dist_out) *dist_out = rg_path_dist(dp);
    if (key_out) *key_out = rg_route_key(dead, dp, gw, (cells[pi] & C_SURF_MASK) == S_STAIR, (gw & RG_GOAL_FRONTIER) && frontier_at(pi), dirs);
    if (tier_out) *tier_out = (uint8_t)tier;
    return 0;
}
// Every qualifier gets its key, the keys are sorted, the first cap become rows: the plain form of what k_monsters keeps in registers.
static inline int rgh_monsters(std::string &err, const uint16_t *cells, int height, int width, int px, int py, int dead, int n_mon, const int32_t *mon_x, const int32_t *mon_y,
                               const int32_t *mon_type, const int32_t *mon_active, const int32_t *mon_hp, const int32_t *mon_alive, int room_num_x, int room_num_y,
                               const uint32_t *room_rect, const int32_t *room_meta, uint32_t mode, int cap, int16_t *table_out, int32_t *threat_out) {
    if (mon_args_check(err, "rg_monsters_host", mode, cap, table_out != nullptr, threat_out != nullptr, "table_out", "threat_out")) return 1;
    if (grid_check(err, "rg_monsters_host", cells, height, width) || player_check(err, "rg_monsters_host", px, py, height, width)) return 1;
    if (n_mon < 0 || n_mon > RG_MAX_ROOMS) { err = "rg_monsters_host: n_mon must satisfy 0 <= n_mon <= " + std::to_string(RG_MAX_ROOMS) + ", got " + std::to_string(n_mon); return 1; }
    if (n_mon > 0 && (!mon_x || !mon_y || !mon_type || !mon_active || !mon_hp)) { err = "rg_monsters_host: mon_x, mon_y, mon_type, mon_active and mon_hp must not be NULL"; return 1; }
    if (room_num_x < 1 || room_num_y < 1 || room_num_x > width || room_num_y > height || room_num_x * room_num_y > RG_MAX_ROOMS) {
        err = "rg_monsters_host: room_num_x, room_num_y = (" + std::to_string(room_num_x) + ", " + std::to_string(room_num_y) + ") do not fit the grid";
        return 1;
    }
    if (!room_rect || !room_meta) { err = "rg_monsters_host: room_rect and room_meta must not be NULL"; return 1; }
    for (int i = 0; i < n_mon; i++) {
        if (mon_alive && !mon_alive[i]) continue;
        if (mon_x[i] < 0 || mon_y[i] < 0 || mon_x[i] >= width || mon_y[i] >= height) {
            err = "rg_monsters_host: monster " + std::to_string(i) + " at (" + std::to_string(mon_x[i]) + ", " + std::to_string(mon_y[i]) + ") is outside the grid";
            return 1;
        }
        if (mon_type[i] < 0 || mon_type[i] > 25) { err = "rg_monsters_host: mon_type[" + std::to_string(i) + "] = " + std::to_string(mon_type[i]) + " is not a tile index 0 .. 25"; return 1; }
    }
    RgMonEnv E = {px, py, height, 0, 0, 0, 0, 0, 0, 0, 0, false, false};
    const int id = rg_mon_area(E, px, py, width, height, room_num_x, room_num_y);
    if (id >= 0) rg_mon_room(E, room_rect[id], (uint32_t)room_meta[id]);
    RgMonThreat T;
    rg_mon_threat_init(T);
    std::vector<std::pair<uint64_t, uint32_t>> list;
    for (int i = 0; i < n_mon && !dead; i++) {
        if (mon_alive && !mon_alive[i]) continue;
        const int x = mon_x[i], y = mon_y[i];
        const bool shown = rg_mon_shown(E, cells[y * width + x], x, y), q = mode == RG_MON_ALL || shown;
        rg_mon_threat_add(T, px, py, x, y, shown, q);
        if (q) list.emplace_back(rg_mon_key(px, py, x, y, shown, i), rg_mon_pay((uint32_t)('A' + mon_type[i]), mon_active[i] != 0, mon_hp[i]));
    }
    std::sort(list.begin(), list.end());
    if (table_out)
        for (int r = 0; r < cap; r++) {
            uint32_t row[4];
            rg_mon_row(r < (int)list.size() ? list[r].first : RG_MON_EMPTY_KEY, r < (int)list.size() ? list[r].second : 0u, px, py, mode, row);
            memcpy(table_out + (size_t)r * RG_MON_COLS, row, 16);
        }
    if (threat_out) { threat_out[0] = T.adjacent; threat_out[1] = T.nearest; threat_out[2] = T.attack; threat_out[3] = T.count; }
    return 0;
}
// One search from the player's cell over rg_route.h's moves, only when a table is asked for: the objects it meets, sorted by (walk, y, x), and the first cap
// of them are the table.
static inline int rgh_objects(std::string &err, const uint16_t *cells, int height, int width, int px, int py, int dead, uint32_t kinds, uint32_t mode, int cap, int16_t *table_out,
                              int32_t *count_out) {
    if (obj_args_check(err, "rg_objects_host", kinds, mode, cap, table_out != nullptr, count_out != nullptr, "table_out", "count_out")) return 1;
    if (grid_check(err, "rg_objects_host", cells, height, width) || player_check(err, "rg_objects_host", px, py, height, width)) return 1;
    const int hw = height * width, pi = py * width + px;
    int32_t count[4] = {0, 0, 0, 0};
    std::vector<std::pair<uint32_t, uint32_t>> list;  // (walk << 16 | y << 8 | x, kind): the order of the table
    if (!dead) {
        std::vector<uint8_t> kind((size_t)hw);
        for (int i = 0; i < hw; i++) {
            kind[i] = (uint8_t)rg_obj_kind(cells[i], kinds, mode, i == pi, rg_unknown_beside(cells, height, width, pi, i));
            for (int k = 0; k < 4; k++) count[k] += (kind[i] >> k) & 1;
        }
        if (table_out) {
            std::vector<uint16_t> D;
            auto listed = [&](int i) { if (kind[i]) list.emplace_back((uint32_t)D[i] << 16 | (uint32_t)(i / width) << 8 | (uint32_t)(i % width), kind[i]); return true; };
            // (the player's own cell starts the search whatever its word; any other cell is in the queue only because it passed)
            rg_grid_search(height, width, D, [&](int i) { return i == pi; }, [](int) { return true; }, [&](int i) { return rg_route_pass(cells[i], mode, i == pi); },
                           [&](int i) { return rg_route_corner(cells[i], mode, i == pi); }, listed);
            std::sort(list.begin(), list.end());
        }
    }
    if (table_out)
        for (int r = 0; r < cap; r++) {
            uint32_t row[4] = {0u, 0u, 0u, 0u};
            if (r < (int)list.size()) rg_obj_row(list[r].second, px, py, (int)(list[r].first & 0xffu), (int)((list[r].first >> 8) & 0xffu), list[r].first >> 16, row);
            memcpy(table_out + (size_t)r * RG_OBJ_COLS, row, 16);
        }
    if (count_out) memcpy(count_out, count, sizeof count);
    return 0;
}
// the scout reward of one step: the cells known for the first time, `seen` advanced
static inline int rgh_scout(std::string &err, const uint16_t *cells, int height, int width, uint8_t *seen_inout, int32_t *fresh_out) {
    if (!cells) { err = "rg_scout_host: cells must not be NULL"; return 1; }
    if (!seen_inout) { err = "rg_scout_host: seen_inout must not be NULL"; return 1; }
    if (grid_check(err, "rg_scout_host", cells, height, width)) return 1;
    const int hw = height * width, sb = rg_ep_seen_bytes(hw);
    int32_t fresh = 0;
    for (int j = 0; j < sb; j++) {
        uint32_t s = seen_inout[j];
        fresh += __builtin_popcount(rg_ep_fresh(rg_ep_known_byte(cells, j, hw, width), s, false) & 0xffu);
        seen_inout[j] = (uint8_t)(s & rg_ep_row_bits(j, hw, width));  // (bits that can never count are written 0, whatever the caller passed)
    }
    if (fresh_out) *fresh_out = fresh;
    return 0;
}
// ---- count-based novelty (rg_novelty.h) ----
// what the enable and the hash twin ask of `what` and the radii; `w` = the entry's name and a colon
static inline int nov_key_check(std::string &err, const std::string &w, int what, int radius_y, int radius_x) {
    if (what != RG_NOV_POS && what != RG_NOV_SCREEN && what != RG_NOV_CROP) {
        err = w + "what must be RG_NOV_POS (1), RG_NOV_SCREEN (2) or RG_NOV_CROP (3), got " + std::to_string(what);
        return 1;
    }
    if (what == RG_NOV_CROP ? (radius_y < 0 || radius_y > RG_MAX_H - 1 || radius_x < 0 || radius_x > RG_MAX_W - 1) : (radius_y != 0 || radius_x != 0)) {
        err = w + (what == RG_NOV_CROP ? "radius_y, radius_x must satisfy 0 <= radius_y <= " + std::to_string(RG_MAX_H - 1) + " and 0 <= radius_x <= " + std::to_string(RG_MAX_W - 1)
                                       : std::string("radius_y, radius_x must be 0 unless what is RG_NOV_CROP")) +
              ", got (" + std::to_string(radius_y) + ", " + std::to_string(radius_x) + ")";
        return 1;
    }
    return 0;
}
// the hash of one screen: the words one after the other
static inline int rgh_nov_hash(std::string &err, int what, int level, int height, int width, const uint8_t *screen, int px, int py, int radius_y, int radius_x, uint64_t *hash) {
    const std::string w = "rg_novelty_hash_host: ";
    if (!screen) { err = w + "screen must not be NULL"; return 1; }
    if (!hash) { err = w + "hash must not be NULL"; return 1; }
    if (height < 3 || width < 1 || height > RG_MAX_H || width > RG_MAX_W) {
        err = w + "height, width must satisfy 3 <= height <= " + std::to_string(RG_MAX_H) + " and 1 <= width <= " + std::to_string(RG_MAX_W) + ", got (" + std::to_string(height) + ", " +
              std::to_string(width) + ")";
        return 1;
    }
    if (level < 0) { err = w + "level must not be negative, got " + std::to_string(level); return 1; }
    if (nov_key_check(err, w, what, radius_y, radius_x) || player_check(err, "rg_novelty_hash_host", px, py, height, width)) return 1;
    const uint32_t L = rg_nov_key_len(what, height, width, radius_y, radius_x), m = (L + 7) / 8;
    uint64_t acc = 0;
    for (uint32_t i = 0; i < m; i++)
        acc += rg_nov_term(what == RG_NOV_POS ? rg_nov_pos_word(px, py) : rg_nov_key_word(what, screen, height, width, px, py, radius_y, radius_x, L, i), i);
    *hash = rg_nov_finish(acc, rg_nov_salt((uint32_t)what, level, L));
    return 0;
}
// the episodic insert on a table in host memory
static inline int rgh_nov_insert(std::string &err, void *slots, int cap, uint32_t gen, uint64_t hash, uint32_t *count) {
    const std::string w = "rg_novelty_insert_host: ";
    if (!slots || ((uintptr_t)slots & 15)) { err = w + "slots must be a non-null, 16-byte aligned pointer"; return 1; }
    if (!count) { err = w + "count must not be NULL"; return 1; }
    if (!rg_nov_pow2_in(cap, 1, RG_NOV_CAP_MAX)) { err = w + "cap must be a power of two, 1 <= cap <= " + std::to_string(RG_NOV_CAP_MAX) + ", got " + std::to_string(cap); return 1; }
    *count = rg_nov_insert(static_cast<RgNovSlot *>(slots), (uint32_t)cap, gen, hash);
    return 0;
}
