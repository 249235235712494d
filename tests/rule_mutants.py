"""The mutants of the product's rule headers (rogue-gym_amd/csrc/rg_policy.h, rg_policy_grad.h, rg_action_mask.h, rg_path.h, rg_route.h, rg_objects.h, rg_monsters.h,
rg_novelty.h and the scout part of rg_episode.h): ONE textual misreading per clause of each header's comment.  The kernels and their CPU twins compile these
headers both, so "kernel equals twin" on the GPU cannot see a wrong rule; what pins the rule is the CPU tests that hold the twin against an independent
statement (float64 chains, Python integers, a Python grid search, grids answered by hand).  kill_matrix() asks which of them notices which mutant.

CPU ONLY.  A mutant is built for the host twins alone (the four host units that include rg_readers_host.h) and run in CPU tests alone: a mutated kernel could
read out of bounds, so none is ever compiled for the device.  Shared by tests/test_rule_mutations.py and tools/rule_pin_map.py."""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rogue-gym_amd")
HOST_UNITS = ("rg_api_readers.cpp", "rg_api_learn.cpp", "rg_api_episode.cpp", "rg_api_state.cpp")     # the units that include rg_readers_host.h
SIDE_LIBS = ("novelty", "archive", "obsfix", "stepenc", "policy", "learn")
# the host test files that hold a header's twin against an independent statement
TESTS = {
    "rg_policy.h": ("test_policy_host.py", "test_policy_grad_host.py"),
    "rg_policy_grad.h": ("test_policy_grad_host.py",),
    "rg_action_mask.h": ("test_action_mask_host.py", "test_constructed_grids_host.py"),
    "rg_path.h": ("test_path_host.py", "test_constructed_grids_host.py"),
    "rg_route.h": ("test_route_host.py", "test_constructed_grids_host.py"),
    # (the hand-answered cases first, so that a pin names an independent hand-written answer where there is one and not a sampled run of 90 s)
    "rg_objects.h": (("test_objects_host.py", "not through_play and not following_the_explorer and not engines_drawing"), "test_constructed_grids_host.py", "test_objects_host.py"),
    "rg_monsters.h": ("test_monsters_host.py", "test_constructed_grids_host.py"),
    "rg_novelty.h": ("test_novelty_host.py",),
    "rg_episode.h": ("test_episode_host.py",),
}
RULE, EQUIVALENT = "rule", "equivalent"


def M(name, header, old, new, clause, cls=RULE, reason=None):
    return dict(name=name, header=header, old=old, new=new, clause=clause, cls=cls, reason=reason)


MUTANTS = [
    # ---- rg_policy.h
    M("draw_ge", "rg_policy.h", "if (c > t) pol = k;", "if (c >= t) pol = k;", "the first legal key whose running sum EXCEEDS t wins"),
    M("beta_le", "rg_policy.h", "if (v < o.beta) {", "if (v <= o.beta) {", "v < beta: the teacher key"),
    M("epsilon_le", "rg_policy.h", "} else if (v < o.beta + o.epsilon) {", "} else if (v <= o.beta + o.epsilon) {", "else v < beta + epsilon: the uniform draw"),
    M("u_low_bit", "rg_policy.h", "(float)(uint32_t)(z >> 40)", "(float)(uint32_t)((z >> 40) & ~1ull)", "bits 63..40: u = field * 2^-24, all 24 bits of it"),
    M("v_field", "rg_policy.h", "(z >> 16) & 0xffffffull", "(z >> 8) & 0xffffffull", "bits 39..16: v"),
    M("uniform_modulo", "rg_policy.h", "(uint32_t)(((z & 0xffffull) * (uint64_t)count) >> 16)", "(uint32_t)((z & 0xffffull) % (uint64_t)count)",
      "bits 15..0: the (field * count >> 16)-th legal key"),
    M("no_stream", "rg_policy.h", "0xD1B54A32D192ED03ull * draw + RG_ACT_STREAM;", "0xD1B54A32D192ED03ull * draw;", "a stream constant of its own (RG_ACT_STREAM)"),
    M("env_plus_0", "rg_policy.h", "((uint64_t)env + 1ull)", "((uint64_t)env)", "z = seed + 0x9E37... * (env + 1) + ..."),
    M("given_flat_source", "rg_policy.h", "        a = given;\n        src = 0u;", "        a = given;", "RG_ACT_GIVEN: ... source 0 (whatever the row)"),
    M("cutoff_120", "rg_policy.h", "if (!(t >= -125.0f)) return 0.0f;", "if (!(t >= -120.0f)) return 0.0f;", "w = 0 where the argument is below -125"),
    M("ln_fold_1_5", "rg_policy.h", "if (mant > 0x3504f3u)", "if (mant > 0x400000u)", "the mantissa folded into [sqrt(1/2), sqrt 2)"),
    M("ln_coefficient", "rg_policy.h", "0.33333346247673035f", "0.33333546247673035f", "ln(1 + u) / u interpolated to 1.6e-9 (a coefficient off by 2e-6)"),
    M("exp2_coefficient", "rg_policy.h", "0.24022650718688965f", "0.24023650718688965f", "(2^f - 1) / f interpolated to 3.9e-9 (a coefficient off by 1e-5)"),
    M("exp2_floor", "rg_policy.h", "if ((float)i > h) i -= 1;", "", "i = floor(t + 1/2)"),
    M("entropy_clamp", "rg_policy.h", "        if (!(ent > 0.0f)) ent = 0.0f;\n", "", "entropy ..., not below 0", EQUIVALENT,
      "ent = lnS - T * inv with lnS >= +0 (rg_pol_ln is never negative on [1, 32]: tests/policy_poly_main.cpp, every float32) and T * inv <= +0 (T sums w * d with "
      "w >= 0, d <= 0; inv > 0), so the difference is never below +0.0 nor -0.0; policy_poly_main.cpp searches 10^6 rows with one dominant key and finds none"),
    M("draw_guard", "rg_policy.h", "if (pol < 0) pol = 31 - __builtin_clz(row);", "if (pol < 0) pol = __builtin_ctz(row);", "the guard behind the loop answers the last legal key",
      EQUIVALENT, "unreachable: t = u * S with u <= 1 - 2^-24 rounds to a float32 below S, and the loop's running sum ends at S itself (the same weights in the same order)"),
    M("t_guard", "rg_policy.h", "if (w != 0.0f) T = __builtin_fmaf(w, d, T);", "T = __builtin_fmaf(w, d, T);", "T = the sum of w * d over the keys that weigh"),
    M("entropy_sign", "rg_policy.h", "ent = lnS - T * inv;", "ent = lnS + T * inv;", "entropy = ln S - (sum w * d) / S"),
    M("plus_inf", "rg_policy.h", "if (x == rg_pol_f(0x7f800000u)) x = rg_pol_f(0x7f7fffffu);", "", "+inf is FLT_MAX"),
    M("nan_weighs", "rg_policy.h", "weighs = x == x && x != rg_pol_f(0xff800000u);", "weighs = x != rg_pol_f(0xff800000u);", "NaN weighs 0"),
    M("ninf_weighs", "rg_policy.h", "weighs = x == x && x != rg_pol_f(0xff800000u);", "weighs = x == x;", "-inf weighs 0 (an all -inf row is flat)"),
    M("greedy_last_tie", "rg_policy.h", "(best < 0 || x > m)", "(best < 0 || x >= m)", "RG_ACT_GREEDY: ties to the lowest index"),
    M("greedy_flat_last", "rg_policy.h", "a = flat ? __builtin_ctz(row) : best;", "a = flat ? 31 - __builtin_clz(row) : best;", "no key weighs: the lowest legal index"),
    M("teacher_illegal", "rg_policy.h", "if (teacher >= 0 && ((row >> teacher) & 1u))", "if (teacher >= 0)", "the teacher key, if it is ... legal now, else the policy's draw"),
    M("logp_illegal", "rg_policy.h", "if (a < 0 || a >= n_keys || !((row >> a) & 1u)) {", "if (a < 0 || a >= n_keys) {", "RG_ACT_GIVEN: logp -inf when it is ... illegal"),
    M("logp_flat", "rg_policy.h", "r.logp = 0.0f - lnS;", "r.logp = 0.0f;", "no legal key weighs: logp = -ln count"),
    M("logp_weightless", "rg_policy.h", "(ok && rg_pol_exp2(d * log2e) != 0.0f) ? d - lnS : ninf", "ok ? d - lnS : ninf", "logp[k] = -inf where w[k] == 0"),
    M("grave_source", "rg_policy.h", "RgActOut r = {0, 0.0f, 0.0f, 3u};", "RgActOut r = {0, 0.0f, 0.0f, 1u};", "no legal key at all: ... source 3"),
    M("f16_subnormal_widen", "rg_policy.h", "(uint32_t)__builtin_clz(m) - 21u;", "(uint32_t)__builtin_clz(m) - 22u;", "f16 widens exactly (subnormals included)"),
    # ---- rg_policy_grad.h
    M("f16_subnormal_tie_up", "rg_policy_grad.h", "(rem > half || (rem == half && (q & 1u)))", "(rem >= half)", "rounded to nearest EVEN (a subnormal binary16)"),
    M("f16_tie_2_25", "rg_policy_grad.h", "if (a <= 0x33000000u) return s;", "if (a < 0x33000000u) return s;", "the tie at 2^-25 goes to the even 0", EQUIVALENT,
      "at a = 2^-25 the subnormal branch computes sh = 24, q = 0, rem = half: a tie under an even q, not rounded up -- the same s | 0"),
    M("f16_overflow_edge", "rg_policy_grad.h", "if (a >= 0x47800000u) return s | 0x7c00u;", "if (a > 0x47800000u) return s | 0x7c00u;", "2^16 and above: infinity", EQUIVALENT,
      "at a = 2^16 the normal branch computes r = 0x0f800000, (r + 0xfff + 0) >> 13 = 0x7c00: the same bits"),
    M("bf16_any_nan", "rg_policy_grad.h", "if (a > 0x7f800000u) return 0x7fc0u;", "", "NaN is the canonical quiet NaN of the type", EQUIVALENT,
      "rg_pg_canon has made every NaN 0x7fc00000 before rg_pol_narrow sees it, and (0x7fc00000 + 0x7fff + 0) >> 16 = 0x7fc0 already"),
    M("f16_tie_up", "rg_policy_grad.h", "(r + 0xfffu + ((r >> 13) & 1u)) >> 13", "(r + 0x1000u) >> 13", "rounded to nearest EVEN (a normal binary16)"),
    M("bf16_tie_up", "rg_policy_grad.h", "(u + 0x7fffu + ((u >> 16) & 1u)) >> 16", "(u + 0x8000u) >> 16", "rounded to nearest EVEN (bfloat16)"),
    M("weightless_counts", "rg_policy_grad.h", "counts = ok && rg_pol_exp2((x - st.m) * log2e) != 0.0f;", "counts = ok;", "the action does not count when it is ... weightless"),
    M("grad_entropy_sign", "rg_policy_grad.h", "rg_pg_canon(inv_temp * (t1 - t2))", "rg_pg_canon(inv_temp * (t1 + t2))", "dlogit[k] = inv_temp * (t1 - t2)"),
    M("grad_no_inv_temp", "rg_policy_grad.h", "rg_pg_canon(inv_temp * (t1 - t2))", "rg_pg_canon(t1 - t2)", "dlogit[k] = INV_TEMP * (t1 - t2)"),
    M("grad_no_canon", "rg_policy_grad.h", "rg_pg_canon(inv_temp * (t1 - t2))", "inv_temp * (t1 - t2)", "a NaN result is written as the canonical quiet NaN"),
    M("grad_raw_entropy", "rg_policy_grad.h", "(pi * (lp + st.ent))", "(pi * (lp + (st.lnS - st.T * st.inv)))", "the entropy H exactly as rg_pol_stats computes it (H after its clamp at 0)",
      EQUIVALENT, "the same f32 expression as rg_pol_stats' own, whose clamp never acts (see entropy_clamp): the same bits"),
    M("grad_weightless_key", "rg_policy_grad.h", "            if (w != 0.0f) {", "            if (true) {", "dlogit[k] = +0.0 for ... a weight that underflowed to 0"),
    M("grad_lp_term", "rg_policy_grad.h", "(k == a ? 1.0f : 0.0f) - pi", "(k == a ? 1.0f : 0.0f) - w", "pi = w[k] * inv"),
    # ---- rg_action_mask.h
    M("corner_or", "rg_action_mask.h", "ok = ok && rg_walkable(cell[py * W + x]) && rg_walkable(cell[y * W + px]);",
      "ok = ok && (rg_walkable(cell[py * W + x]) || rg_walkable(cell[y * W + px]));", "for a diagonal BOTH orthogonal neighbours ... walkable"),
    M("locked_hidden_ignored", "rg_action_mask.h", "bool ok = rg_walkable(t) && !(t & (C_HIDDEN | C_LOCKED));", "bool ok = rg_walkable(t);", "the target ... neither hidden nor locked"),
    M("locked_ignored", "rg_action_mask.h", "bool ok = rg_walkable(t) && !(t & (C_HIDDEN | C_LOCKED));", "bool ok = rg_walkable(t) && !(t & C_HIDDEN);", "the target ... nor LOCKED"),
    M("none_walkable", "rg_action_mask.h", "return !(s == S_WALLX || s == S_WALLY || s == S_NONE);", "return !(s == S_WALLX || s == S_WALLY);", "Surface::can_walk: not S_NONE"),
    M("sample_low_word", "rg_action_mask.h", "(uint32_t)(((z >> 32) * (uint64_t)count) >> 32)", "(uint32_t)(((z & 0xffffffffull) * (uint64_t)count) >> 32)",
      "the HIGH word scaled to [0, count)"),
    M("sample_env_plus_0", "rg_action_mask.h", "((uint64_t)env + 1ull)", "((uint64_t)env)", "a splitmix64 finalizer over the three (env + 1)"),
    M("run_keys_unfolded", "rg_action_mask.h", "switch (key | 0x20) {", "switch (key) {", "a run key (MoveUntil) is judged by its first move"),
    M("j_is_up", "rg_action_mask.h", "case 'k': return 0; case 'j': return 1;", "case 'k': return 1; case 'j': return 0;", "j is down, k is up"),
    M("search_not_always", "rg_action_mask.h", "(key == '.' || key == 's')", "(key == '.')", "the keys that always act ('.' NoOp, 's' Search)"),
    M("dead_still_legal", "rg_action_mask.h", "return dead ? 0u : b;", "return b;", "an env in the Grave modal answers every key ... with IgnoredInput: 0"),
    M("stair_anywhere", "rg_action_mask.h", "(uint32_t)((cell[py * W + px] & C_SURF_MASK) == S_STAIR) << RG_LB_STAIR;", "1u << RG_LB_STAIR;", "'>' asks for the surface under the player"),
    # ---- rg_path.h
    M("gold_under_player_goal", "rg_path.h", "((goals & RG_GOAL_GOLD) && (c & C_GOLD) && !own)", "((goals & RG_GOAL_GOLD) && (c & C_GOLD))", "gold is taken by moving ONTO it (not the own cell)"),
    M("last_direction", "rg_path.h", "return rg_path_dir_key(__builtin_ctz(dirs & 0xffu));", "return rg_path_dir_key(31 - __builtin_clz(dirs & 0xffu));",
      "the first direction in Direction enum order"),
    M("unreachable_noop", "rg_path.h", "if (d == RG_PATH_INF || !(dirs & 0xffu)) return (uint8_t)'s';", "if (d == RG_PATH_INF || !(dirs & 0xffu)) return (uint8_t)'.';",
      "unreachable: 's' (Search is what reveals hidden cells)"),
    M("on_stairs_noop", "rg_path.h", "(stairs_here ? '>' : '.')", "('.')", "d == 0 on the stairs: '>'"),
    M("path_through_secrets", "rg_path.h", "return rg_walkable(c) && !(c & (C_HIDDEN | C_LOCKED)); }", "return rg_walkable(c); }", "a cell a move may end on: what rg_can_move demands"),
    M("path_dead_key", "rg_path.h", "if (dead) return (uint8_t)'.';", "if (dead) return (uint8_t)'s';", "dead: '.'"),
    M("path_dist_unreachable", "rg_path.h", "return d == RG_PATH_INF ? -1 : (int32_t)d;", "return d == RG_PATH_INF ? 0 : (int32_t)d;", "unreachable: distance -1"),
    M("stairs_goal_any_surface", "rg_path.h", "((goals & RG_GOAL_STAIRS) && (c & C_SURF_MASK) == S_STAIR)", "((goals & RG_GOAL_STAIRS) && (c & C_SURF_MASK) >= S_STAIR)",
      "the stairs goal is the stairs surface"),
    # ---- rg_route.h
    M("known_without_visible", "rg_route.h", "return (c & (C_DRAWN | C_VISIBLE)) != 0 || own; }", "return (c & C_DRAWN) != 0 || own; }", "on the player's map: drawn OR IN VIEW"),
    M("known_without_own", "rg_route.h", "return (c & (C_DRAWN | C_VISIBLE)) != 0 || own; }", "return (c & (C_DRAWN | C_VISIBLE)) != 0; }", "... or the player's own"),
    M("k_whatever_mode", "rg_route.h", "return !(mode & RG_ROUTE_KNOWN) || rg_route_known(c, own); }", "return rg_route_known(c, own); }", "K binds with RG_ROUTE_KNOWN only"),
    M("corner_without_k", "rg_route.h", "return rg_walkable(c) && rg_route_k(c, mode, own); }", "return rg_walkable(c); }", "the corner rule asks K of the two orthogonal neighbours"),
    M("goal_without_k", "rg_route.h", "(rg_route_k(c, mode, own) && rg_path_goal(c, goals & (RG_GOAL_STAIRS | RG_GOAL_GOLD), own, false))",
      "(rg_path_goal(c, goals & (RG_GOAL_STAIRS | RG_GOAL_GOLD), own, false))", "stairs and gold ... but only where K"),
    M("search_before_descend", "rg_route.h", "((goals & RG_GOAL_STAIRS) && on_stairs) ? '>' : ((goals & RG_GOAL_FRONTIER) && own_frontier) ? 's' : '.'",
      "((goals & RG_GOAL_FRONTIER) && own_frontier) ? 's' : ((goals & RG_GOAL_STAIRS) && on_stairs) ? '>' : '.'", "d == 0: '>' on the stairs before 's' on a frontier cell"),
    M("secret_without_locked", "rg_route.h", "return (c & (C_HIDDEN | C_LOCKED)) != 0; }", "return (c & C_HIDDEN) != 0; }", "a secret cell: hidden or LOCKED"),
    M("secret_by_surface", "rg_route.h", "(rg_route_secret(c) ? (mode & RG_ROUTE_SECRETS) != 0 : rg_walkable(c))", "((rg_route_secret(c) && (mode & RG_ROUTE_SECRETS) != 0) || rg_walkable(c))",
      "a secret cell is a cell of the route by its attr ALONE: without RG_ROUTE_SECRETS it is none, whatever its surface"),
    M("frontier_without_pass", "rg_route.h", "return rg_route_pass(c, mode, own) && unknown_beside; }", "return unknown_beside; }", "a frontier cell: PASS, with an unknown orthogonal neighbour"),
    # ---- rg_objects.h
    M("object_gold_under_player", "rg_objects.h", "(((c & C_GOLD) && !own) ? RG_OBJ_GOLD : 0u)", "((c & C_GOLD) ? RG_OBJ_GOLD : 0u)", "gold where K and not under the player"),
    M("kind_without_k", "rg_objects.h", "    if (!rg_route_k(c, mode, own)) return 0u;\n", "", "stairs and doors by the surface WHERE K"),
    M("cheb_as_manhattan", "rg_objects.h", "r[3] = (uint32_t)(ax > ay ? ax : ay);", "r[3] = (uint32_t)(ax + ay);", "a row: ... max(|dx|, |dy|)"),
    M("frontier_unasked", "rg_objects.h", "(((kinds & RG_OBJ_FRONTIER) && rg_route_frontier(c, mode, own, unknown_beside)) ? RG_OBJ_FRONTIER : 0u)",
      "(rg_route_frontier(c, mode, own, unknown_beside) ? RG_OBJ_FRONTIER : 0u)", "the OR of the ASKED kinds it satisfies"),
    M("row_walk_dropped", "rg_objects.h", "r[1] = ((uint32_t)dy & 0xffffu) | (walk & 0xffffu) << 16;", "r[1] = ((uint32_t)dy & 0xffffu);", "a row: kind, dx | dy, WALK | x, y | ..."),
    # ---- rg_monsters.h
    M("gold_over_monster", "rg_monsters.h", " || (c & C_GOLD) || (x == E.px && y == E.py)) return false;", " || (x == E.px && y == E.py)) return false;",
      "the cell holds no gold (gold is drawn over a monster)"),
    M("shown_rows_0_and_last", "rg_monsters.h", "if (y < 1 || y >= E.H - 1 || !(c & (C_VISIBLE | C_DRAWN))", "if (!(c & (C_VISIBLE | C_DRAWN))", "its row is in 1 .. H-2"),
    M("shown_d2_1", "rg_monsters.h", "return dx * dx + dy * dy <= 2 ||", "return dx * dx + dy * dy <= 1 ||", "either dx*dx + dy*dy <= 2 ..."),
    M("empty_room_clause", "rg_monsters.h", "    if (E.empty) return true;\n", "", "unless the room is Empty, both cells inside the room's rect or both outside"),
    M("in_out_of_rect", "rg_monsters.h", "return in == E.p_in;", "return true;", "both cells inside the room's rect or both outside it"),
    M("shown_without_drawn", "rg_monsters.h", "!(c & (C_VISIBLE | C_DRAWN))", "!(c & C_VISIBLE)", "its cell word has C_VISIBLE or C_DRAWN"),
    M("shown_own_cell", "rg_monsters.h", " || (x == E.px && y == E.py)) return false;", ") return false;", "it is not the player's cell"),
    M("area_last_row", "rg_monsters.h", "    if ((cy + 1) * rsy == H && y == H - 1) return -1;\n", "", "rg_mon_area: -1 = ... the last row"),
    M("area_first_row", "rg_monsters.h", "if (y < 1 || x < 0 || cx >= rnx || cy >= rny) return -1;", "if (x < 0 || cx >= rnx || cy >= rny) return -1;", "rg_mon_area: -1 = row 0"),
    M("area_starts_row_0", "rg_monsters.h", "E.ay0 = cy == 0 ? 1 : cy * rsy;", "E.ay0 = cy * rsy;", "Room::assigned_area: the top areas start at row 1", EQUIVALENT,
      "rg_mon_area is asked for the player's cell alone and E.ay0 bounds only a MONSTER's row in rg_mon_same_room; a monster in row 0 was refused by rg_mon_shown's "
      "y < 1 before, so 0 and 1 admit the same cells (the player in row 0 is area_first_row's clause)"),
    M("hp_clamp", "rg_monsters.h", "const int32_t h = hp > 32767 ? 32767 : hp < -32768 ? -32768 : hp;", "const int32_t h = hp;", "min(hp, 32767) as an int16"),
    M("order_without_d2", "rg_monsters.h", "(uint64_t)(dx * dx + dy * dy) << 40 | ", "", "ascending by (cheb, dx*dx + dy*dy, x<<8|y)"),
    M("nearest_le", "rg_monsters.h", "cheb < T.nearest", "cheb <= T.nearest", "the least cheb of a shown monster", EQUIVALENT, "at cheb == T.nearest the assignment stores the value that is there"),
    M("count_over_shown", "rg_monsters.h", "    T.count += (int32_t)qualifies;\n    if (!shown) return;", "    if (!shown) return;\n    T.count += (int32_t)qualifies;",
      "[3] the monsters that qualify in the call's MODE"),
    M("active_leaks", "rg_monsters.h", "r[2] = shown | (all ? ((pay >> 8) & 1u) << 16 : 0u);", "r[2] = shown | ((pay >> 8) & 1u) << 16;", "ALL only: active"),
    # ---- rg_novelty.h
    M("hash_0_kept", "rg_novelty.h", "return h ? h : 1ull;", "return h;", "a result of 0 becomes 1"),
    M("crop_rows_0_and_last", "rg_novelty.h", "(y >= 1 && y <= H - 2 && x >= 0 && x < W)", "(y >= 0 && y <= H - 1 && x >= 0 && x < W)", "a window cell outside rows 1 .. H-2 ... is ' '"),
    M("one_probe_fewer", "rg_novelty.h", "for (uint32_t p = 0; p < cap; p++,", "for (uint32_t p = 0; p + 1 < cap; p++,", "at most cap probes"),
    M("salt_length_shift", "rg_novelty.h", "((uint64_t)L << 32)", "((uint64_t)L << 24)", "salt = what | dungeon_level << 8 | (u64)L << 32"),
    M("salt_level_shift", "rg_novelty.h", "((uint64_t)(uint32_t)level << 8)", "((uint64_t)(uint32_t)level << 16)", "salt = what | dungeon_level << 8 | ..."),
    M("pos_y_mask", "rg_novelty.h", "(uint64_t)(uint32_t)(py & 0xffff) << 16", "(uint64_t)(uint32_t)(py & 0xff) << 16", "RG_NOV_POS: y as u16 LE", EQUIVALENT,
      "py < height <= RG_MAX_H = 48 on the host (player_check) and 8 bits in the device's position word: bits 8..15 of y are always 0"),
    M("pos_y_shift", "rg_novelty.h", "(uint64_t)(uint32_t)(py & 0xffff) << 16", "(uint64_t)(uint32_t)(py & 0xffff) << 8", "RG_NOV_POS: x as u16 LE, THEN y as u16 LE"),
    M("term_index_from_0", "rg_novelty.h", "(uint64_t)(i + 1) * RG_NOV_GOLD", "(uint64_t)i * RG_NOV_GOLD", "mix(w_i ^ ((i + 1) * 0x9e37...))"),
    M("screen_from_row_0", "rg_novelty.h", "return screen[(uint32_t)W + k];", "return screen[k];", "RG_NOV_SCREEN: rows 1 .. H-2"),
    # ---- rg_episode.h (the scout part)
    M("row_bits_lo", "rg_episode.h", "lo = W - c0,", "lo = 0 - c0,", "which cells can count: rows 1 .. (row 0 does not)"),
    M("row_bits_hi", "rg_episode.h", "hi = hw - W - c0;", "hi = hw - c0;", "which cells can count: rows .. H - 2 (the last row does not)"),
    M("ep_known_own", "rg_episode.h", "(uint32_t)rg_route_known(c, false)", "(uint32_t)rg_route_known(c, true)", "the known bit of one cell word: drawn or in view"),
    M("fresh_ignores_drop", "rg_episode.h", "const uint32_t old = drop ? 0u : seen,", "const uint32_t old = seen,", "drop: the bits belong to another level: start from nothing",
      EQUIVALENT, "on the host: rg_scout_host has no level and passes drop = false always, so no output of a twin can change.  The clause acts on the device alone "
      "(k_episode), where tests/test_gpu_episode.py holds the scout reward against a Python bitmap across level changes (the first-floor test: most envs reach level 2)"),
    M("fresh_pays_twice", "rg_episode.h", "seen = old | fresh;", "seen = known;", "a cell that drops off the player's map stays in `seen` and is never paid twice"),
]


def header_path(root, header):
    return os.path.join(root, "rogue-gym_amd", "csrc", header)


def occurrences():
    """{mutant name: how often its old text stands in the checked-out header}"""
    return {m["name"]: open(header_path(ROOT, m["header"])).read().count(m["old"]) for m in MUTANTS}


def _product_flags():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return ["--offload-arch=gfx950", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", '-DRG_BUILD_ID="%s"' % g.source_id()]


def _units():
    out = subprocess.check_output(["bash", "-c", '. "$0" && printf "%s" "$UNITS"', os.path.join(PKG, "csrc", "units.sh")], text=True)
    return [u.split(":") for u in out.split()]


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def build_variant(work, mutant, other_objs):
    """A copy of csrc/ and include/ under `work` (laid out as the checkout: work/rogue-gym_amd/csrc, work/include) with the mutant's change applied (None: unchanged),
    its four host units compiled with the product's flags and linked with the product's other objects -> the path of work/rogue-gym_amd/librogue_gym_hip.so."""
    pkg = os.path.join(work, "rogue-gym_amd")
    shutil.copytree(os.path.join(PKG, "csrc"), os.path.join(pkg, "csrc"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(work, "include"))
    if mutant is not None:
        p = header_path(work, mutant["header"])
        text = open(p).read()
        assert text.count(mutant["old"]) == 1, mutant["name"]
        open(p, "w").write(text.replace(mutant["old"], mutant["new"]))
    flags, objs, jobs = _product_flags(), [], []
    for src in HOST_UNITS:
        objs.append(os.path.join(pkg, src[:-4] + ".o"))
        jobs.append(subprocess.Popen([_hipcc()] + flags + ["-O2", "-c", os.path.join(pkg, "csrc", src), "-o", objs[-1]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [j.communicate()[0] for j in jobs]
    if any(j.returncode != 0 for j in jobs):
        raise RuntimeError("%s does not compile:\n%s" % (mutant and mutant["name"], "\n".join(logs)[-3000:]))
    so = os.path.join(pkg, "librogue_gym_hip.so")
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared"] + other_objs + objs + ["-L" + PKG] + ["-lrogue_gym_" + s for s in SIDE_LIBS] + ["-Wl,-rpath," + PKG, "-o", so],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return so


def other_objects(scratch):
    """The product's objects of every unit but the four host units, from rogue-gym_amd/build (where build() leaves them); one that is missing there -- a tree that
    carries the libraries without their objects -- is compiled into `scratch`, from the checkout's sources, never into the checkout.  build() must have run: a
    missing or stale product library is an error here, not a reason to rebuild."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    if g.library_id(os.path.join(PKG, "librogue_gym_hip.so")) != g.source_id():
        raise RuntimeError("rogue-gym_amd/librogue_gym_hip.so is missing or was not built from the checked-out sources: run __graft_entry__.build() first (nothing is built into the checkout here)")
    objs, jobs = [], []
    for src, opt in _units():
        if src in HOST_UNITS:
            continue
        obj = os.path.join(PKG, "build", src.rsplit(".", 1)[0] + ".o")
        if not os.path.exists(obj):
            obj = os.path.join(scratch, src.rsplit(".", 1)[0] + ".o")
            jobs.append(subprocess.Popen([_hipcc()] + _product_flags() + [opt, "-c", os.path.join(PKG, "csrc", src), "-o", obj]))
        objs.append(obj)
    if any(j.wait() != 0 for j in jobs):
        raise RuntimeError("hipcc failed")
    return objs


def run_tests(so, entries, timeout=900):
    """The host test files in child pytests against the library `so` (the loader honours ROGUE_GYM_HIP_LIB; RULE_MUTANT_PKG names the rogue-gym_amd/ copy beside
    it, whose csrc/ the stand-alone polynomial program of test_policy_host.py compiles) -> the id of the first failing test, None = all passed.  An entry is a
    file, or (file, -k expression): one pytest run each, in order.  The sanitizer tests compile the checkout's own sources, which no mutant touches: deselected."""
    env = dict(os.environ, ROGUE_GYM_HIP_LIB=so, RULE_MUTANT_PKG=os.path.dirname(so), PYTHONDONTWRITEBYTECODE="1")
    for entry in entries:
        f, expr = (entry, "not sanitizers") if isinstance(entry, str) else (entry[0], "(%s) and not sanitizers" % entry[1])
        cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-k", expr, "-rfE", os.path.join(ROOT, "tests", f)]
        try:
            p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            return "timeout"
        if p.returncode == 0:
            continue
        m = re.search(r"^(?:FAILED|ERROR) (?:tests/)?(\S+?\.py::\S+)", p.stdout, re.M)
        if m is None:
            raise RuntimeError("pytest ended with %d and named no test:\n%s" % (p.returncode, (p.stdout + p.stderr)[-3000:]))
        return m.group(1).split("[")[0]
    return None


def kill_matrix(only=None, workers=None):
    """{mutant name ("" = the unmutated build): the first failing test of its header's host test files, or None} for every mutant (or those of the headers `only`).
    Every build and run happens in a temporary directory; the checkout's sources and libraries are read, never written.  At most 16 processes at a time."""
    todo = [m for m in MUTANTS if only is None or m["header"] in only]
    headers = sorted({m["header"] for m in todo})
    base_files = sorted({f for h in headers for f in TESTS[h] if isinstance(f, str)})
    workers = workers or max(1, min(4, (os.cpu_count() or 2) // 2))      # each worker compiles four units side by side: 16 compilers at the most
    with tempfile.TemporaryDirectory(prefix="rule_mutants_") as tmp:
        others = other_objects(tmp)

        def one(m):
            work = os.path.join(tmp, m["name"] if m else "_base")
            so = build_variant(work, m, others)
            res = run_tests(so, TESTS[m["header"]] if m else base_files)
            shutil.rmtree(work, ignore_errors=True)
            return ("" if m is None else m["name"]), res

        with ThreadPoolExecutor(workers) as pool:
            return dict(pool.map(one, [None] + todo))


def by_name():
    return {m["name"]: m for m in MUTANTS}
