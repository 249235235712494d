// A stand-alone host program around the readers' CPU rules (rogue-gym_amd/csrc/rg_readers_host.h), built by tests/test_readers_host_sanitizers.py with
// -fsanitize=address,undefined: every input and output is allocated on the heap at its exact size, so a read or write one element past a grid, a field, a
// table or a monster array ends the run.  Each search is compared with a restatement that has no queue -- relaxation sweeps over the rule headers' per-cell
// predicates until nothing changes -- and every refusal of every twin is made once, into guard bytes that must stay untouched.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rg_readers_host.h"

static uint32_t rnd_state = 2463534242u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static int rnd_in(int n) { return (int)(rnd() % (uint32_t)n); }

static int bad = 0, runs = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { bad++; if (bad <= 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

typedef std::vector<uint16_t> Grid;
static const uint32_t INF = RG_PATH_INF;

// random words, or a level-like mix: most surfaces walkable and most cells on the player's map, so that searches reach far
static Grid make_grid(int H, int W, bool mix) {
    static const uint16_t surf[16] = {S_FLOOR, S_FLOOR, S_FLOOR, S_FLOOR, S_FLOOR, S_FLOOR, S_FLOOR, S_PASSAGE, S_PASSAGE, S_DOOR, S_STAIR, S_TRAP, S_WALLX, S_WALLY, S_NONE, S_FLOOR};
    Grid g((size_t)H * W);
    for (auto &c : g) {
        if (!mix) { c = (uint16_t)rnd(); continue; }
        c = surf[rnd_in(16)];
        if (rnd_in(10) < 8) c |= rnd_in(2) ? C_DRAWN : C_VISIBLE;
        if (rnd_in(20) == 0) c |= C_HIDDEN;
        if (rnd_in(30) == 0) c |= C_LOCKED;
        if (rnd_in(20) == 0) c |= C_GOLD;
    }
    return g;
}

// D = 0 at the sources; sweeps, forwards and backwards in turn, until nothing changes: D[a] = 1 + min over the moves a -> b of D[b].  move(a, ax, ay, dx, dy) says
// whether the move from cell a in direction (dx, dy), whose target is inside the grid, is one of the graph.
template <class Move>
static void relax(int H, int W, std::vector<uint32_t> &D, const std::vector<uint8_t> &source, Move move) {
    const int hw = H * W;
    for (bool changed = true, fwd = true; changed; fwd = !fwd) {
        changed = false;
        for (int n = 0; n < hw; n++) {
            const int a = fwd ? n : hw - 1 - n, ax = a % W, ay = a / W;
            if (source[a]) continue;
            for (int d = 0; d < 8; d++) {
                const int dx = rg_path_dx(d), dy = rg_path_dy(d), bx = ax + dx, by = ay + dy;
                if (bx < 0 || by < 0 || bx >= W || by >= H) continue;
                const uint32_t db = D[by * W + bx];
                if (db != INF && db + 1 < D[a] && move(a, ax, ay, dx, dy)) { D[a] = db + 1; changed = true; }
            }
        }
    }
}
static bool unknown4(const Grid &g, int H, int W, int pi, int i) {
    static const int ox[4] = {-1, 1, 0, 0}, oy[4] = {0, 0, -1, 1};
    for (int k = 0; k < 4; k++) {
        const int x = i % W + ox[k], y = i / W + oy[k];
        if (x >= 0 && y >= 0 && x < W && y < H && !rg_route_known(g[y * W + x], y * W + x == pi)) return true;
    }
    return false;
}
// a move of rg_route's graph between cells a and b = a + (dx, dy): both pass (the cell `free` whatever its word), both corner cells of a diagonal corner
static bool route_move(const Grid &g, int W, uint32_t mode, int pi, int a, int ax, int ay, int dx, int dy, int free) {
    const int b = (ay + dy) * W + ax + dx;
    if (!(a == free || rg_route_pass(g[a], mode, a == pi)) || !(b == free || rg_route_pass(g[b], mode, b == pi))) return false;
    if (dx == 0 || dy == 0) return true;
    const int c0 = ay * W + ax + dx, c1 = (ay + dy) * W + ax;
    return rg_route_corner(g[c0], mode, c0 == pi) && rg_route_corner(g[c1], mode, c1 == pi);
}
// a move key among a finite distance's answers steps onto a cell one move closer
static void check_key_step(const char *what, uint8_t key, const std::vector<uint32_t> &R, int H, int W, int px, int py) {
    for (int d = 0; d < 8; d++)
        if (key == rg_path_dir_key(d)) {
            const int x = px + rg_path_dx(d), y = py + rg_path_dy(d);
            EXPECT(x >= 0 && y >= 0 && x < W && y < H && R[y * W + x] + 1 == R[py * W + px], "%s: key '%c' does not step closer (%dx%d)", what, key, H, W);
        }
}
static bool same_field(const std::vector<uint16_t> &F, const std::vector<uint32_t> &R) {
    for (size_t i = 0; i < F.size(); i++)
        if (F[i] != R[i]) return false;
    return true;
}

static void check_path(const Grid &g, int H, int W, int px, int py, int dead, uint32_t goals, int cy, int cx) {
    const int hw = H * W, pi = py * W + px;
    std::vector<uint16_t> field((size_t)hw);
    std::vector<int32_t> dist(1), dist2(1);
    std::vector<uint8_t> key(1), key2(1), src((size_t)hw);
    std::string err;
    runs++;
    if (rgh_path(err, g.data(), H, W, px, py, dead, goals, cy, cx, field.data(), dist.data(), key.data())) { EXPECT(false, "path refused: %s", err.c_str()); return; }
    std::vector<uint32_t> R((size_t)hw, INF);
    for (int i = 0; i < hw; i++)
        if ((src[i] = rg_path_goal(g[i], goals, i == pi, i % W == cx && i / W == cy))) R[i] = 0;
    relax(H, W, R, src, [&](int a, int ax, int ay, int dx, int dy) { return rg_path_ok(g[a]) && rg_can_move(g.data(), H, W, ax, ay, dx, dy); });
    EXPECT(same_field(field, R), "path field %dx%d goals %u", H, W, goals);
    EXPECT(dist[0] == (R[pi] == INF ? -1 : (int32_t)R[pi]), "path dist %dx%d", H, W);
    if (!dead && R[pi] != 0 && R[pi] != INF) check_key_step("path", key[0], R, H, W, px, py);
    EXPECT(!rgh_path(err, g.data(), H, W, px, py, dead, goals, cy, cx, nullptr, dist2.data(), key2.data()) && dist2[0] == dist[0] && key2[0] == key[0], "path without field %dx%d", H, W);
}

static void check_route(const Grid &g, int H, int W, int px, int py, int dead, uint32_t goals, uint32_t fallback, uint32_t mode, int cy, int cx) {
    const int hw = H * W, pi = py * W + px;
    std::vector<uint16_t> field((size_t)hw);
    std::vector<int32_t> dist(1), dist2(1);
    std::vector<uint8_t> key(1), tier(1), key2(1), tier2(1), src((size_t)hw);
    std::string err;
    runs++;
    if (rgh_route(err, g.data(), H, W, px, py, dead, goals, fallback, mode, cy, cx, field.data(), dist.data(), key.data(), tier.data())) { EXPECT(false, "route refused: %s", err.c_str()); return; }
    std::vector<uint32_t> R;
    uint32_t want_tier = RG_ROUTE_NO_TIER;
    for (uint32_t t = 0; t < 2 && want_tier == RG_ROUTE_NO_TIER; t++) {
        if (t && !fallback) break;
        const uint32_t gw = t ? fallback : goals;
        R.assign((size_t)hw, INF);
        for (int i = 0; i < hw; i++) {
            src[i] = rg_route_goal(g[i], gw, mode, i == pi, i % W == cx && i / W == cy) || ((gw & RG_GOAL_FRONTIER) && rg_route_frontier(g[i], mode, i == pi, unknown4(g, H, W, pi, i)));
            if (src[i]) R[i] = 0;
        }
        relax(H, W, R, src, [&](int a, int ax, int ay, int dx, int dy) { return route_move(g, W, mode, pi, a, ax, ay, dx, dy, -1); });
        if (R[pi] != INF) want_tier = t;
    }
    EXPECT(same_field(field, R), "route field %dx%d goals %u fallback %u mode %u", H, W, goals, fallback, mode);
    EXPECT(dist[0] == (R[pi] == INF ? -1 : (int32_t)R[pi]), "route dist %dx%d", H, W);
    EXPECT(tier[0] == want_tier, "route tier %dx%d: %u, want %u", H, W, tier[0], want_tier);
    if (!dead && R[pi] != 0 && R[pi] != INF) check_key_step("route", key[0], R, H, W, px, py);
    // without a field the search stops early: the same answers
    EXPECT(!rgh_route(err, g.data(), H, W, px, py, dead, goals, fallback, mode, cy, cx, nullptr, dist2.data(), key2.data(), tier2.data()) && dist2[0] == dist[0] && key2[0] == key[0] &&
               tier2[0] == tier[0],
           "route without field %dx%d goals %u fallback %u mode %u", H, W, goals, fallback, mode);
}

static void check_objects(const Grid &g, int H, int W, int px, int py, int dead, uint32_t kinds, uint32_t mode, int cap) {
    const int hw = H * W, pi = py * W + px;
    std::vector<int16_t> table((size_t)cap * RG_OBJ_COLS);
    std::vector<int32_t> count(4), count2(4);
    std::string err;
    runs++;
    if (rgh_objects(err, g.data(), H, W, px, py, dead, kinds, mode, cap, table.data(), count.data())) { EXPECT(false, "objects refused: %s", err.c_str()); return; }
    std::vector<uint32_t> R((size_t)hw, INF), kind((size_t)hw);
    std::vector<uint8_t> src((size_t)hw, 0);
    int32_t want[4] = {0, 0, 0, 0};
    R[pi] = 0; src[pi] = 1;
    // (the graph is symmetric: the walk to a cell is the walk from it; the player's own cell starts the search whatever its word)
    relax(H, W, R, src, [&](int a, int ax, int ay, int dx, int dy) { return route_move(g, W, mode, pi, a, ax, ay, dx, dy, pi); });
    for (int i = 0; i < hw; i++) {
        kind[i] = dead ? 0u : rg_obj_kind(g[i], kinds, mode, i == pi, unknown4(g, H, W, pi, i));
        for (int k = 0; k < 4; k++) want[k] += (kind[i] >> k) & 1;
    }
    for (int k = 0; k < 4; k++) EXPECT(count[k] == want[k], "objects count[%d] %dx%d: %d, want %d", k, H, W, count[k], want[k]);
    int listed = 0;
    long prev = -1;
    for (int r = 0; r < cap; r++) {
        const int16_t *t = table.data() + (size_t)r * RG_OBJ_COLS;
        if (t[0] == 0) {
            for (int c = 0; c < RG_OBJ_COLS; c++) EXPECT(t[c] == 0, "objects: row %d past the list is not zero (%dx%d)", r, H, W);
            continue;
        }
        EXPECT(r == listed, "objects: a listed row behind an empty one (%dx%d)", H, W);
        listed++;
        const int x = t[4], y = t[5];
        if (!(x >= 0 && y >= 0 && x < W && y < H)) { EXPECT(false, "objects: row %d names a cell outside the grid", r); continue; }
        const int i = y * W + x, dx = x - px, dy = y - py, cheb = std::max(abs(dx), abs(dy));
        EXPECT((uint32_t)t[0] == kind[i] && t[1] == dx && t[2] == dy && t[6] == cheb && t[7] == 0, "objects: row %d columns (%dx%d)", r, H, W);
        EXPECT((uint32_t)(uint16_t)t[3] == R[i], "objects: row %d walk %d, relaxed %u (%dx%d mode %u)", r, t[3], R[i], H, W, mode);
        const long order = ((long)(uint16_t)t[3] << 16) | (y << 8) | x;
        EXPECT(order > prev, "objects: rows do not ascend in (walk, y, x) at row %d (%dx%d)", r, H, W);
        prev = order;
    }
    int reachable = 0;
    for (int i = 0; i < hw; i++) reachable += kind[i] != 0 && R[i] != INF;
    EXPECT(listed == std::min(cap, reachable), "objects: %d rows listed, %d objects reached, cap %d (%dx%d)", listed, reachable, cap, H, W);
    // the rows are the nearest ones: no reached object that is not listed comes before the last listed row
    if (listed == cap && reachable > cap) {
        int before = 0;
        for (int i = 0; i < hw; i++) before += kind[i] != 0 && R[i] != INF && (((long)R[i] << 16) | ((i / W) << 8) | (i % W)) <= prev;
        EXPECT(before == cap, "objects: the table is not the first %d of the order (%dx%d)", cap, H, W);
    }
    EXPECT(!rgh_objects(err, g.data(), H, W, px, py, dead, kinds, mode, cap, nullptr, count2.data()) && count2 == count, "objects counts alone %dx%d", H, W);
}

static void check_mask(const Grid &g, int H, int W, int px, int py, int dead) {
    static const char moves[9] = "kjhlyubn";  // Direction enum order
    const int n = 1 + rnd_in(RG_MASK_MAX_KEYS);
    std::vector<uint8_t> keys((size_t)n), out((size_t)n);
    for (auto &k : keys) k = (uint8_t)".hjklnbuy>sHJKLNBUY"[rnd_in(19)];
    std::string err;
    runs++;
    if (rgh_action_mask(err, g.data(), H, W, px, py, dead, keys.data(), n, out.data())) { EXPECT(false, "mask refused: %s", err.c_str()); return; }
    for (int k = 0; k < n; k++) {
        int want = keys[k] == '.' || keys[k] == 's';
        if (keys[k] == '>') want = (g[py * W + px] & C_SURF_MASK) == S_STAIR;
        for (int d = 0; d < 8; d++)
            if ((keys[k] | 0x20) == moves[d]) want = rg_can_move(g.data(), H, W, px, py, rg_path_dx(d), rg_path_dy(d));
        EXPECT(out[k] == (dead ? 0 : want), "mask key '%c' %dx%d", keys[k], H, W);
    }
    std::vector<uint8_t> all(sizeof(RG_ACTION_KEYS) - 1);  // NULL keys: the action list, exactly that many answers
    EXPECT(!rgh_action_mask(err, g.data(), H, W, px, py, dead, nullptr, 0, all.data()), "mask with the default keys refused");
}

static void check_scout(const Grid &g, int H, int W) {
    const int hw = H * W, sb = rg_ep_seen_bytes(hw);
    std::vector<uint8_t> seen((size_t)sb), before;
    for (auto &b : seen) b = (uint8_t)(rnd() & rnd());
    before = seen;
    std::vector<int32_t> fresh(1);
    std::string err;
    runs++;
    if (rgh_scout(err, g.data(), H, W, seen.data(), fresh.data())) { EXPECT(false, "scout refused: %s", err.c_str()); return; }
    int32_t want = 0;
    for (int i = 0; i < 8 * sb; i++) {
        const bool counts = i >= W && i < hw - W, was = counts && ((before[i / 8] >> (i % 8)) & 1), known = counts && rg_route_known(g[i], false);
        want += known && !was;
        EXPECT(((seen[i / 8] >> (i % 8)) & 1) == (was || known), "scout seen bit %d (%dx%d)", i, H, W);
    }
    EXPECT(fresh[0] == want, "scout fresh %dx%d: %d, want %d", H, W, fresh[0], want);
}

static void check_monsters(const Grid &g, int H, int W, int px, int py, int dead, int cap) {
    const int rnx = 1 + rnd_in(std::min(W, 8)), rny = 1 + rnd_in(std::min(H, 6)), n_mon = rnd_in(std::min(H * W, 24) + 1);
    const uint32_t mode = rnd_in(2);
    std::vector<int32_t> mx((size_t)n_mon), my((size_t)n_mon), type((size_t)n_mon), active((size_t)n_mon), hp((size_t)n_mon), alive((size_t)n_mon), meta((size_t)rnx * rny), threat(4), threat2(4);
    std::vector<uint32_t> rect((size_t)rnx * rny);
    for (int i = 0; i < n_mon; i++) {
        mx[i] = rnd_in(4) ? rnd_in(W) : (rnd_in(2) ? 0 : W - 1);
        my[i] = rnd_in(4) ? rnd_in(H) : (rnd_in(2) ? 0 : H - 1);
        type[i] = rnd_in(26); active[i] = rnd_in(2); hp[i] = rnd_in(70000) - 100; alive[i] = rnd_in(8) != 0;
    }
    for (int r = 0; r < rnx * rny; r++) {
        const int x0 = rnd_in(W), y0 = rnd_in(H), x1 = x0 + rnd_in(W - x0 + 1), y1 = y0 + rnd_in(H - y0 + 1);
        rect[r] = (uint32_t)x0 | (uint32_t)y0 << 8 | (uint32_t)x1 << 16 | (uint32_t)y1 << 24;
        meta[r] = rnd_in(3) | (rnd_in(2) ? RM_DARK : 0);
    }
    const int32_t *al = rnd_in(3) ? alive.data() : nullptr;
    std::vector<int16_t> table((size_t)cap * RG_MON_COLS);
    std::string err;
    runs++;
    if (rgh_monsters(err, g.data(), H, W, px, py, dead, n_mon, mx.data(), my.data(), type.data(), active.data(), hp.data(), al, rnx, rny, rect.data(), meta.data(), mode, cap, table.data(),
                     threat.data())) { EXPECT(false, "monsters refused: %s", err.c_str()); return; }
    // the qualifiers by a plain scan; the rows ascend in (cheb, dx*dx + dy*dy, x, y) and are as many as qualify, up to cap
    RgMonEnv E = {px, py, H, 0, 0, 0, 0, 0, 0, 0, 0, false, false};
    const int id = rg_mon_area(E, px, py, W, H, rnx, rny);
    if (id >= 0) rg_mon_room(E, rect[id], (uint32_t)meta[id]);
    int want = 0, adjacent = 0;
    for (int i = 0; i < n_mon && !dead; i++) {
        if (al && !al[i]) continue;
        const bool shown = rg_mon_shown(E, g[my[i] * W + mx[i]], mx[i], my[i]);
        want += mode == RG_MON_ALL || shown;
        adjacent += shown && std::max(abs(mx[i] - px), abs(my[i] - py)) == 1;
    }
    EXPECT(threat[3] == want && threat[0] == adjacent, "monsters threat %dx%d: count %d want %d, adjacent %d want %d", H, W, threat[3], want, threat[0], adjacent);
    long prev = -1;
    for (int r = 0; r < cap; r++) {
        const int16_t *t = table.data() + (size_t)r * RG_MON_COLS;
        if (r >= want) {
            for (int c = 0; c < RG_MON_COLS; c++) EXPECT(t[c] == 0, "monsters: row %d past the list is not zero", r);
            continue;
        }
        const int dx = t[1], dy = t[2], x = px + dx, y = py + dy;
        EXPECT(t[0] >= 'A' && t[0] <= 'Z' && x >= 0 && y >= 0 && x < W && y < H && t[3] == std::max(abs(dx), abs(dy)), "monsters: row %d columns (%dx%d)", r, H, W);
        const long order = ((long)t[3] << 40) | ((long)(dx * dx + dy * dy) << 16) | (x << 8) | y;
        EXPECT(order >= prev, "monsters: rows do not ascend at row %d", r);
        prev = order;
    }
    EXPECT(!rgh_monsters(err, g.data(), H, W, px, py, dead, n_mon, mx.data(), my.data(), type.data(), active.data(), hp.data(), al, rnx, rny, rect.data(), meta.data(), mode, 0, nullptr,
                         threat2.data()) && threat2 == threat, "monsters threat alone %dx%d", H, W);
}

// every refusal of every twin, into guard bytes
static void check_refusals() {
    const int H = 5, W = 7;
    Grid g = make_grid(H, W, true);
    std::vector<uint8_t> guard(64, 0xAB);
    uint8_t *o8 = guard.data();
    uint16_t *o16 = reinterpret_cast<uint16_t *>(guard.data());
    int16_t *t16 = reinterpret_cast<int16_t *>(guard.data());
    int32_t *o32 = reinterpret_cast<int32_t *>(guard.data());
    std::string err;
    int n = 0;
    auto refused = [&](int rc, const char *prefix) {
        n++;
        EXPECT(rc == 1 && err.compare(0, strlen(prefix), prefix) == 0 && err.size() > strlen(prefix) + 2 && err[strlen(prefix)] == ':', "refusal %d of %s: rc %d, \"%s\"", n, prefix, rc, err.c_str());
        err.clear();
    };
    const uint8_t good[2] = {'h', '>'}, wrong[2] = {'h', 'x'};
    refused(rgh_action_mask(err, g.data(), H, W, 1, 1, 0, good, 0, o8), "rg_action_mask_host");
    refused(rgh_action_mask(err, g.data(), H, W, 1, 1, 0, good, RG_MASK_MAX_KEYS + 1, o8), "rg_action_mask_host");
    refused(rgh_action_mask(err, g.data(), H, W, 1, 1, 0, wrong, 2, o8), "rg_action_mask_host");
    refused(rgh_action_mask(err, nullptr, H, W, 1, 1, 0, good, 2, o8), "rg_action_mask_host");
    refused(rgh_action_mask(err, g.data(), H, W, 1, 1, 0, good, 2, nullptr), "rg_action_mask_host");
    refused(rgh_action_mask(err, g.data(), H, W, W, 1, 0, good, 2, o8), "rg_action_mask_host");
    refused(rgh_action_mask(err, g.data(), 0, 0, 0, 0, 0, good, 2, o8), "rg_action_mask_host");

    refused(rgh_path(err, g.data(), H, W, 1, 1, 0, 0, 0, 0, o16, o32, o8), "rg_path_host");
    refused(rgh_path(err, g.data(), H, W, 1, 1, 0, RG_GOAL_FRONTIER, 0, 0, o16, o32, o8), "rg_path_host");
    refused(rgh_path(err, g.data(), H, W, 1, 1, 0, RG_GOAL_STAIRS, 0, 0, nullptr, nullptr, nullptr), "rg_path_host");
    refused(rgh_path(err, nullptr, H, W, 1, 1, 0, RG_GOAL_STAIRS, 0, 0, o16, o32, o8), "rg_path_host");
    refused(rgh_path(err, g.data(), 0, W, 1, 1, 0, RG_GOAL_STAIRS, 0, 0, o16, o32, o8), "rg_path_host");
    refused(rgh_path(err, g.data(), RG_MAX_H + 1, W, 1, 1, 0, RG_GOAL_STAIRS, 0, 0, o16, o32, o8), "rg_path_host");
    refused(rgh_path(err, g.data(), H, RG_MAX_W + 1, 1, 1, 0, RG_GOAL_STAIRS, 0, 0, o16, o32, o8), "rg_path_host");
    refused(rgh_path(err, g.data(), H, W, -1, 1, 0, RG_GOAL_STAIRS, 0, 0, o16, o32, o8), "rg_path_host");
    refused(rgh_path(err, g.data(), H, W, 1, H, 0, RG_GOAL_STAIRS, 0, 0, o16, o32, o8), "rg_path_host");

    refused(rgh_route(err, g.data(), H, W, 1, 1, 0, 0, 0, 0, 0, 0, o16, o32, o8, o8), "rg_route_host");
    refused(rgh_route(err, g.data(), H, W, 1, 1, 0, 16, 0, 0, 0, 0, o16, o32, o8, o8), "rg_route_host");
    refused(rgh_route(err, g.data(), H, W, 1, 1, 0, RG_GOAL_STAIRS, 16, 0, 0, 0, o16, o32, o8, o8), "rg_route_host");
    refused(rgh_route(err, g.data(), H, W, 1, 1, 0, RG_GOAL_STAIRS, 0, 4, 0, 0, o16, o32, o8, o8), "rg_route_host");
    refused(rgh_route(err, g.data(), H, W, 1, 1, 0, RG_GOAL_FRONTIER, 0, RG_ROUTE_SECRETS, 0, 0, o16, o32, o8, o8), "rg_route_host");
    refused(rgh_route(err, g.data(), H, W, 1, 1, 0, RG_GOAL_STAIRS, RG_GOAL_FRONTIER, 0, 0, 0, o16, o32, o8, o8), "rg_route_host");
    refused(route_args_check(err, "rg_route", RG_GOAL_CELL, 0, 0, false, "cells_dev"), "rg_route");  // (the twin always has its cell: the device entry's refusal)
    refused(route_args_check(err, "rg_route", RG_GOAL_STAIRS, RG_GOAL_CELL, 0, false, "cells_dev"), "rg_route");
    refused(rgh_route(err, g.data(), H, W, 1, 1, 0, RG_GOAL_STAIRS, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr), "rg_route_host");
    refused(rgh_route(err, nullptr, H, W, 1, 1, 0, RG_GOAL_STAIRS, 0, 0, 0, 0, o16, o32, o8, o8), "rg_route_host");
    refused(rgh_route(err, g.data(), H, 0, 1, 1, 0, RG_GOAL_STAIRS, 0, 0, 0, 0, o16, o32, o8, o8), "rg_route_host");
    refused(rgh_route(err, g.data(), H, W, 1, -1, 0, RG_GOAL_STAIRS, 0, 0, 0, 0, o16, o32, o8, o8), "rg_route_host");

    std::vector<int32_t> m1(2, 1), mbad(2, 99), meta(4, 0);
    std::vector<uint32_t> rect(4, 0);
    auto mon = [&](const uint16_t *cells, int h, int w, int px, int py, int n_mon, const int32_t *x, const int32_t *type, int rnx, int rny, const uint32_t *rr, const int32_t *rm, uint32_t mode,
                   int cap, int16_t *table, int32_t *threat) {
        return rgh_monsters(err, cells, h, w, px, py, 0, n_mon, x, m1.data(), type, m1.data(), m1.data(), nullptr, rnx, rny, rr, rm, mode, cap, table, threat);
    };
    refused(mon(g.data(), H, W, 1, 1, 2, m1.data(), m1.data(), 2, 2, rect.data(), meta.data(), 2, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, m1.data(), m1.data(), 2, 2, rect.data(), meta.data(), 0, 1, nullptr, nullptr), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, m1.data(), m1.data(), 2, 2, rect.data(), meta.data(), 0, 0, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, m1.data(), m1.data(), 2, 2, rect.data(), meta.data(), 0, RG_MON_MAX_CAP + 1, t16, o32), "rg_monsters_host");
    refused(mon(nullptr, H, W, 1, 1, 2, m1.data(), m1.data(), 2, 2, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, RG_MAX_W + 1, 1, 1, 2, m1.data(), m1.data(), 2, 2, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, W, 1, 2, m1.data(), m1.data(), 2, 2, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, -1, m1.data(), m1.data(), 2, 2, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, RG_MAX_ROOMS + 1, m1.data(), m1.data(), 2, 2, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, nullptr, m1.data(), 2, 2, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, m1.data(), m1.data(), 0, 2, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, m1.data(), m1.data(), W + 1, 1, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, m1.data(), m1.data(), 2, 2, nullptr, meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, m1.data(), m1.data(), 2, 2, rect.data(), nullptr, 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, mbad.data(), m1.data(), 2, 2, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");
    refused(mon(g.data(), H, W, 1, 1, 2, m1.data(), mbad.data(), 2, 2, rect.data(), meta.data(), 0, 1, t16, o32), "rg_monsters_host");

    refused(rgh_objects(err, g.data(), H, W, 1, 1, 0, 0, 0, 1, t16, o32), "rg_objects_host");
    refused(rgh_objects(err, g.data(), H, W, 1, 1, 0, 16, 0, 1, t16, o32), "rg_objects_host");
    refused(rgh_objects(err, g.data(), H, W, 1, 1, 0, RG_OBJ_GOLD, 4, 1, t16, o32), "rg_objects_host");
    refused(rgh_objects(err, g.data(), H, W, 1, 1, 0, RG_OBJ_FRONTIER, RG_ROUTE_SECRETS, 1, t16, o32), "rg_objects_host");
    refused(rgh_objects(err, g.data(), H, W, 1, 1, 0, RG_OBJ_GOLD, 0, 1, nullptr, nullptr), "rg_objects_host");
    refused(rgh_objects(err, g.data(), H, W, 1, 1, 0, RG_OBJ_GOLD, 0, 0, t16, o32), "rg_objects_host");
    refused(rgh_objects(err, g.data(), H, W, 1, 1, 0, RG_OBJ_GOLD, 0, RG_OBJ_MAX_CAP + 1, t16, o32), "rg_objects_host");
    refused(rgh_objects(err, nullptr, H, W, 1, 1, 0, RG_OBJ_GOLD, 0, 1, t16, o32), "rg_objects_host");
    refused(rgh_objects(err, g.data(), RG_MAX_H + 1, W, 1, 1, 0, RG_OBJ_GOLD, 0, 1, t16, o32), "rg_objects_host");
    refused(rgh_objects(err, g.data(), H, W, 1, H, 0, RG_OBJ_GOLD, 0, 1, t16, o32), "rg_objects_host");

    refused(rgh_scout(err, nullptr, H, W, o8, o32), "rg_scout_host");
    refused(rgh_scout(err, g.data(), H, W, nullptr, o32), "rg_scout_host");
    refused(rgh_scout(err, g.data(), H, RG_MAX_W + 1, o8, o32), "rg_scout_host");
    for (uint8_t b : guard) EXPECT(b == 0xAB, "a refusal wrote into its output");
    runs += n;
}

// the env-id list check of the cuts, the partial reset, the records and rg_seed_envs: each list on the heap at its exact size
static void check_env_ids() {
    const int n = 8;
    std::string err;
    auto ids = [](std::initializer_list<int32_t> l) { return std::vector<int32_t>(l); };
    auto accepted = [&](const std::vector<int32_t> &l, int k, bool unique, const char *what) {
        runs++;
        EXPECT(rgh_env_ids_check(err, "rg_x", l.data(), k, n, unique) == 0 && err.empty(), "env ids %s: refused, \"%s\"", what, err.c_str());
        err.clear();
    };
    auto refused = [&](const std::vector<int32_t> &l, int k, bool unique, const char *word, const char *what) {
        runs++;
        EXPECT(rgh_env_ids_check(err, "rg_x", l.data(), k, n, unique) == 1 && err.compare(0, 6, "rg_x: ") == 0 && err.find("env_ids") != std::string::npos &&
                   err.find(word) != std::string::npos, "env ids %s: \"%s\"", what, err.c_str());
        err.clear();
    };
    for (int unique = 0; unique < 2; unique++) {
        accepted(ids({}), 0, unique, "k = 0");
        accepted(ids({7, 6, 5, 4, 3, 2, 1, 0}), n, unique, "k = n, all distinct");
        refused(ids({3, -1}), 2, unique, "out of range", "id -1");
        refused(ids({0, n}), 2, unique, "out of range", "id n");
        refused(ids({}), -1, unique, "k = -1", "k < 0");
    }
    accepted(ids({2, 5, 2}), 3, false, "a duplicate without unique");
    refused(ids({2, 5, 2}), 3, true, "twice", "a duplicate with unique");
    accepted(ids({0, 1, 2, 3, 4, 5, 6, 7, 0}), n + 1, false, "k = n + 1 without unique");
    refused(ids({0, 1, 2, 3, 4, 5, 6, 7, 0}), n + 1, true, "k = 9", "k = n + 1 with unique");
    runs++;  // a device-side list: only its length is judged
    EXPECT(rgh_env_ids_check(err, "rg_x", nullptr, n, n, true) == 0 && rgh_env_ids_check(err, "rg_x", nullptr, n + 1, n, true) == 1, "env ids NULL list");
}

int main() {
    static const int sizes[8][2] = {{1, 1}, {1, 7}, {5, 1}, {16, 32}, {17, 33}, {24, 80}, {RG_MAX_H, RG_MAX_W}, {9, 11}};
    for (auto &s : sizes) {
        const int H = s[0], W = s[1], reps = std::max(12, std::min(120, 60000 / (H * W)));
        for (int rep = 0; rep < reps; rep++) {
            const Grid g = make_grid(H, W, rep % 4 != 3);
            const int corner = rep % 6, px = corner == 0 || corner == 2 ? 0 : corner == 1 || corner == 3 ? W - 1 : rnd_in(W), py = corner < 2 ? 0 : corner < 4 ? H - 1 : rnd_in(H);
            const int dead = rnd_in(8) == 0;
            // the caller's cell: inside the grid, or outside it on any side
            const int cy = rnd_in(3) ? rnd_in(H) : (rnd_in(2) ? -1 - rnd_in(3) : H + rnd_in(3)), cx = rnd_in(3) ? rnd_in(W) : (rnd_in(2) ? -1 - rnd_in(3) : W + rnd_in(3));
            check_mask(g, H, W, px, py, dead);
            check_path(g, H, W, px, py, dead, 1u + (uint32_t)rnd_in(7), cy, cx);
            const uint32_t mode = (uint32_t)rnd_in(4), frontier = (mode & RG_ROUTE_KNOWN) ? 15u : 7u;
            check_route(g, H, W, px, py, dead, 1u + ((uint32_t)rnd_in(15) & frontier) % frontier, (uint32_t)rnd_in(16) & frontier, mode, cy, cx);
            const uint32_t omode = (uint32_t)rnd_in(4), kinds = 1u + (uint32_t)rnd_in((omode & RG_ROUTE_KNOWN) ? 15 : 7);
            check_objects(g, H, W, px, py, dead, kinds, omode, rep % 3 == 0 ? 1 : rep % 3 == 1 ? RG_OBJ_MAX_CAP : 1 + rnd_in(RG_OBJ_MAX_CAP));
            check_monsters(g, H, W, px, py, dead, rep % 3 == 0 ? 1 : rep % 3 == 1 ? RG_MON_MAX_CAP : 1 + rnd_in(RG_MON_MAX_CAP));
            check_scout(g, H, W);
        }
    }
    check_refusals();
    check_env_ids();
    printf("%d runs, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
