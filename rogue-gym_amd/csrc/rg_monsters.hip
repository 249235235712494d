// rg_monsters.hip -- the nearest monsters of every env as a table of 16-byte rows, and the threat words, on the device (rg_monsters; gfx950).
//
//   k_monsters<K> : one env per lane; the nearest K (4, 8 or 16) qualifiers kept sorted in registers
//
// A pass of its own behind the step, in a translation unit of its own, as rg_episode.hip is: nothing here touches the code generation of the kernels whose
// register counts the resource tests pin.  The rule itself is rg_monsters.h's, shared with the host entry point.
// RG_MON_ALL is PRIVILEGED (rg_monsters.h): it lists monsters the screen does not show, with their hit points.
#include "rg_device.h"
#include "rg_monsters.h"

#define MON_THREADS 256
#define MON_BATCH 4   // slots whose words and cell gathers are in flight together

// what the pass reads of the game state (the few arrays, not RgState by value) and where it writes
struct MonView {
    const uint16_t *p_pos; const uint32_t *flags; const uint16_t *cell; const uint32_t *room_rect; const uint8_t *room_meta;
    const uint32_t *mon_w0; const int32_t *mon_hp; const int32_t *ext;
    int16_t *table; int32_t *threat;
    int32_t n, hw, W, H, rnx, rny, rooms, cap;
    uint32_t mode;
    uint64_t tiles[4];   // RgConfig::mon[k].tile, eight kinds per word: four scalars, selected by compares -- a lane-indexed table would be a memory load
};

// The sorted list: per entry the order key and the word beside it (rg_monsters.h), as two register arrays
template <int K> struct MonList { uint64_t key[K]; uint32_t pay[K]; };

// (key, pay) joins the ascending list and the largest drops out: a chain of K compare-exchanges, every index a compile-time constant
template <int K> static __device__ __forceinline__ void mon_insert(MonList<K> &a, uint64_t key, uint32_t pay) {
#pragma unroll
    for (int i = 0; i < K; i++) {
        const bool lt = key < a.key[i];
        const uint64_t k_lo = lt ? key : a.key[i], k_hi = lt ? a.key[i] : key;
        const uint32_t p_lo = lt ? pay : a.pay[i], p_hi = lt ? a.pay[i] : pay;
        a.key[i] = k_lo; a.pay[i] = p_lo;
        key = k_hi; pay = p_hi;
    }
}

// Per env, loaded once: the player's position, the flag word, the id of the player's assigned area and that room's rect and meta.  The slot loop runs over
// the config's rooms MON_BATCH at a time: the batch's monster words are coalesced loads ([slot][n]), then one gathered cell word per alive slot, all in
// flight together -- three dependent round trips for a config of four rooms: position, flags and monster words; the room and the cells; the stores; a slot joins the list only when some lane of the wave has a qualifier in it (one ballot), so the chain is paid per qualifying monster
// of the wave, not per slot.  The list and the threat words live in registers: no dynamically indexed array, no scratch, no LDS.  A caller's cap uses the
// next instance up and stores cap rows, each one 16-byte store at the env's row of the HANDLE (ext), so config groups fill one table.
template <int K>
__global__ void __launch_bounds__(MON_THREADS) k_monsters(const MonView V) {
    const int e = blockIdx.x * MON_THREADS + threadIdx.x;
    const bool active = e < V.n;
    const int n = V.n;
    const bool all = V.mode == RG_MON_ALL;
    uint32_t fl = RG_FLAG_DEAD;
    RgMonEnv E = {0, 0, V.H, 0, 0, 0, 0, 0, 0, 0, 0, false, false};
    size_t xe = 0;
    if (active) {
        const uint32_t pos = V.p_pos[e];
        fl = V.flags[e];
        xe = V.ext ? (size_t)V.ext[e] : (size_t)e;
        E.px = POS_X(pos); E.py = POS_Y(pos);
        const int id = rg_mon_area(E, E.px, E.py, V.W, V.H, V.rnx, V.rny);
        if (id >= 0) rg_mon_room(E, V.room_rect[(size_t)id * n + e], V.room_meta[(size_t)id * n + e]);
    }
    const bool live = active && !(fl & RG_FLAG_DEAD);
    MonList<K> a;
#pragma unroll
    for (int i = 0; i < K; i++) { a.key[i] = RG_MON_EMPTY_KEY; a.pay[i] = 0u; }
    RgMonThreat T;
    rg_mon_threat_init(T);
    const uint16_t *grid = V.cell + (size_t)(active ? e : 0) * (size_t)V.hw;
    for (int s0 = 0; s0 < V.rooms; s0 += MON_BATCH) {
        uint32_t w[MON_BATCH], c[MON_BATCH];
        int32_t hp[MON_BATCH];
#pragma unroll
        for (int j = 0; j < MON_BATCH; j++) {  // (asked of every env, dead ones included: the first batch is then in flight beside the position and the flag word)
            const bool in = active && s0 + j < V.rooms;
            w[j] = in ? V.mon_w0[(size_t)(s0 + j) * n + e] : 0u;
            hp[j] = in && all ? V.mon_hp[(size_t)(s0 + j) * n + e] : 0;
        }
#pragma unroll
        for (int j = 0; j < MON_BATCH; j++) {
            const int x = POS_X(w[j]), y = POS_Y(w[j]);
            const bool alive = live && ((w[j] >> 24) & MF_ALIVE) && x < V.W && y < V.H;   // (a position outside the grid is no state the stepper makes: nothing is read for it)
            if (!alive) w[j] = 0u;
            c[j] = alive ? grid[y * V.W + x] : 0u;
        }
#pragma unroll
        for (int j = 0; j < MON_BATCH; j++) {
            const bool alive = (w[j] >> 24) & MF_ALIVE;
            const int x = POS_X(w[j]), y = POS_Y(w[j]);
            const bool shown = alive && rg_mon_shown(E, c[j], x, y), q = all ? alive : shown;
            if (alive) rg_mon_threat_add(T, E.px, E.py, x, y, shown, q);
            if (__any(q)) {  // (wave-uniform)
                const uint32_t t = (w[j] >> 16) & 0xffu;
                const uint64_t tq = t < 8 ? V.tiles[0] : t < 16 ? V.tiles[1] : t < 24 ? V.tiles[2] : V.tiles[3];
                mon_insert<K>(a, q ? rg_mon_key(E.px, E.py, x, y, shown, s0 + j) : RG_MON_EMPTY_KEY,
                              q ? rg_mon_pay((uint32_t)(tq >> (8 * (t & 7u))), (w[j] >> 24) & MF_ACTIVE, hp[j]) : 0u);
            }
        }
    }
    if (!active) return;
    if (V.table) {
        u4v *rows = reinterpret_cast<u4v *>(V.table) + xe * (size_t)V.cap;
#pragma unroll
        for (int i = 0; i < K; i++)
            if (i < V.cap) {
                uint32_t r[4];
                rg_mon_row(a.key[i], a.pay[i], E.px, E.py, V.mode, r);
                rows[i] = u4v{r[0], r[1], r[2], r[3]};
            }
    }
    if (V.threat) reinterpret_cast<u4v *>(V.threat)[xe] = u4v{(uint32_t)T.adjacent, (uint32_t)T.nearest, (uint32_t)T.attack, (uint32_t)T.count};
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launcher: defined here against the prototype the host units call it by
// ---------------------------------------------------------------------------------------------
extern "C" {
// mode: RG_MON_SHOWN / RG_MON_ALL; cap: 1 .. RG_MON_MAX_CAP when table is given; table / threat: 16-byte aligned, either may be NULL (checked by the caller)
void rgk_monsters(const RgState *S, const RgConfig *c, uint32_t mode, int cap, int16_t *table, int32_t *threat, hipStream_t st) {
    if (S->n <= 0) return;
    MonView V = {S->p_pos, S->flags, S->cell, S->room_rect, S->room_meta, S->mon_w0, S->mon_hp, S->ext, table, threat,
                 S->n, S->hw, c->width, c->height, c->room_num_x, c->room_num_y, c->room_num_x * c->room_num_y, table ? cap : 0, mode, {0, 0, 0, 0}};
    for (int k = 0; k < RG_MAX_ENEMY_KINDS + 6; k++) V.tiles[k >> 3] |= (uint64_t)c->mon[k].tile << (8 * (k & 7));
    const int blocks = (S->n + MON_THREADS - 1) / MON_THREADS;
    if (V.cap <= 4) hipLaunchKernelGGL((k_monsters<4>), dim3(blocks), dim3(MON_THREADS), 0, st, V);
    else if (V.cap <= 8) hipLaunchKernelGGL((k_monsters<8>), dim3(blocks), dim3(MON_THREADS), 0, st, V);
    else hipLaunchKernelGGL((k_monsters<16>), dim3(blocks), dim3(MON_THREADS), 0, st, V);
}
}
