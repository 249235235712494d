// rg_api_state.cpp -- state records, the cell archive that keeps them per hashed state, the partial reset and rg_seed_envs behind the C-ABI: the entry points that
// serve the envs a caller picks, and the staging of their env-id lists (env_ids_stage, which the cuts of rg_api_episode.cpp share).
#include <cstring>

#include "rg_handle.h"
#include "rg_launch.h"
#include "rg_state_io.h"
#include "rg_readers_host.h"  // rgh_env_ids_check

extern "C" {
// ---- state records (rg_state_io.h / rg_state_io.hip) ----
// The layout of this handle's records: fixed by geometry, room grid and the optional arrays, plus the key-log capacity
static void state_layout(const rg_handle *h, RgIoLayout *L) {
    memset(L, 0, sizeof *L);
    const RgConfig &c = h->cfg;
    const uint32_t hw = (uint32_t)c.width * (uint32_t)c.height, nr = (uint32_t)(c.room_num_x * c.room_num_y);
    L->hw = hw; L->H = (uint32_t)c.height; L->W = (uint32_t)c.width; L->rooms = nr;
    L->sections = (c.n_enemies > 0 ? RG_SEC_DCMAP : 0u) | (h->S.dc_walk ? RG_SEC_DCWALK : 0u) | (h->S.obs_rec ? RG_SEC_OBSREC : 0u) | (h->S.ovl ? RG_SEC_OVL : 0u);
    uint32_t off = RG_STATE_HDR_BYTES;
    L->o_cell = off; off += RG_STATE_PAD16(2 * hw);
    L->o_screen = off; off += RG_STATE_PAD16(hw);
    L->o_hist = off; off += RG_STATE_PAD16(hw);
    if (L->sections & RG_SEC_DCMAP) { L->b_dcmap = 2u * RG_DIST_SLOTS * hw; L->o_dcmap = off; off += RG_STATE_PAD16(L->b_dcmap); }
    if (L->sections & RG_SEC_DCWALK) { L->b_dcwalk = 4u * RG_DIST_SLOTS * (uint32_t)c.height * RG_WALK_WORDS(c.width); L->o_dcwalk = off; off += RG_STATE_PAD16(L->b_dcwalk); }
    L->o_status = off; off += 48;
    if (L->sections & RG_SEC_OBSREC) { L->b_obsrec = 4u * RG_OBS_REC_WORDS(nr); L->o_obsrec = off; off += RG_STATE_PAD16(L->b_obsrec); }
    // the SoA words: 13 player / runtime scalars, 12 RNG words, mon_cnt, 9 dist-cache keys + 4 ring words, 7 per room, rooms + 1 overlay positions
    L->n_words = 13 + 12 + 1 + RG_DIST_SLOTS + 4 + 7 * nr + ((L->sections & RG_SEC_OVL) ? nr + 1 : 0);
    L->o_words = off; off += RG_STATE_PAD16(4 * L->n_words);
    L->base = off;
    L->klog_cap = h->S.klog ? (uint32_t)h->S.klog_cap : 0u;
    L->R = off + RG_STATE_PAD16(L->klog_cap);
    L->fp_lo = (uint32_t)h->state_fp; L->fp_hi = (uint32_t)(h->state_fp >> 32);
}

// the word descriptors of the record's SoA section, in record order (state_layout counts them)
static int state_prepare(rg_handle *h) {
    if (!h->io_mark && !dev_alloc(h, &h->io_mark, (size_t)h->S.n)) return 1;
    if (h->io_desc) return 0;
    const RgState &S = h->S;
    const size_t n = (size_t)S.n;
    const int nr = h->cfg.room_num_x * h->cfg.room_num_y;
    std::vector<uint64_t> d;
    auto add = [&](const void *p, int lg, int slots, bool flags = false) {
        for (int s = 0; s < slots; s++)
            d.push_back(((uint64_t)(uintptr_t)((const uint8_t *)p + ((size_t)s * n << lg)) & RG_IO_DESC_PTR_MASK) | ((uint64_t)lg << RG_IO_DESC_LG_SHIFT) |
                        (flags ? RG_IO_DESC_FLAGS : 0ull));
    };
    add(S.p_pos, 1, 1); add(S.p_hp, 2, 1); add(S.p_hpmax, 2, 1); add(S.p_lvl, 2, 1); add(S.p_exp, 2, 1); add(S.food, 2, 1); add(S.quiet, 2, 1);
    add(S.pack_gold, 2, 1); add(S.dlevel, 2, 1); add(S.steps, 2, 1); add(S.flags, 2, 1, true); add(S.reward, 2, 1); add(S.done, 0, 1);
    add(S.rng, 2, 12); add(S.mon_cnt, 2, 1);
    const size_t i_dk = d.size();
    add(S.dc_key, 1, RG_DIST_SLOTS); add(S.dc_head, 0, 1); add(S.dc_len, 0, 1); add(S.dc_part, 1, 1); add(S.dc_own, 1, 1);
    add(S.room_rect, 2, nr); add(S.room_meta, 0, nr);
    const size_t i_w0 = d.size(); add(S.mon_w0, 2, nr);
    const size_t i_hp = d.size(); add(S.mon_hp, 2, nr); add(S.mon_exp, 2, nr);
    const size_t i_gp = d.size(); add(S.gold_pos, 2, nr);
    const size_t i_ga = d.size(); add(S.gold_amt, 2, nr);
    if (S.ovl) add(S.ovl, 1, nr + 1);
    // the words of an EMPTY slot are stale (whatever the generator's tables held there): a dead monster's hp / exp and an absent gold's amount are
    // written as 0, on save and on load, so that equal states give equal records
    std::vector<uint32_t> g(d.size(), 0u);
    for (int sl = 0; sl < RG_DIST_SLOTS; sl++)  // a dist-cache key outside the ring (dc_head and dc_len follow the keys)
        g[i_dk + sl] = (uint32_t)(i_dk + RG_DIST_SLOTS + 1) | ((uint32_t)sl << RG_IO_GUARD_SHIFT) | RG_IO_GUARD_RING;
    for (int r = 0; r < nr; r++) {
        g[i_hp + r] = g[i_hp + nr + r] = (uint32_t)(i_w0 + r + 1) | (24u << RG_IO_GUARD_SHIFT);  // MF_ALIVE: bit 0 of the flag byte
        g[i_ga + r] = (uint32_t)(i_gp + r + 1) | (16u << RG_IO_GUARD_SHIFT);                       // gold present: 0x10000
    }
    RgIoLayout L;
    state_layout(h, &L);
    if (d.size() != L.n_words) { h->err = "state record: word table and layout disagree"; return 1; }
    uint64_t *dd = nullptr;
    uint32_t *gg = nullptr;
    if (!dev_alloc(h, &dd, d.size()) || !dev_alloc(h, &gg, g.size())) return 1;
    HIPCHK(h, hipMemcpy(dd, d.data(), d.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(gg, g.data(), g.size() * 4, hipMemcpyHostToDevice));
    h->io_desc = dd; h->io_guard = gg; h->io_words = (uint32_t)d.size();
    return 0;
}

// env ids of a save, a load or a cut (rg_api_episode.cpp): a device pointer as given, or the host ids checked (rgh_env_ids_check; unique: a load's and a cut's) and
// uploaded.  ONE staging buffer serves them all: every user enqueues this copy and then its kernel on h->stream, so the next user's copy runs behind the last
// user's kernel, and the pageable source is staged before the call returns.
int env_ids_stage(rg_handle *h, const char *what, const int32_t *env_ids, int k, int on_device, bool unique, const int32_t **out) {
    if (on_device) { *out = env_ids; return 0; }
    if (rgh_env_ids_check(h->err, what, env_ids, k, h->S.n, unique)) return 1;
    if (!h->ids_buf || (size_t)k > h->ids_cap) {  // (the old buffer may still be read by a launch in flight: it stays allocated until rg_destroy)
        size_t cap = h->ids_cap ? h->ids_cap : 256;
        while (cap < (size_t)k) cap *= 2;
        if (!dev_alloc(h, &h->ids_buf, cap)) return 1;
        h->ids_cap = cap;
        HIPCHK(h, hipDeviceSynchronize());  // (the allocation was zeroed on the null stream, which the handle's stream may not wait for)
    }
    if (k) HIPCHK(h, hipMemcpyAsync(h->ids_buf, env_ids, (size_t)k * 4, hipMemcpyHostToDevice, h->stream));  // (pageable source: staged before the call returns)
    *out = h->ids_buf;
    return 0;
}

int rg_state_record_bytes(const rg_t *h) {
    if (!h->sub.empty()) { const_cast<rg_t *>(h)->err = "rg_state_record_bytes: not for a handle with config groups"; return -1; }
    RgIoLayout L;
    state_layout(h, &L);
    return (int)L.R;
}

int rg_state_save(rg_t *h, const int32_t *env_ids, int k, int ids_on_device, uint8_t *out_dev) {
    if (!h->sub.empty()) { h->err = "rg_state_save: not for a handle with config groups (one handle per config)"; return 1; }
    if (!out_dev || ((uintptr_t)out_dev & 15u)) { h->err = "rg_state_save: out_dev must be a 16-byte aligned device buffer"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t *ids = nullptr;
    if (!env_ids) k = h->S.n;
    else {
        if (k < 0) { h->err = "rg_state_save: negative record count"; return 1; }
        if (env_ids_stage(h, "rg_state_save", env_ids, k, ids_on_device, false, &ids)) return 1;
    }
    if (k == 0) return 0;
    if (state_prepare(h) || flush_render(h)) return 1;  // (records hold drawn mirrors: no Redraw is pending in them)
    RgIoLayout L;
    state_layout(h, &L);
    rgk_state_save(&h->S, &L, h->io_desc, h->io_guard, ids, k, out_dev, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int rg_state_load(rg_t *h, const uint8_t *rec_dev, size_t rec_bytes, const int32_t *env_ids, int k, int ids_on_device) {
    if (!h->sub.empty()) { h->err = "rg_state_load: not for a handle with config groups (one handle per config)"; return 1; }
    if (!rec_dev || ((uintptr_t)rec_dev & 15u)) { h->err = "rg_state_load: rec_dev must be a 16-byte aligned device buffer"; return 1; }
    if (rec_bytes < RG_STATE_HDR_BYTES || (rec_bytes & 15u) || rec_bytes > 0x7fffffffu) { h->err = "rg_state_load: rec_bytes is not the size of a state record"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t *ids = nullptr;
    if (!env_ids) k = h->S.n;
    else {
        if (k < 0) { h->err = "rg_state_load: negative record count"; return 1; }
        if (env_ids_stage(h, "rg_state_load", env_ids, k, ids_on_device, true, &ids)) return 1;
    }
    if (k == 0) return 0;
    if (state_prepare(h)) return 1;
    if ((size_t)k > h->io_ok_cap) {
        size_t cap = h->io_ok_cap ? h->io_ok_cap : 256;
        while (cap < (size_t)k) cap *= 2;
        if (!dev_alloc(h, &h->io_ok, cap)) return 1;
        h->io_ok_cap = cap;
    }
    RgIoLayout L;
    state_layout(h, &L);
    // A load changes player positions: it PRODUCES the stair set of the next k_step (rg_state.h), like k_build and the debug descent.  The background
    // generators (k_regen, its gate, rg_regen_lanes.hip) read and write only the spare view and the next-level request / structure words, none of which a
    // load writes (it drops a restored env's structure with the same atomic AND as k_build): stream order is enough, nothing is drained.
    h->S.stair_gen = h->stair_gen++;
    rgk_state_load(&h->S, &L, h->io_desc, h->io_guard, ids, k, rec_dev, (uint32_t)rec_bytes, h->io_ok, h->io_mark, h->stream);
    HIPCHK(h, hipGetLastError());
    h->bound_valid = false;  // the bound observation tensor does not show the restored screens: its next call encodes every env
    return 0;
}

// ---- the cell archive (rg_archive.h; k_arc_* in rg_archive.hip, librogue_gym_archive.so) ----
int rg_archive_enable(rg_t *h, int cells) {
    const std::string w = "rg_archive_enable: ";
    if (!h->sub.empty()) { h->err = w + "not for a handle with config groups (no state records; one handle per config)"; return 1; }
    if (h->arc_on) { h->err = w + "the archive is enabled already"; return 1; }
    if (!rg_arc_pow2_in(cells, RG_ARC_CELLS_MIN, RG_ARC_CELLS_MAX)) {
        h->err = w + "cells must be a power of two, " + std::to_string(RG_ARC_CELLS_MIN) + " <= cells <= " + std::to_string(RG_ARC_CELLS_MAX) + ", got " + std::to_string(cells);
        return 1;
    }
    HIPCHK(h, hipSetDevice(h->device));
    RgIoLayout L;
    state_layout(h, &L);
    const size_t n = (size_t)h->S.n, m = n + RG_ARC_SLACK, c = (size_t)cells, had = h->allocs.size();
    RgArchive A = {};
    A.cells = cells; A.R = L.R;
    const bool ok = dev_alloc(h, &A.key, c) && dev_alloc(h, &A.score, c) && dev_alloc(h, &A.steps, c) && dev_alloc(h, &A.seen, c) && dev_alloc(h, &A.chosen, c) &&
                    dev_alloc(h, &A.when, c) && dev_alloc(h, &A.bid, c) && dev_alloc(h, &A.win, c) && dev_alloc(h, &A.slot, m) && dev_alloc(h, &A.stored, m) &&
                    dev_alloc(h, &A.score_in, m) && dev_alloc(h, &A.steps_in, m) && dev_alloc(h, &A.list, n) && dev_alloc(h, &A.cnt, 4) && dev_alloc(h, &A.stat, 4) &&
                    dev_alloc(h, &A.records, c * (size_t)L.R);
    if (!ok) {  // (a table that does not fit: what this call allocated goes back, the handle is as before)
        while (h->allocs.size() > had) { (void)hipFree(h->allocs.back()); h->allocs.pop_back(); }
        (void)hipGetLastError();
        h->err = w + "cells = " + std::to_string(cells) + " records of " + std::to_string(L.R) + " bytes: " + h->err;
        return 1;
    }
    HIPCHK(h, hipMemset(A.slot, 0xff, n * sizeof(int32_t)));  // no env has a slot yet (the slack stays as allocated: zero)
    h->arc = A;
    h->arc_on = true;
    h->arc_serial = 0;
    HIPCHK(h, hipDeviceSynchronize());  // (the allocations were zeroed on the null stream, which the handle's stream may not wait for)
    return 0;
}
static int archive_on(rg_handle *h, const char *what) {
    if (!h->arc_on) { h->err = std::string(what) + ": the archive is not enabled (rg_archive_enable)"; return 1; }
    return 0;
}
int rg_archive_update(rg_t *h, const uint64_t *key_dev, const int32_t *score_dev, const uint8_t *mask_dev) {
    if (archive_on(h, "rg_archive_update")) return 1;
    if (!key_dev) {
        if (!h->nov_on) { h->err = "rg_archive_update: key_dev is NULL and novelty is not enabled (rg_novelty_enable): there is no hash to take"; return 1; }
        key_dev = h->nov.hash;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (state_prepare(h) || flush_render(h)) return 1;  // (records hold drawn mirrors: no Redraw is pending in them)
    RgIoLayout L;
    state_layout(h, &L);
    rgk_archive_update(&h->S, &L, h->io_desc, h->io_guard, &h->arc, key_dev, score_dev, mask_dev, ++h->arc_serial, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int rg_archive_arrays(rg_t *h, rg_archive_arrays_t *out) {
    if (archive_on(h, "rg_archive_arrays")) return 1;
    if (!out) { h->err = "rg_archive_arrays: out is NULL"; return 1; }
    const RgArchive &A = h->arc;
    *out = rg_archive_arrays_t{A.key, A.score, A.steps, A.seen, A.chosen, A.when, A.records, A.slot, A.stored, A.score_in, A.steps_in};
    return 0;
}
int rg_archive_restore(rg_t *h, const int32_t *slot_ids, const int32_t *env_ids, int k, int ids_on_device) {
    if (archive_on(h, "rg_archive_restore")) return 1;
    if (!slot_ids) { h->err = "rg_archive_restore: slot_ids is NULL"; return 1; }
    if (!env_ids) k = h->S.n;
    if (k < 0) { h->err = "rg_archive_restore: negative record count"; return 1; }
    if (k == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t *sid = slot_ids;
    if (!ids_on_device) {
        for (int i = 0; i < k; i++)
            if (slot_ids[i] < 0 || slot_ids[i] >= h->arc.cells) {
                h->err = "rg_archive_restore: slot_ids[" + std::to_string(i) + "] = " + std::to_string(slot_ids[i]) + " is out of range [0, " + std::to_string(h->arc.cells) + ")";
                return 1;
            }
        // (the env ids are checked before anything is launched, as the load itself will check them)
        if (env_ids && rgh_env_ids_check(h->err, "rg_archive_restore", env_ids, k, h->S.n, true)) return 1;
    }
    bool grown = false;
    if (!ids_on_device && (size_t)k > h->arc_sid_cap) {
        size_t cap = h->arc_sid_cap ? h->arc_sid_cap : 256;
        while (cap < (size_t)k) cap *= 2;
        if (!dev_alloc(h, &h->arc_sid, cap)) return 1;
        h->arc_sid_cap = cap; grown = true;
    }
    if ((size_t)k > h->arc_stage_cap) {
        size_t cap = h->arc_stage_cap ? h->arc_stage_cap : 256;
        while (cap < (size_t)k) cap *= 2;
        if (!dev_alloc(h, &h->arc_stage, cap * (size_t)h->arc.R)) return 1;
        h->arc_stage_cap = cap; grown = true;
    }
    if (grown) HIPCHK(h, hipDeviceSynchronize());  // (the allocation was zeroed on the null stream, which the handle's stream may not wait for)
    if (!ids_on_device) {
        HIPCHK(h, hipMemcpyAsync(h->arc_sid, slot_ids, (size_t)k * 4, hipMemcpyHostToDevice, h->stream));  // (pageable source: staged before the call returns)
        sid = h->arc_sid;
    }
    rgk_archive_gather(&h->arc, sid, k, h->arc_stage, h->stream);
    HIPCHK(h, hipGetLastError());
    if (rg_state_load(h, h->arc_stage, (size_t)h->arc.R, env_ids, k, ids_on_device)) return 1;
    rgk_archive_chosen(&h->arc, sid, k, h->io_ok, h->stream);  // (io_ok: per record, whether the load took it)
    HIPCHK(h, hipGetLastError());
    return 0;
}
int rg_archive_stats(rg_t *h, uint64_t *out) {
    if (archive_on(h, "rg_archive_stats")) return 1;
    if (!out) { h->err = "rg_archive_stats: out is NULL"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    unsigned long long st[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(st, h->arc.stat, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out[0] = st[0]; out[1] = st[1]; out[2] = st[2]; out[3] = h->arc_serial;
    return 0;
}
int rg_archive_clear(rg_t *h) {
    if (archive_on(h, "rg_archive_clear")) return 1;
    HIPCHK(h, hipSetDevice(h->device));
    const RgArchive &A = h->arc;
    const size_t c = (size_t)A.cells;
    HIPCHK(h, hipMemsetAsync(A.key, 0, c * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(A.bid, 0, c * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(A.win, 0, c * 8, h->stream));
    for (void *p : {(void *)A.score, (void *)A.steps, (void *)A.seen, (void *)A.chosen, (void *)A.when}) HIPCHK(h, hipMemsetAsync(p, 0, c * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(A.records, 0, c * (size_t)A.R, h->stream));
    HIPCHK(h, hipMemsetAsync(A.slot, 0xff, (size_t)h->S.n * 4, h->stream));  // (the envs' slots of the last update are gone with the table)
    HIPCHK(h, hipMemsetAsync(A.stored, 0, (size_t)h->S.n, h->stream));
    HIPCHK(h, hipMemsetAsync(A.stat, 0, 4 * sizeof(unsigned long long), h->stream));
    h->arc_serial = 0;
    return 0;
}
int rg_archive_offer_host(void *slots, int cells, uint64_t key, int32_t score, uint32_t steps, uint32_t serial, int32_t *slot, int32_t *stored) {
    return rga_offer_host(g_create_err, slots, cells, key, score, steps, serial, slot, stored);
}

// ---- partial reset: the envs a caller picks (rg_kernels.hip k_reset_compact / k_build_list) ----
static int reset_prepare(rg_handle *h) {
    if (!h->io_mark && !dev_alloc(h, &h->io_mark, (size_t)h->S.n)) return 1;
    if (!h->reset_list && !dev_alloc(h, &h->reset_list, (size_t)h->S.n)) return 1;
    if (!h->reset_cnt && !dev_alloc(h, &h->reset_cnt, 4)) return 1;
    return 0;
}

// reset_list[0 .. reset_cnt[0]) is on its way on the stream: rebuild those envs, then produce the stair set of the next k_step
static int reset_listed(rg_handle *h) {
    RgIoLayout L;
    state_layout(h, &L);
    // The build moves players: like a load it PRODUCES the stair set (rg_state.h), rebuilt envs from their new cell, all others carried forward.  The spares
    // are not consulted: a fixed-seed env's spare was built from the same seed and stays valid, a reseeding env takes its own build ticket (atomic, so safe
    // beside a k_regen in flight) -- stream order is enough, nothing is drained.
    h->S.stair_gen = h->stair_gen++;
    { TimedLaunch t(h, 3); rgk_build_list(&h->S, &h->cfg, h->reset_list, h->reset_cnt, h->io_mark, h->stream); }
    rgk_state_stairs(&h->S, &L, h->io_mark, h->stream);
    HIPCHK(h, hipGetLastError());
    h->render_pending = true;
    h->bound_valid = false;  // (as rg_reset: the bound observation tensor's next call encodes every env)
    return 0;
}

int rg_reset_envs(rg_t *h, const int32_t *env_ids, int k, int ids_on_device) {
    if (!h->sub.empty()) { h->err = "rg_reset_envs: not for a handle with config groups (one handle per config)"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    if (!env_ids) return rg_reset(h);  // every env: the list would be 0 .. n - 1
    // host ids: checked before anything is launched; device ids: only their count can be
    if (rgh_env_ids_check(h->err, "rg_reset_envs", ids_on_device ? nullptr : env_ids, k, h->S.n, true)) return 1;
    if (reset_prepare(h)) return 1;
    const uint32_t cnt = (uint32_t)k;
    HIPCHK(h, hipMemcpyAsync(h->reset_cnt, &cnt, 4, hipMemcpyHostToDevice, h->stream));  // (pageable sources: staged before the call returns)
    if (k) HIPCHK(h, hipMemcpyAsync(h->reset_list, env_ids, (size_t)k * 4, ids_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return reset_listed(h);
}

int rg_reset_mask(rg_t *h, const uint8_t *mask_dev) {
    if (!h->sub.empty()) { h->err = "rg_reset_mask: not for a handle with config groups (one handle per config)"; return 1; }
    if (!mask_dev) { h->err = "rg_reset_mask: mask_dev is NULL"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    if (reset_prepare(h)) return 1;
    rgk_reset_compact(mask_dev, h->S.n, h->reset_list, h->reset_cnt, h->stream);  // the mask never reaches the host
    return reset_listed(h);
}

int rg_seed_envs(rg_t *h, const int32_t *env_ids, const uint64_t *seed_lo, const uint64_t *seed_hi, int k) {
    if (!h->sub.empty()) { h->err = "rg_seed_envs: not for a handle with config groups (one handle per config)"; return 1; }
    if (k < 0 || (k > 0 && (!env_ids || !seed_lo))) { h->err = "rg_seed_envs: env_ids and seed_lo must hold k >= 0 entries"; return 1; }
    if (rgh_env_ids_check(h->err, "rg_seed_envs", env_ids, k, h->S.n, false)) return 1;
    if (k == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->spares) {  // rg_seed's rule, for exactly these envs: their spares were generated from the old seeds
        HIPCHK(h, hipStreamSynchronize(h->side));
        HIPCHK(h, hipStreamSynchronize(h->side2));
        HIPCHK(h, hipStreamSynchronize(h->side3));
    }
    size_t lo = (size_t)h->S.n, hi = 0;
    for (int i = 0; i < k; i++) {  // (a repeated id: the last seed wins)
        const size_t e = (size_t)env_ids[i];
        h->seed_lo[e] = seed_lo[i]; h->seed_hi[e] = seed_hi ? seed_hi[i] : 0; h->reseed[e] = 0;
        lo = e < lo ? e : lo; hi = e > hi ? e : hi;
        if (h->spares)
            for (int sl = 0; sl < h->S.sp_slots; sl++) HIPCHK(h, hipMemsetAsync(h->S.sp_ready + (size_t)sl * h->S.n + e, 0, 4, h->stream));
    }
    // only the span that holds the touched envs travels (the envs between them get the values the device already has: the host copies are what was
    // uploaded last, and a `seed: None` env's copy is the base of its per-build hash, which never changes on the device)
    HIPCHK(h, hipMemcpyAsync(h->S.seed_lo + lo, h->seed_lo.data() + lo, (hi - lo + 1) * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->S.seed_hi + lo, h->seed_hi.data() + lo, (hi - lo + 1) * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->S.reseed + lo, h->reseed.data() + lo, hi - lo + 1, hipMemcpyHostToDevice, h->stream));
    if (h->spares) {
        if (h->regen_idle_after >= 0) h->regen_idle_after = 2;  // rebuild the dropped spares, then idle again
        h->regen_bulk = 2;
    }
    return 0;
}
}  // extern "C"
