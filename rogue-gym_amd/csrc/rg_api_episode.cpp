// rg_api_episode.cpp -- episode accounting and count-based novelty behind the C-ABI: the two passes that follow the envs' episodes, with one list-or-mask rule for their cuts.
#include <algorithm>

#include "rg_handle.h"
#include "rg_launch.h"
#include "rg_readers_host.h"  // nov_key_check, rgh_env_ids_check

extern "C" {
// The envs a cut serves -> the launcher's (slots, ids): no list, the mask's or every env; a list of k, checked before anything is launched when it is the host's (two
// groups on one lane, two lanes on one table would race), taken as given but for its length when it is the device's.
static int cut_targets(rg_handle *h, const char *what, const int32_t *env_ids, int k, int ids_on_device, const uint8_t *mask_dev, int *slots, const int32_t **ids) {
    if (env_ids && mask_dev) { h->err = std::string(what) + ": both env_ids and mask_dev are given: a list or a mask, not both"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    *ids = nullptr;
    *slots = h->S.n;
    if (!env_ids) return 0;
    if (ids_on_device && rgh_env_ids_check(h->err, what, nullptr, k, h->S.n, true)) return 1;
    if (env_ids_stage(h, what, env_ids, k, ids_on_device, true, ids)) return 1;
    *slots = k;
    return 0;
}
// ---- episode accounting and the scout reward (rg_episode.h; k_episode in rg_episode.hip) ----
int rg_episode_enable(rg_t *h, uint32_t what, int log_cap) {
    if (!h->sub.empty()) { h->err = "rg_episode_enable: not for a handle with config groups (one handle per config)"; return 1; }
    if (!h->cfg.auto_reset) { h->err = "rg_episode_enable: the handle was created without auto-reset: its episodes do not end inside rg_step"; return 1; }
    if (h->ep_on) { h->err = "rg_episode_enable: episode accounting is enabled already"; return 1; }
    if (what != RG_EP_STATS && what != RG_EP_WHAT_ALL) { h->err = "rg_episode_enable: what must be RG_EP_STATS (1) or RG_EP_STATS | RG_EP_SCOUT (3), got " + std::to_string(what); return 1; }
    if (log_cap < 0) { h->err = "rg_episode_enable: negative log_cap"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t m = (size_t)h->S.n + RG_EP_SLACK;
    RgEpisode A = {};
    if (!dev_alloc(h, &A.ret, m) || !dev_alloc(h, &A.len, m) || !dev_alloc(h, &A.depth, m) || !dev_alloc(h, &A.level, m) || !dev_alloc(h, &A.scout_sum, m) || !dev_alloc(h, &A.died, m) ||
        !dev_alloc(h, &A.time_limit, m) || !dev_alloc(h, &A.last_return, m) || !dev_alloc(h, &A.last_length, m) || !dev_alloc(h, &A.last_depth, m) || !dev_alloc(h, &A.last_cause, m))
        return 1;
    A.seen_bytes = rg_ep_seen_bytes(h->S.hw);
    if (what & RG_EP_SCOUT)
        if (!dev_alloc(h, &A.scout, m) || !dev_alloc(h, &A.seen, m * (size_t)A.seen_bytes)) return 1;
    A.log_cap = log_cap;
    if (log_cap > 0)
        if (!dev_alloc(h, &A.log, (size_t)log_cap) || !dev_alloc(h, &A.log_cnt, 4)) return 1;
    h->ep = A;
    h->ep_on = true;
    h->ep_serial = 0;
    // (the allocations were zeroed on the null stream, which the handle's stream may not wait for)
    HIPCHK(h, hipDeviceSynchronize());
    rgk_episode(&h->S, &h->cfg, &h->ep, h->S.n, nullptr, nullptr, 1, 0, 0u, h->stream);  // every lane: a cut without record
    HIPCHK(h, hipGetLastError());
    return 0;
}
static int episode_on(rg_handle *h, const char *what) {
    if (!h->ep_on) { h->err = std::string(what) + ": episode accounting is not enabled (rg_episode_enable)"; return 1; }
    return 0;
}
int rg_episode_update(rg_t *h) {
    if (episode_on(h, "rg_episode_update")) return 1;
    HIPCHK(h, hipSetDevice(h->device));
    rgk_episode(&h->S, &h->cfg, &h->ep, h->S.n_keys, nullptr, nullptr, 0, 0, ++h->ep_serial, h->stream);  // the envs the last step played
    HIPCHK(h, hipGetLastError());
    return 0;
}
int rg_episode_cut(rg_t *h, const int32_t *env_ids, int k, int ids_on_device, const uint8_t *mask_dev, int record) {
    if (episode_on(h, "rg_episode_cut")) return 1;
    const int32_t *ids;
    int slots;
    if (cut_targets(h, "rg_episode_cut", env_ids, k, ids_on_device, mask_dev, &slots, &ids)) return 1;
    rgk_episode(&h->S, &h->cfg, &h->ep, slots, ids, mask_dev, 1, record ? 1 : 0, ++h->ep_serial, h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int rg_episode_arrays(rg_t *h, rg_episode_arrays_t *out) {
    if (episode_on(h, "rg_episode_arrays")) return 1;
    if (!out) { h->err = "rg_episode_arrays: out is NULL"; return 1; }
    const RgEpisode &A = h->ep;
    *out = rg_episode_arrays_t{A.ret, A.len, A.depth, A.died, A.time_limit, A.last_return, A.last_length, A.last_depth, A.last_cause, A.scout, A.seen, A.seen_bytes};
    return 0;
}
int rg_episode_log_read(rg_t *h, rg_episode_rec *out_host, int cap, int *n, uint64_t *dropped) {
    if (episode_on(h, "rg_episode_log_read")) return 1;
    if (!n) { h->err = "rg_episode_log_read: n is NULL"; return 1; }
    *n = 0;
    if (dropped) *dropped = 0;
    if (!h->ep.log) return 0;  // no log: nothing to read
    if (!out_host || cap < h->ep.log_cap) { h->err = "rg_episode_log_read: out_host must hold the log's capacity, " + std::to_string(h->ep.log_cap) + " records"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    uint32_t cnt = 0;
    HIPCHK(h, hipMemcpyAsync(&cnt, h->ep.log_cnt, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint32_t got = cnt < (uint32_t)h->ep.log_cap ? cnt : (uint32_t)h->ep.log_cap;
    if (got) HIPCHK(h, hipMemcpy(out_host, h->ep.log, (size_t)got * sizeof(rg_episode_rec), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemsetAsync(h->ep.log_cnt, 0, 4, h->stream));
    std::sort(out_host, out_host + got, [](const rg_episode_rec &a, const rg_episode_rec &b) { return a.serial != b.serial ? a.serial < b.serial : a.env < b.env; });
    *n = (int)got;
    if (dropped) *dropped = cnt - got;
    return 0;
}
// ---- count-based novelty (rg_novelty.h; k_nov_* in rg_novelty.hip) ----
int rg_novelty_enable(rg_t *h, int what, uint32_t scope, int radius_y, int radius_x, int cap, int gcap) {
    const std::string w = "rg_novelty_enable: ";
    if (!h->sub.empty()) { h->err = w + "not for a handle with config groups (one handle per config)"; return 1; }
    if (!h->cfg.auto_reset) { h->err = w + "the handle was created without auto-reset: its episodes do not end inside rg_step"; return 1; }
    if (h->nov_on) { h->err = w + "novelty is enabled already"; return 1; }
    if (nov_key_check(h->err, w, what, radius_y, radius_x)) return 1;
    if (scope == 0 || (scope & ~(RG_NOV_EPISODE | RG_NOV_GLOBAL))) { h->err = w + "scope must be RG_NOV_EPISODE (1), RG_NOV_GLOBAL (2) or both (3), got " + std::to_string(scope); return 1; }
    if ((scope & RG_NOV_EPISODE) && !rg_nov_pow2_in(cap, RG_NOV_CAP_MIN, RG_NOV_CAP_MAX)) {
        h->err = w + "cap must be a power of two, " + std::to_string(RG_NOV_CAP_MIN) + " <= cap <= " + std::to_string(RG_NOV_CAP_MAX) + ", got " + std::to_string(cap);
        return 1;
    }
    if ((scope & RG_NOV_GLOBAL) && !rg_nov_pow2_in(gcap, RG_NOV_GCAP_MIN, RG_NOV_GCAP_MAX)) {
        h->err = w + "gcap must be a power of two, " + std::to_string(RG_NOV_GCAP_MIN) + " <= gcap <= " + std::to_string(RG_NOV_GCAP_MAX) + ", got " + std::to_string(gcap);
        return 1;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->S.n, m = n + RG_NOV_SLACK, had = h->allocs.size();
    RgNovelty A = {};
    A.what = what; A.ry = radius_y; A.rx = radius_x;
    bool ok = dev_alloc(h, &A.hash, m) && dev_alloc(h, &A.gen, n) && dev_alloc(h, &A.stat, 4);
    if (ok && (scope & RG_NOV_EPISODE)) { A.cap = cap; ok = dev_alloc(h, &A.count, m) && dev_alloc(h, &A.tab, n * (size_t)cap); }
    if (ok && (scope & RG_NOV_GLOBAL)) { A.gcap = gcap; ok = dev_alloc(h, &A.gcount, m) && dev_alloc(h, &A.gslot, n) && dev_alloc(h, &A.gtab, (size_t)gcap); }
    if (!ok) {  // (a table that does not fit: what this call allocated goes back, the handle is as before)
        while (h->allocs.size() > had) { (void)hipFree(h->allocs.back()); h->allocs.pop_back(); }
        h->err = w + h->err;
        return 1;
    }
    h->nov = A;
    h->nov_on = true;
    h->nov_calls = 0;
    // (the allocations were zeroed on the null stream, which the handle's stream may not wait for)
    HIPCHK(h, hipDeviceSynchronize());
    if (flush_render(h)) return 1;
    rgk_novelty(&h->S, &h->cfg, &h->nov, h->S.n, nullptr, nullptr, 1, h->stream);  // every env: generation 1, its present state a first visit
    HIPCHK(h, hipGetLastError());
    return 0;
}
static int novelty_on(rg_handle *h, const char *what) {
    if (!h->nov_on) { h->err = std::string(what) + ": novelty is not enabled (rg_novelty_enable)"; return 1; }
    return 0;
}
int rg_novelty_update(rg_t *h) {
    if (novelty_on(h, "rg_novelty_update")) return 1;
    HIPCHK(h, hipSetDevice(h->device));
    if (flush_render(h)) return 1;
    rgk_novelty(&h->S, &h->cfg, &h->nov, h->S.n_keys, nullptr, nullptr, 0, h->stream);  // the envs the last step played
    HIPCHK(h, hipGetLastError());
    h->nov_calls++;
    return 0;
}
int rg_novelty_cut(rg_t *h, const int32_t *env_ids, int k, int ids_on_device, const uint8_t *mask_dev) {
    if (novelty_on(h, "rg_novelty_cut")) return 1;
    const int32_t *ids;
    int slots;
    if (cut_targets(h, "rg_novelty_cut", env_ids, k, ids_on_device, mask_dev, &slots, &ids)) return 1;
    if (flush_render(h)) return 1;
    rgk_novelty(&h->S, &h->cfg, &h->nov, slots, ids, mask_dev, 1, h->stream);
    HIPCHK(h, hipGetLastError());
    h->nov_calls++;
    return 0;
}
int rg_novelty_arrays(rg_t *h, rg_novelty_arrays_t *out) {
    if (novelty_on(h, "rg_novelty_arrays")) return 1;
    if (!out) { h->err = "rg_novelty_arrays: out is NULL"; return 1; }
    *out = rg_novelty_arrays_t{h->nov.hash, h->nov.count, h->nov.gcount};
    return 0;
}
int rg_novelty_stats(rg_t *h, uint64_t *out) {
    if (novelty_on(h, "rg_novelty_stats")) return 1;
    if (!out) { h->err = "rg_novelty_stats: out is NULL"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    unsigned long long st[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(st, h->nov.stat, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out[0] = st[0]; out[1] = st[1]; out[2] = st[2]; out[3] = h->nov_calls;
    return 0;
}
int rg_novelty_table_read(rg_t *h, uint64_t *hashes_host, uint32_t *counts_host, int cap, int *n) {
    if (novelty_on(h, "rg_novelty_table_read")) return 1;
    if (!n) { h->err = "rg_novelty_table_read: n is NULL"; return 1; }
    *n = 0;
    if (!h->nov.gtab) return 0;  // no global table: nothing to read
    if ((hashes_host == nullptr) != (counts_host == nullptr)) { h->err = "rg_novelty_table_read: hashes_host and counts_host go together"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<std::pair<uint64_t, uint32_t>> rows;
    const size_t piece = (size_t)1 << 20;  // slots per copy: 16 MB of host memory at a time, whatever gcap is
    std::vector<RgNovSlot> buf(std::min(piece, (size_t)h->nov.gcap));
    for (size_t at = 0; at < (size_t)h->nov.gcap; at += piece) {
        const size_t cnt = std::min(piece, (size_t)h->nov.gcap - at);
        HIPCHK(h, hipMemcpy(buf.data(), h->nov.gtab + at, cnt * sizeof(RgNovSlot), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; i++)
            if (buf[i].hash) rows.emplace_back(buf[i].hash, buf[i].count);
    }
    *n = (int)rows.size();
    if (!hashes_host) return 0;
    if (cap < (int)rows.size()) { h->err = "rg_novelty_table_read: cap = " + std::to_string(cap) + " entries for " + std::to_string(rows.size()) + " occupied slots"; return 1; }
    std::sort(rows.begin(), rows.end());
    for (size_t i = 0; i < rows.size(); i++) { hashes_host[i] = rows[i].first; counts_host[i] = rows[i].second; }
    return 0;
}
int rg_novelty_clear(rg_t *h) {
    if (novelty_on(h, "rg_novelty_clear")) return 1;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->nov.gtab) HIPCHK(h, hipMemsetAsync(h->nov.gtab, 0, (size_t)h->nov.gcap * sizeof(RgNovSlot), h->stream));
    HIPCHK(h, hipMemsetAsync(h->nov.stat, 0, 4 * sizeof(unsigned long long), h->stream));
    h->nov_calls = 0;
    return 0;
}
}  // extern "C"
