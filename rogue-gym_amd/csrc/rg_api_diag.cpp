// rg_api_diag.cpp -- what reports on a handle behind the C-ABI: the status vector, the action history, the workload counters, the clock probe, the phase trace,
// the launch timings and the config dumps.
#include <cstring>

#include "rg_handle.h"
#include "rg_launch.h"
#include "rg_state_io.h"  // RG_KLOG_PARTIAL

extern "C" {
int rg_status_vec(rg_t *h, uint32_t status_flag, int32_t *out_host) {
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->S.n;
    std::vector<int32_t> st(n * 10);
    HIPCHK(h, hipMemcpyAsync(st.data(), h->S.status, n * 40, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    static const int order[9] = {0, 2, 3, 4, 5, 6, 7, 8, 9};  // StatusFlagInner::to_vector (flags.rs:67-87): gold is not part of it
    size_t k = 0;
    for (size_t e = 0; e < n; e++)
        for (int b = 0; b < 9; b++)
            if (status_flag & (1u << b)) out_host[k++] = st[e * 10 + order[b]];
    return 0;
}

// ---- action-history log (GameState::dump_history, python/src/lib.rs:245-250 -> RunTime::saved_inputs_as_json, core/src/lib.rs:357-375) ----
int rg_history_enable(rg_t *h, int cap_per_env) {
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->sub.empty()) { for (rg_handle *sh : h->sub) SUBCHK(h, sh, rg_history_enable(sh, cap_per_env)); return 0; }
    if (cap_per_env <= 0) { h->err = "rg_history_enable: capacity must be positive"; return 1; }
    if (h->S.klog) { h->err = "rg_history_enable: already enabled"; return 1; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->side) { HIPCHK(h, hipStreamSynchronize(h->side)); HIPCHK(h, hipStreamSynchronize(h->side2)); HIPCHK(h, hipStreamSynchronize(h->side3)); }
    const size_t n = (size_t)h->S.n;
    uint8_t *log = nullptr, *cur = nullptr; uint32_t *len = nullptr;
    if (!dev_alloc(h, &log, n * 2 * (size_t)cap_per_env) || !dev_alloc(h, &len, 2 * n) || !dev_alloc(h, &cur, n)) return 1;
    h->S.klog = log; h->S.klog_len = len; h->S.klog_cur = cur; h->S.klog_cap = cap_per_env;
    h->SP.klog = nullptr;  // the spare view never logs
    return 0;
}

int rg_history_keys(rg_t *h, int env, int which, uint8_t *keys, size_t cap, uint32_t *len) {
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->sub.empty()) {
        if (env < 0 || env >= h->S.n) { h->err = "rg_history_keys: env / which out of range"; return 1; }
        rg_handle *sh = h->sub[h->g_of[env]];
        const int rc = rg_history_keys(sh, h->l_of[env], which, keys, cap, len);
        if (rc) h->err = sh->err;
        return rc;
    }
    if (!h->S.klog) { h->err = "the action history is not enabled (rg_history_enable)"; return 1; }
    if (env < 0 || env >= h->S.n || (which != 0 && which != 1)) { h->err = "rg_history_keys: env / which out of range"; return 1; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->S.n;
    uint8_t cur = 0;
    HIPCHK(h, hipMemcpy(&cur, h->S.klog_cur + env, 1, hipMemcpyDeviceToHost));
    const uint32_t buf = which ? (cur ^ 1u) : cur;
    uint32_t l = 0;
    HIPCHK(h, hipMemcpy(&l, h->S.klog_len + buf * n + env, 4, hipMemcpyDeviceToHost));
    if (len) *len = l & ~RG_KLOG_PARTIAL;
    if (l & RG_KLOG_PARTIAL) { h->err = "action history incomplete: the episode was restored from a state record that did not hold all of its " + std::to_string(l & ~RG_KLOG_PARTIAL) + " keys"; return 2; }
    if (l > (uint32_t)h->S.klog_cap) { h->err = "action history truncated: " + std::to_string(l) + " keys in the episode, capacity " + std::to_string(h->S.klog_cap); return 2; }
    if (keys) {
        if (cap < l) { h->err = "rg_history_keys: buffer too small"; return 3; }
        if (l) HIPCHK(h, hipMemcpy(keys, h->S.klog + ((size_t)env * 2 + buf) * h->S.klog_cap, l, hipMemcpyDeviceToHost));
    }
    return 0;
}

// serde form of InputCode for a key of KeyMap::ai (input.rs:73-100; enum Action / Direction names), pretty-printed like
// serde_json::to_string_pretty (4-space indent), the format of data/learned/*/best-actions.json
static void append_input_code(std::string &s, uint8_t key) {
    static const char *dirs[8] = {"Up", "Down", "Left", "Right", "LeftUp", "RightUp", "LeftDown", "RightDown"};
    const char lower = (char)(key | 0x20);
    int d = -1;
    switch (lower) { case 'k': d = 0; break; case 'j': d = 1; break; case 'h': d = 2; break; case 'l': d = 3; break;
                     case 'y': d = 4; break; case 'u': d = 5; break; case 'b': d = 6; break; case 'n': d = 7; break; }
    s += "    {\n        \"Act\": ";
    if (d >= 0 && key != '.' && key != '>' ) {
        s += std::string("{\n            \"") + ((key & 0x20) ? "Move" : "MoveUntil") + "\": \"" + dirs[d] + "\"\n        }";
    } else s += std::string("\"") + (key == '.' ? "NoOp" : key == 's' ? "Search" : "DownStair") + "\"";
    s += "\n    }";
}

int rg_dump_history(rg_t *h, int env, int which, char *buf, size_t cap, size_t *needed) {
    uint32_t len = 0;
    int rc = rg_history_keys(h, env, which, nullptr, 0, &len);
    if (rc) return rc;
    std::vector<uint8_t> keys(len ? len : 1);
    rc = rg_history_keys(h, env, which, keys.data(), keys.size(), &len);
    if (rc) return rc;
    std::string s = len ? "[\n" : "[]";
    for (uint32_t i = 0; i < len; i++) { append_input_code(s, keys[i]); s += i + 1 < len ? ",\n" : "\n"; }
    if (len) s += "]";
    if (needed) *needed = s.size() + 1;
    if (!buf) return 0;
    if (s.size() + 1 > cap) { h->err = "rg_dump_history: buffer too small"; return 3; }
    memcpy(buf, s.c_str(), s.size() + 1);
    return 0;
}

int rg_counters_ex(rg_t *h, uint64_t *out, int n_out, int reset) {
    HIPCHK(h, hipSetDevice(h->device));
    if (n_out < 0 || n_out > RG_STAT_COLS) { h->err = "rg_counters_ex: at most 16 counters"; return 1; }
    if (!h->sub.empty()) {
        if (out) for (int k = 0; k < n_out; k++) out[k] = 0;
        for (rg_handle *sh : h->sub) {
            uint64_t o[RG_STAT_COLS];
            SUBCHK(h, sh, rg_counters_ex(sh, o, n_out, reset));
            if (out) for (int k = 0; k < n_out; k++) out[k] += o[k];
        }
        return 0;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!h->S.stats) { if (out) memset(out, 0, 8 * (size_t)n_out); return 0; }
    if (out) {
        std::vector<unsigned long long> rows(RG_STAT_COLS * h->stat_rows);
        HIPCHK(h, hipMemcpy(rows.data(), h->S.stats, rows.size() * 8, hipMemcpyDeviceToHost));
        for (int k = 0; k < n_out; k++) out[k] = 0;
        for (size_t r = 0; r < h->stat_rows; r++)
            for (int k = 0; k < n_out; k++) out[k] += rows[r * RG_STAT_COLS + k];
    }
    if (reset) HIPCHK(h, hipMemset(h->S.stats, 0, 8 * RG_STAT_COLS * h->stat_rows));
    return 0;
}
int rg_counters(rg_t *h, uint64_t out[8], int reset) { return rg_counters_ex(h, out, 8, reset); }

int rg_probe_sclk(rg_t *h, double *mhz) {
    HIPCHK(h, hipSetDevice(h->device));
    rgk_probe_clock(h->d_probe, 20000, h->stream);  // ~40 k dependent VALU instructions: 50-100 us
    HIPCHK(h, hipGetLastError());
    unsigned long long r[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(r, h->d_probe, 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (mhz) *mhz = r[1] ? 100.0 * (double)r[0] / (double)r[1] : 0.0;  // s_memrealtime ticks at a constant 100 MHz
    return 0;
}

// development aid: in-kernel phase trace; out = [ceil(n_env / 64)][64] words, one row per wave of the LAST k_step / k_build launch
// (word 0 = record count, words 1.. = phase << 48 | ticks, word 63 = whole-wave ticks)
int rg_prof(rg_t *h, int enable, unsigned long long *out) {
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->sub.empty()) { h->err = "rg_prof: not available for a batch with several config groups"; return 1; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t words = (size_t)((h->S.n + 15) / 16) * 64;  // k_step runs 16..64 envs per wave
    if (out && h->S.prof) HIPCHK(h, hipMemcpy(out, h->S.prof, words * 8, hipMemcpyDeviceToHost));
    if (enable && !h->S.prof) { if (!dev_alloc(h, &h->S.prof, words)) return 1; }
    if (h->S.prof) HIPCHK(h, hipMemset(h->S.prof, 0, words * 8));
    if (!enable) h->S.prof = nullptr;
    return 0;
}

int rg_timing_enable(rg_t *h, int on) {
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->sub.empty()) { for (rg_handle *sh : h->sub) SUBCHK(h, sh, rg_timing_enable(sh, on)); return 0; }
    if (on && h->ev[0].empty())
        for (int k = 0; k < RG_TIMED_KERNELS; k++) {
            h->ev[k].resize(2 * RG_TIMING_MAX);
            for (auto &e : h->ev[k]) HIPCHK(h, hipEventCreate(&e));
        }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->side) { HIPCHK(h, hipStreamSynchronize(h->side)); HIPCHK(h, hipStreamSynchronize(h->side2)); HIPCHK(h, hipStreamSynchronize(h->side3)); }
    for (int k = 0; k < RG_TIMED_KERNELS; k++) { h->ev_used[k] = 0; h->timing_seq[k] = 0; }
    h->timing = on != 0;
    h->timing_stride = on > 1 ? (uint64_t)on : 1;  // on = N > 1: bracket every N-th launch only
    return 0;
}

int rg_timing_read_all(rg_t *h, int n, double *ms, uint64_t *sampled, uint64_t *launches) {
    HIPCHK(h, hipSetDevice(h->device));
    if (n > RG_TIMED_KERNELS) n = RG_TIMED_KERNELS;
    if (!h->sub.empty()) {  // sums over the groups: the counts then are group launches
        for (int k = 0; k < n; k++) { ms[k] = 0; sampled[k] = 0; if (launches) launches[k] = 0; }
        for (rg_handle *sh : h->sub) {
            double m[RG_TIMED_KERNELS]; uint64_t l[RG_TIMED_KERNELS], a[RG_TIMED_KERNELS];
            SUBCHK(h, sh, rg_timing_read_all(sh, n, m, l, a));
            for (int k = 0; k < n; k++) { ms[k] += m[k]; sampled[k] += l[k]; if (launches) launches[k] += a[k]; }
        }
        return 0;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->side) { HIPCHK(h, hipStreamSynchronize(h->side)); HIPCHK(h, hipStreamSynchronize(h->side2)); HIPCHK(h, hipStreamSynchronize(h->side3)); }  // (k_regen's pairs are stamped on the side stream)
    for (int k = 0; k < n; k++) {
        double sum = 0;
        for (size_t i = 0; i + 1 < h->ev_used[k]; i += 2) {
            float t = 0;
            HIPCHK(h, hipEventElapsedTime(&t, h->ev[k][i], h->ev[k][i + 1]));
            sum += t;
        }
        ms[k] = sum; sampled[k] = h->ev_used[k] / 2;
        if (launches) launches[k] = h->timing_seq[k];
        h->ev_used[k] = 0; h->timing_seq[k] = 0;
    }
    return 0;
}
int rg_timing_read(rg_t *h, double ms[4], uint64_t launches[4]) { return rg_timing_read_all(h, 4, ms, launches, nullptr); }
int rg_timing_read_samples(rg_t *h, int kernel, float *ms, int cap, int *n) {
    if (!ms || !n || cap < 0 || kernel < -1 || kernel >= RG_TIMED_KERNELS) { h->err = "rg_timing_read_samples: invalid arguments"; return 1; }
    if (!h->sub.empty()) { h->err = "rg_timing_read_samples: not for a handle with config groups"; return 1; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->side) { HIPCHK(h, hipStreamSynchronize(h->side)); HIPCHK(h, hipStreamSynchronize(h->side2)); HIPCHK(h, hipStreamSynchronize(h->side3)); }
    const int ka = kernel < 0 ? 0 : kernel, kb = kernel < 0 ? 2 : kernel;  // (a step: k_step's begin .. the observation pass's end)
    size_t pairs = (h->ev_used[ka] < h->ev_used[kb] ? h->ev_used[ka] : h->ev_used[kb]) / 2;
    if (pairs > (size_t)cap) pairs = (size_t)cap;
    for (size_t i = 0; i < pairs; i++) HIPCHK(h, hipEventElapsedTime(&ms[i], h->ev[ka][2 * i], h->ev[kb][2 * i + 1]));
    *n = (int)pairs;
    return 0;
}

int rg_dump_config(const rg_t *h, int env, char *buf, size_t cap) {
    if (env < 0 || env >= h->S.n) return 1;
    if (!h->sub.empty()) return rg_dump_config(h->sub[h->g_of[env]], h->l_of[env], buf, cap);
    RgParsed p = h->parsed;  // the group's config with this env's own seed / seed range
    const size_t n = (size_t)h->S.n;
    p.has_seed_range = !h->range_span.empty() && (h->range_span[env] | h->range_span[n + env]) != 0;
    if (p.has_seed_range) {
        p.seed_range[0] = ((unsigned __int128)h->range_lo[n + env] << 64) | h->range_lo[env];
        p.seed_range[1] = p.seed_range[0] + (((unsigned __int128)h->range_span[n + env] << 64) | h->range_span[env]);
    }
    std::string s = rg_dump_config_json(p, h->seed_lo[env], h->seed_hi[env], !h->reseed[env]);
    if (s.size() + 1 > cap) return 1;
    memcpy(buf, s.c_str(), s.size() + 1);
    return 0;
}

int rg_config_schema(char *buf, size_t cap, size_t *needed) {
    std::string s = rg_config_schema_json();
    if (needed) *needed = s.size() + 1;
    if (!buf || s.size() + 1 > cap) return buf ? 1 : 0;
    memcpy(buf, s.c_str(), s.size() + 1);
    return 0;
}

int rg_config_resolved(const char *cfg_json, char *buf, size_t cap) {
    RgParsed p;
    std::string e = rg_parse_config(cfg_json, &p);
    if (!e.empty()) { g_create_err = "Failed to parse config: " + e; return 1; }
    const RgConfig &c = p.cfg;
    std::string s = "{\"weapon\": {\"times\": " + std::to_string(c.wpn_times) + ", \"max\": " + std::to_string(c.wpn_max) + ", \"hit_plus\": " +
                    std::to_string(c.wpn_hit_plus) + ", \"dam_plus\": " + std::to_string(c.wpn_dam_plus) + "}, \"armor_def\": " + std::to_string(c.armor_def) +
                    ", \"init_gold\": " + std::to_string(c.init_gold) + ", \"can_pickup\": " + (c.can_pickup ? "true" : "false") + ", \"init_draws\": [";
    for (size_t i = 0; i + 1 < p.init_draws.size(); i += 2)
        s += std::string(i ? ", " : "") + "[" + std::to_string(p.init_draws[i]) + ", " + std::to_string(p.init_draws[i + 1]) + "]";
    s += "], \"symbols\": " + std::to_string(c.symbols) + ", \"n_enemies\": " + std::to_string(c.n_enemies) + "}";
    if (s.size() + 1 > cap) { g_create_err = "rg_config_resolved: buffer too small"; return 1; }
    memcpy(buf, s.c_str(), s.size() + 1);
    return 0;
}

int rg_config_canonical(const char *cfg_json, char *buf, size_t cap) {
    RgParsed p;
    std::string e = rg_parse_config(cfg_json, &p);
    if (!e.empty()) { g_create_err = "Failed to parse config: " + e; return 1; }
    std::string s = rg_dump_config_json(p, p.seed_lo, p.seed_hi, p.has_seed);
    if (s.size() + 1 > cap) { g_create_err = "buffer too small"; return 1; }
    memcpy(buf, s.c_str(), s.size() + 1);
    return 0;
}

}  // extern "C"
