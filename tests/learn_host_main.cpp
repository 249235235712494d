// A stand-alone host program around the learner's side of the action rule (rogue-gym_amd/csrc/rg_policy_grad.h through rg_readers_host.h's rgh_policy_eval and
// rgh_policy_grad), built by tests/test_policy_grad_host.py with -fsanitize=address,undefined: every array is allocated on the heap at its exact size, so a
// read or write one element past the last row ends the run.  1, 5, 11, 19 and RG_MASK_MAX_KEYS keys, every dtype, masks with 0 to n_keys legal keys and no
// mask, actions of every int32 kind, each upstream gradient present and absent; what comes back is held against the rule's own promises.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rg_readers_host.h"

static uint32_t rnd_state = 2463534242u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static int bad = 0, runs = 0;
#define EXPECT(cond, ...) do { runs++; if (!(cond)) { bad++; if (bad <= 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint16_t to_bf16(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); }
static uint16_t some_f16() {
    static const uint16_t pick[] = {0x0000, 0x8000, 0x0001, 0x83ff, 0x0400, 0x3c00, 0xbc00, 0x4900, 0xc900, 0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00, 0x5500, 0xd500};
    return (rnd() & 1) ? pick[rnd() % 16] : (uint16_t)(0x3000 + rnd() % 0x1800) | (uint16_t)((rnd() & 1) << 15);
}
static float some_f32() {
    static const float pick[] = {0.0f, -0.0f, 1.0f, -1.0f, 80.0f, -80.0f, 3.0e38f, -3.0e38f, INFINITY, -INFINITY, NAN, 1.0e-40f};
    return (rnd() & 3) == 0 ? pick[rnd() % 12] : ((float)(rnd() % 20001) - 10000.0f) * 1.0e-3f;
}
static float some_grad() {
    static const float pick[] = {0.0f, -0.0f, 1.0f, -1.0f, 1.0e30f, -1.0e-30f, INFINITY, NAN};
    return (rnd() & 7) == 0 ? pick[rnd() % 8] : ((float)(rnd() % 8001) - 4000.0f) * 1.0e-3f;
}
static float widen(const void *p, size_t i, int dtype) { return dtype == RG_OBS_F32 ? ((const float *)p)[i] : rg_pol_widen(((const uint16_t *)p)[i], dtype); }

int main() {
    const int key_counts[] = {1, 5, 11, 19, RG_MASK_MAX_KEYS};
    const int64_t row_counts[] = {1, 63, 64, 65, 200};
    for (int nk : key_counts)
        for (int64_t B : row_counts)
            for (int dtype = 0; dtype < 3; dtype++)
                for (int variant = 0; variant < 4; variant++) {  // bit 0: a mask; bit 1: inv_temp 0.7
                    const size_t esz = dtype == RG_OBS_F32 ? 4 : 2, n = (size_t)B * nk;
                    const float inv_temp = (variant & 2) ? 0.7f : 1.0f;
                    void *x = malloc(esz * n), *dx = malloc(esz * n);
                    uint8_t *mask = (variant & 1) ? (uint8_t *)malloc(n) : nullptr;
                    int32_t *a = (int32_t *)malloc(sizeof(int32_t) * B);
                    float *g_lp = (float *)malloc(sizeof(float) * B), *g_ent = (float *)malloc(sizeof(float) * B);
                    float *lp = (float *)malloc(sizeof(float) * B), *ent = (float *)malloc(sizeof(float) * B);
                    for (size_t i = 0; i < n; i++) {
                        if (dtype == RG_OBS_F32) ((float *)x)[i] = some_f32();
                        else if (dtype == RG_OBS_F16) ((uint16_t *)x)[i] = some_f16();
                        else ((uint16_t *)x)[i] = to_bf16(some_f32());
                    }
                    for (int64_t r = 0; r < B; r++) {
                        const int legal = (int)(r % (nk + 1));
                        if (mask)
                            for (int k = 0; k < nk; k++) mask[r * nk + k] = (uint8_t)(((k * 7 + (int)r) % nk) < legal ? 1 + rnd() % 255 : 0);   // (a byte counts as != 0)
                        const int32_t odd[] = {-1, nk, INT32_MIN, INT32_MAX, nk + 31, -33};
                        a[r] = (rnd() & 3) == 0 ? odd[rnd() % 6] : (int32_t)(rnd() % nk);
                        g_lp[r] = some_grad();
                        g_ent[r] = some_grad();
                    }
                    std::string err;
                    EXPECT(rgh_policy_eval(err, B, nk, x, dtype, mask, a, inv_temp, lp, ent) == 0, "eval refused: %s", err.c_str());
                    EXPECT(rgh_policy_eval(err, B, nk, x, dtype, mask, a, inv_temp, nullptr, nullptr) == 0, "eval without outputs refused: %s", err.c_str());
                    for (int which = 0; which < 4; which++) {  // bit 0: g_lp present; bit 1: g_ent present
                        memset(dx, 0x5a, esz * n);
                        EXPECT(rgh_policy_grad(err, B, nk, x, dtype, mask, a, inv_temp, (which & 1) ? g_lp : nullptr, (which & 2) ? g_ent : nullptr, dx) == 0, "grad refused: %s",
                               err.c_str());
                        for (int64_t r = 0; r < B; r++) {
                            int legal = 0, weighs = 0;
                            for (int k = 0; k < nk; k++) {
                                const bool l = !mask || mask[r * nk + k] != 0;
                                const float v = widen(x, (size_t)(r * nk + k), dtype) * inv_temp, d = widen(dx, (size_t)(r * nk + k), dtype);
                                const bool w = l && v == v && v != -INFINITY;
                                legal += l;
                                weighs += w;
                                uint32_t dbits;
                                memcpy(&dbits, &d, 4);
                                if (!w || which == 0) EXPECT(dbits == 0u, "%d keys row %lld key %d dtype %d: the gradient of a key without weight is %g", nk, (long long)r, k, dtype, d);
                                if (d != d) EXPECT(dbits == 0x7fc00000u, "%d keys row %lld key %d dtype %d: NaN bits %08x", nk, (long long)r, k, dtype, dbits);
                            }
                            if (which) continue;
                            EXPECT(ent[r] >= 0.0f && ent[r] <= 3.4657360f, "%d keys row %lld dtype %d: entropy %g", nk, (long long)r, dtype, ent[r]);  // ln 32
                            EXPECT(!(lp[r] > 0.0f), "%d keys row %lld dtype %d: logp %g", nk, (long long)r, dtype, lp[r]);
                            if (legal == 0) EXPECT(lp[r] == 0.0f && ent[r] == 0.0f, "%d keys row %lld dtype %d: no legal key, logp %g entropy %g", nk, (long long)r, dtype, lp[r], ent[r]);
                            else if (a[r] < 0 || a[r] >= nk || (mask && !mask[r * nk + a[r]]))
                                EXPECT(lp[r] == -INFINITY, "%d keys row %lld dtype %d: action %d, logp %g", nk, (long long)r, dtype, a[r], lp[r]);
                            if (weighs == 1) EXPECT(ent[r] == 0.0f, "%d keys row %lld dtype %d: one key weighs, entropy %g", nk, (long long)r, dtype, ent[r]);
                        }
                    }
                    // a refusal writes nothing; no rows is a valid call
                    memset(dx, 0x5a, esz * n);
                    lp[0] = 7.0f;
                    EXPECT(rgh_policy_grad(err, B, nk, x, dtype, mask, a, 0.0f, g_lp, g_ent, dx) != 0 && ((uint8_t *)dx)[0] == 0x5a, "inv_temp 0 was served");
                    EXPECT(rgh_policy_eval(err, B, 33, x, dtype, mask, a, inv_temp, lp, ent) != 0 && lp[0] == 7.0f, "33 keys were served");
                    EXPECT(rgh_policy_eval(err, 0, nk, x, dtype, mask, a, inv_temp, lp, ent) == 0 && lp[0] == 7.0f, "no rows: %s", err.c_str());
                    EXPECT(rgh_policy_grad(err, 0, nk, x, dtype, mask, a, inv_temp, g_lp, g_ent, dx) == 0 && ((uint8_t *)dx)[0] == 0x5a, "no rows: %s", err.c_str());
                    free(x); free(dx); free(mask); free(a); free(g_lp); free(g_ent); free(lp); free(ent);
                }
    // the narrowing against the widening: every binary16 and bfloat16 pattern that is no NaN comes back as it went
    for (uint32_t h = 0; h < 0x10000u; h++)
        for (int dtype = RG_OBS_F16; dtype <= RG_OBS_BF16; dtype++) {
            const float f = rg_pol_widen(h, dtype);
            if (f != f) EXPECT(rg_pol_narrow(f, dtype) == (dtype == RG_OBS_F16 ? 0x7e00u : 0x7fc0u), "NaN %04x dtype %d narrows to %04x", h, dtype, rg_pol_narrow(f, dtype));
            else EXPECT(rg_pol_narrow(f, dtype) == h, "%04x dtype %d narrows to %04x", h, dtype, rg_pol_narrow(f, dtype));
        }
    printf("%d checks, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
