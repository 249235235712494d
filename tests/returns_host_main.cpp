// A stand-alone host program around the returns rule (rogue-gym_amd/csrc/rg_returns.h through rg_readers_host.h's rgh_gae and rgh_vtrace), built by
// tests/test_returns_host.py with -fsanitize=address,undefined: every array is allocated on the heap at its exact size, so a read or write one element past
// row T - 1 or column N - 1 ends the run.  The shapes of the GPU test (N 1 .. 1000, T 1 .. 100), every optional array present and absent, the edge rows (NaN,
// +-inf, -inf log-probabilities, flag bytes 2 and 255), the exact aliases; what comes back is held against the rule's own promises.
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

static float some_f32() {
    static const float pick[] = {0.0f, -0.0f, 1.0f, -1.0f, 3.0e38f, -3.0e38f, INFINITY, -INFINITY, NAN, 1.0e-40f};
    return (rnd() & 15) == 0 ? pick[rnd() % 10] : ((float)(rnd() % 20001) - 10000.0f) * 1.0e-3f;
}
static float some_logp() { return (rnd() & 15) == 0 ? ((rnd() & 1) ? -INFINITY : NAN) : -(float)(rnd() % 30001) * 1.0e-3f; }
static uint8_t some_flag(unsigned per_mille) {
    static const uint8_t on[] = {1, 2, 255, 0x80};
    return rnd() % 1000 < per_mille ? on[rnd() % 4] : 0;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float *floats(size_t n, float (*make)()) {
    float *p = (float *)malloc(sizeof(float) * (n ? n : 1));
    for (size_t i = 0; i < n; i++) p[i] = make();
    return p;
}
static bool canonical(const float *p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (p[i] != p[i] && bits(p[i]) != 0x7fc00000u) return false;
    return true;
}

int main() {
    const int64_t Ns[] = {1, 63, 64, 65, 257, 1000}, Ts[] = {1, 2, 3, 15, 16, 17, 33, 100};
    const unsigned rates[] = {0, 20, 300, 1000};
    std::string err;
    for (int64_t N : Ns)
        for (int64_t T : Ts)
            for (int variant = 0; variant < 32; variant++) {   // bit 0 value, 1 last_value, 2 done, 3 trunc, 4 trunc_value (with trunc alone)
                if ((variant & 16) && !(variant & 8)) continue;
                if (N * T > 20000 && (variant % 5)) continue;  // (the large shapes: a sample of the variants)
                const size_t n = (size_t)(T * N);
                const unsigned rate = rates[(variant + (unsigned)T) % 4];
                float *reward = floats(n, some_f32), *value = floats(n, some_f32), *tv = floats(n, some_f32), *last = floats((size_t)N, some_f32);
                float *lb = floats(n, some_logp), *lt = floats(n, some_logp);
                uint8_t *done = (uint8_t *)malloc(n), *trunc = (uint8_t *)malloc(n);
                for (size_t i = 0; i < n; i++) { done[i] = some_flag(rate); trunc[i] = some_flag(rate / 2); }
                float *adv = (float *)malloc(4 * n), *ret = (float *)malloc(4 * n), *vs = (float *)malloc(4 * n), *pg = (float *)malloc(4 * n);
                const float *V = (variant & 1) ? value : nullptr, *L = (variant & 2) ? last : nullptr, *TV = (variant & 16) ? tv : nullptr;
                const uint8_t *D = (variant & 4) ? done : nullptr, *TR = (variant & 8) ? trunc : nullptr;
                const float gamma = (variant & 1) ? 0.99f : 1.0f, lam = (variant & 2) ? 0.95f : 1.0f;
                EXPECT(rgh_gae(err, T, N, reward, V, L, D, TR, TV, gamma, lam, adv, ret) == 0, "rgh_gae refused: %s", err.c_str());
                EXPECT(canonical(adv, n) && canonical(ret, n), "a NaN that is not canonical (gae, N %ld T %ld variant %d)", (long)N, (long)T, variant);
                // one output alone gives the same bits
                float *only = (float *)malloc(4 * n);
                EXPECT(rgh_gae(err, T, N, reward, V, L, D, TR, TV, gamma, lam, nullptr, only) == 0 && !memcmp(only, ret, 4 * n), "ret alone differs");
                EXPECT(rgh_gae(err, T, N, reward, V, L, D, TR, TV, gamma, lam, only, nullptr) == 0 && !memcmp(only, adv, 4 * n), "adv alone differs");
                // an end at every step: nothing is carried, adv[t] is its own delta
                if (rate == 1000 && D && !TR && V) {
                    bool own = true;
                    for (size_t i = 0; i < n; i++) {
                        const float want = rg_pg_canon(__builtin_fmaf(gamma, 0.0f, reward[i]) - value[i]);
                        own = own && bits(adv[i]) == bits(want);
                    }
                    EXPECT(own, "all done: adv is not the step's own delta (N %ld T %ld)", (long)N, (long)T);
                }
                // V-trace; on-policy with bars of 1 its vs is GAE's ret
                EXPECT(rgh_vtrace(err, T, N, lb, lt, reward, value, L, D, TR, TV, gamma, lam, 1.0f, 1.0f, 2.0f, vs, pg) == 0, "rgh_vtrace refused: %s", err.c_str());
                EXPECT(canonical(vs, n) && canonical(pg, n), "a NaN that is not canonical (vtrace, N %ld T %ld variant %d)", (long)N, (long)T, variant);
                for (size_t i = 0; i < n; i++)
                    if (lb[i] != lb[i] || lb[i] == -INFINITY) lb[i] = -1.0f;
                EXPECT(rgh_vtrace(err, T, N, lb, lb, reward, value, L, D, TR, TV, gamma, lam, 1.0f, 1.0f, 1.0f, vs, nullptr) == 0, "rgh_vtrace refused: %s", err.c_str());
                EXPECT(rgh_gae(err, T, N, reward, value, L, D, TR, TV, gamma, lam, nullptr, only) == 0 && !memcmp(only, vs, 4 * n), "on-policy vs is not GAE's ret (N %ld T %ld)",
                       (long)N, (long)T);
                // the exact aliases: adv over reward, ret over value
                if (V) {
                    float *r2 = (float *)malloc(4 * n), *v2 = (float *)malloc(4 * n);
                    memcpy(r2, reward, 4 * n);
                    memcpy(v2, value, 4 * n);
                    EXPECT(rgh_gae(err, T, N, r2, v2, L, D, TR, TV, gamma, lam, r2, v2) == 0 && !memcmp(r2, adv, 4 * n) && !memcmp(v2, ret, 4 * n), "aliased outputs differ: %s",
                           err.c_str());
                    free(r2);
                    free(v2);
                }
                free(only);
                free(reward); free(value); free(tv); free(last); free(lb); free(lt); free(done); free(trunc); free(adv); free(ret); free(vs); free(pg);
            }
    // refusals write nothing and name the argument; empty rollouts are valid
    float one[4] = {1, 2, 3, 4}, out[4] = {7, 7, 7, 7};
    EXPECT(rgh_gae(err, -1, 2, one, nullptr, nullptr, nullptr, nullptr, nullptr, 0.9f, 0.9f, out, nullptr) != 0 && err.find("n_steps") != std::string::npos, "n_steps: %s", err.c_str());
    EXPECT(rgh_gae(err, 2, 2, one, nullptr, nullptr, nullptr, nullptr, one, 0.9f, 0.9f, out, nullptr) != 0 && err.find("trunc_value") != std::string::npos, "trunc_value: %s", err.c_str());
    EXPECT(rgh_gae(err, 2, 2, one, nullptr, nullptr, nullptr, nullptr, nullptr, 0.9f, 0.9f, one + 1, nullptr) != 0 && err.find("overlaps") != std::string::npos, "overlap: %s", err.c_str());
    EXPECT(rgh_gae(err, 0, 2, one, nullptr, nullptr, nullptr, nullptr, nullptr, 0.9f, 0.9f, out, nullptr) == 0 && out[0] == 7.0f, "T = 0");
    EXPECT(rgh_gae(err, 2, 0, one, nullptr, nullptr, nullptr, nullptr, nullptr, 0.9f, 0.9f, out, nullptr) == 0 && out[0] == 7.0f, "N = 0");
    printf("%d checks, %d bad\n", runs, bad);
    return bad != 0;
}
