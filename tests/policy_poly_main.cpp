// A stand-alone host program around the two polynomials of the action rule (rogue-gym_amd/csrc/rg_policy.h: rg_pol_exp2, rg_pol_ln), built by
// tests/test_policy_host.py without a sanitizer (-O2, contraction off) and held against float64 libm, pattern by pattern:
//   rg_pol_exp2  every float32 in [-125, -2^-12] (159 055 873 patterns) and every 64th pattern in (-2^-12, -0]; t = -0.0 gives exactly 1, below -125 exactly 0
//   rg_pol_ln    every float32 in [1, 32] (41 943 041 patterns); monotone; ln 1 = 0 exactly; never negative
// The bounds are MEASURED against the reference, not derived: the sweep is exhaustive and deterministic on any IEEE host, so it asserts "no worse than the
// worst case found", the value below rounded up in its third digit with no further margin; the strided range takes the same constant times 1.05.
//   measured: exp2 worst relative error 7.376e-8 at t = -0.499245495 (exhaustive) and 2.981e-8 at t = -0.00018700026 (strided); not monotone at 83 385
//             steps of the exhaustive range and none of the strided one, each of one ulp (so monotonicity is NOT asserted, the size of a step back is)
//             ln worst absolute error 1.639e-7 at s = 22.6373043, worst relative error for s > 1.0001 1.067e-7 at s = 1.41483152; monotone
//   6.3 s of CPU time, spread over up to 16 threads.
// A third sweep is the reason the entropy's clamp at 0 (rg_pol_stats) is classed `equivalent` in tests/rule_mutants.py: over 10^6 rows with one dominant key the
// entropy before the clamp, lnS - T * inv, is never negative (nor -0.0) -- lnS >= 0 by the sweep above and T * inv <= 0 by the signs of its factors.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "rg_policy.h"

static const double EXP2_REL = 7.38e-8, LN_ABS = 1.64e-7, LN_REL = 1.07e-7;

static float f_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t u_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

struct Worst {
    double rel = 0, abs = 0, rel_hi = 0;
    float at_rel = 0, at_abs = 0, at_rel_hi = 0;
    long back = 0, back_big = 0, negative = 0;
    void merge(const Worst &o) {
        if (o.rel > rel) { rel = o.rel; at_rel = o.at_rel; }
        if (o.abs > abs) { abs = o.abs; at_abs = o.at_abs; }
        if (o.rel_hi > rel_hi) { rel_hi = o.rel_hi; at_rel_hi = o.at_rel_hi; }
        back += o.back; back_big += o.back_big; negative += o.negative;
    }
};

// patterns lo, lo + step, ... <= hi of NEGATIVE floats (a larger pattern is a smaller value): exp2 falls, or steps back by one ulp
static void sweep_exp2(uint32_t lo, uint32_t hi, uint32_t step, Worst *w) {
    uint32_t prev = u_of(rg_pol_exp2(f_of(lo > 0x80000000u ? lo - step : lo)));
    for (uint64_t b = lo; b <= hi; b += step) {
        const float t = f_of((uint32_t)b), p = rg_pol_exp2(t);
        const double ref = exp2((double)t), rel = fabs((double)p - ref) / ref;
        if (rel > w->rel) { w->rel = rel; w->at_rel = t; }
        const uint32_t pb = u_of(p);
        if (pb > prev) { w->back++; if (pb - prev > 1u) w->back_big++; }
        prev = pb;
    }
}
// patterns lo .. hi of floats >= 1: ln rises
static void sweep_ln(uint32_t lo, uint32_t hi, Worst *w) {
    uint32_t prev = u_of(rg_pol_ln(f_of(lo > 0x3f800000u ? lo - 1u : lo)));
    for (uint64_t b = lo; b <= hi; b++) {
        const float s = f_of((uint32_t)b), p = rg_pol_ln(s);
        const double ref = log((double)s), err = fabs((double)p - ref);
        if (err > w->abs) { w->abs = err; w->at_abs = s; }
        if (s > 1.0001f && err / ref > w->rel_hi) { w->rel_hi = err / ref; w->at_rel_hi = s; }
        if (!(p >= 0.0f) || (u_of(p) >> 31)) w->negative++;
        const uint32_t pb = u_of(p);
        if (pb < prev) w->back++;
        prev = pb;
    }
}

template <class F>
static Worst in_threads(uint32_t lo, uint32_t hi, uint32_t step, F f) {
    unsigned n = std::thread::hardware_concurrency();
    n = n < 1 ? 1 : n > 16 ? 16 : n;
    std::vector<Worst> parts(n);
    std::vector<std::thread> th;
    const uint64_t count = ((uint64_t)hi - lo) / step + 1, per = (count + n - 1) / n;
    for (unsigned i = 0; i < n; i++) {
        const uint64_t a = (uint64_t)lo + (uint64_t)i * per * step, b = a + (per - 1) * step;
        if (a > hi) break;
        th.emplace_back(f, (uint32_t)a, (uint32_t)(b > hi ? hi : b), &parts[i]);
    }
    for (auto &t : th) t.join();
    Worst w;
    for (auto &p : parts) w.merge(p);
    return w;
}

static uint64_t rnd_state = 88172645463325252ull;
static uint32_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return (uint32_t)(rnd_state >> 20); }
static float unit() { return (float)(rnd() & 0xffffffu) * 5.9604644775390625e-08f; }

int main() {
    int bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { bad++; printf("FAILED: "); printf(__VA_ARGS__); printf("\n"); } } while (0)
    // exp2: the ends
    EXPECT(u_of(rg_pol_exp2(-0.0f)) == 0x3f800000u && u_of(rg_pol_exp2(0.0f)) == 0x3f800000u, "exp2(-0.0) is not exactly 1");
    EXPECT(u_of(rg_pol_exp2(-125.0f)) == 0x01000000u, "exp2(-125) is not 2^-125");
    EXPECT(u_of(rg_pol_exp2(f_of(0xc2fa0001u))) == 0u && u_of(rg_pol_exp2(-126.0f)) == 0u && u_of(rg_pol_exp2(-INFINITY)) == 0u && u_of(rg_pol_exp2(NAN)) == 0u,
           "exp2 below -125 is not exactly +0");
    // exp2: every pattern of [-125, -2^-12], then every 64th of (-2^-12, -0]
    const Worst e = in_threads(0xb9800000u, 0xc2fa0000u, 1u, [](uint32_t a, uint32_t b, Worst *w) { sweep_exp2(a, b, 1u, w); });
    printf("exp2 exhaustive [-125, -2^-12]: worst relative error %.4g at t = %.9g; %ld steps back, %ld of them more than one ulp\n", e.rel, e.at_rel, e.back, e.back_big);
    EXPECT(e.rel <= EXP2_REL, "exp2 relative error %.4g above %.4g", e.rel, EXP2_REL);
    EXPECT(e.back_big == 0, "exp2 steps back by more than one ulp");
    const Worst e2 = in_threads(0x80000000u, 0xb97fffffu, 64u, [](uint32_t a, uint32_t b, Worst *w) { sweep_exp2(a, b, 64u, w); });
    printf("exp2 every 64th pattern of (-2^-12, -0]: worst relative error %.4g at t = %.9g; %ld steps back, %ld of them more than one ulp\n", e2.rel, e2.at_rel, e2.back, e2.back_big);
    EXPECT(e2.rel <= EXP2_REL * 1.05, "exp2 (strided) relative error %.4g above %.4g", e2.rel, EXP2_REL * 1.05);
    EXPECT(e2.back_big == 0, "exp2 (strided) steps back by more than one ulp");
    // ln: every pattern of [1, 32]
    EXPECT(u_of(rg_pol_ln(1.0f)) == 0u, "ln 1 is not exactly +0");
    const Worst l = in_threads(0x3f800000u, 0x42000000u, 1u, [](uint32_t a, uint32_t b, Worst *w) { sweep_ln(a, b, w); });
    printf("ln exhaustive [1, 32]: worst absolute error %.4g at s = %.9g, worst relative error for s > 1.0001 %.4g at s = %.9g; %ld steps back, %ld negative\n", l.abs, l.at_abs,
           l.rel_hi, l.at_rel_hi, l.back, l.negative);
    EXPECT(l.abs <= LN_ABS, "ln absolute error %.4g above %.4g", l.abs, LN_ABS);
    EXPECT(l.rel_hi <= LN_REL, "ln relative error %.4g above %.4g", l.rel_hi, LN_REL);
    EXPECT(l.back == 0, "ln is not monotone at %ld places", l.back);
    EXPECT(l.negative == 0, "ln is negative at %ld places", l.negative);
    // the entropy before its clamp, over 10^6 rows with one dominant key: never below +0.0
    long below = 0, zero = 0;
    float row[11];
    for (int r = 0; r < 1000000; r++) {
        const int nk = 2 + (int)(rnd() % 10u), kind = r % 4;
        for (int k = 0; k < nk; k++)
            row[k] = kind == 0 ? -90.0f * unit() : kind == 1 ? -10.0f - 10.0f * unit() : kind == 2 ? -15.0f - 72.0f * unit() : -f_of(0x3f800000u - (rnd() % 0x30000000u));
        row[rnd() % (uint32_t)nk] = 0.0f;
        const RgPolStats st = rg_pol_stats((1u << nk) - 1u, nk, [&](int k) { return row[k]; }, 1.0f);
        const float raw = st.lnS - st.T * st.inv;
        if (!(raw >= 0.0f) || (u_of(raw) >> 31)) below++;
        if (raw == 0.0f) zero++;
    }
    printf("entropy before the clamp over 1000000 rows with one dominant key: %ld below +0.0, %ld exactly 0\n", below, zero);
    EXPECT(below == 0, "the entropy before the clamp is below +0.0 in %ld rows: the clamp is reachable", below);
    printf("policy_poly_main: %d bad\n", bad);
    return bad ? 1 : 0;
}
