// A stand-alone host program around the action rule (rogue-gym_amd/csrc/rg_policy.h through rg_readers_host.h's rgh_act), built by tests/test_policy_host.py
// with -fsanitize=address,undefined: every grid, key list and logit row is allocated on the heap at its exact size, so a read one element past a row or one
// cell past the grid ends the run.  Key lists of 1, 11, 19 and RG_MASK_MAX_KEYS keys, every dtype, every mode, the player on every border cell of the grid;
// what comes back is held against the rule's own promises (a chosen key is legal, logp and entropy are finite where they must be).
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
// binary16 patterns of a few chosen kinds: the rule widens them itself
static uint16_t some_f16() {
    static const uint16_t pick[] = {0x0000, 0x8000, 0x0001, 0x83ff, 0x0400, 0x3c00, 0xbc00, 0x4900, 0xc900, 0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00, 0x5500, 0xd500};
    return (rnd() & 1) ? pick[rnd() % 16] : (uint16_t)(0x3000 + rnd() % 0x1800) | (uint16_t)((rnd() & 1) << 15);
}
static float some_f32() {
    static const float pick[] = {0.0f, -0.0f, 1.0f, -1.0f, 80.0f, -80.0f, 3.0e38f, -3.0e38f, INFINITY, -INFINITY, NAN, 1.0e-40f};
    return (rnd() & 3) == 0 ? pick[rnd() % 12] : ((float)(rnd() % 20001) - 10000.0f) * 1.0e-3f;
}

int main() {
    const char all[] = ".hjklnbuy>sHJKLNBUY";
    std::vector<std::string> lists = {"s", ".hjklnbuy>s", all, ""};
    for (int k = 0; k < RG_MASK_MAX_KEYS; k++) lists[3].push_back(all[(k * 7) % 19]);
    const int sizes[][2] = {{5, 5}, {3, 7}, {1, 1}, {2, 9}};
    for (auto &hw : sizes) {
        const int H = hw[0], W = hw[1];
        for (int py = 0; py < H; py++)
            for (int px = 0; px < W; px++) {
                if (H >= 3 && W >= 3 && px > 0 && py > 0 && px < W - 1 && py < H - 1 && (rnd() & 1)) continue;  // every border cell, half of the inner ones
                uint16_t *cells = (uint16_t *)malloc(sizeof(uint16_t) * H * W);
                for (int i = 0; i < H * W; i++) cells[i] = (uint16_t)((rnd() % 8) | ((rnd() % 4 == 0) ? 0x20 : 0) | ((rnd() % 8 == 0) ? 0x100 : 0));
                for (const std::string &list : lists)
                    for (int dtype = 0; dtype < 3; dtype++)
                        for (uint32_t mode = 0; mode < 3; mode++) {
                            const int nk = (int)list.size();
                            uint8_t *keys = (uint8_t *)malloc(nk);
                            memcpy(keys, list.data(), nk);
                            const size_t esz = dtype == RG_OBS_F32 ? 4 : 2;
                            void *logits = malloc(esz * nk);
                            for (int k = 0; k < nk; k++) {
                                if (dtype == RG_OBS_F32) ((float *)logits)[k] = some_f32();
                                else if (dtype == RG_OBS_F16) ((uint16_t *)logits)[k] = some_f16();
                                else ((uint16_t *)logits)[k] = to_bf16(some_f32());
                            }
                            rg_act_opts o = {(rnd() & 1) ? 1.0f : 0.37f, mode == RG_ACT_SAMPLE ? 0.25f : 0.0f, mode == RG_ACT_SAMPLE ? 0.5f : 0.0f, mode, rnd() * 0x100000001ull, rnd()};
                            const int dead = rnd() % 8 == 0, teacher = (rnd() & 1) ? keys[rnd() % nk] : (int)(rnd() % 256), given = (int)(rnd() % (nk + 2)) - 1;
                            uint8_t key = 0, source = 9;
                            int32_t action = -9;
                            float logp = 7.0f, entropy = -7.0f;
                            std::string err;
                            const int rc = rgh_act(err, cells, H, W, px, py, dead, keys, nk, logits, dtype, &o, rnd(), teacher, given, &key, &action, &logp, &entropy, &source);
                            EXPECT(rc == 0, "refused: %s", err.c_str());
                            uint8_t row[RG_MASK_MAX_KEYS];
                            std::string err2;
                            EXPECT(rgh_action_mask(err2, cells, H, W, px, py, dead, keys, nk, row) == 0, "mask refused: %s", err2.c_str());
                            int legal = 0;
                            for (int k = 0; k < nk; k++) legal += row[k];
                            const char *where = "%dx%d (%d, %d) %d keys dtype %d mode %u: key %u action %d logp %g entropy %g source %u";
                            EXPECT(entropy >= 0.0f && entropy <= 3.4657360f, where, W, H, px, py, nk, dtype, mode, key, action, logp, entropy, source);  // ln 32
                            EXPECT(!(logp > 0.0f), where, W, H, px, py, nk, dtype, mode, key, action, logp, entropy, source);
                            if (legal == 0) {
                                EXPECT(key == keys[0] && action == 0 && logp == 0.0f && entropy == 0.0f && source == 3, where, W, H, px, py, nk, dtype, mode, key, action, logp,
                                       entropy, source);
                            } else if (mode == RG_ACT_GIVEN) {
                                EXPECT(action == given && source == 0 && (given >= 0 && given < nk ? key == keys[given] : key == keys[0]), where, W, H, px, py, nk, dtype, mode, key,
                                       action, logp, entropy, source);
                                if (given < 0 || given >= nk || !row[given]) EXPECT(logp == -INFINITY, where, W, H, px, py, nk, dtype, mode, key, action, logp, entropy, source);
                            } else {
                                EXPECT(action >= 0 && action < nk && row[action] && key == keys[action] && source <= 2, where, W, H, px, py, nk, dtype, mode, key, action, logp, entropy,
                                       source);
                                if (source == 0) EXPECT(logp > -INFINITY, where, W, H, px, py, nk, dtype, mode, key, action, logp, entropy, source);  // the policy draws no key of weight 0
                                if (source == 2) EXPECT(key == (uint8_t)teacher, where, W, H, px, py, nk, dtype, mode, key, action, logp, entropy, source);
                            }
                            // NULL outputs are skipped, and a refusal writes nothing
                            EXPECT(rgh_act(err, cells, H, W, px, py, dead, keys, nk, logits, dtype, &o, 1u, teacher, given, &key, nullptr, nullptr, nullptr, nullptr) == 0, "NULL outputs");
                            key = 0xAA;
                            o.inv_temp = 0.0f;
                            EXPECT(rgh_act(err, cells, H, W, px, py, dead, keys, nk, logits, dtype, &o, 1u, teacher, given, &key, nullptr, nullptr, nullptr, nullptr) != 0 && key == 0xAA,
                                   "inv_temp 0 was served");
                            free(logits);
                            free(keys);
                        }
                free(cells);
            }
    }
    printf("%d checks, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
