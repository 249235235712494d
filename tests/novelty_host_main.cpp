// A stand-alone host program around the novelty rule (rogue-gym_amd/csrc/rg_novelty.h through rg_readers_host.h), built by tests/test_novelty_host.py with
// -fsanitize=address,undefined: every screen and every table is allocated on the heap at its exact size, so a read one byte past a screen or a probe one slot
// past a table ends the run.  The hash is compared with a restatement on an explicit key vector (the bytes gathered first, then words, then the sum); the
// insert with a restatement on three plain arrays.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rg_readers_host.h"

static uint32_t rnd_state = 2463534242u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static int rnd_in(int n) { return (int)(rnd() % (uint32_t)n); }

static int bad = 0, runs = 0;
#define EXPECT(cond, ...) do { runs++; if (!(cond)) { bad++; if (bad <= 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t mix2(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
static uint64_t hash_of(const std::vector<uint8_t> &key, int what, int level) {
    std::vector<uint8_t> b = key;
    while (b.size() % 8) b.push_back(0);
    uint64_t acc = 0;
    for (size_t i = 0; i < b.size() / 8; i++) {
        uint64_t w = 0;
        for (int k = 7; k >= 0; k--) w = (w << 8) | b[8 * i + k];
        acc += mix2(w ^ ((uint64_t)(i + 1) * 0x9e3779b97f4a7c15ull));
    }
    const uint64_t h = mix2(acc + mix2((uint64_t)what | ((uint64_t)level << 8) | ((uint64_t)key.size() << 32)));
    return h ? h : 1;
}
static std::vector<uint8_t> key_of(int what, const uint8_t *s, int H, int W, int px, int py, int ry, int rx) {
    std::vector<uint8_t> k;
    if (what == RG_NOV_POS) { k = {(uint8_t)px, (uint8_t)(px >> 8), (uint8_t)py, (uint8_t)(py >> 8), 0, 0, 0, 0}; return k; }
    if (what == RG_NOV_SCREEN) { k.assign(s + W, s + (size_t)(H - 1) * W); return k; }
    for (int y = py - ry; y <= py + ry; y++)
        for (int x = px - rx; x <= px + rx; x++) k.push_back(y >= 1 && y <= H - 2 && x >= 0 && x < W ? s[y * W + x] : (uint8_t)' ');
    return k;
}
// exact-size heap copy: the sanitizer's red zone starts right behind the last cell
struct Screen {
    int H, W; uint8_t *p;
    Screen(int h, int w, int fill) : H(h), W(w), p((uint8_t *)malloc((size_t)h * w)) { for (int i = 0; i < h * w; i++) p[i] = fill < 0 ? (uint8_t)rnd() : (uint8_t)fill; }
    ~Screen() { free(p); }
};
static uint64_t twin(int what, int level, const Screen &s, int px, int py, int ry, int rx) {
    std::string err;
    uint64_t h = 0;
    const int rc = rgh_nov_hash(err, what, level, s.H, s.W, s.p, px, py, ry, rx, &h);
    EXPECT(rc == 0, "refused: %s", err.c_str());
    const uint64_t want = hash_of(key_of(what, s.p, s.H, s.W, px, py, ry, rx), what, level);
    EXPECT(h == want && h != 0, "what %d level %d %dx%d at (%d, %d) r (%d, %d): %016llx, restated %016llx", what, level, s.W, s.H, px, py, ry, rx, (unsigned long long)h,
           (unsigned long long)want);
    return h;
}

// the insert restated on plain arrays
struct Plain {
    std::vector<uint64_t> key; std::vector<uint32_t> gen, cnt;
    explicit Plain(int cap) : key(cap, 0), gen(cap, 0), cnt(cap, 0) {}
    uint32_t insert(uint32_t g, uint64_t h) {
        const size_t cap = key.size();
        for (size_t p = 0; p < cap; p++) {
            const size_t at = ((h & (cap - 1)) + p) % cap;
            if (gen[at] != g) { key[at] = h; gen[at] = g; cnt[at] = 1; return 1; }
            if (key[at] == h) return ++cnt[at];
        }
        return 0;
    }
};
static void insert_run(int cap, int distinct, int visits, int episodes, bool same_start) {
    RgNovSlot *tab = new RgNovSlot[cap]();   // (aligned new: 16 bytes)
    Plain ref(cap);
    std::string err;
    uint32_t drops = 0;
    for (int g = 1; g <= episodes; g++)
        for (int v = 0; v < visits; v++) {
            const uint64_t h = same_start ? ((uint64_t)(1 + rnd_in(distinct)) << 20) | (uint64_t)(cap - 1) : (uint64_t)rnd_in(distinct) * 7 + 1;
            uint32_t c = 77;
            const int rc = rgh_nov_insert(err, tab, cap, (uint32_t)g, h, &c);
            const uint32_t want = ref.insert((uint32_t)g, h);
            EXPECT(rc == 0 && c == want, "insert cap %d gen %d hash %llx: count %u, restated %u", cap, g, (unsigned long long)h, c, want);
            drops += c == 0;
        }
    for (int i = 0; i < cap; i++)
        EXPECT(tab[i].hash == ref.key[i] && tab[i].gen == ref.gen[i] && tab[i].count == ref.cnt[i], "cap %d slot %d differs", cap, i);
    EXPECT((distinct > cap) == (drops > 0), "cap %d with %d distinct keys: %u drops", cap, distinct, drops);
    delete[] tab;
}

int main() {
    // screens whose key is no multiple of 8 bytes (33x17: 495), the benchmarked sizes, the smallest
    const int sizes[][2] = {{17, 33}, {16, 32}, {24, 80}, {3, 1}, {5, 7}, {48, 160}};
    for (auto &hw : sizes) {
        Screen s(hw[0], hw[1], -1);
        for (int t = 0; t < 4; t++) {
            const int px = rnd_in(s.W), py = rnd_in(s.H), level = rnd_in(40);
            twin(RG_NOV_SCREEN, level, s, px, py, 0, 0);
            twin(RG_NOV_POS, level, s, px, py, 0, 0);
        }
        // windows over every edge and corner, and wider and taller than the screen
        const int cy[5] = {0, 1, s.H / 2, s.H - 2, s.H - 1}, cx[3] = {0, s.W / 2, s.W - 1};
        const int rr[][2] = {{0, 0}, {1, 1}, {2, 3}, {4, 4}, {5, 0}, {0, 6}, {s.H - 1, s.W - 1}, {RG_MAX_H - 1, RG_MAX_W - 1}};
        for (auto &r : rr)
            for (int py : cy)
                for (int px : cx) twin(RG_NOV_CROP, 3, s, px, py, r[0], r[1]);
    }
    {   // a blank screen, and a swapped pair of cells
        Screen blank(17, 33, ' '), zero(17, 33, 0), s(17, 33, -1);
        const uint64_t hb = twin(RG_NOV_SCREEN, 1, blank, 3, 3, 0, 0);
        EXPECT(hb != twin(RG_NOV_SCREEN, 1, zero, 3, 3, 0, 0), "blank and zero screens share a hash");
        const uint64_t base = twin(RG_NOV_SCREEN, 1, s, 3, 3, 0, 0);
        const int pairs[][2] = {{33, 34}, {33, 66}, {40, 41}, {200, 500}, {33 * 16 - 2, 33 * 16 - 1}, {33, 33 * 16 - 1}};
        for (auto &p : pairs) {
            if (s.p[p[0]] == s.p[p[1]]) continue;
            std::swap(s.p[p[0]], s.p[p[1]]);
            EXPECT(twin(RG_NOV_SCREEN, 1, s, 3, 3, 0, 0) != base, "swapping cells %d and %d kept the hash", p[0], p[1]);
            std::swap(s.p[p[0]], s.p[p[1]]);
        }
        EXPECT(twin(RG_NOV_SCREEN, 1, s, 3, 3, 0, 0) == base, "the screen was not put back");
        uint64_t lv[4];
        for (int l = 0; l < 4; l++) lv[l] = twin(RG_NOV_POS, l, s, 7, 9, 0, 0);
        EXPECT(lv[0] != lv[1] && lv[1] != lv[2] && lv[2] != lv[3] && lv[0] != lv[3], "the level is not in the salt");
    }
    {   // 0 -> 1
        const uint64_t salts[3] = {0, 0x1234, ((uint64_t)1760 << 32) | (3u << 8) | 2u};
        for (uint64_t salt : salts) {
            const uint64_t acc = 0 - mix2(salt);
            EXPECT(rg_nov_finish(acc, salt) == 1, "a zero hash did not become 1");
            EXPECT(rg_nov_finish(acc + 1, salt) == mix2(1), "finish(acc + 1)");
        }
    }
    {   // the insert: wrap-around at the last slot, stale generations, the drop
        insert_run(8, 5, 40, 3, true);      // every key starts at slot cap - 1
        insert_run(8, 12, 80, 3, true);     // ... and more keys than slots: drops
        insert_run(64, 40, 400, 4, false);
        insert_run(64, 90, 600, 4, false);
        insert_run(1, 1, 5, 2, false);
        insert_run(1, 3, 9, 2, false);
        RgNovSlot *tab = new RgNovSlot[4]();
        std::string err;
        uint32_t c = 0;
        for (uint64_t h = 1; h <= 4; h++) { rgh_nov_insert(err, tab, 4, 1, h, &c); EXPECT(c == 1, "first visit"); }
        rgh_nov_insert(err, tab, 4, 1, 9, &c);
        EXPECT(c == 0, "a full table reported count %u", c);
        rgh_nov_insert(err, tab, 4, 2, 9, &c);
        EXPECT(c == 1 && tab[1].hash == 9 && tab[1].gen == 2 && tab[2].gen == 1, "a stale slot was not reused");
        delete[] tab;
    }
    {   // the refusals write nothing
        Screen s(16, 32, -1);
        std::string err;
        uint64_t h = 0xABAB;
        const int bad_args[][7] = {{0, 1, 16, 32, 0, 0, 0}, {4, 1, 16, 32, 0, 0, 0}, {RG_NOV_POS, 1, 16, 32, 0, 1, 0}, {RG_NOV_CROP, 1, 16, 32, 0, 48, 0}, {RG_NOV_CROP, 1, 16, 32, 0, 0, 160},
                                   {RG_NOV_SCREEN, 1, 2, 32, 0, 0, 0}, {RG_NOV_SCREEN, 1, 16, 161, 0, 0, 0}, {RG_NOV_POS, 1, 16, 32, 32, 0, 0}, {RG_NOV_POS, -1, 16, 32, 0, 0, 0}};
        for (auto &a : bad_args) {
            err.clear();
            EXPECT(rgh_nov_hash(err, a[0], a[1], a[2], a[3], s.p, a[4], 0, a[5], a[6], &h) != 0 && err.rfind("rg_novelty_hash_host: ", 0) == 0 && h == 0xABAB, "not refused: %s", err.c_str());
        }
        EXPECT(rgh_nov_hash(err, RG_NOV_POS, 1, 16, 32, nullptr, 0, 0, 0, 0, &h) != 0 && rgh_nov_hash(err, RG_NOV_POS, 1, 16, 32, s.p, 0, 0, 0, 0, nullptr) != 0, "NULL not refused");
        uint32_t c = 7;
        RgNovSlot *tab = new RgNovSlot[8]();
        EXPECT(rgh_nov_insert(err, tab, 6, 1, 5, &c) != 0 && rgh_nov_insert(err, nullptr, 8, 1, 5, &c) != 0 && rgh_nov_insert(err, tab, 8, 1, 5, nullptr) != 0 && c == 7 && tab[5].hash == 0,
               "insert refusals");
        delete[] tab;
    }
    printf("%d checks, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
