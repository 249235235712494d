// A stand-alone host program around the archive rule (rogue-gym_amd/csrc/rg_archive.h), built by tests/test_archive_host.py with
// -fsanitize=address,undefined: every table is allocated on the heap at its exact size, so a probe one slot past a table ends the run, and the packing of
// (score, ~steps) is computed on the extreme values under the undefined-behaviour checks.  The rule is compared with a restatement on a std::map.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "rg_archive.h"

static uint32_t rnd_state = 2463534242u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static int rnd_in(int n) { return (int)(rnd() % (uint32_t)n); }

static int bad = 0, runs = 0;
#define EXPECT(cond, ...) do { runs++; if (!(cond)) { bad++; if (bad <= 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Cell { int64_t score; uint64_t steps; uint32_t seen, when; };
static bool beats_plain(int64_t sa, uint64_t ta, int64_t sb, uint64_t tb) { return sa > sb || (sa == sb && ta < tb); }

static const int32_t SCORES[] = {INT32_MIN, -1, 0, INT32_MAX, 3, -3};
static const uint32_t STEPS[] = {0u, 0xffffffffu, 1u, 0x80000000u, 40u};

// `distinct` keys offered `offers` times to a table of `cells` slots; same_start: every key starts its probe at the last slot
static void run(int cells, int distinct, int offers, bool same_start) {
    RgArcSlot *tab = (RgArcSlot *)calloc((size_t)cells, sizeof(RgArcSlot));   // exact size: the red zone starts right behind the last slot
    std::map<uint64_t, Cell> ref;
    std::vector<uint64_t> keys;
    for (int i = 0; i < distinct; i++) keys.push_back(same_start ? ((uint64_t)(i + 1) << 32) | (uint64_t)(cells - 1) : (uint64_t)rnd() * 2654435761ull + (uint64_t)i);
    keys[0] = 0;   // offered as 1
    std::string err;
    int drops = 0;
    for (int i = 0; i < offers; i++) {
        const uint64_t key = keys[rnd_in(distinct)], k1 = key ? key : 1;
        const int32_t score = rnd_in(2) ? SCORES[rnd_in(6)] : rnd_in(5) - 2;
        const uint32_t steps = rnd_in(2) ? STEPS[rnd_in(5)] : (uint32_t)rnd_in(4);
        const uint32_t serial = 1 + (uint32_t)i / 64;
        int occupied = 0;
        for (int s = 0; s < cells; s++) occupied += tab[s].key != 0;
        int32_t slot = -9, stored = -9;
        const int rc = rga_offer_host(err, tab, cells, key, score, steps, serial, &slot, &stored);
        EXPECT(rc == 0, "refused: %s", err.c_str());
        // (cells <= 1 024 here: the probe covers the whole table, so an offer is dropped iff its key is new and no slot is empty)
        const bool admitted = ref.count(k1) || occupied < cells;
        EXPECT((slot >= 0) == admitted, "cells %d offer %d: slot %d, admitted %d", cells, i, slot, (int)admitted);
        if (!admitted) { drops++; EXPECT(stored == 0, "a dropped offer was stored"); continue; }
        EXPECT(slot >= 0 && slot < cells && tab[slot].key == k1, "cells %d offer %d: the slot does not hold the key", cells, i);
        const bool fresh = !ref.count(k1);
        Cell &c = ref[k1];
        if (fresh) c = Cell{0, 0, 0, 0};
        c.seen++;
        const bool want = c.when == 0 || beats_plain(score, steps, c.score, c.steps);
        if (want) { c.score = score; c.steps = steps; c.when = serial; }
        EXPECT(stored == (want ? 1 : 0), "cells %d offer %d (score %d steps %u): stored %d, restated %d", cells, i, score, steps, stored, (int)want);
    }
    size_t found = 0;
    for (int s = 0; s < cells; s++) {
        if (!tab[s].key) { EXPECT(!tab[s].seen && !tab[s].when && !tab[s].score && !tab[s].steps, "an empty slot holds words"); continue; }
        found++;
        auto it = ref.find(tab[s].key);
        EXPECT(it != ref.end(), "cells %d slot %d: a key nobody offered", cells, s);
        if (it == ref.end()) continue;
        const Cell &c = it->second;
        EXPECT(tab[s].score == c.score && tab[s].steps == c.steps && tab[s].seen == c.seen && tab[s].when == c.when && tab[s].chosen == 0 && tab[s].zero == 0,
               "cells %d slot %d differs", cells, s);
    }
    EXPECT(found == ref.size(), "cells %d: %zu slots for %zu keys", cells, found, ref.size());
    EXPECT((distinct > cells) == (drops > 0), "cells %d with %d distinct keys: %d drops", cells, distinct, drops);
    free(tab);
}

int main() {
    run(1024, 700, 6000, false);
    run(1024, 1500, 12000, false);   // driven to overflow
    run(8, 5, 200, true);            // every probe wraps at the last slot
    run(8, 12, 400, true);
    run(1, 1, 20, false);
    run(1, 3, 30, false);
    {   // the packing on the extremes
        EXPECT(rg_arc_bid(INT32_MIN, 0xffffffffu) == 0ull, "the worst bid is not 0");
        EXPECT(rg_arc_bid(INT32_MAX, 0u) == ~0ull, "the best bid is not all ones");
        EXPECT(rg_arc_bid(0, 5u) > rg_arc_bid(-1, 0u) && rg_arc_bid(0, 4u) > rg_arc_bid(0, 5u) && rg_arc_bid(INT32_MIN, 0u) < rg_arc_bid(INT32_MIN + 1, 0xffffffffu), "bid order");
        EXPECT(rg_arc_beats(INT32_MIN, 0xffffffffu, 0u, INT32_MAX, 0u), "an empty slot was not beaten");
        EXPECT(!rg_arc_beats(7, 3u, 1u, 7, 3u), "an equal offer beat the stored one");
        EXPECT(rg_arc_key(0) == 1 && rg_arc_key(1) == 1 && rg_arc_key(~0ull) == ~0ull, "key 0 -> 1");
        EXPECT(rg_arc_probes(1u << 24) == 1024u && rg_arc_probes(8u) == 8u, "probe limit");
    }
    {   // a table larger than the probe limit: a run of 1 024 occupied slots behind a start slot counts as full
        const int cells = 4096;
        RgArcSlot *tab = (RgArcSlot *)calloc((size_t)cells, sizeof(RgArcSlot));
        std::string err;
        int32_t slot = 0, stored = 0;
        for (int i = 0; i < 1024; i++) {
            rga_offer_host(err, tab, cells, ((uint64_t)(i + 1) << 32) | 3500u, 0, 0, 1, &slot, &stored);
            EXPECT(slot == ((3500 + i) & (cells - 1)) && stored == 1, "run slot %d", slot);
        }
        rga_offer_host(err, tab, cells, ((uint64_t)5000 << 32) | 3500u, 9, 0, 1, &slot, &stored);
        EXPECT(slot == -1 && stored == 0 && tab[(3500 + 1024) & (cells - 1)].key == 0, "the 1 025th key of a run was not dropped");
        rga_offer_host(err, tab, cells, ((uint64_t)5000 << 32) | 3501u, 9, 0, 1, &slot, &stored);
        EXPECT(slot == ((3500 + 1024) & (cells - 1)) && stored == 1, "a start one slot later found the empty slot");
        free(tab);
    }
    {   // the refusals write nothing
        RgArcSlot *tab = (RgArcSlot *)calloc(8, sizeof(RgArcSlot));
        std::string err;
        int32_t slot = -7, stored = -7;
        EXPECT(rga_offer_host(err, nullptr, 8, 1, 0, 0, 1, &slot, &stored) && rga_offer_host(err, tab, 6, 1, 0, 0, 1, &slot, &stored) &&
               rga_offer_host(err, tab, 8, 1, 0, 0, 0, &slot, &stored) && rga_offer_host(err, tab, 8, 1, 0, 0, 1, nullptr, &stored) &&
               rga_offer_host(err, tab, 8, 1, 0, 0, 1, &slot, nullptr) && rga_offer_host(err, (char *)tab + 4, 4, 1, 0, 0, 1, &slot, &stored), "not refused");
        EXPECT(slot == -7 && stored == -7 && tab[1].key == 0 && err.rfind("rg_archive_offer_host: ", 0) == 0, "a refusal wrote something");
        free(tab);
    }
    printf("%d checks, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
