// fetch_plan_host.cpp -- the two plans of a packet fetch (csrc/dsvg_fetch_plan.h: plan_fetch_wait, plan_fetch_layout, coded_events_once)
// on the CPU, for a sanitizer: a few hundred seeded calls whose arrays are exactly as long as the plans may read (a slot table of the
// context's slots, a P table that is short or absent, 3 n plane sizes), the refusals, and the invariants of what comes back.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I digital-subband-video-1_amd/csrc tools/fetch_plan_host.cpp -o fetch_plan_host
//   ./fetch_plan_host
#include <stdio.h>
#include <string.h>
#include <memory>
#include <random>
#include "dsvg_fetch_plan.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "case %d: %s fails (line %d)\n", t, #x, __LINE__); return 1; } } while (0)

int main()
{
    std::mt19937 rng(0xFE7C);
    const auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };
    const FetchGeo geos[2] = { { 0, 19200, {0, 12544, 15872}, {12288, 3072, 3072} }, { 0, 197376, {0, 131328, 164352}, {131072, 32768, 32768} } };
    const int ctxs[4] = {1, 4, 12, 48};
    int nfew = 0, nfell = 0, ngen = 0, nref = 0;
    FetchWait W;
    FetchLayout L;
    for (int t = 0; t < 600; t++) {
        FetchGeo G = geos[t & 1];
        G.out_slots = ctxs[rnd(4)];
        const int n = 1 + rnd(9), O = G.out_slots, ring = t % 3 ? 4 : 10, nchunks = 1 + 3 * rnd(3), al = rnd(4), align = al < 3 ? al + 1 : n + 2;
        const long ncalls = rnd(40);
        const bool cb = rnd(2), no_fast = rnd(4) == 0;
        std::unique_ptr<int[]> slots(new int[n]), ev(new int[O]);
        const int nP = rnd(3) == 0 ? 0 : rnd(2) ? O : (O + 1) / 2;
        std::unique_ptr<char[]> isP(new char[nP ? nP : 1]);
        std::unique_ptr<FetchPlaneSize[]> size(new FetchPlaneSize[3 * n]);
        const int newest = ncalls ? (int)((ncalls - 1) % ring) : -1, evk = rnd(3);
        for (int i = 0; i < O; i++) ev[i] = evk == 0 ? newest : evk == 1 ? (rnd(3) ? newest : -1) : rnd(ring + 1) - 1;
        for (int i = 0; i < nP; i++) isP[i] = (char)(rnd(8) != 0);
        const bool bad_slot = rnd(25) == 0;
        for (int i = 0; i < n; i++) slots[i] = rnd(O);
        if (bad_slot) slots[rnd(n)] = rnd(2) ? O : -1;
        for (int k = 0; k < 3 * n; k++) {
            const size_t cap = G.bits_cap[k % 3], pick[5] = {0, FETCH_FEW_PLANE * 8, FETCH_FEW_PLANE * 8 + 1, cap * 8, (size_t)1 + (size_t)rnd(24000)};
            size_t b = pick[rnd(8) < 4 ? rnd(4) : 4];
            if (b > cap * 8) b = pick[4];
            size[k] = { b, rnd(150) == 0 };
        }
        int rc = plan_fetch_wait(G, {no_fast}, n, slots.get(), ev.get(), nP ? isP.get() : nullptr, (size_t)nP, (size_t)ring, ncalls, nchunks, align, cb, W);
        if (n > O || bad_slot) {
            CHECK(rc == DSVG_ERR_ARG && !strcmp(W.err, n > O ? "bad fetch_pictures arguments" : "out slot out of range") && W.grow == 0 && W.events.empty());
            nref++;
            continue;
        }
        CHECK(rc == DSVG_OK && W.few == W.stream_wait && (W.grow != 0) == W.few && W.copy.size() == (W.few ? 3 * (size_t)n : 0));
        CHECK(!W.few || (n <= 4 && !cb && !no_fast));
        for (size_t i = 0; i < W.events.size(); i++) {
            CHECK(W.events[i] >= 0 && W.events[i] < ring);
            for (size_t j = 0; j < i; j++) CHECK(W.events[i] != W.events[j]);
        }
        for (const FetchCopy &k : W.copy) CHECK(k.dst + k.bytes <= W.grow - 64 && k.src + k.bytes <= (size_t)O * G.bits_per_job);
        bool few = W.few, ovf = false;
        for (int k = 0; k < 3 * n; k++) ovf = ovf || size[k].overflow;
        rc = plan_fetch_layout(G, n, slots.get(), size.get(), few, nchunks, align, cb, L);
        if (ovf) {
            CHECK(rc == DSVG_ERR_OVERFLOW && !strncmp(L.err, "packed plane ", 13) && L.grow == 0 && L.rows.empty() && L.piece.empty());
            nref++;
            continue;
        }
        CHECK(rc == DSVG_OK);
        if (few && L.fits) {
            for (int k = 0; k < 3 * n; k++) CHECK(L.nbytes[k] <= W.copy[k].bytes && L.pay[k] == W.copy[k].dst);
            CHECK(L.grow == 0 && L.rows.empty());
            nfew++;
            continue;
        }
        if (few) { nfell++; CHECK(plan_fetch_layout(G, n, slots.get(), size.get(), false, nchunks, align, cb, L) == DSVG_OK); } else ngen++;
        CHECK(L.rows.size() == 9 * (size_t)n && L.grow == L.total + 64 && L.nchunks >= 1 && L.nchunks <= (cb ? nchunks : 1) && (int)L.piece.size() == L.nchunks);
        size_t at = 0;
        for (int k = 0; k < 3 * n; k++) {
            CHECK(L.rows[3 * k + 1] == at && at % 16 == 0 && L.rows[3 * k + 2] == L.nbytes[k] && L.pay[k] == at);
            CHECK(L.rows[3 * k] == (size_t)slots[k / 3] * G.bits_per_job + G.bits_off[k % 3] && L.nbytes[k] <= G.bits_cap[k % 3]);
            at += (L.nbytes[k] + 15) & ~(size_t)15;
        }
        CHECK(at == L.total);
        for (int j = 0; j < L.nchunks; j++) {
            const FetchPiece &p = L.piece[(size_t)j];
            CHECK(p.first == (j ? L.piece[(size_t)j - 1].end : 0) && p.end > p.first && p.o0 == (j ? L.piece[(size_t)j - 1].o1 : 0) && p.o1 >= p.o0);
            CHECK(j + 1 == L.nchunks ? (p.end == n && p.o1 == L.total) : (p.end % align == 0 && p.o1 == L.pay[3 * (size_t)p.end]));
        }
    }
    {   // the remaining refusals, and the helper on a block of consecutive slots
        const int t = -1, one[1] = {0}, ev[4] = {2, -1, 2, 0};
        FetchGeo G = geos[0];
        G.out_slots = 4;
        CHECK(plan_fetch_wait(G, {false}, 0, one, ev, nullptr, 0, 4, 1, 1, 1, false, W) == DSVG_ERR_ARG);
        CHECK(plan_fetch_wait(G, {false}, 1, nullptr, ev, nullptr, 0, 4, 1, 1, 1, false, W) == DSVG_ERR_ARG);
        CHECK(plan_fetch_wait(G, {false}, 1, one, ev, nullptr, 0, 4, 1, 0, 1, false, W) == DSVG_ERR_ARG);
        CHECK(plan_fetch_wait(G, {false}, 1, one, ev, nullptr, 0, 4, 1, 1, 0, false, W) == DSVG_ERR_ARG && !strcmp(W.err, "bad fetch_pictures arguments"));
        std::vector<int> out;
        coded_events_once(ev, 4, 3, nullptr, 1, out);
        CHECK(out.size() == 2 && out[0] == 2 && out[1] == 0);
        coded_events_once(ev, 4, 0, nullptr, 0, out);
        CHECK(out.empty());
    }
    printf("fetch plans: %d one round trip, %d fell through, %d general, %d refused\n", nfew, nfell, ngen, nref);
    return nfew > 20 && nfell > 5 && ngen > 100 && nref > 20 ? 0 : 1;
}
