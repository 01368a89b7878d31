// dec_plan_host.cpp -- the plan of a decoder call (csrc/dsvg_dec_plan.h: plan_decode, every check and every host decision of
// dsvg_decode_pictures, and dec_intra_list) on the CPU, for a sanitizer: reads the cases tools/dec_plan_dump.py wrote -- the calls and header
// planes of tests/dec_cases.py and the refused calls of tests/test_dec_plan_host.py --, rebuilds each with every array allocated at its exact
// size (the job array, each vector and flag table, each payload at exactly the bytes behind its pointer, the intra list), plans it and
// compares with what the library's query dsvg_decode_plan answered when the cases were written.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I digital-subband-video-1_amd/csrc tools/dec_plan_host.cpp -o dec_plan_host
//   python tools/dec_plan_dump.py cases.bin && ./dec_plan_host cases.bin
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "dsvg_dec_plan.h"

static FILE *f;
static bool rd(void *p, size_t n) { return fread(p, 1, n, f) == n; }
static std::vector<int32_t> ints(size_t n)
{
    std::vector<int32_t> v(n);
    if (n && !rd(v.data(), n * 4)) { fprintf(stderr, "short case\n"); exit(2); }
    return v;
}
static std::vector<int64_t> longs(size_t n)
{
    std::vector<int64_t> v(n);
    if (n && !rd(v.data(), n * 8)) { fprintf(stderr, "short case\n"); exit(2); }
    return v;
}
template <typename T> static int differs(const char *what, const std::vector<int64_t> &want, const std::vector<T> &got, int ncase)
{
    if (want.size() != got.size()) { fprintf(stderr, "case %d: %s has %zu entries, the query had %zu\n", ncase, what, got.size(), want.size()); return 1; }
    for (size_t i = 0; i < want.size(); i++)
        if ((int64_t)got[i] != want[i]) { fprintf(stderr, "case %d: %s[%zu] = %lld, the query had %lld\n", ncase, what, i, (long long)got[i], (long long)want[i]); return 1; }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int ncases = 0, bad = 0, nrefused = 0;
    int32_t g[30];
    while (rd(g, sizeof g)) {
        DecGeo G;
        int k = 0;
        G.n_recon = g[k++]; G.max_jobs = g[k++]; G.nblk = g[k++];
        for (int p = 0; p < 3; p++) G.cw[p] = g[k++];
        for (int p = 0; p < 3; p++) G.ch[p] = g[k++];
        for (int p = 0; p < 3; p++) G.nchunks[p] = g[k++];
        for (int p = 0; p < 2; p++) G.sym_ok[p] = g[k++];
        for (int p = 0; p < 2; p++) G.ov[p] = g[k++];
        G.mc_patch = g[k++]; G.nbh = g[k++]; G.nbv = g[k++]; G.blk_w = g[k++]; G.blk_h = g[k++]; G.hs = g[k++]; G.vs = g[k++];
        for (int p = 0; p < 3; p++) G.pw[p] = g[k++];
        for (int p = 0; p < 3; p++) G.ph[p] = g[k++];
        G.second_stream = g[k++];
        const std::vector<int32_t> hd = ints(11);
        const DecSwitches sw = { hd[0] != 0, hd[1] != 0, hd[2] != 0, hd[3] != 0, hd[4] != 0 };
        const bool force32 = hd[5] != 0, profiled = hd[6] != 0;
        const int draw_mode = hd[7], njobs = hd[8], nj = hd[9], want_rc = hd[10];
        // every table and every payload an allocation of its own, of exactly the bytes the caller has behind the pointer
        std::vector<std::unique_ptr<dsvg_mv[]>> mvt;
        std::vector<std::unique_ptr<unsigned char[]>> bytes;
        std::unique_ptr<dsvg_dec_job[]> jobs(new dsvg_dec_job[nj]);
        for (int i = 0; i < nj; i++) {
            const std::vector<int32_t> j = ints(11);
            dsvg_dec_job &o = jobs[i];
            memset(&o, 0, sizeof o);
            o.ref_recon_slot = j[0]; o.recon_slot = j[1]; o.quant = j[2];
            if (j[3]) { mvt.emplace_back(new dsvg_mv[G.nblk]); if (!rd(mvt.back().get(), sizeof(dsvg_mv) * G.nblk)) return 2; o.mvs = mvt.back().get(); }
            if (j[4]) { bytes.emplace_back(new unsigned char[G.nblk]); if (!rd(bytes.back().get(), G.nblk)) return 2; o.stable_blocks = bytes.back().get(); }
            for (int p = 0; p < 3; p++) {
                o.plane_len[p] = (uint32_t)j[5 + p];
                if (j[8 + p] < 0) continue;
                bytes.emplace_back(new unsigned char[j[8 + p]]);
                if (j[8 + p] && !rd(bytes.back().get(), j[8 + p])) return 2;
                o.plane_data[p] = bytes.back().get();
            }
        }
        DecPlan P;
        const int rc = plan_decode(G, sw, njobs, jobs.get(), force32, profiled, draw_mode, P);
        int d = 0;
        if (rc != want_rc) { fprintf(stderr, "case %d: returns %d, the query returned %d\n", ncases, rc, want_rc); d = 1; }
        if (want_rc) {
            char text[256];
            if (!rd(text, sizeof text)) return 2;
            text[255] = 0;
            if (rc && strcmp(text, P.err)) { fprintf(stderr, "case %d: \"%s\", the query said \"%s\"\n", ncases, P.err, text); d = 1; }
            nrefused++;
        } else {
            const std::vector<int64_t> s = longs(17);
            const size_t n = (size_t)njobs, iln = (size_t)s[14];
            const std::vector<int64_t> order = longs(n), path = longs(n), wide = longs(n), inplace = longs(n), dec_sym = longs(3 * n), dc = longs(3 * n),
                                       runs = longs(3 * n), len = longs(3 * n), bitpos = longs(3 * n), boff = longs(3 * n), moff = longs(3 * n), il = longs(iln);
            if (!rc) {
                // the intra list as the commit stage builds it: per P picture, straight into a list of exactly the entries the query had
                std::unique_ptr<int[]> exact(new int[iln]);
                int got_iln = 0;
                for (int t = P.nI; t < njobs && P.mc == DEC_MC_PATCH; t++)
                    got_iln += dec_intra_list(G, jobs[P.job[(size_t)t].src].mvs, (t - P.nI) * G.nblk, P.ex0, P.ey0, exact.get() + got_iln);
                const std::vector<int> list(exact.get(), exact.get() + std::min((size_t)got_iln, iln));
                const std::vector<int64_t> got = {P.nI, (int64_t)P.blob, (int64_t)P.nmeta, P.max_entries, P.max_chunks, P.insym, P.f0, P.anysym, P.scatter_one,
                                                  P.resolve, P.fork, P.mc, P.ex0, P.ey0, got_iln, P.draw0, P.draw1};
                d |= differs("scalars", s, got, ncases);
                std::vector<int64_t> o_[11];
                for (size_t t = 0; t < n && !d; t++) {
                    const DecPlanJob &o = P.job[t];
                    o_[0].push_back(o.src); o_[1].push_back(o.path); o_[2].push_back(o.wide); o_[3].push_back(o.inplace);
                    for (int p = 0; p < 3; p++) {
                        o_[4].push_back(o.dec_sym[p]); o_[5].push_back(o.dc[p]); o_[6].push_back(o.runs[p]); o_[7].push_back(o.len[p]);
                        o_[8].push_back(o.bitpos[p]); o_[9].push_back((int64_t)o.boff[p]); o_[10].push_back((int64_t)o.moff[p]);
                    }
                }
                if (!d)
                    d |= differs("order", order, o_[0], ncases) | differs("path", path, o_[1], ncases) | differs("wide", wide, o_[2], ncases) |
                         differs("inplace", inplace, o_[3], ncases) | differs("dec_sym", dec_sym, o_[4], ncases) | differs("dc", dc, o_[5], ncases) |
                         differs("runs", runs, o_[6], ncases) | differs("len", len, o_[7], ncases) | differs("bitpos", bitpos, o_[8], ncases) |
                         differs("blob_off", boff, o_[9], ncases) | differs("meta_off", moff, o_[10], ncases) | differs("ilist", il, list, ncases);
            }
        }
        bad += d;
        ncases++;
    }
    fclose(f);
    printf("%d cases (%d refused), %d differ\n", ncases, nrefused, bad);
    return bad || !ncases ? 1 : 0;
}
