// batch_plan_host.cpp -- the plan of a coding call (csrc/dsvg_batch_plan.h: plan_code_batch, every check and every host decision of
// dsvg_code_batch) on the CPU, for a sanitizer: reads the cases tools/batch_plan_dump.py wrote -- the calls of tests/batch_cases.py and
// the refused calls of tests/test_batch_plan_host.py, tables by index --, rebuilds each with every array allocated at its exact size (the
// job array, each vector and flag table, the intra-list table of out_slots * nblk entries), plans it and compares with what the library's
// query dsvg_code_batch_plan answered when the cases were written.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I digital-subband-video-1_amd/csrc tools/batch_plan_host.cpp -o batch_plan_host
//   python tools/batch_plan_dump.py cases.bin && ./batch_plan_host cases.bin
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <memory>
#include <vector>
#include "dsvg_batch_plan.h"

static FILE *f;
static bool rd(void *p, size_t n) { return fread(p, 1, n, f) == n; }
static std::vector<int32_t> ints(size_t n)
{
    std::vector<int32_t> v(n);
    if (n && !rd(v.data(), n * 4)) { fprintf(stderr, "short case\n"); exit(2); }
    return v;
}
template <typename T> static int differs(const char *what, const std::vector<int32_t> &want, const T *got, int ncase)
{
    for (size_t i = 0; i < want.size(); i++)
        if ((int32_t)got[i] != want[i]) { fprintf(stderr, "case %d: %s[%zu] = %d, the query had %d\n", ncase, what, i, (int)got[i], want[i]); return 1; }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int ncases = 0, bad = 0, nrefused = 0;
    int32_t g[18];
    while (rd(g, sizeof g)) {
        BatchGeo G;
        G.nblk = g[0]; G.n_recon = g[1]; G.n_src = g[2]; G.max_jobs = g[3]; G.out_slots = g[4]; G.rc_slots = g[5]; G.mc_fused = g[6];
        G.code_streams = g[7]; G.lazy_border = g[8]; G.blk_w = g[9]; G.blk_h = g[10]; G.nbh = g[11]; G.hs = g[12]; G.vs = g[13];
        G.w[0] = g[14]; G.w[1] = g[15]; G.h[0] = g[16]; G.h[1] = g[17];
        const std::vector<int32_t> hd = ints(10);
        const BatchSwitches sw = { hd[0] != 0, hd[1] != 0 };
        const bool profiled = hd[2] != 0;
        const int nsteps = hd[3], njobs = hd[4], has_rc = hd[5], nmvt = hd[6], nstt = hd[7], nj = hd[8], want_rc = hd[9];
        // every table an allocation of its own, exactly nblk entries: a read past a table's end is caught
        std::vector<std::unique_ptr<dsvg_mv[]>> mvt;
        std::vector<std::unique_ptr<unsigned char[]>> stt;
        for (int i = 0; i < nmvt; i++) { mvt.emplace_back(new dsvg_mv[G.nblk]); if (!rd(mvt.back().get(), sizeof(dsvg_mv) * G.nblk)) return 2; }
        for (int i = 0; i < nstt; i++) { stt.emplace_back(new unsigned char[G.nblk]); if (!rd(stt.back().get(), G.nblk)) return 2; }
        std::unique_ptr<dsvg_pic_job[]> jobs(new dsvg_pic_job[nj]);
        for (int i = 0; i < nj; i++) {
            const std::vector<int32_t> j = ints(14);
            dsvg_pic_job &o = jobs[i];
            memset(&o, 0, sizeof o);
            o.src_slot = j[0]; o.ref_recon_slot = j[1]; o.recon_slot = j[2]; o.quant = j[3];
            o.mvs = j[4] < 0 ? nullptr : mvt[j[4]].get(); o.stable_blocks = j[5] < 0 ? nullptr : stt[j[5]].get();
            o.out_slot = j[6]; o.no_intra_blocks = j[7]; o.has_reach = j[8];
            for (int k = 0; k < 4; k++) o.mv_reach[k] = (short)j[9 + k];
            o.border_hint = j[13];
        }
        std::unique_ptr<dsvg_rc_job[]> rcj;
        if (has_rc) {
            rcj.reset(new dsvg_rc_job[nj]);
            for (int i = 0; i < nj; i++) { const std::vector<int32_t> r = ints(3); rcj[i].rc_slot = r[0]; rcj[i].prefix_len = r[1]; rcj[i].forced_intra = r[2]; }
        }
        std::unique_ptr<int[]> ilist(new int[(size_t)G.out_slots * G.nblk]);
        BatchPlan P;
        const int rc = plan_code_batch(G, sw, nsteps, njobs, jobs.get(), rcj.get(), profiled, ilist.get(), P);
        int d = 0;
        if (rc != want_rc) { fprintf(stderr, "case %d: returns %d, the query returned %d\n", ncases, rc, want_rc); d = 1; }
        if (want_rc) {
            char text[256];
            if (!rd(text, sizeof text)) return 2;
            text[255] = 0;
            if (rc && strcmp(text, P.err)) { fprintf(stderr, "case %d: \"%s\", the query said \"%s\"\n", ncases, P.err, text); d = 1; }
            nrefused++;
        } else {
            const std::vector<int32_t> s = ints(13);
            const int total = s[1], ng = s[2], iln = s[8];
            const std::vector<int32_t> nI = ints(nsteps), order = ints(total), mvu = ints(total), stu = ints(total), mvcp = ints(total), stcp = ints(total),
                                       rc_next = ints(total), ext = ints((size_t)total * 8), ioff = ints((size_t)nsteps * ng), icnt = ints((size_t)nsteps * ng),
                                       noint = ints((size_t)nsteps * ng), keeps = ints((size_t)nsteps * ng), il = ints(iln);
            if (!rc) {
                const int got[13] = {P.base, P.total, P.NG, P.gk[0], P.NG >= 1 ? P.gk[1] : 0, P.NG >= 2 ? P.gk[2] : 0, P.NG >= 3 ? P.gk[3] : 0,
                                     P.NG >= 4 ? P.gk[4] : 0, P.iln, P.nmv, P.nst, P.mv_contig, P.par_enqueue};
                d |= differs("scalars", s, got, ncases);
                if (!d) {
                    d |= differs("nI", nI, P.nI.data(), ncases) | differs("order", order, P.order.data(), ncases) | differs("mvu", mvu, P.mvu.data(), ncases) |
                         differs("stu", stu, P.stu.data(), ncases) | differs("mvcp", mvcp, P.mvcp.data(), ncases) | differs("stcp", stcp, P.stcp.data(), ncases) |
                         differs("ext", ext, P.ext.data(), ncases) | differs("ioff", ioff, P.ioff.data(), ncases) | differs("icnt", icnt, P.icnt.data(), ncases) |
                         differs("noint", noint, P.noint.data(), ncases) | differs("keeps", keeps, P.keeps.data(), ncases) |
                         differs("ilist", il, ilist.get() + (size_t)P.base * G.nblk, ncases);
                    if (has_rc) d |= differs("rc_next", rc_next, P.rc_next.data(), ncases);
                }
            }
        }
        bad += d;
        ncases++;
    }
    fclose(f);
    printf("%d cases (%d refused), %d differ\n", ncases, nrefused, bad);
    return bad || !ncases ? 1 : 0;
}
