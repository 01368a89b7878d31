/* submit_plan_host.c -- the plans of an encoder session's submit (csrc/host/dsv1_submit_plan.h) on the CPU, for a sanitizer: seeded
 * sequences of 1 to 4 calls of the kind tests/test_submit_plan_host.py runs (sources, rungs, frames per call, GOP length, CRF / device
 * ABR / serial ABR, chains, renumbered streams, forced metadata, scene cuts, pictures turned intra), every table allocated at its exact
 * size and freed after the call, the state carried from call to call; after each call the invariants of the job tables are checked.
 *   cc -O1 -g -std=c99 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all tools/submit_plan_host.c -o submit_plan_host
 *   ./submit_plan_host */
#include <stdio.h>
#include <stdlib.h>
#include "../digital-subband-video-1_amd/csrc/host/dsv1_submit_plan.h"

static unsigned rs;
static unsigned rnd(unsigned n) { rs = rs * 1664525u + 1013904223u; return (rs >> 8) % n; }
#define NEW(type, n) ((type *)calloc((size_t)(n), sizeof(type)))         /* (every count here is >= 1) */
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "seed %u call %d: %s (line %d)\n", seed, call, #c, __LINE__); exit(1); } } while (0)

enum { NBLK = 20, THRESH = 50, NPIX = 12, SLOTS = 4096 };

int main(void)
{
    static const int Fs[5] = {1, 3, 4, 6, 12}, gops[5] = {0, 1, 4, 6, 12}, Cs[5] = {0, 0, 1, 2, 4};
    long ncalls_all = 0, njobs_all = 0, nrem_all = 0, next_all = 0, ndrop_all = 0;
    unsigned seed;
    for (seed = 0; seed < 2000; seed++) {
        int chains, S, R, F, N, mode, keep_all, ncall, call, par = 0, nf_prev = 0, carry[2] = {-1, -1}, s, k, t, i;
        unsigned gcount = 0;
        dsv1_submit_src *src;
        dsv1_submit_stream *st;
        dsv1_submit_pic *prev = NULL;
        unsigned *luma;
        int *level;
        long *coded, (*writer)[2];                      /* invariant: slot -> (stream, running picture number) of its newest picture */
        rs = seed * 2654435761u + 12345u;
        chains = Cs[rnd(5)];
        S = chains ? 1 : 1 + (int)rnd(3); R = chains ? 1 : (rnd(2) ? 3 : 1); F = Fs[rnd(5)]; N = S * R;
        mode = chains ? 0 : (int)rnd(3);                /* 0 CRF, 1 ABR on the device, 2 serial ABR */
        keep_all = rnd(5) == 0; ncall = 1 + (int)rnd(4);
        src = NEW(dsv1_submit_src, S); st = NEW(dsv1_submit_stream, N); luma = NEW(unsigned, (2 * F + 1) * S); level = NEW(int, S);
        coded = NEW(long, N); writer = (long (*)[2])calloc(SLOTS, sizeof(*writer));
        for (i = 0; i < SLOTS; i++) writer[i][0] = -1;
        for (s = 0; s < S; s++) {
            src[s].next_fnum = rnd(4) == 0 ? 0xFFFFFFFEu : rnd(2) * 5u; src[s].prev_gop = 0xFFFFFFFFu; src[s].gop = gops[rnd(5)];
            src[s].force_metadata = 1; src[s].do_scd = rnd(10) < 7; src[s].scene_change_delta = 4;
            level[s] = 60 + (int)rnd(120);
            if (s) src[s].gop = src[0].gop;
        }
        for (call = 0; call < ncall; call++) {
            const int nf = (N == 1 && call == ncall - 1 && rnd(2)) ? 1 + (int)rnd((unsigned)F) : F;
            const int abr = mode != 0, serial = mode == 2;
            dsv1_submit_pic *pics = NEW(dsv1_submit_pic, N * F);
            dsv1_submit_stream *before = NEW(dsv1_submit_stream, N);
            int *pair_cur = NEW(int, S * nf), *pair_ref = NEW(int, S * nf), *pair_pic = NEW(int, S * nf), *ext = NEW(int, N), *rem = NEW(int, N);
            dsv1_submit_job *rjobs = NEW(dsv1_submit_job, N), *jobs = NEW(dsv1_submit_job, N * nf);
            dsv1_submit_call *calls = NEW(dsv1_submit_call, nf);
            int *ch = NEW(int, 4 * (nf + 1)), *call_of = NEW(int, N * F);
            int t0, t1, ncalls = 0, dropped = 0, len0, last0 = -1, carry_in = carry[0], firstP;
            dsv1_sp_pictures pp;
            for (s = 0; s < S; s++)
                for (t = 0; t < nf; t++) {
                    if (rnd(8) == 0) level[s] = 20 + (int)rnd(210);
                    luma[dsv1_sp_slot_of(S, 2 * F + 1, s, gcount + (unsigned)t)] = (unsigned)(level[s] + (int)rnd(3)) * NPIX + rnd(NPIX);
                }
            memcpy(before, st, sizeof(*st) * (size_t)N);
            pp = dsv1_sp_plan_pictures(src, src, S, R, F, nf, 2 * F + 1, gcount, par, NPIX, chains, carry[1], luma, st, st, pics, sizeof(*pics),
                                       pair_cur, pair_ref, pair_pic, ext, rem);
            CHECK(pp.npairs <= S * nf && pp.next <= N && pp.nrem <= N);
            if (pp.nrem) {
                CHECK(prev && nf_prev >= 1);
                dsv1_sp_plan_remedy(rem, pp.nrem, N, F, nf_prev, par, prev, sizeof(*prev), st, rjobs);
            }
            for (i = 0; i < pp.nrem; i++) {
                const dsv1_submit_job *j = &rjobs[i];
                k = j->pic / F;
                CHECK(before[k].recon_dropped && j->remedy && !j->border_hint && j->recon_slot >= 0 && j->recon_slot != j->ref_recon_slot);
                if (j->ref_recon_slot >= 0) CHECK(writer[j->ref_recon_slot][0] == k && writer[j->ref_recon_slot][1] == coded[k] - 2);
                writer[j->recon_slot][0] = k; writer[j->recon_slot][1] = coded[k] - 1;
                for (t = 0; t < i; t++) CHECK(rem[t] != rem[i]);
            }
            for (s = 0; s < S; s++)
                for (t = 0; t < nf; t++) {
                    dsv1_submit_pic *pc = &pics[s * R * F + t];
                    if (pc->has_ref) {                  /* a motion field of the picture's own, at its exact size */
                        dsvg_mv *mv = NEW(dsvg_mv, NBLK);
                        const int nin = rnd(7) == 0 ? 11 + (int)rnd(10) : (int)rnd(6);
                        for (i = 0; i < NBLK; i++) { mv[i].mode = i < nin; mv[i].u.mv.x = (int16_t)((int)rnd(64) - 32); mv[i].u.mv.y = (int16_t)((int)rnd(64) - 32); }
                        dsv1_sp_pic_side(pc, mv, NBLK, THRESH);
                        CHECK(pc->n_intra == nin && pc->reach[0] <= 0 && pc->reach[1] >= 0 && pc->isP == (nin * 100 / NBLK <= THRESH));
                        free(mv);
                    } else dsv1_sp_pic_side(pc, NULL, NBLK, THRESH);
                    for (k = 1; k < R; k++) { pics[(s * R + k) * F + t] = *pc; pics[(s * R + k) * F + t].out_slot += k; }
                }
            firstP = pics[0].isP;
            for (k = 0; k < N; k++) {
                int n = 0;
                for (i = 0; i < pp.nrem; i++) n += rem[i] == k;
                CHECK(n <= 1 && !(before[k].recon_dropped && pics[k * F].isP && n != 1));
            }
            for (t0 = 0; t0 < nf; t0 = t1) {
                int n = 1, d = 0;
                t1 = serial ? t0 + 1 : nf;
                if (chains) n = dsv1_sp_plan_chains(pics, sizeof(*pics), nf, chains, keep_all, par * F, carry, st, jobs, calls, ch, &d);
                else { d = dsv1_sp_plan_steps(pics, sizeof(*pics), N, F, nf, t0, t1, abr, serial, keep_all, st, jobs + t0 * N); calls[ncalls].nsteps = t1 - t0; calls[ncalls].njobs = N; calls[ncalls].first = t0 * N; }
                CHECK(n >= 1 && ncalls + n <= nf);
                ncalls += n; dropped += d;
            }
            for (i = 0; i < N * F; i++) call_of[i] = -1;
            for (i = 0; i < ncalls; i++) {
                int st_, j;
                CHECK(calls[i].first >= 0 && calls[i].first + calls[i].nsteps * calls[i].njobs <= N * nf);
                for (st_ = 0; st_ < calls[i].nsteps; st_++)
                    for (j = 0; j < calls[i].njobs; j++) {
                        const dsv1_submit_job *a = &jobs[calls[i].first + st_ * calls[i].njobs + j];
                        int j2;
                        CHECK(a->pic >= 0 && a->pic < N * F && call_of[a->pic] < 0);
                        call_of[a->pic] = i;
                        for (j2 = 0; chains && j2 < j; j2++) {      /* chains coded side by side never share a pair */
                            const dsv1_submit_job *c = &jobs[calls[i].first + st_ * calls[i].njobs + j2];
                            const int pa = (a->recon_slot > a->ref_recon_slot ? a->recon_slot : a->ref_recon_slot), pb = (c->recon_slot > c->ref_recon_slot ? c->recon_slot : c->ref_recon_slot);
                            if (pa >= 0 && pb >= 0) CHECK(pa / 2 != pb / 2);
                        }
                    }
            }
            for (len0 = 1; chains && len0 < nf && pics[len0].isP; len0++) ;
            for (i = 0; chains && i < nf; i++) if (jobs[i].pic < len0) last0 = i;
            for (i = 0; i < N * nf; i++) {
                const dsv1_submit_job *j = &jobs[i];
                const dsv1_submit_pic *pc = &pics[j->pic];
                dsvg_pic_job dj;
                int i2;
                k = j->pic / F; t = j->pic % F;
                CHECK(call_of[j->pic] >= 0 && t < nf && !j->remedy);
                CHECK(j->out_slot >= par * N * F && j->out_slot < (par + 1) * N * F && j->out_slot == pc->out_slot);
                for (i2 = 0; i2 < i; i2++) CHECK(jobs[i2].out_slot != j->out_slot);
                CHECK(j->recon_slot < SLOTS && j->ref_recon_slot < SLOTS);
                if (j->ref_recon_slot >= 0) CHECK(pc->isP && writer[j->ref_recon_slot][0] == k && writer[j->ref_recon_slot][1] == coded[k] + t - 1);
                else CHECK(!pc->isP);
                CHECK(j->recon_slot < 0 || j->recon_slot != j->ref_recon_slot);
                if (j->recon_slot >= 0) { CHECK(pc->is_ref); writer[j->recon_slot][0] = k; writer[j->recon_slot][1] = coded[k] + t; }
                else if (pc->is_ref) {
                    if (t + 1 < nf) CHECK(!pics[j->pic + 1].isP && !serial && !keep_all);
                    else CHECK(st[k].next_gop && !abr && !keep_all && !chains && st[k].recon_dropped);
                }
                if (chains && firstP && i <= last0 && t >= len0) CHECK((j->recon_slot < 0 || j->recon_slot / 2 != carry_in) && (j->ref_recon_slot < 0 || j->ref_recon_slot / 2 != carry_in));
                if (j->border_hint) {
                    if (t + 1 < nf && pics[j->pic + 1].isP) CHECK(call_of[j->pic + 1] == call_of[j->pic]);
                    else if (t + 1 == nf) CHECK(st[k].next_gop);
                }
                dsv1_sp_fill_job(&dj, pc, j);
                CHECK(dj.src_slot == pc->cur_slot && dj.recon_slot == j->recon_slot && dj.has_reach == pc->isP);
            }
            ncalls_all++; njobs_all += N * nf; nrem_all += pp.nrem; next_all += pp.next; ndrop_all += dropped;
            for (k = 0; k < N; k++) coded[k] += nf;
            free(prev); prev = pics;
            free(before); free(pair_cur); free(pair_ref); free(pair_pic); free(ext); free(rem); free(rjobs); free(jobs); free(calls); free(ch); free(call_of);
            gcount += (unsigned)nf; par ^= 1; nf_prev = nf;
            for (s = 0; s < S; s++) {                   /* the caller between calls: renumbered streams, forced metadata */
                const unsigned r = rnd(100);
                if (r < 15) src[s].next_fnum += 1 + rnd(20);
                else if (r < 40 && src[s].next_fnum < 0x80000000u) { const unsigned back = 1 + rnd(src[s].gop > 0 ? (unsigned)src[s].gop : 1u); src[s].next_fnum = src[s].next_fnum > back ? src[s].next_fnum - back : 0; }
                else if (r < 50 && src[s].gop) src[s].next_fnum = src[s].prev_gop + (uint32_t)src[s].gop;
                if (rnd(10) == 0) src[s].force_metadata = 1;
            }
        }
        free(prev); free(src); free(st); free(luma); free(level); free(coded); free(writer);
    }
    printf("submit_plan_host: %ld calls, %ld jobs, %ld remedied, %ld extended, %ld dropped: invariants hold\n", ncalls_all, njobs_all, nrem_all, next_all, ndrop_all);
    return !(nrem_all && next_all && ndrop_all);
}
