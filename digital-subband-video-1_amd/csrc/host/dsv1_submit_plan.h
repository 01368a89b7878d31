/* dsv1_submit_plan.h -- private: what an encoder session's submit (dsv1_enc.c, batch_submit_impl) decides, in pure functions: which
 * pictures start a GOP or a scene, which pairs go to the motion search, which reconstruction slot every picture predicts from and is
 * kept in, which reconstructions nobody reads, which borders may stay short, and -- chain mode -- the chains, rounds and calls.  No
 * device, no batch, no encoder struct, no allocation, no environment: every table is the caller's.  The session commits and enqueues
 * from the results; dsv1_submit_plan (include/dsv1_api.h) answers the same questions on plain arrays.  Restated from the reference's
 * side (dsv_encoder.c:538-554,624-653,665-708) in tests/submit_plan.py.  The types are include/dsv1_api.h's (Submit plan). */
#ifndef DSV1_SUBMIT_PLAN_H
#define DSV1_SUBMIT_PLAN_H

#include <stdlib.h>
#include <string.h>
#include "../../../include/dsv1_api.h"

/* the pictures of a call lie [stream][F] in records of `stride` bytes that begin with a dsv1_submit_pic (the session's own records
 * carry the tables behind it) */
static inline dsv1_submit_pic *dsv1_sp_pic(void *pics, size_t stride, int i) { return (dsv1_submit_pic *)((char *)pics + stride * (size_t)i); }
static inline const dsv1_submit_pic *dsv1_sp_cpic(const void *pics, size_t stride, int i) { return (const dsv1_submit_pic *)((const char *)pics + stride * (size_t)i); }

/* THE GOP RULE (dsv_encoder.c:538-554,702-708): does frame number fnum start a GOP for a source in this state */
static inline int dsv1_sp_gop_starts_at(const dsv1_submit_src *st, uint32_t fnum)
{
    return st->force_metadata || (uint32_t)(st->prev_gop + (uint32_t)st->gop) <= fnum;
}

/* source slot of frame g (the batch's frame counter) of source s: a ring of `rows` rows of S slots */
static inline int dsv1_sp_slot_of(int S, int rows, int s, unsigned g) { return (int)(g % (unsigned)rows) * S + s; }

/* THE OTHER SLOT OF A PAIR {first, first + stride}: where the next reconstruction goes when the newest one is in `cur` (-1: none yet) */
static inline int dsv1_sp_pair_next(int first, int stride, int cur) { return cur == first ? first + stride : first; }

/* STEP 2 of a submit, per source in coding order: frame numbers, GOP starts, scene cuts (luma[]: raw sums by source slot), the
 * slots.  Writes the lead rung's pictures (stream s * R), the motion-search pairs (cur / ref slot, picture), the reconstructions
 * that need their whole border after all (ext[]: the call before promised a GOP start, the caller renumbered the stream), the
 * streams whose dropped reconstruction is needed after all (rem[]), the sources' state after the call (src_out) and the streams'
 * (st_out: the two promises of the call before are spent; next_gop = the rule for the stream's next frame number). */
typedef struct { int npairs, next, nrem; } dsv1_sp_pictures;
static inline dsv1_sp_pictures dsv1_sp_plan_pictures(const dsv1_submit_src *src, dsv1_submit_src *src_out, int S, int R, int F, int nf, int rows,
                                                     unsigned gcount, int par, int npix_small, int chains, int carry_cur, const unsigned *luma,
                                                     const dsv1_submit_stream *st, dsv1_submit_stream *st_out, void *pics, size_t stride,
                                                     int *pair_cur, int *pair_ref, int *pair_pic, int *ext, int *rem)
{
    const int N = S * R;
    dsv1_sp_pictures o = {0, 0, 0};
    int s, t, k;
    for (s = 0; s < S; s++) {
        dsv1_submit_src e = src[s];
        for (t = 0; t < nf; t++) {
            dsv1_submit_pic *pc = dsv1_sp_pic(pics, stride, s * R * F + t);
            pc->fnum = e.next_fnum++;
            pc->cur_slot = dsv1_sp_slot_of(S, rows, s, gcount + (unsigned)t);
            pc->ref_slot = dsv1_sp_slot_of(S, rows, s, gcount + (unsigned)t + (unsigned)rows - 1u);
            pc->out_slot = par * N * F + t * N + s * R;
            pc->gop_start = 0; pc->forced_intra = 0;
            if (dsv1_sp_gop_starts_at(&e, pc->fnum)) {
                pc->gop_start = 1;
                e.prev_gop = pc->fnum;
                e.force_metadata = 0;
            }
            if (e.gop == DSV_GOP_INTRA) {
                pc->is_ref = 0; pc->has_ref = 0;
            } else {
                pc->is_ref = 1;
                pc->has_ref = !pc->gop_start;
                if (e.do_scd) {
                    const int al = (int)luma[pc->cur_slot] / npix_small;
                    if (abs(e.prev_avg_luma - al) > e.scene_change_delta) { pc->has_ref = 0; pc->forced_intra = 1; }
                    e.prev_avg_luma = al;
                }
            }
            for (k = s * R; t == 0 && k < s * R + R; k++) {     /* (every rung of the source) */
                if (pc->has_ref && st[k].border_skipped) ext[o.next++] = chains ? carry_cur : k + N * st[k].rpar;
                if (pc->has_ref && st[k].recon_dropped) rem[o.nrem++] = k;
            }
            if (pc->has_ref) {
                pair_cur[o.npairs] = pc->cur_slot;
                pair_ref[o.npairs] = pc->ref_slot;
                pair_pic[o.npairs] = s * R * F + t;
                o.npairs++;
            }
        }
        src_out[s] = e;
        for (k = s * R; k < s * R + R; k++) {
            st_out[k] = st[k];
            st_out[k].border_skipped = 0; st_out[k].recon_dropped = 0;
            st_out[k].next_gop = (unsigned char)dsv1_sp_gop_starts_at(&e, e.next_fnum);
        }
    }
    return o;
}

/* the forced-intra rule (dsv_encoder.c:624-653) on a picture's count of intra blocks; isP is final after it */
static inline void dsv1_sp_intra_decide(dsv1_submit_pic *pc, int n_intra, int nblk, int intra_pct_thresh)
{
    if (pc->has_ref) {
        pc->n_intra = n_intra;
        pc->forced_intra = 0;
        if (n_intra * 100 / nblk > intra_pct_thresh) { pc->has_ref = 0; pc->forced_intra = 1; }
    }
    pc->isP = pc->has_ref;
}

/* STEP 4, the half that reads only the motion field: the intra blocks, the full-pel reach of the inter blocks' vectors (each taken
 * with 0), the forced-intra decision */
static inline void dsv1_sp_pic_side(dsv1_submit_pic *pc, const dsvg_mv *mvs, int nblk, int intra_pct_thresh)
{
    int nintra = 0, i, x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    if (pc->has_ref) {
        for (i = 0; i < nblk; i++) {
            const dsvg_mv *m = &mvs[i];
            int dx, dy;
            if (m->mode != 0) { nintra++; continue; }
            dx = m->u.mv.x >> 1; dy = m->u.mv.y >> 1;
            if (dx < x0) x0 = dx;
            if (dx > x1) x1 = dx;
            if (dy < y0) y0 = dy;
            if (dy > y1) y1 = dy;
        }
        pc->reach[0] = (short)x0; pc->reach[1] = (short)x1; pc->reach[2] = (short)y0; pc->reach[3] = (short)y1;
    }
    dsv1_sp_intra_decide(pc, nintra, nblk, intra_pct_thresh);
}

/* THE ONE PLACE a dsvg_pic_job is written.  The quantiser and the pointers to the picture's tables are the caller's. */
static inline void dsv1_sp_fill_job(dsvg_pic_job *j, const dsv1_submit_pic *pc, const dsv1_submit_job *sj)
{
    j->src_slot = pc->cur_slot;
    j->ref_recon_slot = sj->ref_recon_slot;
    j->recon_slot = sj->recon_slot;
    j->out_slot = sj->out_slot;
    j->no_intra_blocks = pc->isP && pc->n_intra == 0;
    j->border_hint = sj->border_hint;
    j->has_reach = sj->remedy ? 0 : pc->isP;            /* (a remedied picture: the whole border, no reach) */
    if (sj->remedy) memset(j->mv_reach, 0, sizeof j->mv_reach);
    else memcpy(j->mv_reach, pc->reach, sizeof pc->reach);
}

/* The REMEDY call (step 3): the last pictures of the call before (prev: its pictures, nf_prev of them per stream) of the streams
 * rem[0..n) once more, each into the other slot of its stream's pair, kept this time: one step of n jobs into the first out slots of
 * the half `par`.  st: the streams' state, updated in place. */
static inline void dsv1_sp_plan_remedy(const int *rem, int n, int N, int F, int nf_prev, int par, const void *prev, size_t stride,
                                       dsv1_submit_stream *st, dsv1_submit_job *jobs)
{
    int i;
    for (i = 0; i < n; i++) {
        const int s = rem[i], cur = s + N * st[s].rpar;
        dsv1_submit_job *sj = &jobs[i];
        sj->pic = s * F + nf_prev - 1;
        sj->ref_recon_slot = dsv1_sp_cpic(prev, stride, sj->pic)->isP ? cur : -1;
        sj->recon_slot = dsv1_sp_pair_next(s, N, cur);
        sj->out_slot = par * N * F + i;
        sj->border_hint = 0; sj->remedy = 1;
        st[s].rpar = (unsigned char)(sj->recon_slot != s);
        st[s].has_recon = 1;
    }
}

/* STEP 5, batch mode, ONE job: picture t of output stream s in a call of nf.  A picture predicts from its stream's current slot and is
 * kept in the pair's other one -- unless nobody reads it (dead: the stream's next picture has no reference; for the call's last picture,
 * its next frame number starts a GOP and the stream is CRF: dsv_encoder.c:665-708).  border_hint: the next picture of the stream is in
 * this call or starts a GOP.  The serial ABR path (one step per call: the next quantiser needs the packet) keeps everything and promises
 * nothing.  st: the stream's state, updated in place; returns 1 where the reconstruction is dropped.  Steps in coding order. */
static inline int dsv1_sp_plan_step_job(const void *pics, size_t stride, int N, int F, int nf, int t, int s, int abr, int serial, int keep_all,
                                        dsv1_submit_stream *st, dsv1_submit_job *sj)
{
    const dsv1_submit_pic *pc = dsv1_sp_cpic(pics, stride, s * F + t);
    const int cur = s + N * st->rpar;
    int dead = 0;
    if (pc->is_ref && !serial && !keep_all)
        dead = t + 1 < nf ? !dsv1_sp_cpic(pics, stride, s * F + t + 1)->has_ref : !abr && st->next_gop;
    sj->pic = s * F + t;
    sj->out_slot = pc->out_slot;
    sj->remedy = 0;
    sj->ref_recon_slot = pc->isP ? cur : -1;
    sj->recon_slot = -1;
    if (pc->is_ref && !dead) {
        sj->recon_slot = dsv1_sp_pair_next(s, N, cur);
        st->rpar = (unsigned char)(sj->recon_slot != s);
        st->has_recon = 1;
    }
    sj->border_hint = !serial && (t + 1 < nf || st->next_gop);
    if (t + 1 == nf) {
        st->recon_dropped = (unsigned char)dead;
        st->border_skipped = (unsigned char)(sj->border_hint && sj->recon_slot >= 0);
    }
    return dead;
}
/* ... and frame steps [t0, t1) across the N streams as a table, jobs[(t - t0) * N + s] (the query; the session fills its device jobs
 * from dsv1_sp_plan_step_job in one pass) */
static inline int dsv1_sp_plan_steps(const void *pics, size_t stride, int N, int F, int nf, int t0, int t1, int abr, int serial, int keep_all,
                                     dsv1_submit_stream *st, dsv1_submit_job *jobs)
{
    int t, s, dropped = 0;
    for (t = t0; t < t1; t++)
        for (s = 0; s < N; s++) dropped += dsv1_sp_plan_step_job(pics, stride, N, F, nf, t, s, abr, serial, keep_all, &st[s], &jobs[(t - t0) * N + s]);
    return dropped;
}

/* STEP 5, chain mode (ONE stream, nf pictures with their final decisions): a picture without a reference starts a chain, the call's
 * first picture continues the chain the call before left open when it is a P picture (carry[0]: its pair, carry[1]: the slot of its
 * newest reconstruction, -1: none).  At most C chains side by side make a round; frame step k of a round codes the k-th picture of
 * each of its live chains; consecutive steps with an equal number of live chains are one call.  C + 1 pairs: the carried one is left
 * alone while its chain goes on.  A chain's last picture whose successor is in this call has no reader: no reconstruction.  Writes
 * the jobs in enqueue order, every picture's out slot (from out_base on, in that order), the calls, and carry / st[0] after the call.
 * ch: 4 * (nf + 1) ints of scratch.  Returns the number of calls; -1: a P picture without a reference picture on the device
 * (nothing written). */
static inline int dsv1_sp_plan_chains(void *pics, size_t stride, int nf, int C, int keep_all, int out_base, int carry[2],
                                      dsv1_submit_stream *st, dsv1_submit_job *jobs, dsv1_submit_call *calls, int *ch, int *dropped)
{
    int *start = ch, *len = ch + (nf + 1), *pair = ch + 2 * (nf + 1), *cur = ch + 3 * (nf + 1);
    const int firstP = dsv1_sp_pic(pics, stride, 0)->isP;
    int nch = 0, t, g0, idx = 0, ncalls = 0;
    if (firstP && carry[1] < 0) return -1;
    *dropped = 0;
    for (t = 0; t < nf; t++) {
        if (t == 0 || !dsv1_sp_pic(pics, stride, t)->isP) { start[nch] = t; len[nch] = 0; nch++; }
        len[nch - 1]++;
    }
    for (g0 = 0; g0 < nch; g0 += C) {
        const int gn = nch - g0 < C ? nch - g0 : C;
        int c, L = 0, k = 0, nextpair = 0;
        for (c = g0; c < g0 + gn; c++) {
            if (len[c] > L) L = len[c];
            if (c == 0 && firstP) { pair[c] = carry[0]; cur[c] = carry[1]; continue; }
            if (g0 == 0 && firstP && nextpair == carry[0]) nextpair++;
            pair[c] = nextpair++;
            cur[c] = -1;
        }
        while (k < L) {
            int nj = 0, k2, kk;
            for (c = g0; c < g0 + gn; c++) nj += len[c] > k;
            for (k2 = k + 1; k2 < L; k2++) {
                int n2 = 0;
                for (c = g0; c < g0 + gn; c++) n2 += len[c] > k2;
                if (n2 != nj) break;
            }
            calls[ncalls].nsteps = k2 - k; calls[ncalls].njobs = nj; calls[ncalls].first = idx;
            ncalls++;
            for (kk = k; kk < k2; kk++)
                for (c = g0; c < g0 + gn; c++) {
                    const int tt = start[c] + kk, last = kk + 1 == len[c];
                    dsv1_submit_pic *pc;
                    dsv1_submit_job *sj;
                    if (len[c] <= kk) continue;
                    pc = dsv1_sp_pic(pics, stride, tt);
                    sj = &jobs[idx++];
                    sj->pic = tt;
                    sj->remedy = 0;
                    sj->ref_recon_slot = pc->isP ? cur[c] : -1;
                    sj->recon_slot = -1;
                    if (pc->is_ref && last && tt + 1 < nf && !keep_all) (*dropped)++;
                    else if (pc->is_ref) sj->recon_slot = cur[c] = dsv1_sp_pair_next(2 * pair[c], 1, cur[c]);
                    sj->out_slot = pc->out_slot = out_base++;
                    /* who predicts from this reconstruction?  The chain's next picture -- in this call (the border then goes as
                     * far as that picture's vectors reach), or in a later one (0: the whole border).  The chain's last picture:
                     * nobody, when the stream's next picture starts the next chain of this call or a GOP; else unknown */
                    sj->border_hint = !last ? kk + 1 < k2 : tt + 1 < nf ? 1 : st[0].next_gop;
                    if (tt + 1 == nf) st[0].border_skipped = (unsigned char)(sj->border_hint && sj->recon_slot >= 0);
                }
            k = k2;
        }
    }
    if (dsv1_sp_pic(pics, stride, nf - 1)->is_ref) {
        carry[0] = pair[nch - 1]; carry[1] = cur[nch - 1];
        st[0].has_recon = 1;
    }
    return ncalls;
}

#endif
