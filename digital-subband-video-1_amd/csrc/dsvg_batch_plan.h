// dsvg_batch_plan.h -- what a coding call (dsvg_code_batch, dsvg_code_batch_rc) decides on the host before it touches the device:
// plain C++17 without a HIP include or a context, so that a stand-alone program can compile it (tools/batch_plan_host.cpp) and the
// device-free query dsvg_code_batch_plan can ask it about any geometry and any switch.  plan_code_batch reads the caller's job, vector
// and flag arrays and BatchGeo, and writes BatchPlan and the intra lists; code_batch_impl (dsvg_pipe.hip) commits the plan to the context,
// fills the job records from it and enqueues from it.  A call the plan refuses has changed nothing.
#ifndef DSVG_BATCH_PLAN_H
#define DSVG_BATCH_PLAN_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <unordered_map>
#include <vector>
#include "../../include/dsvg.h"

#define DSVG_MAX_CODE_STREAMS 4
#ifndef DSVG_BORDER
#define DSVG_BORDER 64       // (dsvg_kernels.hpp has it for the kernels' side)
#endif
static_assert(DSVG_BORDER == DSVG_FRAME_BORDER, "the planned extents are in pixels of the reference's frame border");

// the integers of a context the decisions read (batch_geo in dsvg_pipe.hip derives them, for a context and for the query alike)
struct BatchGeo {
    int nblk, n_recon, n_src, max_jobs, out_slots, rc_slots;
    int mc_fused, code_streams, lazy_border;
    int blk_w, blk_h, nbh, hs, vs, w[2], h[2];        // border_reach: the motion compensation's block grid, luma and chroma plane sizes
};

struct BatchSwitches { bool no_small_split, no_par_enqueue; };      // DSV1_NO_SMALL_SPLIT / DSV1_NO_PAR_ENQUEUE (A/B)
// the process's own, read from the environment once; plan_code_batch takes them as an argument, so a caller can ask it about any setting
static inline const BatchSwitches &batch_switches()
{
    static const BatchSwitches sw = { getenv("DSV1_NO_SMALL_SPLIT") != nullptr, getenv("DSV1_NO_PAR_ENQUEUE") != nullptr };
    return sw;
}

// Device job d = t * njobs + k is the picture at device position k of frame step t; its tables sit at base + d.
struct BatchPlan {
    int nsteps, njobs, total;
    int base;                                   // first out slot of the call's contiguous block
    int NG;                                     // coding streams of the call
    int gk[DSVG_MAX_CODE_STREAMS + 1];          // device positions [gk[g], gk[g+1]) of every step -> stream g
    std::vector<int> nI;                        // [t]: I pictures of the step (they come first)
    std::vector<int> order;                     // [d]: the caller's index, inside its step, of device job d
    std::vector<int> ioff, icnt;                // [NG * t + g]: the (step, group)'s intra blocks in the intra list (mc_fused)
    std::vector<char> noint;                    // ... every P picture of it was scanned for intra blocks (and icnt says how many)
    int iln;                                    // entries of the intra list
    std::vector<int> mvu, stu;                  // [d]: index of the job's vector / flag table among the call's (shared: one index)
    std::vector<char> mvcp, stcp;               // [d]: this job's host table is the one copied there
    int nmv, nst;                               // tables of either kind
    bool mv_contig;                             // the vectors of consecutive device jobs lie back to back (mvs0 of the kernels)
    std::vector<short> ext;                     // [d * 8 + i]: how far the job's reconstruction gets its border written
    std::vector<int> rc_next;                   // [d], rate control: base + the device job of the stream's next picture, -1 in the last step
    std::vector<char> keeps;                    // [NG * t + g]: a picture of the (step, group) keeps its reconstruction
    bool par_enqueue;                           // every group is enqueued by a thread of its own
    char err[256];                              // a refused call: the text for dsvg_last_error
};

// How far a picture with motion field `mv` reads beyond the edges of its reference: the window of an inter block starts at
// the clamped position k_mc / k_fwd_mc_* use (bmc.c:248-255) and is read with a margin of up to 2 pixels before and 3
// after (4-tap luma filter, staging); accumulated (max) into ext[0..3] luma / ext[4..7] chroma of the reference's job.
static inline void border_reach(const BatchGeo &G, const dsvg_mv *mv, const short *reach, short *ext)
{
    int need[8] = {16, 16, 8, 8, 16, 16, 8, 8};           // referenced at all: intra blocks and staging touch the first pixels
    if (reach) {
        // the caller's summary of the vectors: as if the block with the longest vector sat at the edge it points to
        for (int pl = 0; pl < 2; pl++) {
            const int sh = pl ? G.hs : 0, sv = pl ? G.vs : 0;
            int *n = need + 4 * pl;
            n[0] = std::max(n[0], 2 - (reach[0] >> sh));
            n[1] = std::max(n[1], (reach[1] >> sh) + 4);
            n[2] = std::max(n[2], 2 - (reach[2] >> sv));
            n[3] = std::max(n[3], (reach[3] >> sv) + 4);
        }
    } else
    for (int b = 0; b < G.nblk; b++) {
        if (mv[b].mode != 0) continue;
        const int bi = b % G.nbh, bj = b / G.nbh;
        for (int pl = 0; pl < 2; pl++) {
            const int sh = pl ? G.hs : 0, sv = pl ? G.vs : 0;
            const int bw = G.blk_w >> sh, bh = G.blk_h >> sv, pw = G.w[pl], ph = G.h[pl];
            const int x = bi * bw, y = bj * bh;
            if (x >= pw || y >= ph) continue;
            const int cw = std::min(bw, pw - x), ch = std::min(bh, ph - y);
            const int dx = mv[b].u.mv.x >> sh, dy = mv[b].u.mv.y >> sv;
            const int wx = std::min(std::max(x + (dx >> 1), -DSVG_BORDER), pw - bw + DSVG_BORDER - 1);
            const int wy = std::min(std::max(y + (dy >> 1), -DSVG_BORDER), ph - bh + DSVG_BORDER - 1);
            int *n = need + 4 * pl;
            n[0] = std::max(n[0], 2 - wx);
            n[1] = std::max(n[1], wx + cw + 3 - (pw - 1));
            n[2] = std::max(n[2], 2 - wy);
            n[3] = std::max(n[3], wy + ch + 3 - (ph - 1));
        }
    }
    bool whole = false;
    for (int i = 0; i < 8; i++) whole = whole || need[i] > DSVG_BORDER - 4;       // reaches the border's last pixels (or the byte
    for (int i = 0; i < 8; i++)                                                  // after them = the next row's first): everything
        ext[i] = (short)std::max((int)ext[i], whole ? DSVG_BORDER : need[i]);
}

// The plan of one call: nsteps frame steps of njobs pictures each (jobs[step * njobs + j]), rcj = the rate-control jobs of
// dsvg_code_batch_rc or null, profiled = the kernel timing hooks are on.  ilist = the START of the context's intra-list table
// (out_slots * nblk entries): the call's lists go to ilist + base * nblk, and nothing is written before every check has passed.
// Returns DSVG_OK, or the code of the first failed check with its text in P.err -- call arguments, rate-control jobs, the out-slot
// block, then the picture jobs in device order.
static inline int plan_code_batch(const BatchGeo &G, const BatchSwitches &sw, int nsteps, int njobs, const dsvg_pic_job *jobs, const dsvg_rc_job *rcj,
                                  bool profiled, int *ilist, BatchPlan &P)
{
    P.err[0] = 0;
    if (!jobs || nsteps < 1 || njobs < 1 || njobs > G.max_jobs || nsteps * njobs > G.out_slots) {
        snprintf(P.err, sizeof P.err, "bad code_batch arguments"); return DSVG_ERR_ARG;
    }
    if (rcj)
        for (int i = 0; i < nsteps * njobs; i++) {
            if (rcj[i].rc_slot < 0 || rcj[i].rc_slot >= G.rc_slots || rcj[i].prefix_len < 0) { snprintf(P.err, sizeof P.err, "bad rate-control job %d", i); return DSVG_ERR_ARG; }
            if (i >= njobs && rcj[i].rc_slot != rcj[i - njobs].rc_slot) { snprintf(P.err, sizeof P.err, "a stream must keep its position from frame step to frame step (rate-control job %d)", i); return DSVG_ERR_ARG; }
            for (int k = i - i % njobs; k < i; k++)
                if (rcj[k].rc_slot == rcj[i].rc_slot) { snprintf(P.err, sizeof P.err, "two pictures of one rate-controlled stream in one frame step (jobs %d, %d)", k, i); return DSVG_ERR_ARG; }
        }
    const int total = nsteps * njobs;
    int base = jobs[0].out_slot;
    for (int i = 1; i < total; i++) base = std::min(base, jobs[i].out_slot);
    if (base < 0 || base + total > G.out_slots) { snprintf(P.err, sizeof P.err, "out slots of a batch must be a contiguous block"); return DSVG_ERR_ARG; }
    P.nsteps = nsteps; P.njobs = njobs; P.total = total; P.base = base;
    // device order inside a step: intra jobs first, then inter jobs (kernels are specialised per type)
    P.nI.assign((size_t)nsteps, 0);
    P.order.resize((size_t)total);
    for (int t = 0; t < nsteps; t++) {
        const dsvg_pic_job *js = jobs + (size_t)t * njobs;
        int *ord = P.order.data() + (size_t)t * njobs, n = 0;
        for (int i = 0; i < njobs; i++) if (js[i].ref_recon_slot < 0) ord[n++] = i;
        P.nI[t] = n;
        for (int i = 0; i < njobs; i++) if (js[i].ref_recon_slot >= 0) ord[n++] = i;
        for (int k = 0; k < njobs; k++) {
            const dsvg_pic_job &j = js[ord[k]];
            if (j.src_slot < 0 || j.src_slot >= G.n_src || j.ref_recon_slot >= G.n_recon || j.recon_slot >= G.n_recon ||
                j.out_slot < base || j.out_slot >= base + total || !j.stable_blocks || (j.ref_recon_slot >= 0 && !j.mvs)) {
                snprintf(P.err, sizeof P.err, "bad picture job (step %d job %d)", t, ord[k]); return DSVG_ERR_ARG;
            }
        }
    }
    const auto job = [&](int t, int k) -> const dsvg_pic_job & { return jobs[(size_t)t * njobs + P.order[(size_t)t * njobs + k]]; };
    // Two coding streams, each with half of the pictures of every frame step: the chain of a step has a dozen small,
    // latency-bound kernels (levels >= 4, LL quantiser, scan) during which one half leaves the chip to the other
    // half's large kernels.  Needs steps of one picture type (the device order is I jobs, then P jobs) and enough jobs.
    int NG = std::min(std::min(G.code_streams, DSVG_MAX_CODE_STREAMS), njobs / 8);
    // Small frame steps (ABR streams, a GPU's share of a few 4K GOPs, one stream's chains) are bound by the latency of the chain's
    // dozen launches, not by the chip: two halves on two streams run side by side (round 4; DSV1_NO_SMALL_SPLIT=1: one stream)
    if (NG < 2 && njobs >= 2 && G.code_streams >= 2 && !sw.no_small_split) NG = 2;
    if (NG < 1) NG = 1;
    bool anyP = false;
    for (int t = 0; t < nsteps; t++) {
        if (P.nI[t] != 0 && P.nI[t] != njobs) NG = 1;
        anyP = anyP || P.nI[t] == 0;
    }
    if (!anyP) NG = 1;               // I pictures only: their kernels are large and gain nothing (intra-only measured 3 % slower split)
    if (NG > 1) {
        // The groups run on different streams and are only joined at the end of the call: a reconstruction written by
        // group g in step k may be read as a reference in step k+1 only by group g (same stream = ordered), and no two
        // groups may write one slot.  Callers that keep stream s at position s of every step satisfy this; any other
        // job order takes the single-stream path instead of racing.
        std::vector<int> writer((size_t)G.n_recon, -1), now((size_t)G.n_recon);
        for (int t = 0; t < nsteps && NG > 1; t++) {
            std::fill(now.begin(), now.end(), -1);
            for (int k = 0; k < njobs; k++) {
                const dsvg_pic_job &j = job(t, k);
                int gg = 0;                                          // group of device position k (the gk[] split below)
                while (gg + 1 < NG && k >= (int)((long)njobs * (gg + 1) / NG)) gg++;
                if (j.ref_recon_slot >= 0 && writer[j.ref_recon_slot] >= 0 && writer[j.ref_recon_slot] != gg) NG = 1;
                if (j.recon_slot >= 0) {
                    if (now[j.recon_slot] >= 0 && now[j.recon_slot] != gg) NG = 1;
                    if (writer[j.recon_slot] >= 0 && writer[j.recon_slot] != gg) NG = 1;     // overwriting what another group may still read
                    now[j.recon_slot] = gg;
                }
            }
            for (int r = 0; r < G.n_recon; r++) if (now[r] >= 0) writer[r] = now[r];
        }
    }
    P.NG = NG;
    int *gk = P.gk;
    for (int g = 0; g <= NG; g++) gk[g] = (int)((long)njobs * g / NG);
    P.ioff.assign((size_t)NG * nsteps, 0); P.icnt.assign((size_t)NG * nsteps, 0);
    P.noint.assign((size_t)NG * nsteps, 1);
    P.keeps.assign((size_t)NG * nsteps, 0);
    int *il = ilist + (size_t)base * G.nblk;               // intra blocks of each (step, group)'s P pictures (mc_fused)
    int iln = 0;
    for (int t = 0; t < nsteps; t++)
        for (int k = 0; k < njobs; k++) {
            const dsvg_pic_job &j = job(t, k);
            const int isP = j.ref_recon_slot >= 0;
            int g = 0;
            while (k >= gk[g + 1]) g++;
            if (k == gk[g]) P.ioff[NG * t + g] = iln;
            if (j.recon_slot >= 0) P.keeps[NG * t + g] = 1;
            if (isP && !G.mc_fused) P.noint[NG * t + g] = 0;
            if (isP && G.mc_fused && !j.no_intra_blocks) {
                // index relative to the first P job of the group's launch
                const int k0 = std::max(gk[g], P.nI[t]);
                for (int b = 0; b < G.nblk; b++)
                    if (j.mvs[b].mode != 0) il[iln++] = (k - k0) * G.nblk + b;
            }
            P.icnt[NG * t + g] = iln - P.ioff[NG * t + g];
        }
    P.iln = iln;
    // Block tables shared between jobs (quality ladders, dsv1_ladder_open: every rung of a source passes the SAME host arrays for
    // the source's motion field and stability flags): jobs of the call that pass the same pointer get one device copy.  Keyed on
    // the pointer, not the content -- a call that shares no pointer keeps the layout it always had (device job base + i's tables
    // at table index i) and uploads the same bytes.  mvu / stu: table index of job i; mvcp / stcp: job i is the one copied.
    // (Several jobs may now read one source slot: no coding kernel writes it -- JobDev.src / srcp are const, and the in-place
    // luma / chroma of slot_y / slot_cu / slot_cv is the caller's clip, read only.)
    P.mvu.resize((size_t)total); P.stu.resize((size_t)total);
    P.mvcp.assign((size_t)total, 0); P.stcp.assign((size_t)total, 0);
    int nmv = 0, nst = 0;
    {
        std::unordered_map<const void *, int> mvk, stk;
        std::vector<char> mvdone((size_t)total, 0);
        for (int i = 0; i < total; i++) {
            const dsvg_pic_job &j = job(i / njobs, i % njobs);
            const auto s = stk.emplace(j.stable_blocks, nst);
            if (s.second) { P.stcp[(size_t)i] = 1; nst++; }
            P.stu[(size_t)i] = s.first->second;
            if (!j.mvs) P.mvu[(size_t)i] = nmv++;                        // (I pictures need none: never shared)
            else {
                const auto m = mvk.emplace(j.mvs, nmv);
                if (m.second) nmv++;
                P.mvu[(size_t)i] = m.first->second;
            }
            if (j.ref_recon_slot >= 0 && !mvdone[(size_t)P.mvu[(size_t)i]]) { mvdone[(size_t)P.mvu[(size_t)i]] = 1; P.mvcp[(size_t)i] = 1; }
        }
    }
    P.nmv = nmv; P.nst = nst;
    P.mv_contig = nmv == total;
    P.ext.assign((size_t)total * 8, (short)DSVG_BORDER);
    if (G.lazy_border) {
        // Borders of the reconstructions: a reconstruction is read beyond its edges only by the pictures that predict from it,
        // and only as far as their motion vectors point -- which is known here (the vectors of every picture of the call are).
        // A slot rewritten within the call gets the reach of the pictures in between; a slot that outlives the call gets the
        // whole border unless the caller vouches that no later call predicts from it (border_hint).
        std::vector<int> writer((size_t)G.n_recon, -1);
        for (int t = 0; t < nsteps; t++) {
            for (int k = 0; k < njobs; k++) {
                const dsvg_pic_job &j = job(t, k);
                const int w = j.ref_recon_slot >= 0 ? writer[j.ref_recon_slot] : -1;
                if (w >= 0) border_reach(G, j.mvs, j.has_reach ? j.mv_reach : nullptr, &P.ext[(size_t)w * 8]);
            }
            for (int k = 0; k < njobs; k++) {
                const dsvg_pic_job &j = job(t, k);
                for (int i = 0; i < 8; i++) P.ext[(size_t)(t * njobs + k) * 8 + i] = 0;   // (a picture without a reconstruction too: nobody reads the border of its work frame -- advisor round 5)
                if (j.recon_slot < 0) continue;
                writer[j.recon_slot] = t * njobs + k;
            }
        }
        for (int r = 0; r < G.n_recon; r++)
            if (writer[r] >= 0 && !job(writer[r] / njobs, writer[r] % njobs).border_hint)
                for (int i = 0; i < 8; i++) P.ext[(size_t)writer[r] * 8 + i] = DSVG_BORDER;
    }
    P.rc_next.clear();
    if (rcj) {
        // the device job of each stream's next picture: the same caller position in the next frame step
        std::vector<int> dpos((size_t)njobs);                // device position of the caller's job i of the next step
        P.rc_next.assign((size_t)total, -1);
        for (int t = 0; t + 1 < nsteps; t++) {
            for (int k = 0; k < njobs; k++) dpos[(size_t)P.order[(size_t)(t + 1) * njobs + k]] = k;
            for (int k = 0; k < njobs; k++) P.rc_next[(size_t)t * njobs + k] = base + (t + 1) * njobs + dpos[(size_t)P.order[(size_t)t * njobs + k]];
        }
    }
    // (the event brackets of the profiling hooks are kept in one list: profiled calls are enqueued by one thread alone)
    P.par_enqueue = NG > 1 && nsteps * 13 >= 100 && njobs < 64 && !profiled && !sw.no_par_enqueue;
    return DSVG_OK;
}

#endif
