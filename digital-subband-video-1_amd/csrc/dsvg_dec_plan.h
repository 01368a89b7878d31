// dsvg_dec_plan.h -- what a decoder call (dsvg_decode_pictures, and its repeat on int32 coefficients from dec_resolve) decides on the
// host before it touches the context or the device: plain C++17 without a HIP include or a context, so that a stand-alone program can
// compile it (tools/dec_plan_host.cpp) and the device-free query dsvg_decode_plan can ask it about any geometry and any switch.
// plan_decode reads the caller's jobs, their payloads' plane headers and DecGeo, and writes DecPlan; decode_impl (dsvg_pipe.hip) commits
// the plan to the context (dec_commit) and enqueues from it (dec_enqueue).  A call the plan refuses has changed nothing.
#ifndef DSVG_DEC_PLAN_H
#define DSVG_DEC_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../../include/dsvg.h"

#ifndef HZ_CHUNK
#define HZ_CHUNK 2048        // (dsvg_dev.hpp has it for the kernels' side)
#endif

// the integers of a context the decisions read (dec_geo in dsvg_pipe.hip derives them, for a context and for the query alike)
struct DecGeo {
    int n_recon, max_jobs, nblk;
    int cw[3], ch[3];                 // coefficient planes: the bound of a plane's length
    // scan chunks of a plane (make_hz_plane, dsvg_common.hip: ceil(nscan / HZ_CHUNK), nscan summed from the plane's width and height
    // alone -- the quantiser, the picture type and the plane's index only enter the region quantisers): the clamp of max_entries
    int nchunks[3];
    int sym_ok[2], ov[2];             // luma / chroma planes can take the int16 symbol path; have cells shared between scan regions
    int mc_patch;                     // patch motion compensation: the geometry is fusable and the context has an intra list
    int nbh, nbv, blk_w, blk_h, hs, vs, pw[3], ph[3];      // the motion compensation's block grid and pixel planes
    int second_stream;                // a second coding stream and its join event exist
};

// DSV1_NO_DEC_SYM, DSV1_NO_DEC_SYM_I, DSV1_DEC_ONE_STREAM, DSV1_NO_MC_PATCH, DSV1_NO_INPLACE_PRED (A/B): read from the environment by
// dsvg_pipe.hip, once per context or process; plan_decode takes them as an argument, so a caller can ask it about any setting
struct DecSwitches { bool no_dec_sym, no_dec_sym_I, one_stream, no_mc_patch, no_inplace_pred; };

namespace {
struct Rd {                          // MSB-first reader (bs.c:111-125,148-157,209-219), bounded: past `end` bits read as 1
    const uint8_t *p; unsigned pos, end;
    unsigned bit() { if (pos >= end) return 1u; unsigned b = (p[pos >> 3] >> (7 - (pos & 7))) & 1u; pos++; return b; }
    unsigned bits(int n) { unsigned v = 0; while (n--) v = (v << 1) | bit(); return v; }
    unsigned ueg() { unsigned m = 1; int k = 0; while (!bit() && k++ < 32) m = (m << 1) | bit(); return m - 1; }
    int seg() { int v = (int)ueg(); return (v && bit()) ? -v : v; }
    int neg() { int v = (int)ueg() + 1; return bit() ? -v : v; }
    void align() { pos = (pos + 7u) & ~7u; }
};
}

enum { DEC_PATH_I32 = 0, DEC_PATH_SYM_I = 1, DEC_PATH_SYM_P = 2 };     // where a picture's detail entries go
enum { DEC_MC_NONE = 0, DEC_MC_PLAIN = 1, DEC_MC_PATCH = 2 };           // no P picture; k_mc; k_mc_patch plus k_mc by intra list

struct DecPlanJob {                  // one picture, in device order
    int src;                         // the caller's index
    int isP, path;
    int dec_sym[3];                  // per plane: entries into the int16 symbol plane
    bool wide;                       // limits: every level 0x3fffffff (I pictures on the symbol path), else the P picture's ranges
    bool inplace;                    // the prediction is written into the reconstruction slot
    int dc[3], runs[3], len[3];      // the plane header (SEG(DC), the 32-bit run count) and the payload's bytes
    long long bitpos[3];             // first bit of the code chain
    size_t boff[3], moff[3];         // the plane in the call's payload blob (bytes) and among its parse records
};

struct DecPlan {
    int njobs, nI;                   // I pictures come first
    std::vector<DecPlanJob> job;
    size_t blob, nmeta;              // bytes of the payload blob; parse records (one per 128-bit payload chunk, two spare per plane)
    int max_entries, max_chunks;     // the parse / scatter grids
    int insym;                       // enqueue_recon: bit 0 I pictures, bit 1 luma of P pictures, bit 2 chroma of P pictures from symbols
    int f0;                          // first job that may raise a flag / holds symbols to take down again
    bool anysym;                     // some plane of the call is on the symbol path: flags come back, the pending record is armed
    bool scatter_one;                // every plane of the call on the symbol path: one scatter launch instead of three
    bool resolve;                    // k_hz_dec_resolve runs (shared cells on a symbol plane)
    bool fork;                       // motion compensation on the second coding stream
    int mc, ex0, ey0;                // DEC_MC_*; block columns / rows from (ex0, ey0) on hold ragged 8x8 patches in some plane
    int draw0, draw1;                // jobs [draw0, draw1) get the debug overlay
    char err[256];                   // a refused call: the text for dsvg_last_error
};

// Range of a P picture of 8-bit video per transform level: detail <= 4 x the LL below, LL = 4/5 of that (level 1 of a P picture
// unscaled), a dequantised value <= twice its coefficient (hzcc.c:94-128: a non-zero symbol needs 2|v| > q).  wide: I pictures on the
// symbol path, whose inverse dequantises in 32 bits -- the only thing they cannot hold is a symbol beyond int16.
static inline void dec_limits(bool wide, int out[16])
{
    if (wide) { for (int lv = 0; lv < 16; lv++) out[lv] = 0x3fffffff; return; }
    long ll = 512;
    out[1] = 2 * 510;
    for (int lv = 2; lv < 16; lv++) {
        const long det = 4 * ll;
        out[lv] = (int)std::min<long>(2 * det, 0x3fffffff);
        ll = std::min<long>(det * 4 / 5, 0x1fffffff);
    }
    out[0] = (int)std::min<long>(2 * ll, 0x3fffffff);
}

// The blocks of one P picture that k_mc takes by list beside k_mc_patch: the intra blocks and the block columns / rows from (ex0, ey0)
// on (the two kernels share that predicate).  Entries first + block, written to out (nblk entries fit); returns their number.
static inline int dec_intra_list(const DecGeo &G, const dsvg_mv *mv, int first, int ex0, int ey0, int *out)
{
    int n = 0;
    for (int b = 0; b < G.nblk; b++)
        if (mv[b].mode != 0 || b % G.nbh >= ex0 || b / G.nbh >= ey0) out[n++] = first + b;
    return n;
}

// The plan of one call.  force32: the repeat of a flagged call, everything on int32 coefficients; profiled: the kernel timing hooks are
// on; draw_mode: dsvg_ctx_draw_info's.  Returns DSVG_OK, or the code of the first failed check with its text in P.err -- the call's
// arguments, then the planes of all jobs in device order, then the jobs in device order.  Reads the caller's arrays and the first
// bytes of every payload; writes P alone.
static inline int plan_decode(const DecGeo &G, const DecSwitches &sw, int njobs, const dsvg_dec_job *jobs, bool force32, bool profiled, int draw_mode,
                              DecPlan &P)
{
    P.err[0] = 0;
    if (!jobs || njobs < 1 || njobs > G.max_jobs) { snprintf(P.err, sizeof P.err, "bad decode_pictures arguments"); return DSVG_ERR_ARG; }
    // device order: intra jobs first, then inter jobs (kernels are specialised per type)
    P.njobs = njobs;
    P.job.resize((size_t)njobs);
    int nI = 0;
    for (int i = 0; i < njobs; i++) if (jobs[i].ref_recon_slot < 0) P.job[(size_t)nI++].src = i;
    P.nI = nI;
    for (int i = 0, n = nI; i < njobs; i++) if (jobs[i].ref_recon_slot >= 0) P.job[(size_t)n++].src = i;
    // the payloads of the call travel as one blob, each plane with 64 guard bytes behind it, 16-aligned; per 128-bit payload chunk one
    // hand-over record between the parse kernels
    size_t off = 0, moff = 0;
    for (int t = 0; t < njobs; t++) {
        DecPlanJob &o = P.job[(size_t)t];
        const dsvg_dec_job &j = jobs[o.src];
        for (int p = 0; p < 3; p++) {
            // the reference's bound (dsv_decoder.c:397-398: twice the int32 coefficient plane), not the encoder's output capacity
            if (!j.plane_data[p] || (size_t)j.plane_len[p] > (size_t)G.cw[p] * G.ch[p] * 8) {
                snprintf(P.err, sizeof P.err, "plane %d of decode job %d: bad length", p, o.src); return DSVG_ERR_ARG;
            }
            o.boff[p] = off; o.moff[p] = moff;
            off += ((size_t)j.plane_len[p] + 64 + 15) & ~(size_t)15;
            moff += (size_t)j.plane_len[p] / 16 + 2;
        }
    }
    P.blob = off; P.nmeta = moff;
    const bool sparse = !sw.no_dec_sym && !force32;
    // I pictures: symbols into the zero-kept planes as well -- the encoder's I-picture inverse (k_inv_haar_tile<.,1,true>, k_inv_b4t<true>)
    // dequantises them in 32 bits; needs both plane kinds on the symbol path (the I kernels take luma and chroma alike)
    const bool sparseI = sparse && G.sym_ok[0] && G.sym_ok[1] && !sw.no_dec_sym_I;
    P.max_entries = 0; P.max_chunks = 0;
    for (int t = 0; t < njobs; t++) {
        DecPlanJob &o = P.job[(size_t)t];
        const dsvg_dec_job &j = jobs[o.src];
        const int isP = j.ref_recon_slot >= 0;
        if (j.recon_slot < 0 || j.recon_slot >= G.n_recon || j.ref_recon_slot >= G.n_recon || !j.stable_blocks || (isP && !j.mvs)) {
            snprintf(P.err, sizeof P.err, "bad decode job %d", o.src); return DSVG_ERR_ARG;
        }
        o.isP = isP;
        // Sparse decode of P pictures: the detail entries go to the zero-kept int16 symbol planes and the fused inverse of the encoder
        // reconstructs from them (no 12 MB of int32 coefficients to clear and to read per picture); a plane whose scan regions share
        // cells takes it too: k_hz_dec_resolve flags the rare picture in which an absent later symbol must leave the earlier region's
        // VALUE in place (hzcc.c:295-435), and that call is decoded again from int32 coefficients (dec_resolve)
        o.path = isP ? (sparse ? DEC_PATH_SYM_P : DEC_PATH_I32) : (sparseI ? DEC_PATH_SYM_I : DEC_PATH_I32);
        for (int p = 0; p < 3; p++) o.dec_sym[p] = o.path == DEC_PATH_SYM_I ? 1 : (o.path == DEC_PATH_SYM_P ? G.sym_ok[p < 1 ? 0 : 1] : 0);
        o.wide = o.path == DEC_PATH_SYM_I;
        o.inplace = o.path == DEC_PATH_SYM_P && j.recon_slot != j.ref_recon_slot && !sw.no_inplace_pred;     // (ping-pong slots)
        for (int p = 0; p < 3; p++) {
            // the host reads only the plane header (hzcc.c:479-483,307-311): SEG(DC), the 32-bit run count; the
            // code chain is parsed on the device (k_hz_parse) from the uploaded bytes
            Rd rd{j.plane_data[p], 0, (unsigned)j.plane_len[p] * 8u};
            o.dc[p] = rd.seg();
            rd.align();
            o.runs[p] = (int)rd.bits(32);
            rd.align();
            o.bitpos[p] = (long long)rd.pos;
            o.len[p] = (int)j.plane_len[p];
            P.max_entries = std::max(P.max_entries, std::min(o.runs[p], G.nchunks[p] * HZ_CHUNK - 1) + 1);
            P.max_chunks = std::max(P.max_chunks, (int)(j.plane_len[p] / 16 + 2));
        }
    }
    const bool symI = sparseI && nI > 0;             // the call's I pictures are on the symbol path
    P.insym = !sparse ? 0 : (symI ? 1 : 0) | (G.sym_ok[0] ? 2 : 0) | (G.sym_ok[1] ? 4 : 0);
    P.f0 = symI ? 0 : nI;
    P.anysym = ((P.insym & 6) && njobs > nI) || symI;
    P.scatter_one = (P.insym & 6) == 6 && (nI == 0 || symI);
    P.resolve = P.anysym && ((G.ov[0] && G.sym_ok[0]) || (G.ov[1] && G.sym_ok[1]));
    // (a call of one picture gains nothing from the fork: 3 110-3 230 against 3 160-3 340 frames/s)
    P.fork = njobs > nI && njobs >= 4 && !sw.one_stream && !profiled && G.second_stream;
    P.mc = njobs > nI ? (G.mc_patch && !sw.no_mc_patch ? DEC_MC_PATCH : DEC_MC_PLAIN) : DEC_MC_NONE;
    P.ex0 = G.nbh; P.ey0 = G.nbv;
    if (P.mc == DEC_MC_PATCH)
        for (int p = 0; p < 3; p++) {
            const int bw = G.blk_w >> (p ? G.hs : 0), bh = G.blk_h >> (p ? G.vs : 0);
            if (G.pw[p] & 7) P.ex0 = std::min(P.ex0, (G.pw[p] & ~7) / bw);
            if (G.ph[p] & 7) P.ey0 = std::min(P.ey0, (G.ph[p] & ~7) / bh);
        }
    P.draw0 = P.draw1 = njobs;
    if (draw_mode && njobs > nI) P.draw0 = nI;       // the call's P pictures
    return DSVG_OK;
}

#endif
