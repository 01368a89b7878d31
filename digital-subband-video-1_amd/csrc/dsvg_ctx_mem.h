// dsvg_ctx_mem.h -- every buffer a context (dsvg_ctx, dsvg_pipe.hip) owns, and its size: plain C++17 without a HIP include, a context
// or an allocation, so that a stand-alone program can compile it (tools/ctx_mem_host.cpp) and the device-free query dsvg_ctx_mem_plan
// can answer for any geometry.  plan_ctx_mem lists the buffers dsvg_ctx_create_blk allocates, in the order it allocates them;
// ctx_mem_grow gives the capacity of a buffer that is allocated on first use.  The context's one allocator (ctx_alloc / ctx_release /
// ctx_grow in dsvg_pipe.hip) allocates from these answers and keeps a record per id, which ctx_free releases.
// Not in here: the upscale tables of the source-resolution quality (XresGeo, owned by k_quality.hip: xres_geo_build / xres_geo_free)
// and of the output scale (ScaleGeo, k_scale.hip: scale_geo_build / scale_geo_free); memory a caller owns (dsvg_dev_alloc,
// dsvg_host_alloc); the one-shot lanes.
#ifndef DSVG_CTX_MEM_H
#define DSVG_CTX_MEM_H

#include <stddef.h>
#include <algorithm>
#include "../../include/dsvg.h"

#ifndef HZ_CHUNK
#define HZ_CHUNK 2048        // (dsvg_dev.hpp has it for the kernels' side)
#endif
#define CTX_MEM_GUARD ((size_t)256 * 1024)    // == GUARD_BYTES (dsvg_host.hpp): zeroed, in front of and behind a slab

// X(id, name, field of dsvg_ctx): the creation-time buffers in the order of their allocation, then the lazy ones.
// Of src0 .. src5 a context has levels + 1; ilist_h / ilist_d exist where motion compensation is fused into the forward transform.
#define DSVG_CTX_MEM_SLABS(X) \
    X(SRC0, "src0", src[0]) X(SRC1, "src1", src[1]) X(SRC2, "src2", src[2]) X(SRC3, "src3", src[3]) X(SRC4, "src4", src[4]) X(SRC5, "src5", src[5]) \
    X(RECON, "recon", recon) X(XF, "xf", xf) X(PRED, "pred", pred)
#define DSVG_CTX_MEM_CREATE(X) DSVG_CTX_MEM_SLABS(X) DSVG_CTX_MEM_BUFS(X)
#define DSVG_CTX_MEM_BUFS(X) \
    X(COEF, "coef", coef) X(S3, "s3", s3) X(S1, "s1", s1) X(S5, "s5", s5) X(NZPOS, "nzpos", nzpos) X(NZVAL, "nzval", nzval) X(CHUNKS, "chunks", chunks) \
    X(SYM, "sym", sym) X(NZF, "nzf", nzf) X(SYMP, "symP", symP) X(PFLAG, "pflag", pflag) X(CFLAG, "cflag", cflag) X(LLSYM, "llsym", llsym) \
    X(STAT, "stat", stat) X(PSUM, "psum", psum) X(BITS, "bits", bits) X(MVS, "mvs", mvs) X(STABLE, "stable", stable) X(JOBS_D, "jobs_d", jobs_d) \
    X(RC_STATE_D, "rc_state_d", rc_state_d) X(RCJ_D, "rcj_d", rcj_d) X(RCJ_H, "rcj_h", rcj_h) X(MVF, "mvf", mvf) X(AUX_TEX, "aux_tex", aux_tex) \
    X(AUX_VAR, "aux_var", aux_var) X(CSUM, "csum", csum) X(SLOTS_D, "slots_d", slots_d) X(LUMA_SUMS, "luma_sums", luma_sums) X(JOBS_H, "jobs_h", jobs_h) \
    X(GTAB_D, "gtab_d", gtab_d) X(GTAB_H, "gtab_h", gtab_h) X(PSUM_H, "psum_h", psum_h) X(MV_H, "mv_h", mv_h) X(STABLE_H, "stable_h", stable_h) \
    X(SLOTS_H, "slots_h", slots_h) X(LUMA_H, "luma_h", luma_h) X(ASLOTS_H, "aslots_h", aslots_h) X(AMV_H, "amv_h", amv_h) \
    X(ILIST_H, "ilist_h", ilist_h) X(ILIST_D, "ilist_d", ilist_d) \
    X(SLOT_CU_H, "slot_cu_h", slot_cu_h) X(SLOT_CV_H, "slot_cv_h", slot_cv_h) X(SLOT_CS_H, "slot_cs_h", slot_cs_h) \
    X(SLOT_CU_D, "slot_cu_d", slot_cu_d) X(SLOT_CV_D, "slot_cv_d", slot_cv_d) X(SLOT_CS_D, "slot_cs_d", slot_cs_d) \
    X(SLOT_Y_H, "slot_y_h", slot_y_h) X(SLOT_Y_D, "slot_y_d", slot_y_d)
#define DSVG_CTX_MEM_LAZY(X) \
    X(LTAB_D, "ltab_d", ltab_d) X(YUV_STAGE, "yuv_stage", yuv_stage) X(INGEST0, "ingest0", ingest[0]) X(INGEST1, "ingest1", ingest[1]) \
    X(GATH_D, "gath_d", gath_d) X(GATH_H, "gath_h", gath_h) \
    X(Q_DEV0, "q0_dev", q[0].dev) X(Q_DEV1, "q1_dev", q[1].dev) X(Q_DEV2, "q2_dev", q[2].dev) X(Q_DEV3, "q3_dev", q[3].dev) \
    X(Q_HOST0, "q0_host", q[0].host) X(Q_HOST1, "q1_host", q[1].host) X(Q_HOST2, "q2_host", q[2].host) X(Q_HOST3, "q3_host", q[3].host) \
    X(XREF_D, "xref_d", xref_d) X(XREF_H, "xref_h", xref_h) X(OTAB_D, "otab_d", otab_d) X(OSC_SCRATCH, "osc_scratch", osc_scratch) X(OSC_TAB_D, "osc_tab_d", osc_tab_d) \
    X(DEC_H0, "dec_h0", dec_h[0]) X(DEC_H1, "dec_h1", dec_h[1]) X(DEC_D0, "dec_d0", dec_d[0]) X(DEC_D1, "dec_d1", dec_d[1]) X(DEC_META, "dec_meta", dec_meta) \
    X(DEC_FLAG_D, "dec_flag_d", dec_flag_d) X(DEC_FLAG_H, "dec_flag_h", dec_flag_h) X(DRAW_SCRATCH, "draw_scratch", draw_scratch)
enum CtxMemId {
#define X(id, name, field) CM_##id,
    DSVG_CTX_MEM_CREATE(X) DSVG_CTX_MEM_LAZY(X)
#undef X
    CM_N,
    CM_N_CREATE = CM_LTAB_D        // the first lazy id: the creation-time ids lie below it
};
static_assert(CM_N == DSVG_CTX_MEM_IDS, "include/dsvg.h states the number of ids");
inline const char *ctx_mem_name(int id)
{
    static const char *const names[CM_N] = {
#define X(id, name, field) name,
        DSVG_CTX_MEM_CREATE(X) DSVG_CTX_MEM_LAZY(X)
#undef X
    };
    return id >= 0 && id < CM_N ? names[id] : "?";
}

// what the sizes read of a context, as plain integers (ctx_mem_geo in dsvg_pipe.hip fills it, for a context and for the query alike)
struct CtxMemGeo {
    int levels;                                   // pyramid levels below level 0
    size_t pitch[6];                              // FrameLayout.pitch of each level
    size_t total, s3total, s1total, s5total;      // CoefLayout: ints per job
    size_t ll[3];                                 // w3 * h3 of each plane
    size_t nz_total, bits_per_job;                // CtxScan
    int chunks_per_job, nblk;
    int n_src, n_recon, max_jobs, out_slots, nwin, rc_slots, mc_fused;      // out_slots: at least max_jobs (batch_geo)
    size_t sz_chunk_sum, sz_plane_sum, sz_mv, sz_job, sz_rc_job, sz_rc_state, sz_parse_chunk;   // sizeof the device structs
};

// per-plane scan bookkeeping of a job: where a plane's symbols, chunk summaries, packed payload and LL symbols lie in the job's share
struct CtxScan {
    size_t nz_off[3] = {0, 0, 0}, nz_total = 0;
    int chunk_off[3] = {0, 0, 0}, chunks_per_job = 0, max_chunks = 0;
    size_t bits_off[3] = {0, 0, 0}, bits_cap[3] = {0, 0, 0}, bits_per_job = 0;
    int ll_off[3] = {0, 0, 0};
    size_t ll_total = 0;
};
// nchunks: scan chunks of each plane (make_hz_plane); cw, ch: the coefficient planes; ll: w3 * h3
inline void ctx_scan_layout(CtxScan &S, const int nchunks[3], const int cw[3], const int ch[3], const size_t ll[3])
{
    S = CtxScan();
    size_t nzo = 0, bo = 0, lo = 0; int cho = 0;
    for (int p = 0; p < 3; p++) {
        S.nz_off[p] = nzo; nzo += (size_t)nchunks[p] * HZ_CHUNK;
        S.chunk_off[p] = cho; cho += nchunks[p];
        S.max_chunks = std::max(S.max_chunks, nchunks[p]);
        S.bits_cap[p] = ((size_t)cw[p] * ch[p] * 2 + 255) & ~(size_t)255;    // 16 bits/coefficient bound
        S.bits_off[p] = bo; bo += S.bits_cap[p] + 256;
        S.ll_off[p] = (int)lo; lo += (ll[p] + 7) & ~(size_t)7;               // each plane's share padded to 8 entries (16-byte reads in k_hz_collect*)
    }
    S.nz_total = nzo; S.chunks_per_job = cho; S.bits_per_job = bo; S.ll_total = lo;
}

// pad: bytes behind the elements; 0 = the kind's own (a slab's slack and two guards, 256 device, 64 pinned)
static inline void ctx_mem_row(dsvg_ctx_mem_row *&r, int id, int kind, size_t count, size_t size, int zeroed, size_t pad = 0)
{
    if (!pad) pad = kind == DSVG_MEM_SLAB ? 4096 + 2 * CTX_MEM_GUARD : (kind == DSVG_MEM_PINNED ? 64 : 256);
    *r++ = dsvg_ctx_mem_row{id, kind, zeroed, count, size, pad, count * size + pad};
}
// The creation-time buffers in the order of their allocation: rows[CM_N_CREATE] at most, returns their number; totals (may be null):
// [DSVG_MEM_DEVICE] device bytes, slabs among them, [DSVG_MEM_PINNED] pinned host bytes.
inline int plan_ctx_mem(const CtxMemGeo &g, dsvg_ctx_mem_row *rows, size_t totals[2])
{
    enum { D = DSVG_MEM_DEVICE, H = DSVG_MEM_PINNED };
    dsvg_ctx_mem_row *r = rows;
    const size_t J = (size_t)g.max_jobs, O = (size_t)g.out_slots, S = J * (size_t)g.nwin, SO = std::max(S, O), ns = (size_t)g.n_src, nblk = (size_t)g.nblk;
    const size_t ll_total = ((g.ll[0] + 7) & ~(size_t)7) + ((g.ll[1] + 7) & ~(size_t)7) + ((g.ll[2] + 7) & ~(size_t)7);
    for (int l = 0; l <= g.levels; l++) ctx_mem_row(r, CM_SRC0 + l, DSVG_MEM_SLAB, ns, g.pitch[l], 1);
    ctx_mem_row(r, CM_RECON, DSVG_MEM_SLAB, (size_t)g.n_recon, g.pitch[0], 1);
    ctx_mem_row(r, CM_XF, DSVG_MEM_SLAB, J, g.pitch[0], 1);
    ctx_mem_row(r, CM_PRED, DSVG_MEM_SLAB, J, g.pitch[0], 1);
    ctx_mem_row(r, CM_COEF, D, g.total * J, 4, 1);
    ctx_mem_row(r, CM_S3, D, g.s3total * J, 4, 1);
    ctx_mem_row(r, CM_S1, D, g.s1total * J, 4, 1);
    ctx_mem_row(r, CM_S5, D, g.s5total * J, 4, 1);
    ctx_mem_row(r, CM_NZPOS, D, g.nz_total * J, 4, 0);
    ctx_mem_row(r, CM_NZVAL, D, g.nz_total * J, 4, 0);
    ctx_mem_row(r, CM_CHUNKS, D, (size_t)g.chunks_per_job * J, g.sz_chunk_sum, 1);
    ctx_mem_row(r, CM_SYM, D, g.nz_total * J, 2, 1);
    // (one set of symbol / flag planes per work job; round 3's deferred entropy stage kept one per frame step: a measured dead end)
    ctx_mem_row(r, CM_NZF, D, (g.nz_total >> 2) * J, 1, 1);
    ctx_mem_row(r, CM_SYMP, D, g.nz_total * J, 2, 1);
    ctx_mem_row(r, CM_PFLAG, D, g.s3total * J, 1, 1);
    ctx_mem_row(r, CM_CFLAG, D, (size_t)g.chunks_per_job * J, 1, 1);
    ctx_mem_row(r, CM_LLSYM, D, ll_total * J, 4, 1);
    ctx_mem_row(r, CM_STAT, D, 8 * 64, 4, 1);
    ctx_mem_row(r, CM_PSUM, D, 3 * O, g.sz_plane_sum, 1);
    ctx_mem_row(r, CM_BITS, D, g.bits_per_job * O, 1, 1);
    ctx_mem_row(r, CM_MVS, D, nblk * O, g.sz_mv, 1);
    ctx_mem_row(r, CM_STABLE, D, nblk * O, 1, 1);
    ctx_mem_row(r, CM_JOBS_D, D, O, g.sz_job, 1);
    ctx_mem_row(r, CM_RC_STATE_D, D, (size_t)g.rc_slots, g.sz_rc_state, 1);
    ctx_mem_row(r, CM_RCJ_D, D, O, g.sz_rc_job, 1);
    ctx_mem_row(r, CM_RCJ_H, H, SO, g.sz_rc_job, 1);
    ctx_mem_row(r, CM_MVF, D, (size_t)(g.levels + 1) * nblk * O, g.sz_mv, 1);
    ctx_mem_row(r, CM_AUX_TEX, D, nblk * O, 4, 1);
    ctx_mem_row(r, CM_AUX_VAR, D, nblk * O, 4, 1);
    ctx_mem_row(r, CM_CSUM, D, nblk * 4 * ns, 4, 1);
    ctx_mem_row(r, CM_SLOTS_D, D, 3 * O, 4, 1);
    ctx_mem_row(r, CM_LUMA_SUMS, D, ns, 4, 1);
    ctx_mem_row(r, CM_JOBS_H, H, SO, g.sz_job, 1);
    ctx_mem_row(r, CM_GTAB_D, D, 9 * O, 8, 1);
    ctx_mem_row(r, CM_GTAB_H, H, 9 * O, 8, 1);
    ctx_mem_row(r, CM_PSUM_H, H, 3 * O, g.sz_plane_sum, 1);
    ctx_mem_row(r, CM_MV_H, H, nblk * SO, g.sz_mv, 1);
    ctx_mem_row(r, CM_STABLE_H, H, nblk * SO, 1, 1);
    ctx_mem_row(r, CM_SLOTS_H, H, 3 * SO, 4, 1);
    ctx_mem_row(r, CM_LUMA_H, H, ns, 4, 1);
    ctx_mem_row(r, CM_ASLOTS_H, H, 2 * O, 4, 1);
    ctx_mem_row(r, CM_AMV_H, H, nblk * O, g.sz_mv, 1);
    if (g.mc_fused) {
        ctx_mem_row(r, CM_ILIST_H, H, nblk * SO, 4, 1);
        ctx_mem_row(r, CM_ILIST_D, D, nblk * SO, 4, 0);
    }
    // the source slots' plane tables (the chroma ones are filled whole right away): 64 bytes behind each, the device ones too
    ctx_mem_row(r, CM_SLOT_CU_H, H, ns, 8, 0);
    ctx_mem_row(r, CM_SLOT_CV_H, H, ns, 8, 0);
    ctx_mem_row(r, CM_SLOT_CS_H, H, ns, 4, 0);
    ctx_mem_row(r, CM_SLOT_CU_D, D, ns, 8, 0, 64);
    ctx_mem_row(r, CM_SLOT_CV_D, D, ns, 8, 0, 64);
    ctx_mem_row(r, CM_SLOT_CS_D, D, ns, 4, 0, 64);
    ctx_mem_row(r, CM_SLOT_Y_H, H, ns, 8, 1);
    ctx_mem_row(r, CM_SLOT_Y_D, D, ns, 8, 1, 64);
    if (totals) {
        totals[0] = totals[1] = 0;
        for (const dsvg_ctx_mem_row *q = rows; q < r; q++) totals[q->kind == DSVG_MEM_PINNED ? 1 : 0] += q->bytes;
    }
    return (int)(r - rows);
}

// A lazy buffer: elements of `size` bytes, `pad` bytes behind them; `sync`: the streams that may still read a buffer being replaced
// (CTX_SYNC_*: ctx_grow waits for them before it frees one); fixed: its capacity is a function of the geometry, allocated once.
enum { CTX_SYNC_ST = 1, CTX_SYNC_ST_A = 2, CTX_SYNC_ST_L = 4, CTX_SYNC_ST_H = 8 };
struct CtxMemLazy { int kind; size_t size, pad; int zeroed, sync; };
inline CtxMemLazy ctx_mem_lazy(int id, const CtxMemGeo &g)
{
    enum { D = DSVG_MEM_DEVICE, H = DSVG_MEM_PINNED };
    switch (id) {
    case CM_LTAB_D: case CM_OTAB_D: case CM_OSC_TAB_D: return {D, 4, 64, 0, 0};
    // (the stage serves the host-input load on the load stream, dsvg_download_recon on the coding stream and the host output pass)
    case CM_YUV_STAGE: return {D, 1, 256, 0, CTX_SYNC_ST | CTX_SYNC_ST_A | CTX_SYNC_ST_L};
    case CM_INGEST0: case CM_INGEST1: return {D, 1, 256, 0, CTX_SYNC_ST_H | CTX_SYNC_ST_A | CTX_SYNC_ST_L};
    case CM_GATH_D: return {D, 1, 0, 0, 0};              // (a fetch has synchronised its stream before it asks)
    case CM_GATH_H: return {H, 1, 0, 0, 0};
    case CM_Q_DEV0: case CM_Q_DEV1: case CM_Q_DEV2: case CM_Q_DEV3: return {D, 8, 256, 0, 0};
    case CM_Q_HOST0: case CM_Q_HOST1: case CM_Q_HOST2: case CM_Q_HOST3: return {H, 8, 64, 1, 0};
    case CM_XREF_D: return {D, 8, 256, 1, 0};
    case CM_XREF_H: return {H, 8, 64, 1, 0};
    case CM_OSC_SCRATCH: case CM_DRAW_SCRATCH: return {D, 1, 256, 0, 0};
    case CM_DEC_H0: case CM_DEC_H1: return {H, 1, 0, 0, 0};          // (the call has waited for the parity's uploads)
    case CM_DEC_D0: case CM_DEC_D1: return {D, 1, 256, 0, CTX_SYNC_ST};
    case CM_DEC_META: return {D, g.sz_parse_chunk, 0, 0, CTX_SYNC_ST};
    case CM_DEC_FLAG_D: return {D, 4, 0, 0, 0};
    case CM_DEC_FLAG_H: return {H, 4, 0, 0, 0};
    }
    return {D, 0, 0, 0, 0};
}
// The capacity, in elements, of lazy buffer `id` that holds `cap` elements and is asked for `need`: cap where that is enough, else each
// site's own rule.  few: the fetch of a few pictures in one round trip (gath_d / gath_h), which asks for 12 x 64 KB + 64.
inline size_t ctx_mem_grow(int id, const CtxMemGeo &g, size_t need, size_t cap, bool few = false)
{
    if (need <= cap) return cap;
    size_t n = need;
    switch (id) {
    case CM_LTAB_D: n = (size_t)g.n_src; break;
    case CM_GATH_D: case CM_GATH_H: n = few ? (size_t)1 << 20 : (need - std::min(need, (size_t)64)) * 2 + ((size_t)1 << 20); break;   // need = the payloads + 64
    case CM_Q_DEV0: case CM_Q_DEV1: case CM_Q_DEV2: case CM_Q_DEV3:
    case CM_Q_HOST0: case CM_Q_HOST1: case CM_Q_HOST2: case CM_Q_HOST3: n = 3 * (size_t)g.out_slots; break;
    case CM_XREF_D: case CM_XREF_H: n = (size_t)g.out_slots; break;
    case CM_OTAB_D: case CM_OSC_TAB_D: n = 2 * (size_t)g.n_recon; break;
    case CM_DEC_H0: case CM_DEC_H1: case CM_DEC_D0: case CM_DEC_D1: n = need * 2 + ((size_t)1 << 20); break;
    case CM_DEC_META: n = need * 2 + 4096; break;
    case CM_DEC_FLAG_D: case CM_DEC_FLAG_H: n = 2 * (size_t)g.max_jobs; break;
    case CM_DRAW_SCRATCH: n = g.pitch[0] * (size_t)g.max_jobs; break;
    default: break;                                       // yuv_stage, ingest, osc_scratch: what is asked for
    }
    return std::max(n, need);
}
inline size_t ctx_mem_lazy_bytes(int id, const CtxMemGeo &g, size_t cap) { const CtxMemLazy z = ctx_mem_lazy(id, g); return cap * z.size + z.pad; }

#endif
