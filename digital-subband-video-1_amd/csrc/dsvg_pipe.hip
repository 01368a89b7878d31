// dsvg_pipe.hip -- PIPELINE-LEVEL C ABI: device-resident frames, batched over picture jobs.
//
// Everything a GOP batch needs stays in HBM: source frames (bordered reference layout) with their
// luma pyramids, reconstructions, and per-job work buffers (residual/prediction frames, coefficient
// planes, LL scratch, non-zero lists, packed payloads).  One call enqueues the whole per-picture
// kernel chain for njobs pictures on one HIP stream; nothing synchronises until the caller fetches
// results.  The host only ever sees: MV fields, mean luma, per-plane (DC, nruns, payload bytes).
#include <stdlib.h>
#include <algorithm>
#include <cstddef>
#include "dsvg_host.hpp"
#include "dsvg_batch_plan.h"
#include "dsvg_dec_plan.h"
#include "dsvg_fetch_plan.h"
#include "dsvg_load_plan.h"
#include "dsvg_ctx_mem.h"
#include <atomic>
#include <ctime>
extern "C" void dsv1_par_for(int S, void (*fn)(void *ctx, int s, int tid), void *ctx);     // host/dsv1_util.c: the worker pool
extern "C" void dsv1_par_for_long(int S, void (*fn)(void *ctx, int s, int tid), void *ctx);

#define OPCHK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// ---- stream placement ------------------------------------------------------------------------------------------
// The runtime maps HIP streams onto a handful of hardware queues (4 by default), least-loaded first, counting every
// stream the process has -- the framework's, the communication library's.  Two of OUR busy streams on one queue run
// one after the other (measured: -15 % with one unrelated extra stream in the process, none with two).  So the streams
// are not taken as they come: candidates are created and probed pairwise with a 100 us spin kernel each -- both done
// after ~100 us means different queues -- and a set of mutually concurrent ones is kept.
__global__ void k_spin(long long ticks)
{
    const long long t0 = wall_clock64();                   // constant 100 MHz counter
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
static bool streams_concurrent(hipStream_t a, hipStream_t b, hipEvent_t e0, hipEvent_t ea, hipEvent_t eb)
{
    const long long T = 10000;                             // 100 us
    if (hipEventRecord(e0, a) != hipSuccess || hipStreamWaitEvent(b, e0, 0) != hipSuccess) return true;
    hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, a, T);
    hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, b, T);
    (void)hipEventRecord(ea, a); (void)hipEventRecord(eb, b);
    (void)hipEventSynchronize(ea); (void)hipEventSynchronize(eb);
    float ta = 0, tb = 0;
    if (hipEventElapsedTime(&ta, e0, ea) != hipSuccess || hipEventElapsedTime(&tb, e0, eb) != hipSuccess) return true;
    return std::max(ta, tb) < 0.165f;                      // serialised: the later one ends after >= 200 us
}
// `want` streams that run concurrently with each other (as many as can be found among 12 candidates; the rest in
// creation order); returns the number of mutually concurrent ones at the front of out[]
// copy_out (round 5): a stream for the host-to-device copies of a host-fed context -- its FIFTH busy stream, and the runtime has four hardware
// queues by default (GPU_MAX_HW_QUEUES).  Created lazily it landed wherever the runtime put it: behind a coding stream's kernels a batch's 12 GB
// upload (210 ms) and the coding phase (25 ms) took turns -- 236 ms per step, profiles/r05_hostpin_timeline.txt -- elsewhere they did not, and
// which it was changed from run to run (value_host_pinned 0.81 / 0.95 / 0.95 of the link in three runs of one tree).  Now it is probed like the
// others: a queue of its own where the runtime has one left, else one that shares the ANALYSIS stream's queue and no other of ours (the upload in
// front of the same batch's load and motion search: they wait for it anyway).  210 ms per step = the link's rate, three runs of three, with four
// queues and with eight.
// *copy_shared: 0 = own queue, 2 / 3 = own queue as a stream of the lowest / highest priority, 1 = shares the analysis stream's, -1 = no such
// candidate (the caller creates a stream the plain way).
static int pick_streams(hipStream_t *out, int want, hipStream_t *copy_out = nullptr, int *copy_shared = nullptr)
{
    const int NC = 12;
    hipStream_t cand[NC] = {};
    int nc = 0;
    for (; nc < NC; nc++) if (hipStreamCreateWithFlags(&cand[nc], hipStreamNonBlocking) != hipSuccess) break;
    if (nc < want) { for (int i = 0; i < nc; i++) (void)hipStreamDestroy(cand[i]); return -1; }
    hipEvent_t e0 = nullptr, ea = nullptr, eb = nullptr;
    bool probe = !getenv("DSV1_NO_STREAM_PROBE") && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&ea) == hipSuccess && hipEventCreate(&eb) == hipSuccess;
    bool used[NC] = {};
    int n = 0;
    if (probe) {
        (void)streams_concurrent(cand[0], cand[1], e0, ea, eb);          // first launch of the kernel: code load, not timed
        for (int i = 0; i < nc && n < want; i++) {
            bool ok = true;
            for (int k = 0; k < n && ok; k++) ok = streams_concurrent(out[k], cand[i], e0, ea, eb);
            if (ok) { out[n++] = cand[i]; used[i] = true; }
        }
    }
    const int good = n;
    for (int i = 0; i < nc && n < want; i++) if (!used[i]) { out[n++] = cand[i]; used[i] = true; }
    if (copy_out) {
        *copy_out = nullptr;
        if (copy_shared) *copy_shared = -1;
        if (probe && good == want && want >= 2) {
            int with_analysis = -1;
            for (int i = 0; i < nc && !*copy_out; i++) {
                if (used[i]) continue;
                bool all = true, others = true;          // concurrent with every picked stream / with every one but the analysis stream (out[1])
                for (int k = 0; k < want && others; k++) {
                    const bool cc = streams_concurrent(out[k], cand[i], e0, ea, eb);
                    all = all && cc;
                    if (k != 1) others = others && cc;
                }
                if (all) { *copy_out = cand[i]; used[i] = true; if (copy_shared) *copy_shared = 0; }
                else if (others && with_analysis < 0) with_analysis = i;
            }
            if (!*copy_out && !getenv("DSV1_NO_PRIO_COPY_STREAM")) {
                // none left among the plain streams (four hardware queues, all taken): the runtime keeps the queues of the other stream
                // PRIORITIES apart from those -- a stream of the lowest, else the highest priority is probed the same way (a copy engine does
                // not care about the priority of the queue that feeds it)
                int lo = 0, hi = 0;
                if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) {
                    const int prios[2] = {lo, hi};
                    for (int t = 0; t < 2 && !*copy_out; t++) {
                        hipStream_t ps_ = nullptr;
                        if (hipStreamCreateWithPriority(&ps_, hipStreamNonBlocking, prios[t]) != hipSuccess) { (void)hipGetLastError(); continue; }
                        bool all = true;
                        for (int k = 0; k < want && all; k++) all = streams_concurrent(out[k], ps_, e0, ea, eb);
                        if (all) { *copy_out = ps_; if (copy_shared) *copy_shared = 2 + t; }
                        else (void)hipStreamDestroy(ps_);
                    }
                } else (void)hipGetLastError();
            }
            if (!*copy_out && with_analysis >= 0) { *copy_out = cand[with_analysis]; used[with_analysis] = true; if (copy_shared) *copy_shared = 1; }
        }
    }
    for (int i = 0; i < nc; i++) if (!used[i]) (void)hipStreamDestroy(cand[i]);
    if (e0) (void)hipEventDestroy(e0);
    if (ea) (void)hipEventDestroy(ea);
    if (eb) (void)hipEventDestroy(eb);
    return good;
}

struct dsvg_ctx {
    int device = 0;
    hipStream_t st = nullptr;        // residual-coding stream
    hipEvent_t ev_a = nullptr;       // analysis -> coding dependency
    hipStream_t st_c = nullptr;      // fetch stream (gather + D2H of finished pictures)
    std::vector<hipEvent_t> ev_coded;  // ring: completion of each dsvg_code_pictures call
    std::vector<int> slot_ev;          // out slot -> index into ev_coded of the call that produces it
    long ncalls = 0;
    hipStream_t stx[DSVG_MAX_CODE_STREAMS] = {};   // further coding streams (a share of the pictures of every frame step each), created on first use
    hipEvent_t ev_fork = nullptr, ev_join[DSVG_MAX_CODE_STREAMS] = {};
    int code_streams = 1;
    int copy_queue = -1;             // the copy stream's hardware queue: 0 its own, 1 the analysis stream's, -1 wherever the runtime put it (pick_streams)
    int streams_apart = 0;           // how many of {coding, analysis, second coding, fetch} were found on hardware queues of their own
    hipStream_t st_a = nullptr;      // analysis stream (frame load, pyramid, HME): overlaps coding of the previous batch
    hipStream_t st_l = nullptr;      // frame-load stream: st_a itself unless DSV1_CU_LOAD gives the streaming load kernels a CU-masked stream of their own
    hipEvent_t ev_l = nullptr;       // load -> analysis / coding dependency when st_l is a stream of its own
    // DSV1_TIMELINE=1: a batch-level timeline without a profiler in the way (rocprofv3 makes every launch cost the host ~70 us, which
    // serialises a pipeline whose point is that the host runs ahead): timing events on the pipeline's own streams at the boundaries of
    // load / motion search / coding / fetch plus the host clock at the moment each was enqueued; printed by dsvg_ctx_sync / destroy
    struct TlMark { const char *what; hipEvent_t ev; double host_ms; };
    std::vector<TlMark> tl;
    bool tl_on = false;
    unsigned long long border_bytes = 0;   // dsvg_ctx_tile_stats2 out[7]
    bool tl_quiet = false;           // switched on through dsvg_ctx_timeline (the marks are read with dsvg_ctx_timeline_get, nothing is printed)
    double fetch_acc[4] = {0, 0, 0, 0};   // dsvg_fetch_pictures_cb, per call: host ms waiting for the coding, for the sizes, for gather + copy + the caller's pieces; bytes copied
    long fetch_n = 0;
    hipEvent_t ev_mark[2] = {nullptr, nullptr};     // dsvg_ctx_mark
    int w = 0, h = 0, fmt = 0, bw = 0, bh = 0, nbh = 0, nbv = 0, nblk = 0, levels = 0;
    FrameLayout L[6];
    HmeArgs hme;                     // the motion search's arguments, geometry half (make_hme_geo)
    CoefLayout CL;
    SbtGeo3 G;
    McGeo MG;
    bool mc_fused = false;           // P pictures: motion compensation inside the forward transform (k_fwd_mc_pix)
    bool no_inplace_pred = false;    // DSV1_NO_INPLACE_PRED: always keep the prediction in its own frame (A/B switch)
    int n_src = 0, n_recon = 0, max_jobs = 0, out_slots = 0, nwin = 0, win = 0, calls_since_sync = 0;
    Slab src[6], recon, xf, pred;
    int32_t *coef = nullptr, *s3 = nullptr, *s1 = nullptr, *s5 = nullptr, *nzpos = nullptr, *nzval = nullptr;
    HzChunkSum *chunks = nullptr;
    uint8_t *nzf = nullptr;          // per work job: flag byte per 4 scan positions (non-zero symbols of P pictures)
    int16_t *sym = nullptr;          // fused quantiser: per work job, scan-order symbol planes (same indexing as nzpos)
    std::vector<hipEvent_t> ev_fetch;   // one per piece of a chunked fetch (dsvg_fetch_pictures_cb)
    std::vector<short> slot_ext;     // per reconstruction slot: the border extents its last encoder job wrote (dsvg_recon_border)
    bool no_lazy_border = false;     // DSV1_NO_LAZY_BORDER=1: every reconstruction gets its whole border (A/B)
    bool no_list_pack = false;       // DSV1_NO_LIST_PACK=1: a wave per chunk for sparse pictures too (A/B)
    int32_t *llsym = nullptr;        // per work job: LL-region symbols of the encoder (JobDev.llsym)
    bool llq = true;                 // the LL quantiser runs inside k_fwd_haar_mid<4> / k_tail_q (DSV1_NO_LLQ=1: k_hz_quant<true>, A/B)
    int16_t *symP = nullptr;         // the same for P pictures: kept ZERO between pictures (sparse stores, k_hz_collect clears)
    uint8_t *pflag = nullptr;        // per work job: flag byte per 8x8-pixel patch and plane (indexed like s3)
    uint8_t *cflag = nullptr;        // per work job: flag byte per scan chunk (indexed like chunks)
    unsigned *stat = nullptr;        // [4][64] inverse-transform tile counters (general luma / chroma, zero luma / chroma), sharded
    bool stats_on = false;
    bool no_patch_kernel = false;    // DSV1_NO_PATCH_KERNEL: chroma of P pictures stays on the tile kernel (A/B switch)
    bool no_dec_sym_I = false;       // DSV1_NO_DEC_SYM_I: the decoder's I pictures keep int32 coefficients (A/B switch)
    bool no_dec_sym = false;         // DSV1_NO_DEC_SYM: the decoder keeps int32 coefficients for P pictures too (A/B switch)
    HzPlaneSum *psum = nullptr;
    uint8_t *bits = nullptr;
    DMV *mvs = nullptr;
    uint8_t *stable = nullptr;
    JobDev *jobs_d = nullptr, *jobs_h = nullptr;
    std::vector<char> slot_isP;      // per out slot: the picture coded into it last was a P picture (dsvg_fetch_pictures' fast path)
    // quality measurements (k_quality.hip), one record per kind: DSVG_Q_SSE / DSVG_Q_SSIM of the pictures as coded (dsvg_ctx_sse_enable,
    // dsvg_ctx_ssim_enable), DSVG_Q_XSSE / DSVG_Q_XSSIM of the reconstruction upscaled to the reference geometry (dsvg_ctx_xres_enable).
    // Per out slot the three planes' sums -- squared errors, or SSIM's fixed-point window sums (int64 as two's complement) -- and
    // whether the picture coded into the slot last was measured.  Allocated when the kind is first switched on.
    struct Quality {
        bool on = false;
        unsigned long long *dev = nullptr, *host = nullptr;  // [out_slots][3] device / pinned host
        std::vector<char> measured;                          // [out_slots], sized with the tables
    } q[DSVG_Q_KINDS];
    // source-resolution quality: the reference geometry's upscale tables, per out slot the reference frame the next call measures
    // against (xref_next, set by dsvg_ctx_xres_refs and consumed by the call that codes the slot; its pinned staging and device
    // copy xref_h / xref_d)
    XresGeo xg;
    const uint8_t **xref_d = nullptr, **xref_h = nullptr;
    std::vector<const uint8_t *> xref_next;
    // device-resident rate control (dsvg_code_batch_rc): per-stream state, per-job tables (indexed like jobs_h / jobs_d)
    dsvg_rc_state *rc_state_d = nullptr;
    RcJobDev *rcj_d = nullptr, *rcj_h = nullptr;
    int rc_slots = 0;
    // coding calls (dsvg_batch_plan.h): what their plan reads of the context (batch_geo, at creation), and the plan of the call being
    // enqueued -- kept here so that its vectors are allocated once, not per call
    BatchGeo bgeo = {};
    BatchPlan plan;
    // memory (dsvg_ctx_mem.h): what the sizes read of the context, and per buffer id what the context holds -- the allocation, its capacity in
    // elements (lazy buffers) and its bytes.  The typed fields below are copies of mem[].p (ctx_fields).
    CtxMemGeo mgeo = {};
    CtxScan scan;                    // per-plane scan bookkeeping of a job: nz_off .. ll_total
    struct Mem { void *p; size_t cap, bytes; int kind; } mem[CM_N] = {};
    // motion estimation
    DMV *mvf = nullptr;
    unsigned *aux_tex = nullptr;
    unsigned *csum = nullptr;        // [n_src][nblk][4] chroma block sums of every source slot (k_hme_csum)
    int *aux_var = nullptr;
    int *slots_d = nullptr;          // [3 * max_jobs]: cur, ref, recon tables
    unsigned *luma_sums = nullptr;   // [n_src]
    // host pinned staging
    HzPlaneSum *psum_h = nullptr;
    DMV *mv_h = nullptr;
    uint8_t *stable_h = nullptr;
    int *slots_h = nullptr;
    int *aslots_h = nullptr;         // analysis-stream staging (pair tables)
    DMV *amv_h = nullptr;            // analysis-stream staging (motion fields)
    unsigned *luma_h = nullptr;
    uint8_t *dec_h[2] = {nullptr, nullptr}, *dec_d[2] = {nullptr, nullptr};   // decoder: payload blob of one call (pinned / device), by call parity
    hipEvent_t ev_dec[2] = {nullptr, nullptr};   // uploads of the call that last used that parity
    hipEvent_t ev_pack[2] = {nullptr, nullptr};  // decoder, round 5: the packing pass runs on the second coding stream ([0]: the reconstructions are there, [1]: the pass is done)
    bool pack_pending = false;                   // ... and the first stream has not yet been told to wait for it
    hipEvent_t ev_user = nullptr;                // dsvg_ctx_join: a caller's stream ordered behind the first coding stream
    // Chroma planes of every source slot: the bordered copy in the source slab, or -- frames loaded "in place"
    // (dsvg_load_frames_map_ex) -- the caller's packed planar clip: pixel (0,0) of U / V and the row stride, host truth + the
    // device tables the motion search reads (HmeArgs.slot_cu ..)
    std::vector<const uint8_t *> slot_cu, slot_cv;
    std::vector<int> slot_cs;
    unsigned long long *slot_cu_h = nullptr, *slot_cv_h = nullptr, *slot_cu_d = nullptr, *slot_cv_d = nullptr;
    // (round 5) luma in place: per source slot the frame's luma plane in the caller's clip or null (HmeArgs.slot_y, JobDev.srcp[0]); of such a
    // frame's bordered copy k_unpack writes a ring only (ring_x16 x 16 columns, ring_y4 x 4 rows in from each edge)
    std::vector<const uint8_t *> slot_y;
    unsigned long long *slot_y_h = nullptr, *slot_y_d = nullptr;
    bool ydirect_ok = false;
    int deep_r = 0, ring_x16 = 0, ring_y4 = 0;
    long ydirect_frames = 0;
    int *slot_cs_h = nullptr, *slot_cs_d = nullptr;
    bool cdirect_ok = false;         // the geometry allows in-place chroma (even chroma planes, rows of whole 8-byte patches)
    LoadGeo lgeo = {};               // what the plan of a source load reads of the context (dsvg_load_plan.h)
    long cdirect_frames = 0;         // frames loaded that way (tests)
    int dec_par = 0;
    // Decoder, sparse symbol path: a call is enqueued optimistically; its scatter stage flags pictures the int16 symbol planes
    // cannot represent exactly (JobDev.dec_flag).  The flags come back asynchronously and are looked at when the next decoder
    // call starts or a result is read (dec_resolve): a flagged call is decoded again on the int32 coefficient path, and a
    // device-side pack of its pictures that was already enqueued is repeated.
    int *dec_flag_d = nullptr, *dec_flag_h = nullptr;    // [2][max_jobs]
    hipEvent_t ev_flag[2] = {nullptr, nullptr};
    struct DecPending {
        bool active = false, in_redo = false;
        int parity = 0, njobs = 0;
        std::vector<dsvg_dec_job> jobs;                  // the call's jobs in device order, pointing into the parity's pinned staging
        // the one output pass recorded (output_pass; none: no slots): slots, frame indices (empty: identity), destination, format
        std::vector<int> slots, index; void *out = nullptr; size_t pitch = 0;
        bool has_fmt = false; dsvg_pixout fmt;
    } dec_pending;
    // decoder calls (dsvg_dec_plan.h): what their plan reads of the context (dec_geo, at creation), and the plan of the call being
    // enqueued -- kept here so that its vector is allocated once, not per call
    DecGeo dgeo = {};
    DecPlan dec_plan;
    long dec_redone = 0;                // calls decoded again on the int32 path (tests)
    HzParseChunk *dec_meta = nullptr;            // decoder: k_hz_parse -> k_hz_codes records of one call
    uint8_t *yuv_stage = nullptr;    // device staging for host-resident input frames
    int *ltab_d = nullptr;           // slot table of dsvg_load_frames_map
    int *otab_d = nullptr;           // table of the output pass: slots (k_pack_n) or (slot, output frame) pairs (k_pixout)
    // Decoder, debug overlay (dsvg_ctx_draw_info, k_drawinfo.hip): with a mode set, every P picture of a decoder call is copied behind its
    // reconstruction into a scratch frame -- one per job of a call, allocated when the first such picture arrives -- and drawn on there;
    // the reconstruction slots, which later pictures predict from, stay clean.  draw_at[slot]: the scratch frame that stands in for the
    // slot in the output pass and the downloads until the next decoder call, or -1.  Mode 0: nothing of this exists or runs.
    int draw_mode = 0;
    uint8_t *draw_scratch = nullptr;
    std::vector<int> draw_at;
    bool draw_any = false;
    // Decoder, output scale (dsvg_ctx_output_scale, k_scale_slots): with a size set, the output pass resamples every picture it hands out
    // to osc_w x osc_h at the context's subsampling -- straight into the destination for packed planar output, into osc_scratch (packed
    // planar frames osc_fb apart, one per reconstruction slot, allocated by the first pass that needs it) in front of a format.
    // osc_tab_d: that format pass's (scratch frame, output frame) pairs.  Off: nothing of this exists or runs.
    bool osc_on = false;
    int osc_w = 0, osc_h = 0, osc_filter = -1;
    ScaleGeo osc;
    uint8_t *osc_scratch = nullptr;
    size_t osc_fb = 0;
    int *osc_tab_d = nullptr;
    int *ilist_h = nullptr, *ilist_d = nullptr;   // intra blocks of the P pictures of a batch (pinned / device), indexed like jobs_h
    // host-resident input: two device ingest buffers filled on a copy stream of their own, so the upload of the
    // next batch runs under the analysis and coding of the current one
    hipStream_t st_h = nullptr;
    uint8_t *ingest[2] = {nullptr, nullptr};
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_used[2] = {nullptr, nullptr};
    bool up_pending[2] = {false, false}, used_valid[2] = {false, false};
    int ingest_next = 0;
    unsigned long long *gtab_d = nullptr, *gtab_h = nullptr;   // gather table (3 words per plane payload)
    uint8_t *gath_d = nullptr, *gath_h = nullptr;              // compacted payloads (device / pinned host)
    Prof prof;
};

static int dec_resolve(dsvg_ctx *c);     // decoder: settle the flags of the last call (defined with dsvg_decode_pictures)

// DSV1_DEBUG_LINK_REPEAT=n (diagnostic, round 6): every large host <-> device copy of the batched pipeline (the packet fetch, the motion fields down, the
// job / flag / vector tables up) is issued n times -- the same bytes arrive, the link carries n times the traffic: how a box whose link runs at 1/n of the
// usual rate would time a step (bench.py's `step_breakdown` on the driver's slow box of round 5 read 25-29 GB/s against 57)
static int link_repeat() { static const int n = [] { const char *e = getenv("DSV1_DEBUG_LINK_REPEAT"); const int v = e ? atoi(e) : 1; return v < 1 ? 1 : (v > 16 ? 16 : v); }(); return n; }
static double tl_now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
static void tl_mark(dsvg_ctx *c, hipStream_t st, const char *what)
{
    if (!c->tl_on || c->tl.size() >= 16384) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    c->tl.push_back({what, e, tl_now()});
}
// (call with the streams idle: after the syncs of dsvg_ctx_sync / before the context goes)
static void tl_dump(dsvg_ctx *c)
{
    if (!c->tl_on || c->tl.empty()) return;
    fprintf(stderr, "[dsvg timeline] %zu marks; columns: device ms (event time), host ms (when it was enqueued), both from the first mark\n", c->tl.size());
    for (size_t i = 0; i < c->tl.size(); i++) {
        float ms = -1.f;
        if (c->tl[i].ev && c->tl[0].ev) {
            (void)hipEventSynchronize(c->tl[i].ev);
            if (hipEventElapsedTime(&ms, c->tl[0].ev, c->tl[i].ev) != hipSuccess) { (void)hipGetLastError(); ms = -1.f; }
        }
        fprintf(stderr, "[dsvg timeline] %-10s dev %9.3f  host %9.3f\n", c->tl[i].what, ms, c->tl[i].host_ms - c->tl[0].host_ms);
    }
    for (auto &m : c->tl) if (m.ev) (void)hipEventDestroy(m.ev);
    c->tl.clear();
}

static void tl_clear(dsvg_ctx *c)
{
    for (auto &m : c->tl) if (m.ev) (void)hipEventDestroy(m.ev);
    c->tl.clear();
}

// The marks of the pipeline's own streams (load / motion search / table uploads / coding on both streams / fetch) as an API (verdict round 5: the
// bench line could not say where a step's time goes on the box it ran on): dsvg_ctx_timeline(ctx, 1) starts collecting (a timing event per mark:
// ten per batch), dsvg_ctx_timeline_get sums them up.  Call the latter with the context synchronised.
extern "C" int dsvg_ctx_timeline(dsvg_ctx *c, int on)
{
    if (!c) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    tl_clear(c);
    c->tl_on = on != 0;
    c->tl_quiet = on != 0;
    return DSVG_OK;
}
// out[0] = coding phases seen, [1] = device ms from the first mark to the last, then device ms summed over the phases: [2] clip upload, [3] frame load +
// pyramid, [4] motion search, [5] table uploads of the coding calls, [6] coding on the first stream, [7] on the second, [8] fetch (gather + copies),
// [9] = device ms during which NONE of load / search / tables / coding was in flight (the chip waiting for the host), [10] = the same between
// the first coding phase's start and the last one's end only, [11] = ms during which a coding phase and a load / search phase overlapped.
extern "C" int dsvg_ctx_timeline_get(dsvg_ctx *c, double out[12])
{
    if (!c || !out) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    for (int i = 0; i < 12; i++) out[i] = 0.0;
    if (c->tl.empty() || !c->tl[0].ev) return DSVG_OK;
    struct Iv { double a, b; int kind; };
    std::vector<Iv> iv;
    std::vector<double> dev(c->tl.size(), -1.0);
    for (size_t i = 0; i < c->tl.size(); i++) {
        float ms = -1.f;
        if (c->tl[i].ev) {
            HIPCHK(hipEventSynchronize(c->tl[i].ev));
            if (hipEventElapsedTime(&ms, c->tl[0].ev, c->tl[i].ev) != hipSuccess) { (void)hipGetLastError(); ms = -1.f; }
        }
        dev[i] = ms;
    }
    static const struct { const char *a, *b; int kind; } ph[] = {{"up0", "up1", 2}, {"load0", "load1", 3}, {"hme0", "hme1", 4}, {"tab0", "code0", 5},
                                                                 {"code0", "code1", 6}, {"code0", "code1b", 7}, {"fetch0", "fetch1", 8}};
    double last = 0.0;
    for (const auto &q : ph) {
        double start = -1.0;
        for (size_t i = 0; i < c->tl.size(); i++) {
            if (dev[i] < 0) continue;
            last = std::max(last, dev[i]);
            if (!strcmp(c->tl[i].what, q.a)) start = dev[i];
            else if (!strcmp(c->tl[i].what, q.b) && start >= 0) {
                iv.push_back({start, dev[i], q.kind});
                out[q.kind] += dev[i] - start;
                if (q.kind == 6) out[0] += 1.0;
                start = -1.0;
            }
        }
    }
    out[1] = last;
    // union of the compute phases
    std::vector<Iv> cu;
    for (const auto &v : iv) if (v.kind >= 3 && v.kind <= 7) cu.push_back(v);
    std::sort(cu.begin(), cu.end(), [](const Iv &x, const Iv &y) { return x.a < y.a; });
    double c0 = 1e300, c1 = -1.0;
    for (const auto &v : iv) if (v.kind == 6 || v.kind == 7) { c0 = std::min(c0, v.a); c1 = std::max(c1, v.b); }
    double busy = 0.0, busy_in = 0.0, end = -1.0;
    for (const auto &v : cu) {
        const double a = std::max(v.a, end), b = v.b;
        if (b > a) {
            busy += b - a;
            const double ia = std::max(a, c0), ib = std::min(b, c1);
            if (ib > ia) busy_in += ib - ia;
            end = b;
        }
    }
    out[9] = last - busy;
    out[10] = c1 > c0 ? (c1 - c0) - busy_in : 0.0;
    for (const auto &x : iv)
        if (x.kind == 6)
            for (const auto &y : iv)
                if (y.kind == 3 || y.kind == 4) out[11] += std::max(0.0, std::min(x.b, y.b) - std::max(x.a, y.a));
    return DSVG_OK;
}
// the host's side of dsvg_fetch_pictures_cb since the last reset, per call: out[0] = ms waiting for the coding calls that produce the slots, [1] = ms for the
// plane summaries (one small device-to-host round trip), [2] = ms for gather table + gather kernel + the copy in pieces + the caller's work on the
// pieces, [3] = bytes copied, [4] = calls
extern "C" int dsvg_ctx_fetch_prof(dsvg_ctx *c, double out[5], int reset)
{
    if (!c || !out) return DSVG_ERR_ARG;
    const double n = c->fetch_n ? (double)c->fetch_n : 1.0;
    for (int i = 0; i < 4; i++) out[i] = c->fetch_acc[i] / n;
    out[4] = (double)c->fetch_n;
    if (reset) { for (double &v : c->fetch_acc) v = 0.0; c->fetch_n = 0; }
    return DSVG_OK;
}

// ---- the context's memory: one allocator, one owner ---------------------------------------------------------------------------------
// Every buffer of a context is allocated by ctx_alloc and freed by ctx_release, which keep the record dsvg_ctx::mem[id] and the process's
// totals; sizes come from dsvg_ctx_mem.h.  hipMalloc / hipHostMalloc / hipFree / hipHostFree appear in this file in this pair alone (and
// in dsvg_dev_alloc .. dsvg_host_free_on, whose memory the caller owns); slabs go through Slab::alloc / release (dsvg_common.hip).
static std::atomic<long long> g_mem_out[2];       // [DSVG_MEM_DEVICE] (slabs among them), [DSVG_MEM_PINNED]
static std::atomic<int> g_fail_at{0};             // dsvg_debug_fail_alloc_at: allocations to go until one fails
static int ctx_alloc(dsvg_ctx *c, int id, int kind, size_t bytes, bool zero)
{
    dsvg_ctx::Mem &m = c->mem[id];
    const int t = kind == DSVG_MEM_PINNED ? 1 : 0;
    void *p = nullptr;
    int rc = DSVG_OK;
    if (g_fail_at.load() > 0 && g_fail_at.fetch_sub(1) == 1) { dsvg_set_error("%s (%zu bytes): out of memory", ctx_mem_name(id), bytes); return DSVG_ERR_HIP; }
    if (kind == DSVG_MEM_SLAB) {
        Slab s;
        if ((rc = s.alloc(bytes - 2 * GUARD_BYTES))) { const std::string why = dsvg_last_error(); dsvg_set_error("%s (%zu bytes): %s", ctx_mem_name(id), bytes, why.c_str()); }
        p = s.raw;                                   // (zeroed, and the device synchronised behind it)
    } else {
        const hipError_t e = t ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e != hipSuccess) { dsvg_set_error("%s (%zu bytes): %s", ctx_mem_name(id), bytes, hipGetErrorString(e)); return DSVG_ERR_HIP; }
    }
    if (!p) return rc;
    m = {p, 0, bytes, kind};
    g_mem_out[t] += (long long)bytes;
    if (zero && kind == DSVG_MEM_PINNED) memset(p, 0, bytes);
    if (zero && kind == DSVG_MEM_DEVICE) HIPCHK(hipMemset(p, 0, bytes));
    return rc;
}
static void ctx_release(dsvg_ctx *c, int id)
{
    dsvg_ctx::Mem &m = c->mem[id];
    if (!m.p) return;
    if (m.kind == DSVG_MEM_SLAB) { Slab s; s.raw = (uint8_t *)m.p; s.release(); }
    else if (m.kind == DSVG_MEM_PINNED) (void)hipHostFree(m.p);
    else (void)hipFree(m.p);
    g_mem_out[m.kind == DSVG_MEM_PINNED ? 1 : 0] -= (long long)m.bytes;
    m = {};
}
// the typed fields, from the records
static void ctx_fields(dsvg_ctx *c)
{
#define X(id, name, field) { const dsvg_ctx::Mem &m = c->mem[CM_##id]; c->field.raw = (uint8_t *)m.p; c->field.p = m.p ? c->field.raw + GUARD_BYTES : nullptr; c->field.bytes = m.p ? m.bytes - 2 * GUARD_BYTES : 0; }
    DSVG_CTX_MEM_SLABS(X)
#undef X
#define X(id, name, field) c->field = (decltype(c->field))c->mem[CM_##id].p;
    DSVG_CTX_MEM_BUFS(X) DSVG_CTX_MEM_LAZY(X)
#undef X
}
static_assert(GUARD_BYTES == CTX_MEM_GUARD && DSVG_Q_KINDS == 4, "dsvg_ctx_mem.h restates both");
// A buffer allocated on first use: at least `need` elements of buffer `id` (ctx_mem_grow: the new capacity; ctx_mem_lazy: the element,
// the pad and the streams that may still read a buffer being replaced).  *grew: a new buffer was allocated.
static int ctx_grow(dsvg_ctx *c, int id, size_t need, bool few = false, bool *grew = nullptr)
{
    dsvg_ctx::Mem &m = c->mem[id];
    if (grew) *grew = false;
    if (need <= m.cap) return DSVG_OK;            // (nothing asked for, nothing allocated)
    const size_t cap = ctx_mem_grow(id, c->mgeo, need, m.cap, few);
    const CtxMemLazy z = ctx_mem_lazy(id, c->mgeo);
    if (m.p) {
        if ((z.sync & CTX_SYNC_ST_H) && c->st_h) HIPCHK(hipStreamSynchronize(c->st_h));
        if (z.sync & CTX_SYNC_ST) HIPCHK(hipStreamSynchronize(c->st));
        if (z.sync & CTX_SYNC_ST_A) HIPCHK(hipStreamSynchronize(c->st_a));
        if (z.sync & CTX_SYNC_ST_L) HIPCHK(hipStreamSynchronize(c->st_l));
        ctx_release(c, id);
    }
    const int rc = ctx_alloc(c, id, z.kind, cap * z.size + z.pad, z.zeroed != 0);
    if (!rc) m.cap = cap;
    if (grew) *grew = !rc;
    ctx_fields(c);
    return rc;
}
extern "C" void dsvg_debug_fail_alloc_at(int n) { g_fail_at.store(n > 0 ? n : 0); }
extern "C" void dsvg_mem_outstanding(size_t out[2]) { for (int t = 0; t < 2; t++) out[t] = (size_t)g_mem_out[t].load(); }
extern "C" const char *dsvg_ctx_mem_name(int id) { return ctx_mem_name(id); }
extern "C" int dsvg_ctx_mem_live(const dsvg_ctx *c, size_t *bytes_by_id, int n)
{
    if (!c || !bytes_by_id || n < 0 || n > CM_N) { dsvg_set_error("bad ctx_mem_live arguments"); return DSVG_ERR_ARG; }
    for (int i = 0; i < n; i++) bytes_by_id[i] = c->mem[i].bytes;
    return DSVG_OK;
}

static void ctx_free(dsvg_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->tl_on && !c->tl_quiet) { (void)hipDeviceSynchronize(); tl_dump(c); }
    tl_clear(c);
    for (int id = 0; id < CM_N; id++) ctx_release(c, id);
    xres_geo_free(c->xg);
    scale_geo_free(c->osc);
    if (c->st) (void)hipStreamDestroy(c->st);
    for (int i = 0; i < 2; i++) if (c->ev_mark[i]) (void)hipEventDestroy(c->ev_mark[i]);
    if (c->st_l && c->st_l != c->st_a) (void)hipStreamDestroy(c->st_l);
    if (c->ev_l) (void)hipEventDestroy(c->ev_l);
    if (c->st_a) (void)hipStreamDestroy(c->st_a);
    for (int g = 0; g < DSVG_MAX_CODE_STREAMS; g++) {
        if (c->stx[g]) (void)hipStreamDestroy(c->stx[g]);
        if (c->ev_join[g]) (void)hipEventDestroy(c->ev_join[g]);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    for (hipEvent_t e : c->ev_fetch) (void)hipEventDestroy(e);
    if (c->ev_a) (void)hipEventDestroy(c->ev_a);
    if (c->st_c) (void)hipStreamDestroy(c->st_c);
    if (c->st_h) (void)hipStreamDestroy(c->st_h);
    for (int i = 0; i < 2; i++) {
        if (c->ev_up[i]) (void)hipEventDestroy(c->ev_up[i]);
        if (c->ev_used[i]) (void)hipEventDestroy(c->ev_used[i]);
        if (c->ev_dec[i]) (void)hipEventDestroy(c->ev_dec[i]);
        if (c->ev_pack[i]) (void)hipEventDestroy(c->ev_pack[i]);
        if (c->ev_flag[i]) (void)hipEventDestroy(c->ev_flag[i]);
    }
    for (hipEvent_t e : c->ev_coded) (void)hipEventDestroy(e);
    if (c->ev_user) (void)hipEventDestroy(c->ev_user);
    delete c;
}

// The geometry tables of a context as functions of the picture alone: block geometry (blk_w = 0: the encoder's own block size), frame and
// coefficient layout, the transform's plane geometry with l1a, the motion compensation's.  dsvg_ctx_create_blk builds them here, and so
// do the device-free queries below (dsvg_geom_check, dsvg_dispatch_plan, dsvg_inv_plan): what they say is said of a context's tables.
struct CtxGeo {
    int bw, bh, nbh, nbv;
    FrameLayout L;
    CoefLayout CL;
    SbtGeo3 G;
    McGeo MG;
};
static void make_ctx_geo(CtxGeo &o, int width, int height, int subsamp, int blk_w = 0, int blk_h = 0)
{
    block_geometry(width, height, &o.bw, &o.bh, &o.nbh, &o.nbv);
    if (blk_w) {                                            // a decoder: the block size its stream announces
        o.bw = blk_w; o.bh = blk_h;
        o.nbh = (width + blk_w - 1) / blk_w; o.nbv = (height + blk_h - 1) / blk_h;
    }
    make_frame_layout(o.L, subsamp, width, height);
    make_coef_layout(o.CL, subsamp, width, height);
    const FrameLayout &L = o.L;
    const CoefLayout &CL = o.CL;
    McGeo &MG = o.MG;
    memset(&MG, 0, sizeof(MG));
    MG.blk_w = o.bw; MG.blk_h = o.bh; MG.nbh = o.nbh; MG.nbv = o.nbv; MG.hs = L.hs; MG.vs = L.vs;
    for (int p = 0; p < 3; p++) {
        make_sbt_geo(o.G.g[p], CL.w[p], CL.h[p], L.w[p], L.h[p], L.stride[p], L.off[p], CL.off[p], CL.s3off[p], CL.s1off[p], CL.s5off[p]);
        HzPlane hp0;
        make_hz_plane(hp0, CL.w[p], CL.h[p], 100, 1, p, o.nbh, o.nbv);
        o.G.g[p].l1a = ((hp0.r[7].sw | hp0.r[7].base | hp0.r[8].base | hp0.r[9].base) & 3) == 0;
        MG.w[p] = L.w[p]; MG.h[p] = L.h[p]; MG.stride[p] = L.stride[p]; MG.off[p] = L.off[p];
        MG.cw_extra[p] = CL.w[p] > L.w[p];
    }
}

// The geometry half of the motion search's arguments -- all that hme_plan reads -- of a context of these tables: the pyramid's depth
// (pyramid_levels = 0: the encoder's own) and its levels' layouts.  The context keeps it (dsvg_ctx.hme: dsvg_analyse adds the pointers);
// dsvg_dispatch_plan and dsvg_hme_plan ask the plan about the same record.
static void make_hme_geo(HmeArgs &A, const CtxGeo &geo, int width, int height, int subsamp, int pyramid_levels = 0)
{
    memset(&A, 0, sizeof(A));
    A.levels = pyramid_levels > 0 ? std::min(pyramid_levels, DSVG_MAX_PYRAMID) : auto_pyramid_levels(width, height, geo.nbh, geo.nbv);
    A.L[0] = geo.L;
    for (int l = 1; l <= A.levels; l++) make_frame_layout(A.L[l], subsamp, rsu(width, l), rsu(height, l));
    A.nxb = geo.nbh; A.nyb = geo.nbv; A.nblk = geo.nbh * geo.nbv; A.blk_w = geo.bw; A.blk_h = geo.bh;
}
// how the encoder's frame step calls the forward transform of a plane group: quantised, levels 4..5 and the tail launched once per step
static const FwdOpts FWD_FRAME_STEP = { /* quantise */ true, /* llq */ false, /* own_mid4 */ false, /* own_tail */ false };

// What dsvg_ctx_create (encoder block size) answers for a geometry, without a device: the resolution ladder refuses a geometry before
// it allocates anything (dsv1_resladder_open).  The same checks, in the same order, as the context creation below.
// (geo_supported: the checks of the tables themselves, which creation and dsvg_ctx_mem_plan make of a decoder's block size too)
static int geo_supported(const CtxGeo &geo, int width, int height)
{
    const CoefLayout &CL = geo.CL;
    for (int p = 0; p < 3; p++)
        if (!sbt_tail_supported(geo.G.g[p])) { dsvg_set_error("plane %dx%d: LL5 band does not fit the LDS tail kernel", CL.w[p], CL.h[p]); return DSVG_ERR_UNSUPPORTED; }
    if ((width | height) & 1) { dsvg_set_error("odd luma dimensions are not supported (intra B4T needs even planes)"); return DSVG_ERR_UNSUPPORTED; }
    for (int p = 0; p < 3; p++) {
        HzPlane hp; make_hz_plane(hp, CL.w[p], CL.h[p], 100, 0, p, geo.nbh, geo.nbv);
        if (hp.nchunks > hz_scan_items_max()) { dsvg_set_error("plane too large for the scan kernel"); return DSVG_ERR_UNSUPPORTED; }
    }
    return DSVG_OK;
}
static int geom_check(int width, int height, int subsamp, CtxGeo &geo)
{
    if (width < 32 || height < 32) { dsvg_set_error("bad ctx_create arguments"); return DSVG_ERR_ARG; }
    if (subsamp != 0x0 && subsamp != 0x4 && subsamp != 0x5 && subsamp != 0x8) { dsvg_set_error("bad subsampling"); return DSVG_ERR_ARG; }
    make_ctx_geo(geo, width, height, subsamp);
    return geo_supported(geo, width, height);
}
extern "C" int dsvg_geom_check(int width, int height, int subsamp)
{
    CtxGeo geo;
    return geom_check(width, height, subsamp, geo);
}

// What the plan of a coding call reads of a context (dsvg_batch_plan.h), from the arguments of its creation: dsvg_ctx_create_blk takes
// out_slots, rc_slots, mc_fused and the lazy border from here, and dsvg_code_batch_plan asks the plan about the same record without a
// context.  code_streams is the call's own (dsvg_ctx_code_streams may change it from call to call).
static BatchGeo batch_geo(const CtxGeo &geo, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots, bool mc_fusion, bool lazy_border)
{
    BatchGeo B = {};
    B.nblk = geo.nbh * geo.nbv; B.n_recon = n_recon_slots; B.n_src = n_src_slots; B.max_jobs = max_jobs;
    B.out_slots = std::max(out_slots, max_jobs);
    B.rc_slots = std::max(n_recon_slots, max_jobs);
    B.mc_fused = mc_fusable(geo.MG) && mc_fusion;
    B.lazy_border = lazy_border;
    B.blk_w = geo.MG.blk_w; B.blk_h = geo.MG.blk_h; B.nbh = geo.MG.nbh; B.hs = geo.MG.hs; B.vs = geo.MG.vs;
    for (int pl = 0; pl < 2; pl++) { B.w[pl] = geo.MG.w[pl]; B.h[pl] = geo.MG.h[pl]; }
    return B;
}

// What the plan of a decoder call reads of a context (dsvg_dec_plan.h), from the arguments of its creation: dsvg_ctx_create_blk keeps it, and
// dsvg_decode_plan asks the plan about the same record without a context.  second_stream is the call's own (a coding call may create
// the stream later).
static DecGeo dec_geo(const CtxGeo &geo, int n_recon_slots, int max_jobs, bool mc_fusion, bool sym_ov)
{
    DecGeo D = {};
    const CoefLayout &CL = geo.CL;
    D.n_recon = n_recon_slots; D.max_jobs = max_jobs; D.nblk = geo.nbh * geo.nbv;
    for (int p = 0; p < 3; p++) {
        HzPlane hp; make_hz_plane(hp, CL.w[p], CL.h[p], 100, 0, p, geo.nbh, geo.nbv);
        D.cw[p] = CL.w[p]; D.ch[p] = CL.h[p]; D.nchunks[p] = hp.nchunks;
        D.pw[p] = geo.MG.w[p]; D.ph[p] = geo.MG.h[p];
    }
    for (int g2 = 0; g2 < 2; g2++) {
        HzPlane hp; make_hz_plane(hp, CL.w[g2 ? 1 : 0], CL.h[g2 ? 1 : 0], 100, 1, g2, geo.nbh, geo.nbv);
        const bool ov = (2 * hp.s_w[0] > hp.s_w[1]) || (2 * hp.s_h[0] > hp.s_h[1]) || (2 * hp.s_w[1] > hp.s_w[2]) || (2 * hp.s_h[1] > hp.s_h[2]);
        // (the fused inverse from symbol planes also wants the level-1 bands 4-aligned and the plane's LL5 path as usual)
        D.sym_ok[g2] = (CL.off[g2 ? 1 : 0] & 3) == 0 && (CL.off[2] & 3) == 0 && !(ov && !sym_ov);
        D.ov[g2] = ov;
    }
    D.mc_patch = mc_fusable(geo.MG) && mc_fusion;          // (such a context has an intra list)
    D.nbh = geo.MG.nbh; D.nbv = geo.MG.nbv; D.blk_w = geo.MG.blk_w; D.blk_h = geo.MG.blk_h; D.hs = geo.MG.hs; D.vs = geo.MG.vs;
    return D;
}

// What the plan of a source load reads of a context (dsvg_load_plan.h), from the layouts of its pyramid (make_hme_geo) and its block
// size: dsvg_ctx_create_blk keeps it, and dsvg_load_plan asks the plan about the same record without a context.  slabs: the source
// slabs of levels 0 .. levels, or null: bases as Slab::alloc gives them (multiples of 16).
static LoadGeo load_geo(const HmeArgs &A, const Slab *slabs)
{
    LoadGeo G = {};
    G.levels = A.levels;
    for (int l = 0; l <= A.levels; l++) {
        const FrameLayout &L = A.L[l];
        G.w[l] = L.w[0]; G.h[l] = L.h[0];
        bool ok = (L.pitch % 16) == 0 && (!slabs || ((uintptr_t)slabs[l].p % 16) == 0);
        for (int c = 0; c < (l ? 1 : 3); c++) ok = ok && (L.stride[c] % 16) == 0 && (L.off[c] % 16) == 0;
        G.lay16[l] = ok;
    }
    const FrameLayout &L0 = A.L[0], &LT = A.L[A.levels];
    G.cw = L0.w[1]; G.ch = L0.h[1];
    G.c_alike = L0.w[1] == L0.w[2] && L0.h[1] == L0.h[2] && L0.stride[1] == L0.stride[2];
    G.l2_dword = A.levels >= 2 && (A.L[2].stride[0] & 3) == 0 && (A.L[2].off[0] & 3) == 0 && (A.L[2].pitch & 3) == 0;
    G.sum_dword = (LT.stride[0] & 3) == 0 && (LT.off[0] & 3) == 0 && (LT.pitch & 3) == 0 && (!slabs || ((uintptr_t)slabs[A.levels].p & 3) == 0);
    const int deep_r = hme_deep_r(A.levels);
    G.ring_x16 = hme_ring_x16(A.blk_w, deep_r);
    G.ring_y4 = hme_ring_y4(A.blk_h, deep_r);
    return G;
}
// The A/B switches of the source load: the process's own, read once -- this sits on the enqueue path.  plan_load itself takes them as
// an argument, so a caller can ask it about any setting.
static const LoadSwitches &load_switches()
{
    static const LoadSwitches sw = { getenv("DSV1_NO_UNPACK_SIDES") != nullptr, getenv("DSV1_NO_LEVEL_SIDES") != nullptr,
                                     getenv("DSV1_NO_FUSE_LEVEL2") != nullptr };
    return sw;
}
static_assert(KID_UNPACK == LOAD_K_UNPACK && KID_EXTEND == LOAD_K_EXTEND && KID_EXTEND16 == LOAD_K_EXTEND16 && KID_DS2X == LOAD_K_DS2X &&
              KID_LUMA_SUM == LOAD_K_LUMA_SUM, "dsvg_load_plan's kernel order is the profiler's");

// The plan of a source load of n frames in a context of this geometry (include/dsvg.h): plan_load, which load_core launches from, on the
// geometry tables of dsvg_ctx_create, with the switches the caller names instead of the environment's
extern "C" int dsvg_load_plan(int width, int height, int subsamp, int pyramid_levels, int with_pyramid, int src_mod16, int pitch_mod16, unsigned switches,
                              int n, int n_chroma_in_place, int n_luma_in_place, dsvg_load_plan_out *out)
{
    if (!out || n < 1 || pyramid_levels < 0 || src_mod16 < 0 || src_mod16 > 15 || pitch_mod16 < 0 || pitch_mod16 > 15 || n_chroma_in_place < 0 || n_chroma_in_place > n || n_luma_in_place < 0 || n_luma_in_place > n_chroma_in_place) {
        dsvg_set_error("bad load_plan arguments"); return DSVG_ERR_ARG;
    }
    CtxGeo geo;
    const int rc = geom_check(width, height, subsamp, geo);
    if (rc) return rc;
    HmeArgs A;
    make_hme_geo(A, geo, width, height, subsamp, pyramid_levels);
    const LoadSwitches sw = { (switches & DSVG_LOAD_NO_UNPACK_SIDES) != 0, (switches & DSVG_LOAD_NO_LEVEL_SIDES) != 0, (switches & DSVG_LOAD_NO_FUSE_LEVEL2) != 0 };
    plan_load(load_geo(A, nullptr), sw, with_pyramid != 0, src_mod16, pitch_mod16, n, n_chroma_in_place, n_luma_in_place, *out);
    return DSVG_OK;
}

// What the forward launchers decide for an encoder context of this geometry (default block size and pyramid depth, the chroma
// table of the motion search on): the context's geometry tables, handed to the launchers' own decision functions
extern "C" int dsvg_dispatch_plan(int width, int height, int subsamp, dsvg_dispatch *out)
{
    if (!out) { dsvg_set_error("null argument"); return DSVG_ERR_ARG; }
    CtxGeo geo;
    const int rc = geom_check(width, height, subsamp, geo);
    if (rc) return rc;
    memset(out, 0, sizeof(*out));
    out->blk_w = geo.bw; out->blk_h = geo.bh;
    out->fusable = mc_fusable(geo.MG) ? 1 : 0;
    // (code_batch_impl passes general_whole from the pictures' intra blocks; with FWD_FAST_INTRA it does not enter the decision)
    for (int g = 0; g < 2; g++) out->fwd[g] = fwd_sbt_plan(geo.G, 1, g ? 1 : 0, g ? 2 : 1, 1, 0, FWD_FRAME_STEP, out->fusable ? &geo.MG : nullptr, 0, false).mask;
    HmeArgs A;
    make_hme_geo(A, geo, width, height, subsamp);
    const HmePlan H = hme_plan(A, 1, true);
    out->hme_levels = H.levels;
    for (int l = 0; l <= H.levels; l++) {
        const HmeLevelPlan &P = H.lv[l];
        out->hme[l][0] = P.nkbf; out->hme[l][1] = P.fullx; out->hme[l][2] = P.fully; out->hme[l][3] = P.parts;
    }
    out->csum = H.csum;
    out->tail_threads = out->scan_threads = -1;      // (a function of the jobs per launch, not of the geometry)
    return DSVG_OK;
}

// The inverse launcher's plan for one plane group of njobs pictures of an encoder context of this geometry (include/dsvg.h): inv_sbt_plan on
// the context's geometry tables, with the switches the caller names instead of the environment's
extern "C" int dsvg_inv_plan(int width, int height, int subsamp, int group, int isP, int with_tail, int insym, int patch_kernel, int fuse_border,
                             unsigned switches, int njobs, dsvg_inv_step *steps, int cap, int *fb)
{
    if (group < 0 || group > 1 || njobs < 1 || cap < 0 || (cap > 0 && !steps)) { dsvg_set_error("bad inv_plan arguments"); return DSVG_ERR_ARG; }
    CtxGeo geo;
    const int rc = geom_check(width, height, subsamp, geo);
    if (rc) return rc;
    const InvSwitches sw = { (switches & DSVG_INV_NO_PATCH_PART) != 0, (switches & DSVG_INV_NO_EDGE_TILES) != 0,
                             (switches & DSVG_INV_NO_FUSED_BORDER) != 0, (switches & DSVG_INV_NO_XCD_ORDER) != 0 };
    const InvPlan P = inv_sbt_plan(geo.G, njobs, group ? 1 : 0, group ? 2 : 1, isP, with_tail, insym, patch_kernel, fuse_border, sw);
    for (int i = 0; i < P.n && i < cap; i++) {
        const InvStep &s = P.s[i];
        dsvg_inv_step &o = steps[i];
        o.kernel = s.kid;
        o.grid[0] = s.gx; o.grid[1] = s.gy; o.grid[2] = s.gz; o.xcd = s.xcd ? (s.plain ? 2 : 1) : 0;
        for (int k = 0; k < 4; k++) o.args[k] = s.a[k];
        o.bytes = s.bytes;
        o.cover = s.cover; o.cx = s.cx; o.cy = s.cy;
    }
    if (fb) *fb = P.fb;
    return P.n;
}

// The forward plans of an encoder context of this geometry (include/dsvg.h): fwd_sbt_plan as enqueue_group asks it for a plane group of
// njobs I or P pictures, or fwd_step_plan, on the context's geometry tables, with the switches the caller names instead of the environment's
extern "C" int dsvg_fwd_plan(int width, int height, int subsamp, int group, int isP, int general_whole, unsigned switches, int njobs,
                             dsvg_fwd_step *steps, int cap, int *mask)
{
    if (group < 0 || group > DSVG_FWD_GROUP_STEP || njobs < 1 || cap < 0 || (cap > 0 && !steps)) { dsvg_set_error("bad fwd_plan arguments"); return DSVG_ERR_ARG; }
    CtxGeo geo;
    const int rc = geom_check(width, height, subsamp, geo);
    if (rc) return rc;
    const bool fused = mc_fusable(geo.MG) && !(switches & DSVG_FWD_NO_MC_FUSION);
    const FwdPlan P = group == DSVG_FWD_GROUP_STEP ? fwd_step_plan(geo.G, njobs, !(switches & DSVG_FWD_NO_LLQ))
                                                   : fwd_sbt_plan(geo.G, njobs, group ? 1 : 0, group ? 2 : 1, isP, !isP, FWD_FRAME_STEP, fused ? &geo.MG : nullptr,
                                                                  general_whole, (switches & DSVG_FWD_NO_XCD_ORDER) != 0);
    for (int i = 0; i < P.n && i < cap; i++) {
        const FwdStep &s = P.s[i];
        dsvg_fwd_step &o = steps[i];
        o.kernel = s.kid;
        o.grid[0] = s.gx; o.grid[1] = s.gy; o.grid[2] = s.gz; o.xcd = s.xcd ? (s.plain ? 2 : 1) : 0;
        o.block[0] = s.bx; o.block[1] = s.by; o.lds = (unsigned)s.lds;
        for (int k = 0; k < 4; k++) o.args[k] = s.a[k];
        o.bytes = s.bytes;
    }
    if (mask) *mask = P.mask;
    return P.n;
}

// The motion search's plan for npairs pairs of such a context (default pyramid depth), with or without the chroma table
extern "C" int dsvg_hme_plan(int width, int height, int subsamp, int csum_table, int npairs, dsvg_hme_step *steps, int cap)
{
    if (npairs < 1 || cap < 0 || (cap > 0 && !steps)) { dsvg_set_error("bad hme_plan arguments"); return DSVG_ERR_ARG; }
    CtxGeo geo;
    const int rc = geom_check(width, height, subsamp, geo);
    if (rc) return rc;
    HmeArgs A;
    make_hme_geo(A, geo, width, height, subsamp);
    const HmePlan P = hme_plan(A, npairs, csum_table != 0);
    for (int i = 0; i < P.n && i < cap; i++) {
        const HmeStep &s = P.s[i];
        dsvg_hme_step &o = steps[i];
        o.kernel = s.kid; o.l0 = s.l0; o.nkbf = s.nkbf; o.part = s.part;
        o.level = s.level; o.count = s.cnt; o.fullx = s.fullx; o.fully = s.fully; o.inv_per = s.inv_per; o.inv_row = s.inv_row;
        o.grid[0] = s.gx; o.grid[1] = s.gy; o.block = s.bx;
        o.bytes = s.bytes; o.cont = s.cont;
    }
    return P.n;
}

// the argument checks of dsvg_ctx_create_blk that need no device (dsvg_ctx_mem_plan makes them too)
static int ctx_args_check(int width, int height, int subsamp, int n_src_slots, int n_recon_slots, int max_jobs, int blk_w, int blk_h)
{
    if ((blk_w || blk_h) && (blk_w < 16 || blk_w > 64 || blk_h < 16 || blk_h > 64 || (blk_w & 3) || (blk_h & 3))) {
        dsvg_set_error("block size %dx%d: multiples of 4 in 16..64 (dsv_decoder.c:351-356)", blk_w, blk_h);
        return DSVG_ERR_ARG;
    }
    if (width < 32 || height < 32 || n_src_slots < 1 || n_recon_slots < 1 || max_jobs < 1) { dsvg_set_error("bad ctx_create arguments"); return DSVG_ERR_ARG; }
    if (subsamp != 0x0 && subsamp != 0x4 && subsamp != 0x5 && subsamp != 0x8) { dsvg_set_error("bad subsampling"); return DSVG_ERR_ARG; }
    return DSVG_OK;
}
// What the sizes of a context's buffers read of it (dsvg_ctx_mem.h), and its per-plane scan bookkeeping, from the tables of its
// creation: dsvg_ctx_create_blk keeps both, and dsvg_ctx_mem_plan asks the plan about the same record without a context.
static void ctx_mem_geo(CtxMemGeo &M, CtxScan &S, const CtxGeo &geo, const HmeArgs &A, const BatchGeo &B)
{
    const CoefLayout &CL = geo.CL;
    int nchunks[3];
    M = CtxMemGeo();
    for (int p = 0; p < 3; p++) {
        HzPlane hp; make_hz_plane(hp, CL.w[p], CL.h[p], 100, 0, p, geo.nbh, geo.nbv);
        nchunks[p] = hp.nchunks;
        M.ll[p] = (size_t)CL.w3[p] * CL.h3[p];
    }
    ctx_scan_layout(S, nchunks, CL.w, CL.h, M.ll);
    M.levels = A.levels;
    for (int l = 0; l <= A.levels; l++) M.pitch[l] = A.L[l].pitch;
    M.total = CL.total; M.s3total = CL.s3total; M.s1total = CL.s1total; M.s5total = CL.s5total;
    M.nz_total = S.nz_total; M.bits_per_job = S.bits_per_job; M.chunks_per_job = S.chunks_per_job; M.nblk = B.nblk;
    M.n_src = B.n_src; M.n_recon = B.n_recon; M.max_jobs = B.max_jobs; M.out_slots = B.out_slots; M.rc_slots = B.rc_slots; M.mc_fused = B.mc_fused;
    M.nwin = (B.out_slots + B.max_jobs - 1) / B.max_jobs + 1;
    M.sz_chunk_sum = sizeof(HzChunkSum); M.sz_plane_sum = sizeof(HzPlaneSum); M.sz_mv = sizeof(DMV); M.sz_job = sizeof(JobDev);
    M.sz_rc_job = sizeof(RcJobDev); M.sz_rc_state = sizeof(dsvg_rc_state); M.sz_parse_chunk = sizeof(HzParseChunk);
}
// the same for the arguments of a creation, checked as it checks them (the switches: the environment's, as at creation)
static int ctx_mem_geo_of(CtxMemGeo &M, int width, int height, int subsamp, int pyramid_levels, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots,
                          int blk_w, int blk_h)
{
    OPCHK(ctx_args_check(width, height, subsamp, n_src_slots, n_recon_slots, max_jobs, blk_w, blk_h));
    CtxGeo geo;
    make_ctx_geo(geo, width, height, subsamp, blk_w, blk_h);
    OPCHK(geo_supported(geo, width, height));
    HmeArgs A;
    make_hme_geo(A, geo, width, height, subsamp, pyramid_levels);
    CtxScan S;
    ctx_mem_geo(M, S, geo, A, batch_geo(geo, n_src_slots, n_recon_slots, max_jobs, out_slots, !getenv("DSV1_NO_MC_FUSION"), !getenv("DSV1_NO_LAZY_BORDER")));
    return DSVG_OK;
}
extern "C" int dsvg_ctx_mem_plan(int width, int height, int subsamp, int pyramid_levels, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots,
                                 int blk_w, int blk_h, dsvg_ctx_mem_row *rows, int cap, size_t totals[2])
{
    if (cap < 0 || (cap > 0 && !rows)) { dsvg_set_error("bad ctx_mem_plan arguments"); return DSVG_ERR_ARG; }
    CtxMemGeo M;
    OPCHK(ctx_mem_geo_of(M, width, height, subsamp, pyramid_levels, n_src_slots, n_recon_slots, max_jobs, out_slots, blk_w, blk_h));
    dsvg_ctx_mem_row all[CM_N_CREATE];
    const int n = plan_ctx_mem(M, all, totals);
    for (int i = 0; i < n && i < cap; i++) rows[i] = all[i];
    return n;
}
extern "C" size_t dsvg_ctx_mem_grow(int width, int height, int subsamp, int pyramid_levels, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots,
                                    int blk_w, int blk_h, int id, size_t need, size_t cap, int few)
{
    CtxMemGeo M;
    if (id < CM_N_CREATE || id >= CM_N || ctx_mem_geo_of(M, width, height, subsamp, pyramid_levels, n_src_slots, n_recon_slots, max_jobs, out_slots, blk_w, blk_h)) return 0;
    return ctx_mem_lazy_bytes(id, M, ctx_mem_grow(id, M, need, cap, few != 0));
}

extern "C" int dsvg_ctx_create(dsvg_ctx **out, int device, int width, int height, int subsamp,
                               int pyramid_levels, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots)
{
    return dsvg_ctx_create_blk(out, device, width, height, subsamp, pyramid_levels, n_src_slots, n_recon_slots, max_jobs, out_slots, 0, 0);
}
extern "C" int dsvg_ctx_create_blk(dsvg_ctx **out, int device, int width, int height, int subsamp,
                                   int pyramid_levels, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots, int blk_w, int blk_h)
{
    if (!out) { dsvg_set_error("bad ctx_create arguments"); return DSVG_ERR_ARG; }
    OPCHK(ctx_args_check(width, height, subsamp, n_src_slots, n_recon_slots, max_jobs, blk_w, blk_h));
    if (dsvg_device_count() <= device) { dsvg_set_error("HIP device %d not present", device); return DSVG_ERR_NODEVICE; }
    HIPCHK(hipSetDevice(device));
    dsvg_ctx *c = new dsvg_ctx();
    *out = nullptr;
    c->device = device;
    c->w = width; c->h = height; c->fmt = subsamp;
    {
        CtxGeo geo;
        make_ctx_geo(geo, width, height, subsamp, blk_w, blk_h);
        c->bw = geo.bw; c->bh = geo.bh; c->nbh = geo.nbh; c->nbv = geo.nbv;
        c->L[0] = geo.L; c->CL = geo.CL; c->G = geo.G; c->MG = geo.MG;
        make_hme_geo(c->hme, geo, width, height, subsamp, pyramid_levels);
        c->levels = c->hme.levels;
        for (int l = 1; l <= c->levels; l++) c->L[l] = c->hme.L[l];
        c->bgeo = batch_geo(geo, n_src_slots, n_recon_slots, max_jobs, out_slots, !getenv("DSV1_NO_MC_FUSION"), !getenv("DSV1_NO_LAZY_BORDER"));
        c->dgeo = dec_geo(geo, n_recon_slots, max_jobs, !getenv("DSV1_NO_MC_FUSION"), !getenv("DSV1_NO_DEC_SYM_OV"));
        const int rc = geo_supported(geo, width, height);
        if (rc) { delete c; return rc; }
        ctx_mem_geo(c->mgeo, c->scan, geo, c->hme, c->bgeo);
    }
    out_slots = c->bgeo.out_slots;                          // (at least max_jobs)
    c->n_src = n_src_slots; c->n_recon = n_recon_slots; c->max_jobs = max_jobs; c->out_slots = out_slots;
    c->nwin = c->mgeo.nwin;
    c->nblk = c->nbh * c->nbv;
    c->mc_fused = c->bgeo.mc_fused != 0;
    c->no_inplace_pred = getenv("DSV1_NO_INPLACE_PRED") != nullptr;
    c->no_dec_sym = getenv("DSV1_NO_DEC_SYM") != nullptr;
    c->no_dec_sym_I = getenv("DSV1_NO_DEC_SYM_I") != nullptr;
    c->no_patch_kernel = getenv("DSV1_NO_PATCH_KERNEL") != nullptr;
    c->no_list_pack = getenv("DSV1_NO_LIST_PACK") != nullptr;
    c->no_lazy_border = !c->bgeo.lazy_border;
    // two coding streams by default: with the analysis and fetch streams that is four, the number of hardware queues
    // the runtime maps streams onto (three coding streams measured 18.5 ms per step against 14.3 with two and 15.4 with one)
    { const char *e = getenv("DSV1_CODE_STREAMS"); c->code_streams = e ? atoi(e) : 2; }
    int rc = DSVG_OK;
    // (a failed allocation also leaves HIP's per-thread last error set: it is taken here, or the next context's first
    // hipGetLastError check -- a smaller ladder tried after one that did not fit -- would report this failure as its own)
    auto fail = [&](int r) { (void)hipGetLastError(); ctx_free(c); return r; };
    if (max_jobs >= 16) {
        // throughput contexts (several coding streams will run): coding, analysis, further coding streams on hardware
        // queues of their own; the fetch stream (idle most of the time) takes what is left.  The probe costs ~30 ms.
        const int ncs = std::max(1, std::min(c->code_streams, DSVG_MAX_CODE_STREAMS));
        hipStream_t ps[3 + DSVG_MAX_CODE_STREAMS] = {};
        const int want = 2 + std::max(ncs, 2);
        int copy_shared = -1;
        const int good = pick_streams(ps, want, &c->st_h, &copy_shared);
        c->copy_queue = copy_shared;
        if (getenv("DSV1_STREAM_DEBUG")) fprintf(stderr, "[dsvg] %d of %d streams on hardware queues of their own; copy stream: %s\n", good, want,
                                                 copy_shared == 0 ? "a queue of its own" : (copy_shared >= 2 ? "a queue of its own (priority stream)" : (copy_shared == 1 ? "shares the analysis stream's queue" : "as the runtime places it")));
        if (good < 0) { dsvg_set_error("hipStreamCreate failed"); return fail(DSVG_ERR_HIP); }
        c->st = ps[0]; c->st_a = ps[1];
        for (int g = 1; g < std::max(ncs, 2); g++) c->stx[g] = ps[1 + g];      // every stream is owned by the ctx before anything can fail
        c->st_c = ps[want - 1];
        for (int g = 1; g < std::max(ncs, 2); g++)
            if (hipEventCreateWithFlags(&c->ev_join[g], hipEventDisableTiming) != hipSuccess) { dsvg_set_error("hipEventCreate failed"); return fail(DSVG_ERR_HIP); }
        c->streams_apart = good;
    } else if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&c->st_a, hipStreamNonBlocking) != hipSuccess ||
               hipStreamCreateWithFlags(&c->st_c, hipStreamNonBlocking) != hipSuccess) {
        dsvg_set_error("hipStreamCreate failed"); return fail(DSVG_ERR_HIP);      // one picture (or a few) at a time: streams as they come
    }
    if (!c->st_l) c->st_l = c->st_a;
    c->tl_on = getenv("DSV1_TIMELINE") != nullptr;
    if (hipEventCreateWithFlags(&c->ev_a, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_l, hipEventDisableTiming) != hipSuccess) { dsvg_set_error("hipEventCreate failed"); return fail(DSVG_ERR_HIP); }
    c->ev_coded.resize((size_t)2 * c->nwin + 2);
    for (auto &e : c->ev_coded)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { dsvg_set_error("hipEventCreate failed"); return fail(DSVG_ERR_HIP); }
    c->slot_ev.assign((size_t)out_slots, -1);
    sbt_set_func_attributes();
    {   // every buffer of the plan, in its order (slabs, work and result buffers, pinned staging, the source slots' plane tables)
        dsvg_ctx_mem_row rows[CM_N_CREATE];
        const int nrows = plan_ctx_mem(c->mgeo, rows, nullptr);
        for (int i = 0; i < nrows; i++)
            if ((rc = ctx_alloc(c, rows[i].id, rows[i].kind, rows[i].bytes, rows[i].zeroed != 0))) return fail(rc);
        ctx_fields(c);
    }
    c->llq = !getenv("DSV1_NO_LLQ");
    c->rc_slots = c->bgeo.rc_slots;
    {   // every source slot's chroma starts as the bordered copy in the slab
        const size_t ns = (size_t)n_src_slots;
        c->slot_cu.resize(ns); c->slot_cv.resize(ns); c->slot_cs.assign(ns, c->L[0].stride[1]);
        for (size_t sl = 0; sl < ns; sl++) {
            c->slot_cu[sl] = c->src[0].p + sl * c->L[0].pitch + c->L[0].off[1];
            c->slot_cv[sl] = c->src[0].p + sl * c->L[0].pitch + c->L[0].off[2];
            c->slot_cu_h[sl] = (unsigned long long)(uintptr_t)c->slot_cu[sl]; c->slot_cv_h[sl] = (unsigned long long)(uintptr_t)c->slot_cv[sl];
            c->slot_cs_h[sl] = c->slot_cs[sl];
        }
        if (hipMemcpy(c->slot_cu_d, c->slot_cu_h, 8 * ns, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(c->slot_cv_d, c->slot_cv_h, 8 * ns, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(c->slot_cs_d, c->slot_cs_h, 4 * ns, hipMemcpyHostToDevice) != hipSuccess) { dsvg_set_error("slot tables: upload failed"); return fail(DSVG_ERR_HIP); }
        // in place: the forward transforms read whole 8-byte patch rows and never leave the picture when the chroma planes are
        // even (no extra coefficient column: frame.c:39-42) and a multiple of 8 wide; both chroma planes alike
        c->slot_y.assign(ns, nullptr);                  // (slot_y_h / slot_y_d: zeroed by the allocator)
        // (the geometry's side of both rules: dsvg_load_plan.h)
        c->lgeo = load_geo(c->hme, c->src);
        c->cdirect_ok = load_chroma_in_place_geo(c->lgeo) && !getenv("DSV1_NO_CHROMA_IN_PLACE");
        // luma in place (round 5): the geometry must take the motion search's full-block body and k_unpack's fused pyramid levels 1 and 2
        // (the bordered copy is then read by the level-0 search alone), and the ring must leave an interior worth the trouble
        c->deep_r = hme_deep_r(c->levels);
        c->ring_x16 = c->lgeo.ring_x16;
        c->ring_y4 = c->lgeo.ring_y4;
        c->ydirect_ok = c->cdirect_ok && load_luma_in_place_geo(c->lgeo) && !getenv("DSV1_NO_LUMA_IN_PLACE") && !getenv("DSV1_NO_FUSE_LEVEL2");
    }
    // the pipeline streams are non-blocking (no implicit ordering against the NULL stream the memsets above ran on)
    if (hipDeviceSynchronize() != hipSuccess) { dsvg_set_error("hipDeviceSynchronize failed"); return fail(DSVG_ERR_HIP); }
    *out = c;
    return DSVG_OK;
}

#ifdef DSVG_CLOCK_PROBE
extern "C" void dsvg_clk_dump_sbt();
extern "C" void dsvg_clk_dump_hme();
extern "C" void dsvg_ctx_destroy(dsvg_ctx *ctx) { if (ctx) { (void)hipDeviceSynchronize(); dsvg_clk_dump_sbt(); dsvg_clk_dump_hme(); } ctx_free(ctx); }
#else
extern "C" void dsvg_ctx_destroy(dsvg_ctx *ctx) { ctx_free(ctx); }
#endif

extern "C" int dsvg_ctx_mark(dsvg_ctx *c, int which)
{
    if (!c || which < 0 || which > 1) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (!c->ev_mark[which]) HIPCHK(hipEventCreate(&c->ev_mark[which]));
    HIPCHK(hipEventRecord(c->ev_mark[which], c->st));
    return DSVG_OK;
}
extern "C" int dsvg_ctx_mark_ms(dsvg_ctx *c, float *ms)
{
    if (!c || !ms || !c->ev_mark[0] || !c->ev_mark[1]) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_mark[1]));
    HIPCHK(hipEventElapsedTime(ms, c->ev_mark[0], c->ev_mark[1]));
    return DSVG_OK;
}

extern "C" int dsvg_ctx_geom(const dsvg_ctx *c, dsvg_geom *g)
{
    if (!c || !g) return DSVG_ERR_ARG;
    memset(g, 0, sizeof(*g));
    g->width = c->w; g->height = c->h; g->subsamp = c->fmt;
    g->blk_w = c->bw; g->blk_h = c->bh; g->nblocks_h = c->nbh; g->nblocks_v = c->nbv;
    g->pyramid_levels = c->levels;
    g->frame_bytes = (size_t)c->L[0].w[0] * c->L[0].h[0] + 2 * (size_t)c->L[0].w[1] * c->L[0].h[1];
    for (int p = 0; p < 3; p++) g->plane_out_cap[p] = c->scan.bits_cap[p];
    g->frame_alloc_bytes = c->L[0].bytes;
    return DSVG_OK;
}

extern "C" int dsvg_ctx_sync(dsvg_ctx *c)
{
    if (!c) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    OPCHK(dec_resolve(c));
    if (c->st_h) HIPCHK(hipStreamSynchronize(c->st_h));
    for (int g = 1; g < DSVG_MAX_CODE_STREAMS; g++) if (c->stx[g]) HIPCHK(hipStreamSynchronize(c->stx[g]));
    if (c->st_l != c->st_a) HIPCHK(hipStreamSynchronize(c->st_l));
    HIPCHK(hipStreamSynchronize(c->st_a));
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipStreamSynchronize(c->st_c));
    if (!c->tl_quiet) tl_dump(c);           // (DSV1_TIMELINE: printed and cleared at every sync; dsvg_ctx_timeline: kept for dsvg_ctx_timeline_get)
    c->calls_since_sync = 0;
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}
extern "C" int dsvg_ctx_code_streams(dsvg_ctx *c, int n)
{
    if (!c) return DSVG_ERR_ARG;
    const int old = c->code_streams;
    if (n >= 1) c->code_streams = std::min(n, DSVG_MAX_CODE_STREAMS);
    return old;
}
extern "C" int dsvg_ctx_streams_apart(const dsvg_ctx *c) { return c ? c->streams_apart : 0; }
extern "C" int dsvg_ctx_copy_queue(const dsvg_ctx *c) { return c ? c->copy_queue : -1; }
extern "C" int dsvg_ctx_tile_stats2(dsvg_ctx *c, unsigned long long out[8], int enable)
{
    if (!c || !out) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    OPCHK(dsvg_ctx_sync(c));
    unsigned v[8 * 64];
    HIPCHK(hipMemcpyAsync(v, c->stat, sizeof(v), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemsetAsync(c->stat, 0, sizeof(v), c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    for (int i = 0; i < 8; i++) {
        out[i] = 0;
        for (int k = 0; k < 64; k++) out[i] += v[64 * i + k];
    }
    out[7] = c->border_bytes;          // bytes of reconstruction border written by the fused inverse kernels (host-side tally)
    c->border_bytes = 0;
    c->stats_on = enable != 0;
    return DSVG_OK;
}
extern "C" int dsvg_ctx_tile_stats(dsvg_ctx *c, unsigned long long out[4], int enable)
{
    unsigned long long v[8];
    if (!out) return DSVG_ERR_ARG;
    const int rc = dsvg_ctx_tile_stats2(c, v, enable);
    if (rc == DSVG_OK) for (int i = 0; i < 4; i++) out[i] = v[i];
    return rc;
}
// The ordering contract of the handle (advisor round 5): work a caller puts on it AFTER this call runs behind everything the context has enqueued
// so far -- including a packing pass of device output that dsvg_pack_recons put on the second coding stream (the first stream is told to wait
// for it here, at the latest).
static int join_pack(dsvg_ctx *c)
{
    if (c->pack_pending) {
        if (hipSetDevice(c->device) != hipSuccess || hipStreamWaitEvent(c->st, c->ev_pack[1], 0) != hipSuccess) { dsvg_set_error("could not order the first coding stream behind the packing pass"); return DSVG_ERR_HIP; }
        c->pack_pending = false;
    }
    return DSVG_OK;
}
extern "C" void *dsvg_ctx_stream(dsvg_ctx *c) { return c && join_pack(c) == DSVG_OK ? (void *)c->st : nullptr; }
// the frame-load stream waits, on the device, for a HIP event of the caller's (the resolution ladder's scale of this context's frames)
extern "C" int dsvg_ctx_load_wait(dsvg_ctx *c, void *event)
{
    if (!c || !event) { dsvg_set_error("bad load_wait arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamWaitEvent(c->st_l, (hipEvent_t)event, 0));
    return DSVG_OK;
}
extern "C" int dsvg_ctx_join(dsvg_ctx *c, void *stream)
{
    if (!c) { dsvg_set_error("no context"); return DSVG_ERR_ARG; }
    OPCHK(join_pack(c));
    if (stream && (hipStream_t)stream != c->st) {
        if (!c->ev_user) HIPCHK(hipEventCreateWithFlags(&c->ev_user, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_user, c->st));
        HIPCHK(hipStreamWaitEvent((hipStream_t)stream, c->ev_user, 0));
    }
    return DSVG_OK;
}

extern "C" int dsvg_dev_alloc(dsvg_ctx *c, void **dptr, size_t bytes)
{
    if (!c || !dptr) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(dptr, bytes + 256));
    return DSVG_OK;
}
extern "C" int dsvg_dev_free(dsvg_ctx *c, void *dptr)
{
    if (!c) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipFree(dptr));
    return DSVG_OK;
}
extern "C" int dsvg_dev_upload(dsvg_ctx *c, void *dptr, const void *src, size_t bytes)
{
    if (!c) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(dptr, src, bytes, hipMemcpyHostToDevice));
    return DSVG_OK;
}

extern "C" int dsvg_dev_download(dsvg_ctx *c, void *dst, const void *dptr, size_t bytes)
{
    if (!c || !dst || !dptr) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(dst, dptr, bytes, hipMemcpyDeviceToHost));
    return DSVG_OK;
}
extern "C" int dsvg_host_alloc(dsvg_ctx *c, void **hptr, size_t bytes)
{
    if (!c || !hptr) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipHostMalloc(hptr, bytes + 64, hipHostMallocDefault));
    return DSVG_OK;
}
extern "C" int dsvg_host_free(dsvg_ctx *c, void *hptr)
{
    if (!c) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipHostFree(hptr));
    return DSVG_OK;
}

// reserve the next ingest buffer for a clip of `bytes` bytes; the copy stream waits for the buffer's last readers
static int ingest_reserve(dsvg_ctx *c, size_t bytes, int *kout)
{
    HIPCHK(hipSetDevice(c->device));
    if (!c->st_h) {
        // (small contexts, or no probed candidate: pick_streams placed none.  A stream with a CU mask of all ones would get a hardware queue of its
        // own and hung dsv_enc's frame-at-a-time ingest in a third of the runs: DESIGN section 7, dead ends)
        HIPCHK(hipStreamCreateWithFlags(&c->st_h, hipStreamNonBlocking));
    }
    if (!c->ev_up[0]) {
        for (int i = 0; i < 2; i++) {
            HIPCHK(hipEventCreateWithFlags(&c->ev_up[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->ev_used[i], hipEventDisableTiming));
        }
    }
    const int k = c->ingest_next;
    c->ingest_next ^= 1;
    bool grew;                                   // (an old buffer may still be read by load kernels / an earlier copy: ctx_grow waits)
    OPCHK(ctx_grow(c, CM_INGEST0 + k, bytes, false, &grew));
    if (grew) c->used_valid[k] = false;
    if (c->used_valid[k]) HIPCHK(hipStreamWaitEvent(c->st_h, c->ev_used[k], 0));    // its last readers (analysis stream)
    *kout = k;
    return DSVG_OK;
}

extern "C" int dsvg_ingest_begin(dsvg_ctx *c, const void *yuv_host, size_t bytes, void **dptr)
{
    if (!c || !yuv_host || !dptr || !bytes) { dsvg_set_error("bad ingest arguments"); return DSVG_ERR_ARG; }
    int k;
    OPCHK(ingest_reserve(c, bytes, &k));
    tl_mark(c, c->st_h, "up0");
    HIPCHK(hipMemcpyAsync(c->ingest[k], yuv_host, bytes, hipMemcpyHostToDevice, c->st_h));
    tl_mark(c, c->st_h, "up1");
    HIPCHK(hipEventRecord(c->ev_up[k], c->st_h));
    c->up_pending[k] = true;
    *dptr = c->ingest[k];
    return DSVG_OK;
}

// The same for a clip that arrives piece by piece (dsv_enc: a frame per call): open reserves the buffer, every part is
// queued on the copy stream as soon as the caller has it -- the link is busy while the caller gathers the next frames, not
// in one burst when the batch is complete.  A load from the buffer waits for the parts queued before it.
extern "C" int dsvg_ingest_open(dsvg_ctx *c, size_t bytes, void **dptr)
{
    if (!c || !dptr || !bytes) { dsvg_set_error("bad ingest arguments"); return DSVG_ERR_ARG; }
    int k;
    OPCHK(ingest_reserve(c, bytes, &k));
    *dptr = c->ingest[k];
    return DSVG_OK;
}
extern "C" int dsvg_ingest_part(dsvg_ctx *c, void *dptr, size_t offset, const void *host, size_t bytes)
{
    if (!c || !dptr || !host || !bytes) { dsvg_set_error("bad ingest arguments"); return DSVG_ERR_ARG; }
    for (int k = 0; k < 2; k++)
        if (c->ingest[k] && dptr == (void *)c->ingest[k]) {
            if (offset + bytes > c->mem[CM_INGEST0 + k].cap) { dsvg_set_error("ingest part beyond the reserved clip"); return DSVG_ERR_ARG; }
            HIPCHK(hipSetDevice(c->device));
            HIPCHK(hipMemcpyAsync(c->ingest[k] + offset, host, bytes, hipMemcpyHostToDevice, c->st_h));
            HIPCHK(hipEventRecord(c->ev_up[k], c->st_h));
            c->up_pending[k] = true;
            return DSVG_OK;
        }
    dsvg_set_error("not an open ingest buffer");
    return DSVG_ERR_ARG;
}

// a frame source inside an ingest buffer: the analysis stream waits for the upload; returns the buffer index or -1
static int ingest_acquire(dsvg_ctx *c, const void *dsrc)
{
    for (int k = 0; k < 2; k++) {
        const uint8_t *b = c->ingest[k], *p = (const uint8_t *)dsrc;
        if (b && p >= b && p < b + c->mem[CM_INGEST0 + k].cap) {
            if (c->up_pending[k]) {
                if (hipStreamWaitEvent(c->st_l, c->ev_up[k], 0) != hipSuccess) return -2;
                c->up_pending[k] = false;
            }
            return k;
        }
    }
    return -1;
}
static int ingest_release(dsvg_ctx *c, int k)
{
    if (k < 0) return DSVG_OK;
    HIPCHK(hipEventRecord(c->ev_used[k], c->st_l));
    c->used_valid[k] = true;
    return DSVG_OK;
}

// ------------------------------------------------------------------------------------------------
static int load_core(dsvg_ctx *c, int first_slot, int n, const uint8_t *dsrc, size_t pitch, int with_pyramid, const int *tab_d, int n_chroma = -1, int n_ring = 0)
{
    if (!tab_d) {       // contiguous slots, chroma copied: those slots' chroma is the bordered copy (again)
        bool changed = false, ychanged = false;
        for (int sl = first_slot; sl < first_slot + n; sl++)
            if (c->slot_y[sl]) { c->slot_y[sl] = nullptr; c->slot_y_h[sl] = 0; ychanged = true; }
        if (ychanged) HIPCHK(hipMemcpyAsync(c->slot_y_d, c->slot_y_h, 8 * (size_t)c->n_src, hipMemcpyHostToDevice, c->st_l));
        for (int sl = first_slot; sl < first_slot + n; sl++) {
            const uint8_t *u = c->src[0].p + (size_t)sl * c->L[0].pitch + c->L[0].off[1], *v = c->src[0].p + (size_t)sl * c->L[0].pitch + c->L[0].off[2];
            if (c->slot_cu[sl] != u || c->slot_cs[sl] != c->L[0].stride[1]) {
                c->slot_cu[sl] = u; c->slot_cv[sl] = v; c->slot_cs[sl] = c->L[0].stride[1];
                c->slot_cu_h[sl] = (unsigned long long)(uintptr_t)u; c->slot_cv_h[sl] = (unsigned long long)(uintptr_t)v; c->slot_cs_h[sl] = c->L[0].stride[1];
                changed = true;
            }
        }
        if (changed) {
            HIPCHK(hipMemcpyAsync(c->slot_cu_d, c->slot_cu_h, 8 * (size_t)c->n_src, hipMemcpyHostToDevice, c->st_l));
            HIPCHK(hipMemcpyAsync(c->slot_cv_d, c->slot_cv_h, 8 * (size_t)c->n_src, hipMemcpyHostToDevice, c->st_l));
            HIPCHK(hipMemcpyAsync(c->slot_cs_d, c->slot_cs_h, 4 * (size_t)c->n_src, hipMemcpyHostToDevice, c->st_l));
        }
    }
    // what the load launches: decided in one place (plan_load, dsvg_load_plan.h), from the geometry, the source's alignment and the
    // switches; the launches below follow the plan
    if (n_chroma < 0) n_chroma = n;
    dsvg_load_plan_out P;
    plan_load(c->lgeo, load_switches(), with_pyramid != 0, (int)((uintptr_t)dsrc & 15), (int)(pitch & 15), n, n - n_chroma, n_ring, P);
    tl_mark(c, c->st_l, "load0");
    launch_unpack(c->st_l, dsrc, pitch, c->src[0].p, c->L[0], first_slot, n, &c->prof, tab_d, P.fuse1 ? c->src[1].p : nullptr, P.fuse1 ? &c->L[1] : nullptr,
                  P.sides != 0, P.sides1 != 0, P.fuse2 ? c->src[2].p : nullptr, P.fuse2 ? &c->L[2] : nullptr, P.sides2 != 0, n_chroma, P.ring_x16, P.ring_y4, n_ring);
    for (int l = 0; l <= c->levels; l++) {
        const dsvg_load_level &o = P.level[l];
        if (o.border == DSVG_BORDER_NONE) continue;                     // (the pyramid's levels without the pyramid)
        if (o.ds2x) launch_ds2x(c->st_l, c->src[l - 1].p, c->L[l - 1], c->src[l].p, c->L[l], first_slot, n, &c->prof, tab_d, o.ds2x_sides != 0);
        launch_extend(c->st_l, c->src[l].p, c->L[l], first_slot, n, l ? 1 : 3, tab_d, &c->prof, nullptr, o.tb_only != 0);
    }
    if (P.luma_sum) {
        // (a mapped load clears the sums of ALL slots, a contiguous one those of its own: include/dsvg.h, dsvg_load_frames_map)
        if (tab_d) HIPCHK(hipMemsetAsync(c->luma_sums, 0, sizeof(unsigned) * c->n_src, c->st_l));
        else       HIPCHK(hipMemsetAsync(c->luma_sums + first_slot, 0, sizeof(unsigned) * n, c->st_l));
        launch_luma_sum(c->st_l, c->src[c->levels].p, c->L[c->levels], first_slot, n, c->luma_sums, &c->prof, tab_d);
    }
    tl_mark(c, c->st_l, "load1");
    if (c->st_l != c->st_a) {      // the motion search and the coding streams take the frames from the analysis stream's order
        HIPCHK(hipEventRecord(c->ev_l, c->st_l));
        HIPCHK(hipStreamWaitEvent(c->st_a, c->ev_l, 0));
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

extern "C" int dsvg_load_frames(dsvg_ctx *c, int first_slot, int n, const void *yuv, int yuv_on_device, int with_pyramid)
{
    if (!c || !yuv || n < 1 || first_slot < 0 || first_slot + n > c->n_src) { dsvg_set_error("bad load_frames arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const size_t fb = (size_t)c->L[0].w[0] * c->L[0].h[0] + 2 * (size_t)c->L[0].w[1] * c->L[0].h[1];
    const uint8_t *dsrc = (const uint8_t *)yuv;
    if (!yuv_on_device) {
        OPCHK(ctx_grow(c, CM_YUV_STAGE, fb * n));
        HIPCHK(hipMemcpyAsync(c->yuv_stage, yuv, fb * n, hipMemcpyHostToDevice, c->st_l));
        dsrc = c->yuv_stage;
    }
    return load_core(c, first_slot, n, dsrc, fb, with_pyramid, nullptr);
}

extern "C" int dsvg_load_frames_strided(dsvg_ctx *c, int first_slot, int n, const void *yuv_dev, size_t frame_pitch, int with_pyramid)
{
    if (!c || !yuv_dev || n < 1 || first_slot < 0 || first_slot + n > c->n_src) { dsvg_set_error("bad load_frames arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return load_core(c, first_slot, n, (const uint8_t *)yuv_dev, frame_pitch, with_pyramid, nullptr);
}

// Frame i (at yuv_dev + i * frame_pitch) goes to source slot slots[i].  chroma_in_place (one flag per frame, or null): the
// frame's chroma planes are NOT copied -- the forward transform and the motion search's chroma test read them from the
// caller's packed clip, which only the luma plane leaves (bordered copy + pyramid: what a frame needs as a motion search
// REFERENCE).  The caller keeps the clip unchanged until the pictures coded from those slots have been fetched and until the
// next frame of each stream has been analysed; refused (plain copy) where the geometry or the clip's alignment does not allow it.
extern "C" int dsvg_load_frames_map_ex(dsvg_ctx *c, int n, const int *slots, const void *yuv_dev, size_t frame_pitch, int with_pyramid,
                                       const unsigned char *chroma_in_place)
{
    if (!c || !yuv_dev || !slots || n < 1 || n > c->n_src) { dsvg_set_error("bad load_frames arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    for (int i = 0; i < n; i++)
        if (slots[i] < 0 || slots[i] >= c->n_src) { dsvg_set_error("slot out of range"); return DSVG_ERR_ARG; }
    OPCHK(ctx_grow(c, CM_LTAB_D, 1));
    const size_t ysz = (size_t)c->L[0].w[0] * c->L[0].h[0], csz = (size_t)c->L[0].w[1] * c->L[0].h[1];
    const bool can = chroma_in_place && c->cdirect_ok && ((uintptr_t)yuv_dev % 16) == 0 && (frame_pitch % 16) == 0 && (ysz % 16) == 0 && (csz % 16) == 0;
    std::vector<int> tab((size_t)n);
    bool changed = false, ychanged = false;
    int n_direct = 0, n_ydirect = 0;
    for (int i = 0; i < n; i++) {
        const int sl = slots[i];
        const bool direct = can && chroma_in_place[i];
        n_direct += direct;
        const uint8_t *fr = (const uint8_t *)yuv_dev + (size_t)i * frame_pitch;
        const uint8_t *u = direct ? fr + ysz : c->src[0].p + (size_t)sl * c->L[0].pitch + c->L[0].off[1];
        const uint8_t *v = direct ? fr + ysz + csz : c->src[0].p + (size_t)sl * c->L[0].pitch + c->L[0].off[2];
        const int st = direct ? c->L[0].w[1] : c->L[0].stride[1];
        if (c->slot_cu[sl] != u || c->slot_cv[sl] != v || c->slot_cs[sl] != st) {
            c->slot_cu[sl] = u; c->slot_cv[sl] = v; c->slot_cs[sl] = st;
            c->slot_cu_h[sl] = (unsigned long long)(uintptr_t)u; c->slot_cv_h[sl] = (unsigned long long)(uintptr_t)v; c->slot_cs_h[sl] = st;
            changed = true;
        }
        // ... and its luma plane (round 5): the level-0 search and the forward transforms read it in the clip, the bordered copy gets its ring
        const bool ydirect = direct && c->ydirect_ok && with_pyramid;
        const uint8_t *yp = ydirect ? fr : nullptr;
        if (c->slot_y[sl] != yp) { c->slot_y[sl] = yp; c->slot_y_h[sl] = (unsigned long long)(uintptr_t)yp; ychanged = true; }
        tab[(size_t)i] = sl | (direct ? 0x40000000 : 0) | (ydirect ? 0x20000000 : 0);
        c->cdirect_frames += direct;
        c->ydirect_frames += ydirect;
        n_ydirect += ydirect;
    }
    if (ychanged) HIPCHK(hipMemcpyAsync(c->slot_y_d, c->slot_y_h, 8 * (size_t)c->n_src, hipMemcpyHostToDevice, c->st_l));
    if (changed) {
        // (the pinned mirrors are only rewritten here, and every load is followed by a host wait on this stream -- the luma
        // sums or the motion search -- before the next one: no copy of an older state is still in flight)
        HIPCHK(hipMemcpyAsync(c->slot_cu_d, c->slot_cu_h, 8 * (size_t)c->n_src, hipMemcpyHostToDevice, c->st_l));
        HIPCHK(hipMemcpyAsync(c->slot_cv_d, c->slot_cv_h, 8 * (size_t)c->n_src, hipMemcpyHostToDevice, c->st_l));
        HIPCHK(hipMemcpyAsync(c->slot_cs_d, c->slot_cs_h, 4 * (size_t)c->n_src, hipMemcpyHostToDevice, c->st_l));
    }
    HIPCHK(hipMemcpyAsync(c->ltab_d, tab.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->st_l));   // pageable: staged by the runtime
    const int k = ingest_acquire(c, yuv_dev);
    if (k == -2) { dsvg_set_error("hipStreamWaitEvent failed"); return DSVG_ERR_HIP; }
    const int rc = load_core(c, 0, n, (const uint8_t *)yuv_dev, frame_pitch, with_pyramid, c->ltab_d, n - n_direct, n_ydirect);
    return rc ? rc : ingest_release(c, k);
}
extern "C" int dsvg_load_frames_map(dsvg_ctx *c, int n, const int *slots, const void *yuv_dev, size_t frame_pitch, int with_pyramid)
{
    return dsvg_load_frames_map_ex(c, n, slots, yuv_dev, frame_pitch, with_pyramid, nullptr);
}
extern "C" long dsvg_ctx_chroma_in_place_frames(const dsvg_ctx *c) { return c ? c->cdirect_frames : 0; }
extern "C" long dsvg_ctx_luma_in_place_frames(const dsvg_ctx *c) { return c ? c->ydirect_frames : 0; }

extern "C" int dsvg_get_luma_sums(dsvg_ctx *c, int first_slot, int n, unsigned *sums_out)
{
    if (!c || !sums_out || first_slot < 0 || first_slot + n > c->n_src) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->luma_h, c->luma_sums + first_slot, sizeof(unsigned) * n, hipMemcpyDeviceToHost, c->st_l));
    HIPCHK(hipStreamSynchronize(c->st_l));
    memcpy(sums_out, c->luma_h, sizeof(unsigned) * n);
    return DSVG_OK;
}

extern "C" int dsvg_get_avg_luma(dsvg_ctx *c, int first_slot, int n, int *avg_out)
{
    if (!c || !avg_out || first_slot < 0 || first_slot + n > c->n_src) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->luma_h, c->luma_sums + first_slot, sizeof(unsigned) * n, hipMemcpyDeviceToHost, c->st_l));
    HIPCHK(hipStreamSynchronize(c->st_l));
    const FrameLayout &L = c->L[c->levels];
    for (int i = 0; i < n; i++) avg_out[i] = (int)c->luma_h[i] / (L.w[0] * L.h[0]);     // frame.c:237
    return DSVG_OK;
}

extern "C" int dsvg_analyse(dsvg_ctx *c, int npairs, const int *cur_slots, const int *ref_slots, dsvg_mv *mvs_out)
{
    if (!c || npairs < 1 || npairs > c->out_slots || !cur_slots || !ref_slots || !mvs_out) { dsvg_set_error("bad analyse arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->st_a));       // aslots_h / amv_h staging reuse
    for (int i = 0; i < npairs; i++) {
        if (cur_slots[i] < 0 || cur_slots[i] >= c->n_src || ref_slots[i] < 0 || ref_slots[i] >= c->n_src) { dsvg_set_error("slot out of range"); return DSVG_ERR_ARG; }
        c->aslots_h[i] = cur_slots[i];
        c->aslots_h[c->out_slots + i] = ref_slots[i];
    }
    HIPCHK(hipMemcpyAsync(c->slots_d, c->aslots_h, sizeof(int) * 2 * c->out_slots, hipMemcpyHostToDevice, c->st_a));
    const size_t per = (size_t)(c->levels + 1) * c->nblk;
    // (every vector a later level, k_hme_detail or the copy below reads is written by the launch of its level -- blocks beyond a
    // pyramid level's frame write their zero vector themselves: no clearing of the field, 116 MB per 320-GOP step through a slow fill)
    HmeArgs A = c->hme;
    for (int l = 0; l <= c->levels; l++) A.slab[l] = c->src[l].p;
    A.cur_slots = c->slots_d; A.ref_slots = c->slots_d + c->out_slots;
    A.slot_cu = c->slot_cu_d; A.slot_cv = c->slot_cv_d; A.slot_cs = c->slot_cs_d;
    A.slot_y = c->ydirect_ok ? c->slot_y_d : nullptr; A.deep_r = c->deep_r;
    A.mvf = c->mvf; A.aux_tex = c->aux_tex; A.aux_var = c->aux_var;
    A.csum = getenv("DSV1_NO_CHROMA_SUMS") ? nullptr : c->csum;
    tl_mark(c, c->st_a, "hme0");
    launch_hme(c->st_a, A, npairs, &c->prof);
    tl_mark(c, c->st_a, "hme1");
    for (int r = 0; r < link_repeat(); r++)
    HIPCHK(hipMemcpy2DAsync(c->amv_h, (size_t)c->nblk * sizeof(DMV), c->mvf, per * sizeof(DMV),
                            (size_t)c->nblk * sizeof(DMV), (size_t)npairs, hipMemcpyDeviceToHost, c->st_a));
    HIPCHK(hipStreamSynchronize(c->st_a));
    HIPCHK(hipGetLastError());
    memcpy(mvs_out, c->amv_h, (size_t)npairs * c->nblk * sizeof(DMV));
    return DSVG_OK;
}

// ------------------------------------------------------------------------------------------------
static void fill_job(dsvg_ctx *c, JobDev &jb, int t, int isP, int quant, int d = -1)
{
    if (d < 0) d = t;
    memset(&jb, 0, sizeof(jb));
    const CoefLayout &CL = c->CL;
    jb.xf = c->xf.p + (size_t)t * c->L[0].pitch;
    jb.pred = c->pred.p + (size_t)t * c->L[0].pitch;
    jb.coef = c->coef + (size_t)t * CL.total;
    jb.s3 = c->s3 + (size_t)t * CL.s3total;
    jb.s1 = c->s1 + (size_t)t * CL.s1total;
    jb.s5 = c->s5 + (size_t)t * CL.s5total;
    jb.mvs = c->mvs + (size_t)d * c->nblk;
    jb.stable = c->stable + (size_t)d * c->nblk;
    jb.nzpos = c->nzpos + (size_t)t * c->scan.nz_total;
    jb.nzval = c->nzval + (size_t)t * c->scan.nz_total;
    jb.chunks = c->chunks + (size_t)t * c->scan.chunks_per_job;
    jb.sym = c->sym + (size_t)t * c->scan.nz_total;
    jb.pflag = c->pflag + (size_t)t * CL.s3total;
    jb.cflag = c->cflag + (size_t)t * c->scan.chunks_per_job;
    jb.stat = c->stats_on ? c->stat : nullptr;
    jb.psum = c->psum + (size_t)t * 3;
    jb.bits = c->bits + (size_t)t * c->scan.bits_per_job;
    for (int p = 0; p < 3; p++) {
        jb.pf_off[p] = (int)CL.s3off[p];
        jb.bits_off[p] = c->scan.bits_off[p]; jb.bits_cap[p] = c->scan.bits_cap[p];
        jb.nz_off[p] = c->scan.nz_off[p]; jb.hz_coef_off[p] = CL.off[p]; jb.chunk_off[p] = c->scan.chunk_off[p];
        make_hz_plane(jb.hz[p], CL.w[p], CL.h[p], quant, isP, p, c->nbh, c->nbv);
    }
    make_hqp(jb.hqp, quant, isP);
    jb.isP = isP; jb.quant = quant;
    for (int i = 0; i < 8; i++) jb.ext[i] = DSVG_BORDER;
}

// enqueue the reconstruction half shared by encoder and decoder: inverse transform (+prediction) and
// border extension of kept reconstructions, for device jobs [0,nI) intra and [nI,n) inter
// insym: details come from the symbol planes -- bit 0: I pictures, bit 1: luma of P pictures, bit 2: chroma of P pictures
static int enqueue_recon(dsvg_ctx *c, int nI, int n, int d0 = 0, int insym = 0, hipStream_t st = nullptr, bool lazy_border = false,
                         bool tail_done = false)
{
    if (!st) st = c->st;
    const JobDev *jd = c->jobs_d + d0;
    if (!tail_done) launch_inv_plan(st, jd, c->G, 0, 3, inv_tail_plan(c->G, n, 0, 3), &c->prof);      // all planes, I and P jobs alike (encoder with llq: k_tail_q did it)
    // levels 5..4 of every plane of every job (I and P alike) in ONE launch (round 4: up to three launches less per frame step)
    static const bool no54all = getenv("DSV1_NO_INV54_ALL") != nullptr;       // (A/B)
    const int wt = no54all ? 0 : 2;
    if (wt) launch_inv54_all(st, jd, n, c->G, &c->prof);
    if (nI > 0) {
        launch_inv_sbt(st, jd, nI, c->G, 0, 1, 0, &c->prof, wt, insym & 1);
        launch_inv_sbt(st, jd, nI, c->G, 1, 2, 0, &c->prof, wt, insym & 1);
    }
    bool fused = false;
    if (n > nI) {
        const int symY = (insym >> 1) & 1, symC = (insym >> 2) & 1, pkY = symY && !c->no_patch_kernel, pkC = symC && !c->no_patch_kernel;
        // round 5: where the chroma patch kernel covers its planes completely (1080p, 4K, 720p, CIF ...) its edge patches write the borders
        // of all three planes -- k_extend16 then only serves the I pictures of the step: one launch less in the chain of every P frame step.
        // The chroma plan says so (fb), and is the one that is launched: the question is asked once
        const InvPlan pc = inv_sbt_plan(c->G, n - nI, 1, 2, 1, wt, symC, pkC, lazy_border, inv_switches());
        fused = pc.fb != 0;
        launch_inv_sbt(st, jd + nI, n - nI, c->G, 0, 1, 1, &c->prof, wt, symY, pkY);
        launch_inv_plan(st, jd + nI, c->G, 1, 2, pc, &c->prof);
    }
    if (fused && c->stats_on) {
        // what the fused border writes (counted beside the tiles: bench.py prices k_inv_patch_c with it): per plane the rows above / below over the
        // widened width and the columns left / right of the picture's own rows, by the extents border_reach left in the jobs
        for (int k = nI; k < n; k++) {
            const short *e = c->jobs_h[d0 + k].ext;
            for (int pl = 0; pl < 3; pl++) {
                const short *x = e + (pl ? 4 : 0);
                const long long w = c->L[0].w[pl ? 1 : 0], h = c->L[0].h[pl ? 1 : 0];
                c->border_bytes += (unsigned long long)((w + x[0] + x[1]) * (long long)(x[2] + x[3]) + h * (long long)(x[0] + x[1]));
            }
        }
    }
    const int next = fused ? nI : n;                    // (device order: I jobs first)
    if (next > 0) launch_extend(st, c->recon.p, c->L[0], 0, next, 3, c->slots_d + 2 * c->out_slots + d0, &c->prof, lazy_border ? jd : nullptr);
    return DSVG_OK;
}

// The launch sequence of one coding stream (group g) for frame steps [t_first, t_end) of a planned call.  The groups' sequences are
// independent of each other (different HIP streams, disjoint jobs), so for calls with many small frame steps -- where the HOST's enqueue
// rate is what the device waits for: 13 launches x 30 steps x 4 us -- each group is enqueued by a thread of its own (round 4).
static int enqueue_group(dsvg_ctx *c, const BatchPlan &P, const dsvg_rc_job *rcj, int g, int t_first, int t_end)
{
    const int base = P.base, njobs = P.njobs, NG = P.NG;
    const int *gk = P.gk;
    const bool sse = c->q[DSVG_Q_SSE].on, ssim = c->q[DSVG_Q_SSIM].on, xres = c->q[DSVG_Q_XSSE].on || c->q[DSVG_Q_XSSIM].on;
    hipStream_t st = g ? c->stx[g] : c->st;
    if (rcj && t_first == 0)       // the quantisers of the first frame step, from the state the streams' last packets left
        launch_rc(st, c->jobs_d, c->rcj_d, c->rc_state_d, base + gk[g], gk[g + 1] - gk[g], 0);
    for (int t = t_first; t < t_end; t++) {
        const int k0 = gk[g], n = gk[g + 1] - gk[g];                                // device jobs [k0, k0 + n) of the step
        const int d0 = base + t * njobs + k0;
        const int nI = std::min(std::max(P.nI[t] - k0, 0), n);                      // I jobs among them come first
        const JobDev *jd = c->jobs_d + d0;
        const FwdOpts &fq = FWD_FRAME_STEP;                                         // quantised; levels 4..5 and the tail launched once below
        if (nI > 0) {
            launch_fwd_sbt(st, jd, nI, c->G, 0, 1, 0, 1, fq, &c->prof);
            launch_fwd_sbt(st, jd, nI, c->G, 1, 2, 0, 1, fq, &c->prof);
        }
        if (n > nI) {
            const int nP = n - nI;
            const DMV *mv0 = P.mv_contig ? c->mvs + (size_t)(d0 + nI) * c->nblk : nullptr;     // (shared tables: JobDev.mvs)
            if (c->mc_fused) {
                // inter blocks are predicted inside the forward transform; k_mc only serves the intra blocks (block means)
                if (P.icnt[NG * t + g]) launch_mc(st, jd + nI, nP, c->MG, 1, &c->prof, mv0, c->ilist_d + (size_t)base * c->nblk + P.ioff[NG * t + g], P.icnt[NG * t + g]);
                const int gw = P.icnt[NG * t + g] || !P.noint[NG * t + g];      // intra blocks somewhere in these pictures (or not known)
                launch_fwd_sbt(st, jd + nI, nP, c->G, 0, 1, 1, 0, fq, &c->prof, &c->MG, mv0, gw);
                launch_fwd_sbt(st, jd + nI, nP, c->G, 1, 2, 1, 0, fq, &c->prof, &c->MG, mv0, gw);
            } else {
                launch_mc(st, jd + nI, nP, c->MG, 1, &c->prof, mv0);
                launch_fwd_sbt(st, jd + nI, nP, c->G, 0, 1, 1, 0, fq, &c->prof);
                launch_fwd_sbt(st, jd + nI, nP, c->G, 1, 2, 1, 0, fq, &c->prof);
            }
        }
        // levels >= 6 in LDS; the LL quantiser (inside the tail kernel and k_fwd_haar_mid<4> when llq, else k_hz_quant<true>);
        // then the reconstruction (P pictures: straight from the symbol planes), then the entropy stage:
        // k_hz_collect* is the LAST reader of the sparse symbol planes and clears what it reads
        launch_fwd_plan(st, jd, c->G, 0, 3, fwd_step_plan(c->G, n, c->llq), &c->prof);   // levels 4..5, tail: all planes, I and P jobs alike
        if (!c->llq) {
            launch_hz_quant(st, jd, n, c->scan.chunks_per_job, &c->prof, (double)c->CL.total, 0,
                            (c->CL.w3[0] * c->CL.h3[0] + HZ_CHUNK - 1) / HZ_CHUNK);
        }
        // (pictures nobody predicts from -- intra-only streams -- have no reconstruction to make (dsv_encoder.c:665); a group without a single kept reconstruction skips the inverse transform altogether)
        // Measured pictures all need theirs: a job without a kept slot gets it in its work frame (JobDev.xf), where the inverse
        // kernels put it; k_sse / k_ssim read it there, in stream order behind the reconstruction and before anything can overwrite it.
        // With both measurements on, k_ssim makes the SSE too: one pass over the pictures
        const bool keeps = sse || ssim || xres || P.keeps[NG * t + g];
        if (keeps) OPCHK(enqueue_recon(c, nI, n, d0, 7, st, true, c->llq));
        if (ssim) launch_ssim(st, jd, n, c->L[0], c->psum, c->q[DSVG_Q_SSIM].dev, sse ? c->q[DSVG_Q_SSE].dev : nullptr);
        else if (sse) launch_sse(st, jd, n, c->L[0], c->psum, c->q[DSVG_Q_SSE].dev);
        // (the same place and ordering argument: the reconstruction upscaled to the reference geometry, k_xres_quality)
        if (xres) launch_xres(st, jd, n, c->L[0], c->xg, c->xref_d, c->psum, c->q[DSVG_Q_XSSE].on ? c->q[DSVG_Q_XSSE].dev : nullptr, c->q[DSVG_Q_XSSIM].on ? c->q[DSVG_Q_XSSIM].dev : nullptr);
        launch_hz_pack(st, jd, n, c->scan.chunks_per_job, &c->prof, (double)c->CL.total, 0, c->no_list_pack ? -1 : nI);
        // rate control: the sizes of these packets -> the quantiser tables of the same streams' pictures of the next step
        if (rcj) launch_rc(st, c->jobs_d, c->rcj_d, c->rc_state_d, d0, n, 1);
    }
    return DSVG_OK;
}

// Enqueue nsteps frame steps of njobs pictures each (jobs[step*njobs + j]); step k+1 may use the
// reconstructions step k produces.  All host-built tables of the whole call travel in ONE set of
// host-to-device copies up front, then the kernel chains of the steps follow back to back.
// The out slots of the call must form one contiguous block (they also index the device tables).
// rcj (dsvg_code_batch_rc): the frame quantisers are chosen ON THE DEVICE by the rate control of each job's stream -- k_rc before
// the first frame step and after every step's k_hz_scan (k_rc.hip); jobs[].quant is ignored.
// Plan (plan_code_batch, dsvg_batch_plan.h: every check and every decision), commit, job records, uploads, enqueue, join.
static int code_batch_impl(dsvg_ctx *c, int nsteps, int njobs, const dsvg_pic_job *jobs, const dsvg_rc_job *rcj)
{
    if (!c) { dsvg_set_error("bad code_batch arguments"); return DSVG_ERR_ARG; }
    static const bool cprof = getenv("DSV1_HOST_PROF") != nullptr;
    const auto cnow = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; };
    const double tc0 = cprof ? cnow() : 0.0;
    BatchPlan &P = c->plan;
    {   // a refused call leaves the context as it found it: no event recorded, no call counted, no reference frame taken
        BatchGeo geo = c->bgeo;
        geo.code_streams = c->code_streams;
        const int rc = plan_code_batch(geo, batch_switches(), nsteps, njobs, jobs, rcj, c->prof.mask != 0, c->ilist_h, P);
        if (rc) { dsvg_set_error("%s", P.err); return rc; }
    }
    const int total = P.total, base = P.base, NG = P.NG;
    HIPCHK(hipSetDevice(c->device));
    const bool xres = c->q[DSVG_Q_XSSE].on || c->q[DSVG_Q_XSSIM].on;   // (dsvg_ctx_xres_enable)
    // source frames are produced on the analysis stream: make the coding stream wait for them
    HIPCHK(hipEventRecord(c->ev_a, c->st_a));
    HIPCHK(hipStreamWaitEvent(c->st, c->ev_a, 0));
    // the staging block [base, base+total) was last used when these out slots were coded before; that
    // call completed long ago if its results were fetched -- make sure anyway
    const long call = c->ncalls++;
    {
        std::vector<int> evs;                                    // the block may have been coded last by several calls
        coded_events_once(c->slot_ev.data(), c->ev_coded.size(), total, nullptr, base, evs);
        for (int e : evs) HIPCHK(hipEventSynchronize(c->ev_coded[(size_t)e]));
    }
    // what the call leaves in the context, per picture in device order: its type and whether it is measured (fetch), the reference frame
    // it takes, its reconstruction slot and the border extents written there (what dsvg_recon_border reports)
    if (c->slot_isP.size() != (size_t)c->out_slots) c->slot_isP.assign((size_t)c->out_slots, 0);
    if (c->slot_ext.size() != (size_t)c->n_recon * 8) c->slot_ext.assign((size_t)c->n_recon * 8, (short)DSVG_BORDER);
    for (int i = 0; i < total; i++) {
        const dsvg_pic_job &j = jobs[i - i % njobs + P.order[(size_t)i]];
        c->slot_isP[(size_t)j.out_slot] = (char)(j.ref_recon_slot >= 0);
        const uint8_t *xr = nullptr;
        if (xres) {
            // the reference frame dsvg_ctx_xres_refs set for the slot, taken by this call (none: the picture is not measured)
            xr = c->xref_next[(size_t)j.out_slot];
            c->xref_next[(size_t)j.out_slot] = nullptr;
            c->xref_h[j.out_slot] = xr;
        }
        for (int kind = 0; kind < DSVG_Q_KINDS; kind++) {
            dsvg_ctx::Quality &q = c->q[kind];
            if (!q.measured.empty()) q.measured[(size_t)j.out_slot] = (char)(q.on && (kind < DSVG_Q_XSSE || xr));
        }
        c->slots_h[base + i] = j.recon_slot;
        if (j.recon_slot >= 0) memcpy(&c->slot_ext[(size_t)j.recon_slot * 8], &P.ext[(size_t)i * 8], sizeof(short) * 8);
    }
    {   // the job records themselves (quantiser tables of three planes, pointers, copies of the block tables): independent per
        // job, built on the session layer's worker pool (1 920 jobs: 1.5 ms on one thread)
        struct BuildCtx { dsvg_ctx *c; const BatchPlan *P; const dsvg_pic_job *jobs; } bc = {c, &P, jobs};
        dsv1_par_for(total, [](void *vp, int idx, int) {
            BuildCtx &B = *static_cast<BuildCtx *>(vp);
            dsvg_ctx *c = B.c;
            const BatchPlan &P = *B.P;
            const int k = idx % P.njobs, d = P.base + idx;
            const dsvg_pic_job &j = B.jobs[idx - k + P.order[(size_t)idx]];
            const int isP = j.ref_recon_slot >= 0;
            JobDev &jb = c->jobs_h[d];
            fill_job(c, jb, k, isP, j.quant, d);
            jb.fused = 1;                      // quantisation fused into the forward transform (I and P pictures)
            jb.llq = c->llq ? 1 : 0;           // ... and the LL region's into the kernels that produce it
            const size_t kk = (size_t)k;
            jb.llsym = c->llsym + kk * c->scan.ll_total;
            for (int p = 0; p < 3; p++) jb.ll_off[p] = c->scan.ll_off[p];
            jb.cflag = c->cflag + kk * c->scan.chunks_per_job;
            // P pictures run sparse: zero-kept symbol planes + non-zero flags (k_hz_collect takes both down again)
            jb.nzf = isP ? c->nzf + kk * (c->scan.nz_total >> 2) : nullptr;
            if (isP) jb.sym = c->symP + kk * c->scan.nz_total;
            jb.psum = c->psum + (size_t)j.out_slot * 3;
            jb.bits = c->bits + (size_t)j.out_slot * c->scan.bits_per_job;
            jb.src = c->src[0].p + (size_t)j.src_slot * c->L[0].pitch;
            jb.srcp[0] = jb.src + c->L[0].off[0]; jb.srcs[0] = c->L[0].stride[0];
            if (c->slot_y[(size_t)j.src_slot]) { jb.srcp[0] = c->slot_y[(size_t)j.src_slot]; jb.srcs[0] = c->L[0].w[0]; }      // luma in place (round 5)
            jb.srcp[1] = c->slot_cu[(size_t)j.src_slot]; jb.srcp[2] = c->slot_cv[(size_t)j.src_slot]; jb.srcs[1] = jb.srcs[2] = c->slot_cs[(size_t)j.src_slot];
            jb.ref = isP ? c->recon.p + (size_t)j.ref_recon_slot * c->L[0].pitch : nullptr;
            jb.recon = j.recon_slot >= 0 ? c->recon.p + (size_t)j.recon_slot * c->L[0].pitch : nullptr;
            // the reconstruction goes to another slot than the reference: the prediction is written straight into it and the
            // inverse transform only touches the tiles that carry a residual (ping-pong slots, see dsv1_enc.c)
            if (isP && jb.recon && j.recon_slot != j.ref_recon_slot && !c->no_inplace_pred) jb.pred = jb.recon;
            const size_t um = (size_t)P.base + (size_t)P.mvu[(size_t)idx], us = (size_t)P.base + (size_t)P.stu[(size_t)idx];
            jb.mvs = c->mvs + um * c->nblk;
            jb.stable = c->stable + us * c->nblk;
            if (P.stcp[(size_t)idx]) memcpy(c->stable_h + us * c->nblk, j.stable_blocks, (size_t)c->nblk);
            if (P.mvcp[(size_t)idx]) memcpy(c->mv_h + um * c->nblk, j.mvs, (size_t)c->nblk * sizeof(DMV));
            memcpy(jb.ext, &P.ext[(size_t)idx * 8], sizeof(short) * 8);      // how far the reconstruction's border is written
        }, &bc);
    }
    if (getenv("DSV1_BORDER_DEBUG"))
        for (int t = 0; t < nsteps; t++) {
            const short *e = &P.ext[(size_t)t * njobs * 8], *r = jobs[(size_t)t * njobs + P.order[(size_t)t * njobs]].mv_reach;
            fprintf(stderr, "[dsvg border] step %d job 0: luma %d %d %d %d chroma %d %d %d %d; reach %d %d %d %d\n", t, e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7],
                    r[0], r[1], r[2], r[3]);
        }
    if (rcj) {
        // the rate-control table of every device job: its stream's state, the bytes in front of the quantiser field, and the
        // device job of the stream's next picture (same caller position in the next frame step)
        for (int i = 0; i < total; i++) {
            RcJobDev &r = c->rcj_h[base + i];
            const dsvg_rc_job &q = rcj[i - i % njobs + P.order[(size_t)i]];
            r.slot = q.rc_slot; r.prefix_len = q.prefix_len; r.forced_intra = q.forced_intra;
            r.next = P.rc_next[(size_t)i];
        }
        HIPCHK(hipMemcpyAsync(c->rcj_d + base, c->rcj_h + base, sizeof(RcJobDev) * total, hipMemcpyHostToDevice, c->st));
    }
    const double tc1 = cprof ? cnow() : 0.0;
    tl_mark(c, c->st, "tab0");
    if (P.iln) HIPCHK(hipMemcpyAsync(c->ilist_d + (size_t)base * c->nblk, c->ilist_h + (size_t)base * c->nblk, sizeof(int) * (size_t)P.iln, hipMemcpyHostToDevice, c->st));
    for (int r = 0; r < link_repeat(); r++) {
    HIPCHK(hipMemcpyAsync(c->jobs_d + base, c->jobs_h + base, sizeof(JobDev) * total, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->stable + (size_t)base * c->nblk, c->stable_h + (size_t)base * c->nblk, (size_t)c->nblk * P.nst, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->mvs + (size_t)base * c->nblk, c->mv_h + (size_t)base * c->nblk, (size_t)c->nblk * P.nmv * sizeof(DMV), hipMemcpyHostToDevice, c->st));
    }
    HIPCHK(hipMemcpyAsync(c->slots_d + 2 * c->out_slots + base, c->slots_h + base, sizeof(int) * total, hipMemcpyHostToDevice, c->st));
    // the measurements' sums of the call's out slots start at zero (k_sse / k_ssim add into them); before the fork: every coding stream is behind it
    for (int kind = 0; kind < DSVG_Q_KINDS; kind++) {
        // (the reference frames of the call's out slots go up between the two pairs of kinds, where they always did)
        if (kind == DSVG_Q_XSSE && xres) HIPCHK(hipMemcpyAsync(c->xref_d + base, c->xref_h + base, sizeof(const uint8_t *) * total, hipMemcpyHostToDevice, c->st));
        if (c->q[kind].on) HIPCHK(hipMemsetAsync(c->q[kind].dev + (size_t)3 * base, 0, sizeof(unsigned long long) * 3 * (size_t)total, c->st));
    }
    tl_mark(c, c->st, "code0");
    if (NG > 1) {
        if (!c->ev_fork) HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_fork, c->st));            // tables uploaded, source frames ready (st waited for ev_a)
        for (int g = 1; g < NG; g++) {
            if (!c->stx[g]) {
                HIPCHK(hipStreamCreateWithFlags(&c->stx[g], hipStreamNonBlocking));
                HIPCHK(hipEventCreateWithFlags(&c->ev_join[g], hipEventDisableTiming));
            }
            HIPCHK(hipStreamWaitEvent(c->stx[g], c->ev_fork, 0));
        }
    }
    if (P.par_enqueue) {
        // (HIP's last error and this library's error text are per THREAD: each worker checks its own launches and hands its text over)
        struct PE { dsvg_ctx *c; const BatchPlan *P; const dsvg_rc_job *rcj; int rc[DSVG_MAX_CODE_STREAMS]; char msg[DSVG_MAX_CODE_STREAMS][256]; } pe = {c, &P, rcj, {0}, {{0}}};
        dsv1_par_for_long(NG, [](void *vp, int g, int) {
            PE &E = *static_cast<PE *>(vp);
            if (hipSetDevice(E.c->device) != hipSuccess) { E.rc[g] = DSVG_ERR_HIP; snprintf(E.msg[g], sizeof E.msg[g], "hipSetDevice failed on an enqueue thread"); return; }      // (the current device is per thread)
            (void)hipGetLastError();
            E.rc[g] = enqueue_group(E.c, *E.P, E.rcj, g, 0, E.P->nsteps);
            const hipError_t e = hipGetLastError();
            if (E.rc[g]) snprintf(E.msg[g], sizeof E.msg[g], "%s", dsvg_last_error());
            else if (e != hipSuccess) { E.rc[g] = DSVG_ERR_HIP; snprintf(E.msg[g], sizeof E.msg[g], "launch failed on coding stream %d: %s", g, hipGetErrorString(e)); }
        }, &pe);
        for (int g = 0; g < NG; g++) if (pe.rc[g]) { dsvg_set_error("%s", pe.msg[g]); return pe.rc[g]; }
    } else {
        for (int t = 0; t < nsteps; t++)
            for (int g = 0; g < NG; g++) OPCHK(enqueue_group(c, P, rcj, g, t, t + 1));
    }
    if (NG > 1) { tl_mark(c, c->st, "code1a"); tl_mark(c, c->stx[1], "code1b"); }
    for (int g = 1; g < NG; g++) {
        HIPCHK(hipEventRecord(c->ev_join[g], c->stx[g]));
        HIPCHK(hipStreamWaitEvent(c->st, c->ev_join[g], 0));
    }
    tl_mark(c, c->st, "code1");
    if (cprof) fprintf(stderr, "[dsvg code_batch] %d jobs: tables %.2f ms, uploads + %d frame steps of launches %.2f ms\n", total, tc1 - tc0, nsteps, cnow() - tc1);
    {   // completion marker of this call; fetch waits on it from its own stream
        const int e = (int)(call % (long)c->ev_coded.size());
        HIPCHK(hipEventRecord(c->ev_coded[e], c->st));
        for (int i = 0; i < total; i++) c->slot_ev[base + i] = e;
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

// What plan_code_batch decides for a call of an encoder context created with these arguments (include/dsvg.h), without a device:
// the context's own derivation of BatchGeo on the geometry tables, with the switches the caller names instead of the environment's
extern "C" int dsvg_code_batch_plan(int width, int height, int subsamp, int n_recon_slots, int n_src_slots, int max_jobs, int out_slots, int code_streams,
                                    unsigned switches, int nsteps, int njobs, const dsvg_pic_job *jobs, const dsvg_rc_job *rc, dsvg_batch_plan *out)
{
    if (!out || n_src_slots < 1 || n_recon_slots < 1 || max_jobs < 1) { dsvg_set_error("bad code_batch_plan arguments"); return DSVG_ERR_ARG; }
    CtxGeo geo;
    int r = geom_check(width, height, subsamp, geo);
    if (r) return r;
    BatchGeo B = batch_geo(geo, n_src_slots, n_recon_slots, max_jobs, out_slots, !(switches & DSVG_BATCH_NO_MC_FUSION), !(switches & DSVG_BATCH_NO_LAZY_BORDER));
    B.code_streams = code_streams;
    const BatchSwitches sw = { (switches & DSVG_BATCH_NO_SMALL_SPLIT) != 0, (switches & DSVG_BATCH_NO_PAR_ENQUEUE) != 0 };
    std::vector<int> ilist(B.mc_fused ? (size_t)B.out_slots * B.nblk : 0);
    BatchPlan P;
    if ((r = plan_code_batch(B, sw, nsteps, njobs, jobs, rc, (switches & DSVG_BATCH_PROFILED) != 0, ilist.data(), P))) { dsvg_set_error("%s", P.err); return r; }
    const int total = P.total, nsg = nsteps * P.NG;
    out->nblk = B.nblk; out->mc_fused = B.mc_fused;
    out->base = P.base; out->total = total; out->ng = P.NG;
    static_assert(sizeof out->gk / sizeof out->gk[0] == DSVG_MAX_CODE_STREAMS + 1, "dsvg_batch_plan.gk holds every group boundary");
    for (int g = 0; g <= DSVG_MAX_CODE_STREAMS; g++) out->gk[g] = g <= P.NG ? P.gk[g] : 0;
    out->iln = P.iln; out->nmv = P.nmv; out->nst = P.nst; out->mv_contig = P.mv_contig; out->par_enqueue = P.par_enqueue;
    if (!out->nI || !out->order || !out->mvu || !out->stu || !out->mvcp || !out->stcp || !out->ext || !out->rc_next || !out->ioff || !out->icnt ||
        !out->noint || !out->keeps || !out->ilist) { dsvg_set_error("code_batch_plan: null array"); return DSVG_ERR_ARG; }
    if (out->cap_steps < nsteps || out->cap_jobs < total || out->cap_groups < nsg || out->cap_ilist < P.iln) {
        dsvg_set_error("code_batch_plan: the arrays are too small (%d steps, %d jobs, %d step groups, %d intra blocks)", nsteps, total, nsg, P.iln);
        return DSVG_ERR_ARG;
    }
    for (int t = 0; t < nsteps; t++) out->nI[t] = P.nI[t];
    for (int i = 0; i < total; i++) {
        out->order[i] = P.order[i]; out->mvu[i] = P.mvu[i]; out->stu[i] = P.stu[i]; out->mvcp[i] = P.mvcp[i]; out->stcp[i] = P.stcp[i];
        out->rc_next[i] = rc ? P.rc_next[i] : -1;
        for (int k = 0; k < 8; k++) out->ext[i * 8 + k] = P.ext[(size_t)i * 8 + k];
    }
    for (int i = 0; i < nsg; i++) { out->ioff[i] = P.ioff[i]; out->icnt[i] = P.icnt[i]; out->noint[i] = P.noint[i]; out->keeps[i] = P.keeps[i]; }
    for (int i = 0; i < P.iln; i++) out->ilist[i] = ilist[(size_t)P.base * B.nblk + i];
    return DSVG_OK;
}

extern "C" int dsvg_code_batch(dsvg_ctx *c, int nsteps, int njobs, const dsvg_pic_job *jobs) { return code_batch_impl(c, nsteps, njobs, jobs, nullptr); }
extern "C" int dsvg_code_batch_rc(dsvg_ctx *c, int nsteps, int njobs, const dsvg_pic_job *jobs, const dsvg_rc_job *rc)
{
    if (!rc) { dsvg_set_error("dsvg_code_batch_rc without rate-control jobs"); return DSVG_ERR_ARG; }
    return code_batch_impl(c, nsteps, njobs, jobs, rc);
}
extern "C" int dsvg_rc_set_params(dsvg_ctx *c, int first_slot, int n, const dsvg_rc_state *states)
{
    if (!c || !states || first_slot < 0 || n < 1 || first_slot + n > c->rc_slots) { dsvg_set_error("bad rate-control slots"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const size_t off = offsetof(dsvg_rc_state, bitrate), wid = sizeof(dsvg_rc_state) - off;
    // the tail of every record, behind the coding work already enqueued (the other coding streams join the first one at the end of
    // every call and fork from it at the start of the next)
    HIPCHK(hipMemcpy2DAsync((char *)(c->rc_state_d + first_slot) + off, sizeof(dsvg_rc_state), (const char *)states + off, sizeof(dsvg_rc_state), wid, (size_t)n,
                            hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));               // (pageable source; a parameter change is a rare event)
    return DSVG_OK;
}
extern "C" int dsvg_rc_upload(dsvg_ctx *c, int first_slot, int n, const dsvg_rc_state *states)
{
    if (!c || !states || first_slot < 0 || n < 1 || first_slot + n > c->rc_slots) { dsvg_set_error("bad rate-control slots"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    // ordered on the first coding stream like the tables of a coding call (the other coding streams fork from it after those)
    HIPCHK(hipMemcpyAsync(c->rc_state_d + first_slot, states, sizeof(dsvg_rc_state) * (size_t)n, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));               // (pageable source: the caller's array may go away)
    return DSVG_OK;
}
extern "C" int dsvg_rc_download(dsvg_ctx *c, int first_slot, int n, dsvg_rc_state *states)
{
    if (!c || !states || first_slot < 0 || n < 1 || first_slot + n > c->rc_slots) { dsvg_set_error("bad rate-control slots"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    OPCHK(dsvg_ctx_sync(c));
    HIPCHK(hipMemcpy(states, c->rc_state_d + first_slot, sizeof(dsvg_rc_state) * (size_t)n, hipMemcpyDeviceToHost));
    return DSVG_OK;
}

extern "C" int dsvg_code_pictures(dsvg_ctx *c, int njobs, const dsvg_pic_job *jobs)
{
    return dsvg_code_batch(c, 1, njobs, jobs);
}

// What the plans of a fetch read of a context (dsvg_fetch_plan.h)
static FetchGeo fetch_geo(int out_slots, const CtxScan &S)
{
    FetchGeo G = { out_slots, S.bits_per_job, {}, {} };
    for (int p = 0; p < 3; p++) { G.bits_off[p] = S.bits_off[p]; G.bits_cap[p] = S.bits_cap[p]; }
    return G;
}
// plan_fetch_layout on the plane summaries that have arrived in psum_h
static int fetch_layout(const HzPlaneSum *psum_h, const FetchGeo &G, int n, const int *out_slots, bool few, int nchunks, int align, bool has_cb, FetchLayout &L)
{
    std::vector<FetchPlaneSize> size(3 * (size_t)n);
    for (int i = 0; i < n; i++)
        for (int p = 0; p < 3; p++) {
            const HzPlaneSum &ps = psum_h[3 * (size_t)out_slots[i] + p];
            size[3 * (size_t)i + p] = { ps.total_bits, ps.overflow };
        }
    const int rc = plan_fetch_layout(G, n, out_slots, size.data(), few, nchunks, align, has_cb, L);
    if (rc) dsvg_set_error("%s", L.err);
    return rc;
}
// the caller's records: the plane summaries of the slots, the payloads where the plan put them
static void fill_pic_out(dsvg_pic_out *outs, int n, const int *out_slots, const FetchLayout &L, const HzPlaneSum *psum_h, const uint8_t *gath_h)
{
    for (int i = 0; i < n; i++) {
        const HzPlaneSum *ps = psum_h + 3 * (size_t)out_slots[i];
        dsvg_pic_out &po = outs[i];
        for (int p = 0; p < 3; p++) {
            po.dc[p] = ps[p].dc; po.nruns[p] = ps[p].nruns;
            po.nbytes[p] = L.nbytes[3 * (size_t)i + p];
            po.payload[p] = gath_h + L.pay[3 * (size_t)i + p];
        }
        po.rc_quant = ps[0].rc; po.rc_pkt_len = (uint32_t)ps[1].rc;
    }
}

// Check, wait, sizes, layout, commit, enqueue: plan_fetch_wait and plan_fetch_layout (dsvg_fetch_plan.h) decide, this walks what they say.
extern "C" int dsvg_fetch_pictures_cb(dsvg_ctx *c, int n, const int *out_slots, dsvg_pic_out *outs, int nchunks, int align, dsvg_fetch_cb cb, void *arg)
{
    if (!c || !outs) { dsvg_set_error("bad fetch_pictures arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    static const bool no_fast_fetch = getenv("DSV1_NO_FETCH_FAST") != nullptr;     // (A/B)
    const double tfw = tl_now();
    const FetchGeo G = fetch_geo(c->out_slots, c->scan);
    FetchWait W;                     // (per call, like the plan's pieces: a callback may fetch)
    FetchLayout L;
    {   // a refused call leaves the context as it found it
        const int rc = plan_fetch_wait(G, {no_fast_fetch}, n, out_slots, c->slot_ev.data(), c->slot_isP.data(), c->slot_isP.size(), c->ev_coded.size(), c->ncalls,
                                       nchunks, align, cb != nullptr, W);
        if (rc) { dsvg_set_error("%s", W.err); return rc; }
    }
    for (int e : W.events) {
        if (W.stream_wait) HIPCHK(hipStreamWaitEvent(c->st_c, c->ev_coded[(size_t)e], 0));
        else HIPCHK(hipEventSynchronize(c->ev_coded[(size_t)e]));
    }
    static const bool fprof = getenv("DSV1_HOST_PROF") != nullptr;
    const auto tnow = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; };
    const double tf0 = tnow();
    c->fetch_acc[0] += tf0 - tfw; c->fetch_n++;
    // a few pictures in ONE round trip (plan_fetch_wait says when and why); a plane that does not fit sends the call down the general path
    if (W.few) {
        OPCHK(ctx_grow(c, CM_GATH_D, W.grow, true));
        OPCHK(ctx_grow(c, CM_GATH_H, W.grow, true));
        for (int i = 0; i < n; i++) {
            const int o = out_slots[i];
            HIPCHK(hipMemcpyAsync(c->psum_h + 3 * (size_t)o, c->psum + 3 * (size_t)o, sizeof(HzPlaneSum) * 3, hipMemcpyDeviceToHost, c->st_c));
            for (int p = 0; p < 3; p++) {
                const FetchCopy &k = W.copy[3 * (size_t)i + p];
                HIPCHK(hipMemcpyAsync(c->gath_h + k.dst, c->bits + k.src, k.bytes, hipMemcpyDeviceToHost, c->st_c));
            }
        }
        HIPCHK(hipStreamSynchronize(c->st_c));
        HIPCHK(hipGetLastError());
        OPCHK(fetch_layout(c->psum_h, G, n, out_slots, true, nchunks, align, cb != nullptr, L));
        if (L.fits) {
            fill_pic_out(outs, n, out_slots, L, c->psum_h, c->gath_h);
            if (fprof) fprintf(stderr, "[dsvg fetch] %d picture(s), one round trip: %.2f ms\n", n, tnow() - tf0);
            return DSVG_OK;
        }
    }
    // 1. plane summaries (sizes)
    HIPCHK(hipMemcpyAsync(c->psum_h + 3 * (size_t)W.lo, c->psum + 3 * (size_t)W.lo, sizeof(HzPlaneSum) * 3 * (size_t)(W.hi - W.lo + 1),
                          hipMemcpyDeviceToHost, c->st_c));
    HIPCHK(hipStreamSynchronize(c->st_c));
    HIPCHK(hipGetLastError());
    const double tf1 = tnow();
    c->fetch_acc[1] += tf1 - tf0;
    // 2. compact every payload into one buffer on the device, then ONE device-to-host copy
    OPCHK(fetch_layout(c->psum_h, G, n, out_slots, false, nchunks, align, cb != nullptr, L));
    OPCHK(ctx_grow(c, CM_GATH_D, L.grow));
    OPCHK(ctx_grow(c, CM_GATH_H, L.grow));
    memcpy(c->gtab_h, L.rows.data(), sizeof(unsigned long long) * L.rows.size());
    tl_mark(c, c->st_c, "fetch0");
    HIPCHK(hipMemcpyAsync(c->gtab_d, c->gtab_h, sizeof(unsigned long long) * 9 * (size_t)n, hipMemcpyHostToDevice, c->st_c));
    launch_gather_bits(c->st_c, c->bits, c->gtab_d, 3 * n, c->gath_d);
    if (fprof) HIPCHK(hipStreamSynchronize(c->st_c));
    const double tf2 = fprof ? tnow() : 0.0;
    fill_pic_out(outs, n, out_slots, L, c->psum_h, c->gath_h);
    // 3. the copy, in pieces that end on multiples of `align` pictures: the caller's work on a piece (packet assembly) runs while
    //    the later pieces are still on the link
    while ((int)c->ev_fetch.size() < L.nchunks) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->ev_fetch.push_back(e);
    }
    for (int j = 0; j < L.nchunks; j++) {
        const FetchPiece &k = L.piece[(size_t)j];
        for (int r = 0; r < link_repeat(); r++)
        if (k.o1 > k.o0) HIPCHK(hipMemcpyAsync(c->gath_h + k.o0, c->gath_d + k.o0, k.o1 - k.o0, hipMemcpyDeviceToHost, c->st_c));
        HIPCHK(hipEventRecord(c->ev_fetch[j], c->st_c));
    }
    tl_mark(c, c->st_c, "fetch1");
    for (int j = 0; j < L.nchunks; j++) {
        HIPCHK(hipEventSynchronize(c->ev_fetch[j]));
        const FetchPiece &k = L.piece[(size_t)j];
        if (cb && k.end > k.first) cb(arg, k.first, k.end - k.first);
    }
    if (c->tl_on && c->tl.size() < 16384) c->tl.push_back({"asm_done", nullptr, tl_now()});
    c->fetch_acc[2] += tnow() - tf1; c->fetch_acc[3] += (double)L.total;
    if (fprof) fprintf(stderr, "[dsvg fetch] wait for coding + sizes %.2f ms, gather %.2f ms, D2H of %.1f MB (+ the caller's work on %d pieces) %.2f ms\n", tf1 - tf0, tf2 - tf1, L.total / 1e6, L.nchunks, tnow() - tf2);
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

// the measurements' switches and fetches, by kind: per out slot three 64-bit sums on the device, a pinned copy and whether the
// picture coded into the slot last was measured (dsvg_ctx::Quality)
static int quality_enable(dsvg_ctx *c, int kind, int on)
{
    if (!c) { dsvg_set_error("null context"); return DSVG_ERR_ARG; }
    dsvg_ctx::Quality &q = c->q[kind];
    if (on && !q.dev) {                         // (every call zeroes the sums of its out slots itself)
        HIPCHK(hipSetDevice(c->device));
        q.measured.assign((size_t)c->out_slots, 0);             // (first: sized wherever a table exists)
        OPCHK(ctx_grow(c, CM_Q_DEV0 + kind, 1));
        OPCHK(ctx_grow(c, CM_Q_HOST0 + kind, 1));
    }
    q.on = on != 0;
    return DSVG_OK;
}

static int quality_fetch(dsvg_ctx *c, int kind, const char *what, int n, const int *out_slots, void *out)
{
    if (!c || n < 0 || (n > 0 && (!out_slots || !out))) { dsvg_set_error("bad %s arguments", what); return DSVG_ERR_ARG; }
    dsvg_ctx::Quality &q = c->q[kind];
    int lo = c->out_slots, hi = -1;
    for (int i = 0; i < n; i++) {
        const int s = out_slots[i];
        if (s < 0 || s >= c->out_slots) { dsvg_set_error("%s: out slot %d out of range", what, s); return DSVG_ERR_ARG; }
        if (!q.dev || !q.host || !q.measured[(size_t)s]) {
            dsvg_set_error("%s: the picture in out slot %d was coded with the measurement off", what, s); return DSVG_ERR_ARG;
        }
        lo = std::min(lo, s); hi = std::max(hi, s);
    }
    if (n == 0) return DSVG_OK;
    HIPCHK(hipSetDevice(c->device));
    // behind the calls that coded those slots, on the fetch stream; one copy of the range they span
    std::vector<int> evs;
    coded_events_once(c->slot_ev.data(), c->ev_coded.size(), n, out_slots, 0, evs);
    for (int e : evs) HIPCHK(hipStreamWaitEvent(c->st_c, c->ev_coded[(size_t)e], 0));
    HIPCHK(hipMemcpyAsync(q.host + (size_t)3 * lo, q.dev + (size_t)3 * lo, sizeof(unsigned long long) * 3 * (size_t)(hi - lo + 1), hipMemcpyDeviceToHost, c->st_c));
    HIPCHK(hipStreamSynchronize(c->st_c));
    for (int i = 0; i < n; i++) memcpy((unsigned long long *)out + (size_t)3 * i, q.host + (size_t)3 * out_slots[i], 3 * sizeof(unsigned long long));
    return DSVG_OK;
}

extern "C" int dsvg_ctx_sse_enable(dsvg_ctx *c, int on) { return quality_enable(c, DSVG_Q_SSE, on); }
extern "C" int dsvg_ctx_ssim_enable(dsvg_ctx *c, int on) { return quality_enable(c, DSVG_Q_SSIM, on); }
extern "C" int dsvg_fetch_sse(dsvg_ctx *c, int n, const int *out_slots, uint64_t *sse_out) { return quality_fetch(c, DSVG_Q_SSE, "dsvg_fetch_sse", n, out_slots, sse_out); }
extern "C" int dsvg_fetch_ssim(dsvg_ctx *c, int n, const int *out_slots, int64_t *ssim_out) { return quality_fetch(c, DSVG_Q_SSIM, "dsvg_fetch_ssim", n, out_slots, ssim_out); }
extern "C" int dsvg_fetch_xres_sse(dsvg_ctx *c, int n, const int *out_slots, uint64_t *sse_out) { return quality_fetch(c, DSVG_Q_XSSE, "dsvg_fetch_xres_sse", n, out_slots, sse_out); }
extern "C" int dsvg_fetch_xres_ssim(dsvg_ctx *c, int n, const int *out_slots, int64_t *ssim_out) { return quality_fetch(c, DSVG_Q_XSSIM, "dsvg_fetch_xres_ssim", n, out_slots, ssim_out); }

extern "C" int dsvg_fetch_quality(dsvg_ctx *c, int kind, int n, const int *out_slots, uint64_t *out)
{
    if (kind < 0 || kind >= DSVG_Q_KINDS) { dsvg_set_error("dsvg_fetch_quality: bad kind %d", kind); return DSVG_ERR_ARG; }
    return quality_fetch(c, kind, "dsvg_fetch_quality", n, out_slots, out);
}

extern "C" int dsvg_ctx_xres_enable(dsvg_ctx *c, int sse_on, int ssim_on, int ref_w, int ref_h, int filter)
{
    if (!c) { dsvg_set_error("null context"); return DSVG_ERR_ARG; }
    if (!sse_on && !ssim_on) { c->q[DSVG_Q_XSSE].on = c->q[DSVG_Q_XSSIM].on = false; return DSVG_OK; }     // (the tables stay for the next switch-on)
    if (filter != 0 && filter != 1) { dsvg_set_error("dsvg_ctx_xres_enable: bad filter %d", filter); return DSVG_ERR_ARG; }
    if (ref_w < 1 || ref_h < 1) { dsvg_set_error("dsvg_ctx_xres_enable: bad reference geometry"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    if (!c->xg.planes_d || c->xg.rw != ref_w || c->xg.rh != ref_h || c->xg.filter != filter) {
        HIPCHK(hipDeviceSynchronize());             // (no call in flight may still read the tables being replaced)
        OPCHK(xres_geo_build(c->xg, c->L[0], ref_w, ref_h, filter));
        c->xref_next.assign((size_t)c->out_slots, nullptr);                 // (frames of another geometry: set them again)
    }
    if (!c->xref_d) {
        OPCHK(ctx_grow(c, CM_XREF_D, 1));
        OPCHK(ctx_grow(c, CM_XREF_H, 1));
        c->xref_next.assign((size_t)c->out_slots, nullptr);
    }
    OPCHK(quality_enable(c, DSVG_Q_XSSE, sse_on));
    return quality_enable(c, DSVG_Q_XSSIM, ssim_on);
}

extern "C" int dsvg_ctx_xres_refs(dsvg_ctx *c, const void *ref_clip, int n, const int *out_slots, const int *frames)
{
    if (!c || n < 0 || (n > 0 && (!out_slots || !frames))) { dsvg_set_error("bad dsvg_ctx_xres_refs arguments"); return DSVG_ERR_ARG; }
    if (!c->xg.planes_d) { dsvg_set_error("dsvg_ctx_xres_refs: the measurement was never switched on"); return DSVG_ERR_ARG; }
    for (int i = 0; i < n; i++)
        if (out_slots[i] < 0 || out_slots[i] >= c->out_slots || frames[i] < 0) { dsvg_set_error("dsvg_ctx_xres_refs: entry %d out of range", i); return DSVG_ERR_ARG; }
    for (int i = 0; i < n; i++)
        c->xref_next[(size_t)out_slots[i]] = ref_clip ? (const uint8_t *)ref_clip + (size_t)frames[i] * c->xg.rfb : nullptr;
    return DSVG_OK;
}

extern "C" int dsvg_fetch_pictures(dsvg_ctx *c, int n, const int *out_slots, dsvg_pic_out *outs)
{
    return dsvg_fetch_pictures_cb(c, n, out_slots, outs, 1, 1, nullptr, nullptr);
}

// What the two plans decide for a fetch (include/dsvg.h), without a device or a context: the call's own sequence -- the wait plan, the
// layout of the path it chose, and the general layout behind a one-round-trip path whose planes do not fit
extern "C" int dsvg_fetch_plan(int ctx_out_slots, int n, const int *out_slots, const int *slot_ev, int n_isP, const unsigned char *slot_isP, int nring,
                               long long ncalls, int has_cb, unsigned switches, const unsigned long long bits[7], const unsigned long long *total_bits,
                               const int *overflow, int nchunks, int align, dsvg_fetch_plan_out *out)
{
    if (!out || !slot_ev || ctx_out_slots < 1 || n_isP < 0 || (n_isP > 0 && !slot_isP) || nring < 1 || ncalls < 0 || !bits || !total_bits || !overflow) {
        dsvg_set_error("bad fetch_plan arguments"); return DSVG_ERR_ARG;
    }
    out->few = out->stream_wait = out->nwait = out->lo = out->hi = out->fits = out->general = out->nchunks = 0;
    out->grow_few = out->total = out->grow = 0;
    const FetchGeo G = { ctx_out_slots, (size_t)bits[0], {(size_t)bits[1], (size_t)bits[2], (size_t)bits[3]}, {(size_t)bits[4], (size_t)bits[5], (size_t)bits[6]} };
    FetchWait W;
    FetchLayout L;
    L.fits = false;
    int r = plan_fetch_wait(G, {(switches & DSVG_FETCH_NO_FAST) != 0}, n, out_slots, slot_ev, (const char *)slot_isP, (size_t)n_isP, (size_t)nring, (long)ncalls,
                            nchunks, align, has_cb != 0, W);
    if (r) { dsvg_set_error("%s", W.err); return r; }
    if (out->cap_pics < n || !out->wait || !out->copies || !out->rows || !out->nbytes || !out->pay) {
        dsvg_set_error("fetch_plan: the arrays are missing or too small (%d pictures)", n); return DSVG_ERR_ARG;
    }
    out->few = W.few; out->stream_wait = W.stream_wait; out->nwait = (int)W.events.size(); out->lo = W.lo; out->hi = W.hi; out->grow_few = W.grow;
    for (size_t i = 0; i < W.events.size(); i++) out->wait[i] = W.events[i];
    for (size_t k = 0; k < W.copy.size(); k++) { out->copies[3 * k] = W.copy[k].src; out->copies[3 * k + 1] = W.copy[k].dst; out->copies[3 * k + 2] = W.copy[k].bytes; }
    std::vector<FetchPlaneSize> size(3 * (size_t)n);
    for (size_t k = 0; k < size.size(); k++) size[k] = { total_bits[k], overflow[k] };
    if (W.few) {
        if ((r = plan_fetch_layout(G, n, out_slots, size.data(), true, nchunks, align, has_cb != 0, L))) { dsvg_set_error("%s", L.err); return r; }
        out->fits = L.fits;
    }
    if (!L.fits) {
        if ((r = plan_fetch_layout(G, n, out_slots, size.data(), false, nchunks, align, has_cb != 0, L))) { dsvg_set_error("%s", L.err); return r; }
        if (out->cap_pieces < L.nchunks || !out->piece || !out->piece_bytes) {
            dsvg_set_error("fetch_plan: the piece arrays are missing or too small (%d pieces)", L.nchunks); return DSVG_ERR_ARG;
        }
        out->general = 1; out->total = L.total; out->grow = L.grow; out->nchunks = L.nchunks;
        for (size_t k = 0; k < L.rows.size(); k++) out->rows[k] = L.rows[k];
        for (int j = 0; j < L.nchunks; j++) {
            const FetchPiece &k = L.piece[(size_t)j];
            out->piece[2 * j] = k.first; out->piece[2 * j + 1] = k.end; out->piece_bytes[2 * j] = k.o0; out->piece_bytes[2 * j + 1] = k.o1;
        }
    }
    for (size_t k = 0; k < 3 * (size_t)n; k++) { out->nbytes[k] = L.nbytes[k]; out->pay[k] = L.pay[k]; }
    return DSVG_OK;
}



// the frame a reader of decoded pictures takes for a slot: the slot's reconstruction, or the overlay's scratch copy of it (ask after dec_resolve)
static uint8_t *shown_frame(const dsvg_ctx *c, int slot)
{
    return c->draw_any && c->draw_at[(size_t)slot] >= 0 ? c->draw_scratch + (size_t)c->draw_at[(size_t)slot] * c->L[0].pitch : c->recon.p + (size_t)slot * c->L[0].pitch;
}

extern "C" int dsvg_ctx_draw_info(dsvg_ctx *c, int mode)
{
    if (!c || mode < 0) { dsvg_set_error("bad draw_info mode"); return DSVG_ERR_ARG; }
    c->draw_mode = mode;
    return DSVG_OK;
}

extern "C" int dsvg_ctx_output_scale(dsvg_ctx *c, int out_w, int out_h, int filter)
{
    if (!c) { dsvg_set_error("null context"); return DSVG_ERR_ARG; }
    if (out_w == 0 && out_h == 0) {
        if (c->osc_on) { OPCHK(dec_resolve(c)); c->osc_on = false; }       // (the tables stay for the next switch-on)
        return DSVG_OK;
    }
    if (filter != 0 && filter != 1) { dsvg_set_error("dsvg_ctx_output_scale: bad filter %d", filter); return DSVG_ERR_ARG; }
    if (out_w < 1 || out_h < 1) { dsvg_set_error("dsvg_ctx_output_scale: bad size %dx%d", out_w, out_h); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    OPCHK(dec_resolve(c));                               // a recorded pass is replayed, if at all, under the setting it was made with
    if (!c->osc.planes_d || c->osc_w != out_w || c->osc_h != out_h || c->osc_filter != filter) {
        HIPCHK(hipDeviceSynchronize());                 // (no pass in flight may still read the tables or the scratch being replaced)
        OPCHK(scale_geo_build(c->osc, c->L[0], c->fmt, out_w, out_h, filter));   // (refused: the setting in force stays)
        ctx_release(c, CM_OSC_SCRATCH);
        ctx_fields(c);
        c->osc_w = out_w; c->osc_h = out_h; c->osc_filter = filter;
        c->osc_fb = (c->osc.dfb + 255) & ~(size_t)255;
    }
    c->osc_on = true;
    return DSVG_OK;
}

extern "C" int dsvg_download_recon(dsvg_ctx *c, int recon_slot, uint8_t *yuv_out)
{
    if (!c || !yuv_out || recon_slot < 0 || recon_slot >= c->n_recon) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    OPCHK(dec_resolve(c));
    const size_t fb = (size_t)c->L[0].w[0] * c->L[0].h[0] + 2 * (size_t)c->L[0].w[1] * c->L[0].h[1];
    OPCHK(ctx_grow(c, CM_YUV_STAGE, fb));
    launch_pack(c->st, c->yuv_stage, shown_frame(c, recon_slot), c->L[0]);
    HIPCHK(hipMemcpyAsync(yuv_out, c->yuv_stage, fb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return DSVG_OK;
}

extern "C" int dsvg_extend_recon(dsvg_ctx *c, int recon_slot)
{
    if (!c || recon_slot < 0 || recon_slot >= c->n_recon) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    launch_extend(c->st, c->recon.p, c->L[0], recon_slot, 1, 3, nullptr, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

extern "C" int dsvg_recon_border(dsvg_ctx *c, int recon_slot, short *ext_out)
{
    if (!c || !ext_out || recon_slot < 0 || recon_slot >= c->n_recon) return DSVG_ERR_ARG;
    for (int i = 0; i < 8; i++) ext_out[i] = c->slot_ext.size() == (size_t)c->n_recon * 8 ? c->slot_ext[(size_t)recon_slot * 8 + i] : (short)DSVG_BORDER;
    return DSVG_OK;
}

extern "C" int dsvg_host_free_on(int device, void *hptr)
{
    if (!hptr) return DSVG_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipHostFree(hptr));
    return DSVG_OK;
}
extern "C" int dsvg_download_recon_frame(dsvg_ctx *c, int recon_slot, void *raw_out, size_t bytes)
{
    if (!c || !raw_out || recon_slot < 0 || recon_slot >= c->n_recon || bytes > c->L[0].bytes) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    OPCHK(dec_resolve(c));                               // (a flagged call is decoded again from int32 coefficients first)
    HIPCHK(hipMemcpyAsync(raw_out, shown_frame(c, recon_slot), bytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return DSVG_OK;
}
extern "C" int dsvg_download_recon_asis(dsvg_ctx *c, int recon_slot, uint8_t *raw_out, size_t bytes)
{
    if (!c || !raw_out || recon_slot < 0 || recon_slot >= c->n_recon || bytes > c->L[0].bytes) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    OPCHK(dec_resolve(c));
    OPCHK(dsvg_ctx_sync(c));
    HIPCHK(hipMemcpy(raw_out, c->recon.p + (size_t)recon_slot * c->L[0].pitch, bytes, hipMemcpyDeviceToHost));
    return DSVG_OK;
}

extern "C" int dsvg_upload_recon_raw(dsvg_ctx *c, int recon_slot, const uint8_t *raw, size_t bytes)
{
    if (!c || !raw || recon_slot < 0 || recon_slot >= c->n_recon || bytes > c->L[0].bytes) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    OPCHK(dsvg_ctx_sync(c));
    HIPCHK(hipMemcpy(c->recon.p + (size_t)recon_slot * c->L[0].pitch, raw, bytes, hipMemcpyHostToDevice));
    return DSVG_OK;
}

extern "C" int dsvg_download_recon_raw(dsvg_ctx *c, int recon_slot, uint8_t *raw_out, size_t bytes)
{
    if (!c || !raw_out || recon_slot < 0 || recon_slot >= c->n_recon || bytes > c->L[0].bytes) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    OPCHK(dec_resolve(c));
    OPCHK(dsvg_ctx_sync(c));
    OPCHK(dsvg_extend_recon(c, recon_slot));            // the encoder writes only the part of the border that is read
    OPCHK(dsvg_ctx_sync(c));
    HIPCHK(hipMemcpy(raw_out, c->recon.p + (size_t)recon_slot * c->L[0].pitch, bytes, hipMemcpyDeviceToHost));
    return DSVG_OK;
}

// a source slot's allocation at one pyramid level, as the loads enqueued so far leave it (tests): waits for the load stream alone
extern "C" int dsvg_download_source_raw(dsvg_ctx *c, int src_slot, int level, uint8_t *raw_out, size_t bytes)
{
    if (!c || !raw_out || src_slot < 0 || src_slot >= c->n_src || level < 0 || level > c->levels || bytes > c->L[level].bytes) return DSVG_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->st_l));
    HIPCHK(hipMemcpy(raw_out, c->src[level].p + (size_t)src_slot * c->L[level].pitch, bytes, hipMemcpyDeviceToHost));
    return DSVG_OK;
}

// The output pass of decoded pictures: n reconstruction slots to frames of `out`, in the context's packed planar frames (fmt == nullptr,
// k_pack_n: frame i at position i) or in an output format (k_pixout: frame i at position index[i]; index == nullptr: i).  Device
// output is written optimistically and recorded while the decoder call's escape flags are not back (dsvg_ctx::DecPending); host
// output settles the call first, since it synchronises anyway.  With an output scale set (dsvg_ctx_output_scale) the pictures are
// resampled on the way (k_scale_slots): packed planar frames of the scaled geometry straight into the destination, or into the
// context's scratch, which the format's pass (k_pixout, k_rgbout) then reads in place of the slots.
static int output_pass(dsvg_ctx *c, int n, const int *slots, const int *index, void *out, size_t pitch, int on_device, const dsvg_pixout *fmt)
{
    if (!c || !slots || !out || n < 1 || n > c->n_recon) { dsvg_set_error("bad %s arguments", fmt ? "export_recons" : "pack_recons"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const FrameLayout &L = c->L[0];
    const bool sc = c->osc_on;
    PoSource S;
    for (int p = 0; p < 3; p++) { S.w[p] = L.w[p]; S.h[p] = L.h[p]; S.pitch[p] = L.stride[p]; S.off[p] = (long long)L.off[p]; }
    S.fb = (long long)L.pitch;
    if (sc) {                                           // what a format reads then: the scratch's packed planar frames of the scaled geometry
        long long o = 0;
        for (int p = 0; p < 3; p++) {
            S.w[p] = p ? rsu(c->osc_w, fmt_hs(c->fmt)) : c->osc_w; S.h[p] = p ? rsu(c->osc_h, fmt_vs(c->fmt)) : c->osc_h;
            S.pitch[p] = S.w[p]; S.off[p] = o;
            o += (long long)S.w[p] * S.h[p];
        }
        S.fb = (long long)c->osc_fb;
    }
    const size_t fb = fmt ? fmt->frame_bytes : sc ? c->osc.dfb : (size_t)L.w[0] * L.h[0] + 2 * (size_t)L.w[1] * L.h[1];
    if (pitch < fb) { dsvg_set_error("output pitch smaller than a frame"); return DSVG_ERR_ARG; }
    if (fmt && pixout_check(fmt, S, pitch)) { dsvg_set_error("the output format does not fit the context's frames"); return DSVG_ERR_ARG; }
    // the table the kernel reads: the slots (k_pack_n), or (slot, output frame) pairs (k_pixout).  Scaled: (slot, frame i) pairs for
    // k_scale_slots -- frame i of the destination, or of the scratch, which a format then reads by its own (frame i, output frame) pairs
    std::vector<int> pairs, fpairs;
    int last = 0;
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= c->n_recon) { dsvg_set_error("slot out of range"); return DSVG_ERR_ARG; }
        if (!fmt && !sc) continue;
        const int o = fmt && index ? index[i] : i;
        if (o < 0) { dsvg_set_error("negative output frame index"); return DSVG_ERR_ARG; }
        pairs.push_back(slots[i]); pairs.push_back(sc ? i : o);
        if (sc && fmt && index) { fpairs.push_back(i); fpairs.push_back(o); }
        last = std::max(last, o);
    }
    const int tw = fmt || sc ? 2 : 1;                   // ints per table entry
    const int *tab = tw == 2 ? pairs.data() : slots;
    const size_t tab_bytes = sizeof(int) * (size_t)n * tw;
    dsvg_ctx::DecPending &P = c->dec_pending;
    if (!on_device) OPCHK(dec_resolve(c));              // (a flagged decoder call is repeated first)
    else if (P.active && !P.in_redo && P.slots.empty()) {
        // the first pass over a decoder call whose flags are not back yet: repeated by dec_resolve, as it was asked for, if need be
        P.slots.assign(slots, slots + n);
        P.index.assign(index, index + (fmt && index ? n : 0));
        P.out = out; P.pitch = pitch;
        P.has_fmt = fmt != nullptr;
        if (fmt) P.fmt = *fmt;
    } else if (P.active && !P.in_redo) OPCHK(dec_resolve(c));   // a second pass over the same call: settle it now
    // debug overlay: pictures drawn on are read from their scratch frames -- the table names the scratch frame, and the pass is launched
    // once per run of entries that read the same slab (with the overlay off: one run, the table as it is)
    std::vector<int> shown;
    std::vector<char> alt((size_t)n, 0);
    if (c->draw_any) {
        shown.assign(tab, tab + (size_t)n * tw);
        for (int i = 0; i < n; i++) {
            int &e = shown[(size_t)i * tw];
            if (c->draw_at[(size_t)e] >= 0) { e = c->draw_at[(size_t)e]; alt[(size_t)i] = 1; }
        }
        tab = shown.data();
    }
    OPCHK(ctx_grow(c, CM_OTAB_D, 1));
    if (sc && fmt) OPCHK(ctx_grow(c, CM_OSC_SCRATCH, c->osc_fb * (size_t)c->n_recon));
    if (!fpairs.empty()) OPCHK(ctx_grow(c, CM_OSC_TAB_D, 1));
    // One pass at a time: the first coding stream waits for the pass before, which keeps the passes in order and the table whole.
    // Round 5: device output of four pictures or more goes to the second coding stream -- beside the next call's entropy decoding, which
    // touches neither the reconstructions nor the caller's frames (70 us of a 620 us step of 64 pictures).  Whatever rewrites a
    // reconstruction slot next waits for the pass (dsvg_decode_pictures, in front of its inverse transform); dsvg_ctx_sync waits for
    // every stream.
    OPCHK(join_pack(c));
    static const bool one_stream = getenv("DSV1_DEC_ONE_STREAM") != nullptr;      // (A/B)
    hipStream_t st = c->st;
    if (on_device && !one_stream && n >= 4 && !P.in_redo && !c->prof.mask && c->stx[1]) {
        for (int i = 0; i < 2; i++) if (!c->ev_pack[i]) HIPCHK(hipEventCreateWithFlags(&c->ev_pack[i], hipEventDisableTiming));
        st = c->stx[1];
        HIPCHK(hipEventRecord(c->ev_pack[0], c->st));
        HIPCHK(hipStreamWaitEvent(st, c->ev_pack[0], 0));
    }
    HIPCHK(hipMemcpyAsync(c->otab_d, tab, tab_bytes, hipMemcpyHostToDevice, st));   // pageable: staged by the runtime
    if (!fpairs.empty()) HIPCHK(hipMemcpyAsync(c->osc_tab_d, fpairs.data(), sizeof(int) * fpairs.size(), hipMemcpyHostToDevice, st));
    uint8_t *dst = (uint8_t *)out;
    size_t dpitch = pitch, span = 0;
    if (!on_device) {
        // Host output goes through the stage.  Packed planar: frames at a 256-aligned pitch.  A format: the stage mirrors the caller's
        // buffer, frame for frame at `pitch`; dense frames (no padding in or between them, every one written) come back with one copy,
        // else the buffer goes up first, so that the copy back returns what the pass left alone
        if (!fmt) dpitch = (fb + 255) & ~(size_t)255;
        span = fmt ? pitch * (size_t)last + fmt->planes_bytes : dpitch * (size_t)n;
        OPCHK(ctx_grow(c, CM_YUV_STAGE, span));
        dst = c->yuv_stage;
        bool dense = fmt && !index && fmt->planes_bytes == pitch;
        for (int s = 0; dense && s < fmt->nseg; s++) {
            const dsvg_pixout_seg &G = fmt->seg[s];
            const size_t end = s + 1 < fmt->nseg ? fmt->seg[s + 1].off : fmt->planes_bytes;
            dense = G.off + G.pitch * (size_t)G.rows == end && (s ? true : G.off == 0) && (G.kind == DSVG_PIXOUT_PLAIN || G.kind == DSVG_PIXOUT_PAIR) &&
                    G.pitch == (size_t)G.width * (fmt->wide ? 2 : 1) * (size_t)G.nin;
        }
        if (fmt && !dense) HIPCHK(hipMemcpyAsync(dst, out, span, hipMemcpyHostToDevice, st));
    }
    for (int i0 = 0, i1; i0 < n; i0 = i1) {
        for (i1 = i0 + 1; i1 < n && alt[(size_t)i1] == alt[(size_t)i0]; i1++) ;
        const uint8_t *slab = alt[(size_t)i0] ? c->draw_scratch : c->recon.p;
        if (sc) launch_scale_slots(st, c->osc, slab, L.pitch, c->otab_d + 2 * (size_t)i0, i1 - i0, fmt ? c->osc_scratch : dst, fmt ? c->osc_fb : dpitch, &c->prof);
        else if (fmt) OPCHK(launch_pixout(st, fmt, S, slab, c->otab_d + 2 * (size_t)i0, i1 - i0, dst, dpitch, &c->prof));
        else launch_pack_n(st, dst + (size_t)i0 * dpitch, dpitch, slab, L, c->otab_d + i0, i1 - i0, &c->prof);
    }
    if (sc && fmt) OPCHK(launch_pixout(st, fmt, S, c->osc_scratch, fpairs.empty() ? nullptr : c->osc_tab_d, n, dst, dpitch, &c->prof));
    if (st != c->st) { HIPCHK(hipEventRecord(c->ev_pack[1], st)); c->pack_pending = true; }
    if (!on_device) {
        if (fmt) HIPCHK(hipMemcpyAsync(out, dst, span, hipMemcpyDeviceToHost, st));
        else if (pitch == dpitch) HIPCHK(hipMemcpyAsync(out, dst, dpitch * (size_t)(n - 1) + fb, hipMemcpyDeviceToHost, st));
        else HIPCHK(hipMemcpy2DAsync(out, pitch, dst, dpitch, fb, (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

extern "C" int dsvg_pack_recons(dsvg_ctx *c, int n, const int *recon_slots, void *yuv_out, size_t out_pitch, int out_on_device)
{
    return output_pass(c, n, recon_slots, nullptr, yuv_out, out_pitch, out_on_device, nullptr);
}

extern "C" int dsvg_export_recons(dsvg_ctx *c, int n, const int *recon_slots, const int *out_index, void *out, size_t out_pitch, int out_on_device,
                                  const dsvg_pixout *fmt)
{
    if (!fmt) { dsvg_set_error("bad export_recons arguments"); return DSVG_ERR_ARG; }
    return output_pass(c, n, recon_slots, out_index, out, out_pitch, out_on_device, fmt);
}

// ------------------------------------------------------------------------------------------------
static int dec_plan(dsvg_ctx *c, DecPlan &P, int njobs, const dsvg_dec_job *jobs, bool force32);
static int decode_impl(dsvg_ctx *c, const DecPlan &P, const dsvg_dec_job *jobs);

// look at the flags of the last decoder call (see dsvg_ctx::dec_pending); decode it again on the int32 path if it asks for it
static int dec_resolve(dsvg_ctx *c)
{
    dsvg_ctx::DecPending &P = c->dec_pending;
    if (!P.active || P.in_redo) return DSVG_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_flag[P.parity]));
    P.active = false;
    int any = 0;
    for (int t = 0; t < P.njobs; t++) any |= c->dec_flag_h[(size_t)P.parity * c->max_jobs + t];
    if (!any) return DSVG_OK;
    static const bool verbose = getenv("DSV1_DEC_VERBOSE") != nullptr;
    if (verbose) fprintf(stderr, "[dsvg decode] flags %#x: the call's %d picture(s) are decoded again from int32 coefficients\n", any, P.njobs);
    P.in_redo = true;
    c->dec_redone++;
    std::vector<dsvg_dec_job> jobs = P.jobs;             // (decode_impl overwrites the pending record)
    const std::vector<int> slots = P.slots, index = P.index;
    void *out = P.out; const size_t pitch = P.pitch;
    const bool has_fmt = P.has_fmt; const dsvg_pixout fmt = P.fmt;
    DecPlan R;                                           // (the context's plan holds the call that waits behind this repeat)
    int rc = dec_plan(c, R, (int)jobs.size(), jobs.data(), true);
    if (!rc) rc = decode_impl(c, R, jobs.data());
    if (!rc && !slots.empty()) rc = output_pass(c, (int)slots.size(), slots.data(), index.empty() ? nullptr : index.data(), out, pitch, 1, has_fmt ? &fmt : nullptr);
    P.in_redo = false;
    P.active = false;
    return rc;
}

extern "C" long dsvg_ctx_decoder_redone(const dsvg_ctx *c) { return c ? c->dec_redone : 0; }

extern "C" int dsvg_decode_pictures(dsvg_ctx *c, int njobs, const dsvg_dec_job *jobs)
{
    if (!c) { dsvg_set_error("bad decode_pictures arguments"); return DSVG_ERR_ARG; }
    // A P picture that updates its reference in place (recon_slot == ref_recon_slot) can be decoded only once: the second pass of a
    // flagged call would predict from what the first pass wrote.  A call with such a picture takes the int32 path, which raises no
    // flag, from the start (the plan's force32, as the second pass itself asks for it).
    bool once = false;
    if (jobs && njobs >= 1 && njobs <= c->max_jobs)
        for (int i = 0; i < njobs; i++) once = once || (jobs[i].ref_recon_slot >= 0 && jobs[i].recon_slot == jobs[i].ref_recon_slot);
    // a refused call leaves the context as it found it: the call before is not settled, no parity flipped, no staging written
    OPCHK(dec_plan(c, c->dec_plan, njobs, jobs, once));
    OPCHK(dec_resolve(c));                               // the call before may have to be decoded again first (its pictures are references)
    return decode_impl(c, c->dec_plan, jobs);
}

// the A/B switches of a decoder call: the context's own, read at its creation, and the process's, read once
static DecSwitches dec_switches(const dsvg_ctx *c)
{
    static const bool one_stream = getenv("DSV1_DEC_ONE_STREAM") != nullptr, no_mc_patch = getenv("DSV1_NO_MC_PATCH") != nullptr;
    return { c->no_dec_sym, c->no_dec_sym_I, one_stream, no_mc_patch, c->no_inplace_pred };
}

// the plan of a call of this context (plan_decode, dsvg_dec_plan.h: every check and every decision)
static int dec_plan(dsvg_ctx *c, DecPlan &P, int njobs, const dsvg_dec_job *jobs, bool force32)
{
    DecGeo geo = c->dgeo;
    geo.second_stream = c->stx[1] && c->ev_join[1];
    const int rc = plan_decode(geo, dec_switches(c), njobs, jobs, force32, c->prof.mask != 0, c->draw_mode, P);
    if (rc) dsvg_set_error("%s", P.err);
    return rc;
}

// Commit a planned call to the context and upload it: the parity's pinned staging (job records, payloads, block tables, the pending
// record), then the six uploads.  k: the call's parity, for dec_enqueue.
static int dec_commit(dsvg_ctx *c, const DecPlan &P, const dsvg_dec_job *jobs, int &k)
{
    const int njobs = P.njobs;
    if (c->draw_any) { std::fill(c->draw_at.begin(), c->draw_at.end(), -1); c->draw_any = false; }
    // Host staging (payload blob, job / flag / vector tables) is double-buffered by call parity: a call only waits for
    // the uploads of the call before the previous one, so the caller's parsing of the next packets overlaps the device.
    k = c->dec_par;
    if (!c->ev_dec[k]) HIPCHK(hipEventCreateWithFlags(&c->ev_dec[k], hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(c->ev_dec[k]));
    c->dec_par ^= 1;
    const size_t blob = P.blob, nmeta = P.nmeta;
    OPCHK(ctx_grow(c, CM_DEC_H0 + k, blob));
    OPCHK(ctx_grow(c, CM_DEC_D0 + k, blob));
    // per 128-bit payload chunk one hand-over record between the parse kernels (device only, consumed in stream order)
    OPCHK(ctx_grow(c, CM_DEC_META, nmeta));
    const size_t hb = (size_t)k * c->max_jobs;          // this parity's part of the pinned tables
    if (!c->dec_flag_d) {
        OPCHK(ctx_grow(c, CM_DEC_FLAG_D, 1));
        OPCHK(ctx_grow(c, CM_DEC_FLAG_H, 1));
        for (int i = 0; i < 2; i++) HIPCHK(hipEventCreateWithFlags(&c->ev_flag[i], hipEventDisableTiming));
    }
    dsvg_ctx::DecPending &pend = c->dec_pending;
    const bool was_redo = pend.in_redo;
    if (!was_redo) { pend.jobs.resize((size_t)njobs); pend.slots.clear(); }
    int lim[2][16];
    dec_limits(false, lim[0]);
    dec_limits(true, lim[1]);
    for (int t = 0; t < njobs; t++) {
        const DecPlanJob &o = P.job[(size_t)t];
        const dsvg_dec_job &j = jobs[o.src];
        JobDev &jb = c->jobs_h[hb + t];
        fill_job(c, jb, t, o.isP, j.quant);
        jb.ref = o.isP ? c->recon.p + (size_t)j.ref_recon_slot * c->L[0].pitch : nullptr;
        jb.recon = c->recon.p + (size_t)j.recon_slot * c->L[0].pitch;
        jb.dec_flag = c->dec_flag_d + hb + t;
        memcpy(jb.dec_lim, lim[o.wide ? 1 : 0], sizeof jb.dec_lim);
        if (o.path != DEC_PATH_I32) jb.sym = c->symP + (size_t)t * c->scan.nz_total;
        if (o.path == DEC_PATH_SYM_P) jb.nzf = c->nzf + (size_t)t * (c->scan.nz_total >> 2);      // (marks the job as sparse for the inverse; the flags themselves are the encoder's)
        for (int p = 0; p < 3; p++) jb.dec_sym[p] = o.dec_sym[p];
        if (o.inplace) jb.pred = jb.recon;              // prediction written in place
        c->slots_h[hb + t] = j.recon_slot;
        memcpy(c->stable_h + (hb + t) * c->nblk, j.stable_blocks, (size_t)c->nblk);
        if (o.isP) memcpy(c->mv_h + (hb + t) * c->nblk, j.mvs, (size_t)c->nblk * sizeof(DMV));
        if (!was_redo) {                                // what a repetition of this call needs, out of the pinned staging (intact until the parity comes round again)
            dsvg_dec_job &sj = pend.jobs[(size_t)t];
            sj = j;
            sj.stable_blocks = c->stable_h + (hb + t) * c->nblk;
            sj.mvs = reinterpret_cast<const dsvg_mv *>(c->mv_h + (hb + t) * c->nblk);
        }
        jb.bits = c->dec_d[k];                          // the payloads of the call travel as one blob
        for (int p = 0; p < 3; p++) {
            jb.dec_dc[p] = o.dc[p];
            jb.dec_runs[p] = o.runs[p];
            jb.dec_bitpos[p] = o.bitpos[p];
            jb.dec_len[p] = o.len[p];
            jb.dec_cnt[p] = 0;
            jb.dec_meta[p] = c->dec_meta + o.moff[p];
            jb.bits_off[p] = o.boff[p];
            uint8_t *stage = c->dec_h[k] + o.boff[p];
            if (!was_redo) pend.jobs[(size_t)t].plane_data[p] = stage;
            memcpy(stage, j.plane_data[p], j.plane_len[p]);
            memset(stage + j.plane_len[p], 0, 64);
        }
    }
    HIPCHK(hipMemcpyAsync(c->dec_d[k], c->dec_h[k], blob, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->jobs_d, c->jobs_h + hb, sizeof(JobDev) * njobs, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->stable, c->stable_h + hb * c->nblk, (size_t)c->nblk * njobs, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->mvs, c->mv_h + hb * c->nblk, (size_t)c->nblk * njobs * sizeof(DMV), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->slots_d + 2 * c->out_slots, c->slots_h + hb, sizeof(int) * njobs, hipMemcpyHostToDevice, c->st));
    if (P.anysym) HIPCHK(hipMemsetAsync(c->dec_flag_d + hb, 0, sizeof(int) * (size_t)njobs, c->st));
    // (round 5, measured dead end: the six commands above as ONE kernel that reads the pinned tables in place -- 3 180-3 220 against 3 250 frames/s)
    HIPCHK(hipEventRecord(c->ev_dec[k], c->st));
    return DSVG_OK;
}

// The launches of a committed call, from its plan: clear, parse and scatter, resolve and flag copy, the fork, motion compensation, the
// join, the pack wait, the reconstruction, unscatter, overlay.
static int dec_enqueue(dsvg_ctx *c, const DecPlan &P, int k)
{
    const int njobs = P.njobs, nI = P.nI, f0 = P.f0;
    const size_t hb = (size_t)k * c->max_jobs;          // this parity's part of the pinned tables
    dsvg_ctx::DecPending &pend = c->dec_pending;
    const bool was_redo = pend.in_redo;
    launch_dec_clear(c->st, c->jobs_d, njobs);
    launch_hz_parse_scatter(c->st, c->jobs_d, njobs, 0, 3, P.max_entries, P.max_chunks, &c->prof, P.scatter_one);
    if (P.anysym) {
        // what the symbol planes cannot hold (JobDev.dec_flag): shared cells that keep the earlier region's value; symbols
        // beyond int16 were flagged by the scatter itself.  The flags travel back now and are read by dec_resolve later.
        if (P.resolve) launch_hz_dec_resolve(c->st, c->jobs_d + f0, njobs - f0, 0, 3);
        HIPCHK(hipMemcpyAsync(c->dec_flag_h + hb, c->dec_flag_d + hb, sizeof(int) * (size_t)njobs, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipEventRecord(c->ev_flag[k], c->st));
        if (!was_redo) { pend.active = true; pend.parity = k; pend.njobs = njobs; }
    } else if (!was_redo) pend.active = false;
    // Round 5: the motion compensation of a step depends on the step before (its reconstructions) and on this call's tables, not on this
    // call's entropy decoding: it runs on the second coding stream beside the parse chain (five latency-bound kernels, 160 us of a 620 us
    // step of 64 pictures) and joins in front of the inverse transform.  The fork waits for ev_dec -- recorded on the first stream behind
    // this call's uploads, i.e. behind everything of the step before -- so nothing of that step still reads the prediction frames.
    hipStream_t sm = c->st;
    if (P.fork) {
        sm = c->stx[1];
        HIPCHK(hipStreamWaitEvent(sm, c->ev_dec[k], 0));
    }
    if (P.mc != DEC_MC_NONE) {
        if (P.mc == DEC_MC_PATCH) {
            // the encoder's lean motion compensation by itself (k_mc_patch: a thread per 8x8 patch) for the inter blocks; k_mc, by
            // list (dec_intra_list), for the intra blocks and for the block columns / rows from (ex0, ey0) on, which hold ragged
            // patches in some plane (the two kernels share that predicate).  The list is the one host effect left to this stage: it
            // goes straight into the parity's pinned list HERE, behind the parse chain's launches, where the device has work while
            // the host walks the blocks (in front of the uploads the 64-picture call with host output measured 0.8 % slower)
            int *il = c->ilist_h + hb * c->nblk, iln = 0;
            for (int t = nI; t < njobs; t++)
                iln += dec_intra_list(c->dgeo, reinterpret_cast<const dsvg_mv *>(c->mv_h + (hb + t) * c->nblk), (t - nI) * c->nblk, P.ex0, P.ey0, il + iln);
            const DMV *mv0 = c->mvs + (size_t)nI * c->nblk;
            if (iln) {
                HIPCHK(hipMemcpyAsync(c->ilist_d + hb * c->nblk, il, sizeof(int) * (size_t)iln, hipMemcpyHostToDevice, sm));
                launch_mc(sm, c->jobs_d + nI, njobs - nI, c->MG, 0, &c->prof, mv0, c->ilist_d + hb * c->nblk, iln);
            }
            launch_mc_patch(sm, c->jobs_d + nI, njobs - nI, c->G, c->MG, mv0, P.ex0, P.ey0, &c->prof);
        } else launch_mc(sm, c->jobs_d + nI, njobs - nI, c->MG, 0, &c->prof);
        if (sm != c->st) {
            HIPCHK(hipEventRecord(c->ev_join[1], sm));
            HIPCHK(hipStreamWaitEvent(c->st, c->ev_join[1], 0));
        }
    }
    if (c->pack_pending) {               // the packing pass of the call before (dsvg_pack_recons) may still read the slot this call's inverse transform writes
        HIPCHK(hipStreamWaitEvent(c->st, c->ev_pack[1], 0));
        c->pack_pending = false;
    }
    OPCHK(enqueue_recon(c, nI, njobs, 0, P.insym));
    if (P.anysym) launch_hz_unscatter(c->st, c->jobs_d + f0, njobs - f0, P.max_entries);
    if (P.draw0 < P.draw1) {
        // debug overlay on the call's P pictures (jobs nI .. njobs - 1, whose tables lie in c->mvs / c->stable in that order): each is
        // copied to the scratch frame of its job and drawn on there, in stream order behind its reconstruction
        const FrameLayout &L = c->L[0];
        const int d0 = P.draw0;
        OPCHK(ctx_grow(c, CM_DRAW_SCRATCH, 1));
        if (c->draw_at.empty()) c->draw_at.assign((size_t)c->n_recon, -1);
        for (int t = d0; t < P.draw1; t++) {
            const int slot = c->slots_h[hb + t];
            HIPCHK(hipMemcpyAsync(c->draw_scratch + (size_t)t * L.pitch, c->recon.p + (size_t)slot * L.pitch, L.bytes, hipMemcpyDeviceToDevice, c->st));
            c->draw_at[(size_t)slot] = t;
        }
        c->draw_any = true;
        launch_drawinfo(c->st, c->draw_scratch + (size_t)d0 * L.pitch + L.off[0], L.pitch, L.w[0], L.h[0], L.stride[0], c->bw, c->bh, c->draw_mode,
                        c->mvs + (size_t)d0 * c->nblk, c->stable + (size_t)d0 * c->nblk, P.draw1 - d0);
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

// A planned call (dec_plan: a call it refuses never gets here): commit, uploads, enqueue.
static int decode_impl(dsvg_ctx *c, const DecPlan &P, const dsvg_dec_job *jobs)
{
    HIPCHK(hipSetDevice(c->device));
    int k = 0;
    OPCHK(dec_commit(c, P, jobs, k));
    return dec_enqueue(c, P, k);
}

// What plan_decode decides for a call of a context created with these arguments (include/dsvg.h), without a device: the context's own
// derivation of DecGeo on the geometry tables, with the switches the caller names instead of the environment's
extern "C" int dsvg_decode_plan(int width, int height, int subsamp, int n_recon_slots, int max_jobs, unsigned switches, int force32, int draw_mode,
                                int njobs, const dsvg_dec_job *jobs, dsvg_dec_plan *out)
{
    if (!out || n_recon_slots < 1 || max_jobs < 1) { dsvg_set_error("bad decode_plan arguments"); return DSVG_ERR_ARG; }
    CtxGeo geo;
    int r = geom_check(width, height, subsamp, geo);
    if (r) return r;
    DecGeo D = dec_geo(geo, n_recon_slots, max_jobs, !(switches & DSVG_DEC_NO_MC_FUSION), !(switches & DSVG_DEC_NO_SYM_OV));
    D.second_stream = max_jobs >= 16;                    // (dsvg_ctx_create_blk: throughput contexts pick their coding streams at creation)
    const DecSwitches sw = { (switches & DSVG_DEC_NO_SYM) != 0, (switches & DSVG_DEC_NO_SYM_I) != 0, (switches & DSVG_DEC_ONE_STREAM) != 0,
                             (switches & DSVG_DEC_NO_MC_PATCH) != 0, (switches & DSVG_DEC_NO_INPLACE_PRED) != 0 };
    DecPlan P;
    if ((r = plan_decode(D, sw, njobs, jobs, force32 != 0, (switches & DSVG_DEC_PROFILED) != 0, draw_mode, P))) { dsvg_set_error("%s", P.err); return r; }
    out->nblk = D.nblk; out->nbh = D.nbh; out->mc_patch = D.mc_patch; out->second_stream = D.second_stream;
    for (int g = 0; g < 2; g++) { out->sym_ok[g] = D.sym_ok[g]; out->ov[g] = D.ov[g]; }
    for (int p = 0; p < 3; p++) out->nchunks[p] = D.nchunks[p];
    dec_limits(false, out->lim[0]);
    dec_limits(true, out->lim[1]);
    out->nI = P.nI; out->blob = (long long)P.blob; out->nmeta = (long long)P.nmeta; out->max_entries = P.max_entries; out->max_chunks = P.max_chunks;
    out->insym = P.insym; out->f0 = P.f0; out->anysym = P.anysym; out->scatter_one = P.scatter_one; out->resolve = P.resolve; out->fork = P.fork;
    out->mc = P.mc; out->ex0 = P.ex0; out->ey0 = P.ey0; out->draw0 = P.draw0; out->draw1 = P.draw1;
    std::vector<int> ilist(P.mc == DEC_MC_PATCH ? (size_t)(njobs - P.nI) * D.nblk : 0);
    int iln = 0;
    for (int t = P.nI; t < njobs && P.mc == DEC_MC_PATCH; t++)
        iln += dec_intra_list(D, jobs[P.job[(size_t)t].src].mvs, (t - P.nI) * D.nblk, P.ex0, P.ey0, ilist.data() + iln);
    out->iln = iln;
    if (!out->order || !out->path || !out->dec_sym || !out->wide || !out->inplace || !out->dc || !out->runs || !out->len || !out->bitpos ||
        !out->blob_off || !out->meta_off || !out->ilist) { dsvg_set_error("decode_plan: null array"); return DSVG_ERR_ARG; }
    if (out->cap_jobs < njobs || out->cap_ilist < iln) {
        dsvg_set_error("decode_plan: the arrays are too small (%d jobs, %d listed blocks)", njobs, iln);
        return DSVG_ERR_ARG;
    }
    for (int t = 0; t < njobs; t++) {
        const DecPlanJob &o = P.job[(size_t)t];
        out->order[t] = o.src; out->path[t] = o.path; out->wide[t] = o.wide; out->inplace[t] = o.inplace;
        for (int p = 0; p < 3; p++) {
            const int i = 3 * t + p;
            out->dec_sym[i] = o.dec_sym[p]; out->dc[i] = o.dc[p]; out->runs[i] = o.runs[p]; out->len[i] = o.len[p];
            out->bitpos[i] = o.bitpos[p]; out->blob_off[i] = (long long)o.boff[p]; out->meta_off[i] = (long long)o.moff[p];
        }
    }
    for (int i = 0; i < iln; i++) out->ilist[i] = ilist[(size_t)i];
    return DSVG_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" int dsvg_prof_kernels(void) { return KID_N; }
extern "C" const char *dsvg_prof_kernel_name(int kid) { return kid_name(kid); }
extern "C" int dsvg_prof_enable(dsvg_ctx *c, unsigned long long kernel_mask)
{
    if (!c) return DSVG_ERR_ARG;
    c->prof.collect();
    c->prof.mask = kernel_mask;
    return DSVG_OK;
}
extern "C" int dsvg_prof_reset(dsvg_ctx *c) { if (!c) return DSVG_ERR_ARG; c->prof.reset(); return DSVG_OK; }
extern "C" int dsvg_prof_get(dsvg_ctx *c, int kid, double *ms, long *launches, double *alg_bytes)
{
    if (!c || kid < 0 || kid >= KID_N) return DSVG_ERR_ARG;
    c->prof.collect();
    if (ms) *ms = c->prof.ms[kid];
    if (launches) *launches = c->prof.launches[kid];
    if (alg_bytes) *alg_bytes = c->prof.bytes[kid];
    return DSVG_OK;
}
