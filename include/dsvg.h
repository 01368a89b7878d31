/*
 * dsvg.h -- C ABI of the MI355X-native DSV1 hot path (libdsv1_mi355x.so).
 *
 * Plain C, plain pointers and sizes: this is what a host written in C (the reference's own
 * language) binds.  Two seams are exported:
 *
 *   1. OPERATOR LEVEL (dsvg_op_*): one twin per function of the reference's operator API
 *      (dsv_internal.h:94-109, dsv.h:169, dsv_encoder.h:132).  Same argument meaning, host
 *      pointers in and out, results byte-identical; each call stages through HBM and runs the
 *      HIP kernels.  This is the seam the parity tests drive.
 *
 *   2. PIPELINE LEVEL (dsvg_ctx_* / dsvg_load_frames / dsvg_analyse / dsvg_code_pictures /
 *      dsvg_fetch_pictures): device-resident frames, batched over many closed GOPs, used by the
 *      session layer (dsv_enc / dsv_enc_gops in dsv1_api.h) and by bench.py.
 *
 * All functions return DSVG_OK (0) or a negative DSVG_ERR_* code; nothing here falls back to a
 * CPU implementation -- if no HIP device is usable the call fails.
 *
 * Struct layouts are ABI-identical to the reference's DSV_PLANE / DSV_COEFS / DSV_FRAME /
 * DSV_MV / DSV_PARAMS / DSV_STABILITY / DSV_BS / DSV_HME (dsv.h:86-198, dsv_internal.h:39-49,
 * dsv_encoder.h:124-130) so existing callers can pass their own structs.
 */
#ifndef DSVG_H
#define DSVG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSVG_OK               0
#define DSVG_ERR_HIP         (-1)   /* a HIP runtime call or kernel failed (see dsvg_last_error) */
#define DSVG_ERR_ARG         (-2)   /* bad argument */
#define DSVG_ERR_UNSUPPORTED (-3)   /* geometry outside what the kernels handle */
#define DSVG_ERR_OVERFLOW    (-4)   /* packed plane exceeded its output bound */
#define DSVG_ERR_NODEVICE    (-5)   /* no usable MI355X/HIP device */
#define DSVG_ERR_NOMEM       (-7)   /* a host allocation failed (the object being built is unwound) */
#define DSVG_ERR_RC          (-6)   /* device-resident rate control: the host's replay of a picture disagrees with what the device chose */

#define DSVG_FRAME_BORDER 64        /* DSV_FRAME_BORDER dsv_internal.h:37 */
#define DSVG_MAX_PYRAMID  5         /* DSV_MAX_PYRAMID_LEVELS dsv_encoder.h:35 */

typedef struct { int width, height, subsamp, fps_num, fps_den, aspect_num, aspect_den; } dsvg_meta; /* DSV_META */
typedef struct { uint8_t *data; int len, format, stride, w, h, hs, vs; } dsvg_plane;             /* DSV_PLANE */
typedef struct { int32_t *data; int width, height; } dsvg_coefs;                                 /* DSV_COEFS */
typedef struct { uint8_t *alloc; dsvg_plane planes[3]; int refcount, format, width, height, border; } dsvg_frame; /* DSV_FRAME */
typedef struct {                                                                                 /* DSV_MV */
    union { struct { int16_t x, y; } mv; int32_t all; } u;
    uint8_t mode, submask, lo_var, lo_tex, high_detail;
} dsvg_mv;
typedef struct { dsvg_meta *vidmeta; int is_ref, has_ref, blk_w, blk_h, nblocks_h, nblocks_v; } dsvg_params;     /* DSV_PARAMS */
typedef struct { dsvg_params *params; unsigned char *stable_blocks; unsigned char cur_plane, isP; } dsvg_stability; /* DSV_STABILITY */
typedef struct { uint8_t *start; unsigned pos; } dsvg_bs;                                        /* DSV_BS */
typedef struct {                                                                                 /* DSV_HME */
    dsvg_params *params;
    dsvg_frame *src[DSVG_MAX_PYRAMID + 1];
    dsvg_frame *ref[DSVG_MAX_PYRAMID + 1];
    dsvg_mv *mvf[DSVG_MAX_PYRAMID + 1];
    int levels;
} dsvg_hme;

/* ---------------------------------------------------------------------------------------------
 * library
 * ------------------------------------------------------------------------------------------- */
const char *dsvg_last_error(void);          /* thread-local description of the last failure */
int dsvg_device_count(void);                /* number of HIP devices (0 = none) */
int dsvg_set_device(int device);            /* device used by the operator-level calls (default 0) */
/* the host <-> device link as the pipeline's own copies use it: hipHostMalloc'd memory first touched by the calling thread, `reps` asynchronous
 * copies of `bytes` each way on a stream of their own, timed by HIP events.  gbs[0] = host -> device, gbs[1] = device -> host, GB/s.  A
 * diagnostic (bench.py's `link`, shard.py's choice of the NUMA node to run on): call it from a short-lived process of the affinity in question. */
int dsvg_link_probe(int device, size_t bytes, int reps, double gbs[2]);

/* ---------------------------------------------------------------------------------------------
 * 1. operator level -- twins of the reference operator API
 * ------------------------------------------------------------------------------------------- */
/* dsv_fwd_sbt  sbt.c:630   */ int dsvg_op_fwd_sbt(const dsvg_plane *src, dsvg_coefs *dst, int isP);
/* dsv_inv_sbt  sbt.c:654   */ int dsvg_op_inv_sbt(dsvg_plane *dst, dsvg_coefs *src, int q, int isP, int c);
/* dsv_encode_plane hzcc.c:449 */ int dsvg_op_encode_plane(dsvg_bs *bs, dsvg_coefs *src, int q, const dsvg_stability *stab);
/* dsv_decode_plane hzcc.c:479 */ int dsvg_op_decode_plane(uint8_t *in, unsigned len, dsvg_coefs *dst, int q, const dsvg_stability *stab);
/* dsv_sub_pred bmc.c:318   */ int dsvg_op_sub_pred(const dsvg_mv *mv, const dsvg_params *p, dsvg_frame *dif, dsvg_frame *inp, const dsvg_frame *ref);
/* dsv_add_pred bmc.c:333   */ int dsvg_op_add_pred(const dsvg_mv *mv, const dsvg_params *p, dsvg_frame *dif, dsvg_frame *out, const dsvg_frame *ref);
/* dsv_frame_add bmc.c:304  */ int dsvg_op_frame_add(dsvg_frame *dst, const dsvg_frame *src);
/* dsv_hme      hme.c:730   */ int dsvg_op_hme(dsvg_hme *hme, int *intra_pct); /* mvf[0..levels] from dsv_alloc: the caller frees them with dsv_free, as dsv_encoder.c:239-244 does */
/* dsvg_op_hme with the two arrangements a batch context gives the level-0 search (flags 0: dsvg_op_hme itself):
 *   DSVG_HME_TABLE    the chroma variance test of full blocks reads k_hme_csum's table instead of fetching the chroma blocks per block;
 *   DSVG_HME_IN_CLIP  both level-0 luma planes are also given packed (row stride = the picture's width), as a caller's clip holds them: a
 *                     block's source rows come from there unless its statistics window leaves the picture, its reference rows when it lies
 *                     (2 << levels) + 8 pixels or more from every edge.  Of the bordered copies the search may then read only the border and
 *                     a ring of a block and twice that distance in from each edge: the luma samples inside the ring are replaced by their
 *                     complement on the device, so a read from the wrong copy changes the result.  Needs width % 16 == 0, height % 4 == 0. */
#define DSVG_HME_TABLE   1u
#define DSVG_HME_IN_CLIP 2u
int dsvg_op_hme_ex(dsvg_hme *hme, int *intra_pct, unsigned flags);
/* the allocator behind memory the operator calls hand to their caller (the motion fields above).  Default (or NULLs): this library's dsv_alloc /
 * dsv_free.  A build that keeps the reference's own dsv.c passes ITS pair, so that its dsv_free -- which steps back over a 16-byte header when
 * DSV_MEMORY_STATS is on, dsv.c:41-66 -- gets blocks its dsv_alloc made (oracle/opswap_shim.c does). */
void dsvg_set_allocator(void *(*alloc_fn)(int), void (*free_fn)(void *));
/* dsv_extend_frame frame.c:263 */ int dsvg_op_extend_frame(dsvg_frame *f);
/* dsv_extend_frame_luma frame.c:297 */ int dsvg_op_extend_frame_luma(dsvg_frame *f);
/* dsv_ds2x_frame_luma frame.c:240 */ int dsvg_op_ds2x_frame_luma(dsvg_frame *dst, const dsvg_frame *src);
/* dsv_frame_avg_luma frame.c:223 */ int dsvg_op_frame_avg_luma(const dsvg_frame *f, int *avg);
/* dsv_get_quant hzcc.c:77, dsv_lb2 hzcc.c:437: host scalars */
int dsvg_get_quant(int q, int isP, int level);
int dsvg_lb2(unsigned n);
/* The rate-control kernel on its own (tests; k_rc, include/dsvg_rc.h; restated in tests/rc_model.py): ONE launch_rc(d0, count, mode)
 * over n job records built on the device from `jobs`, with the nslots states of `states` (in and out).  Every record's quantiser
 * tables, its quant word and the rc words of its three plane sums start as DSVG_OP_RC_POISON (quant: jobs[].quant, what a mode-1
 * picture was coded with); out[j] returns them as the launch left them: tables = plane-major (qp, qp_h) of the ten scan regions
 * of the three planes, then hqp[16].  mode 0: pick for jobs [d0, d0 + count); mode 1: packet size, statistics, and the pick of
 * jobs[].next (an absolute index, -1: none; may lie outside the launched range).  slot < 0: the job is skipped.  Refused
 * (DSVG_ERR_ARG) before anything runs: a range outside [0, n), a slot >= nslots, a next >= n. */
#define DSVG_OP_RC_POISON 0x5A5A5A5A
typedef struct {
    int isP, forced_intra, prefix_len, slot, next, quant;
    int dc[3];
    int pad;
    unsigned long long total_bits[3];
} dsvg_op_rc_job;
typedef struct { int quant; int tables[76]; int rc[3]; } dsvg_op_rc_out;
struct dsvg_rc_state;
int dsvg_op_rc(int n, const dsvg_op_rc_job *jobs, int nslots, struct dsvg_rc_state *states, int d0, int count, int mode, dsvg_op_rc_out *out);

/* ---------------------------------------------------------------------------------------------
 * 2. pipeline level -- device-resident, batched
 * ------------------------------------------------------------------------------------------- */
typedef struct dsvg_ctx dsvg_ctx;

typedef struct {
    int width, height, subsamp;
    int blk_w, blk_h, nblocks_h, nblocks_v;   /* dsv_encoder.c:556-595 */
    int pyramid_levels;                       /* dsv_encoder.c:602-613 (after auto) */
    size_t frame_bytes;                       /* tightly packed planar input frame */
    size_t plane_out_cap[3];                  /* capacity of one packed plane payload */
    size_t frame_alloc_bytes;                 /* one frame in the reference layout, borders included (dsvg_download_recon_raw) */
} dsvg_geom;

/* n_src_slots source frames (padded + pyramid) and n_recon_slots reconstructions stay resident;
 * max_jobs = widest batch handed to dsvg_code_pictures in one call (sizes the per-step work
 * buffers); out_slots = number of coded pictures whose packed planes stay resident until fetched
 * (>= max_jobs; a whole GOP batch = streams x frames can be enqueued without a host sync) and the
 * largest number of frame pairs one dsvg_analyse call may carry. */
int dsvg_ctx_create(dsvg_ctx **out, int device, int width, int height, int subsamp,
                    int pyramid_levels, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots);
/* the same with the block size given (0, 0 = the encoder's rule for the frame size, dsv_encoder.c:557-592): decoders take it
 * from their stream (dsv_decoder.c:335-360); multiples of 4 in 16..64 */
int dsvg_ctx_create_blk(dsvg_ctx **out, int device, int width, int height, int subsamp,
                        int pyramid_levels, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots, int blk_w, int blk_h);
void dsvg_ctx_destroy(dsvg_ctx *ctx);
int dsvg_ctx_geom(const dsvg_ctx *ctx, dsvg_geom *g);
int dsvg_ctx_sync(dsvg_ctx *ctx);
/* Coding streams: dsvg_code_batch shares the pictures of every frame step out over n HIP streams (default 2, or
 * DSV1_CODE_STREAMS), so one group's small latency-bound kernels run under another group's large ones.  n >= 1 sets
 * it (takes effect at the next batch), n = 0 only queries; returns the previous value. */
int dsvg_ctx_code_streams(dsvg_ctx *ctx, int n);
/* how many of the context's four streams (coding, analysis, second coding, fetch) were placed on hardware queues of
 * their own by the probe at creation (4 = all apart; 0 = probe switched off with DSV1_NO_STREAM_PROBE) */
int dsvg_ctx_streams_apart(const dsvg_ctx *ctx);
/* where a throughput context's host-to-device copy stream sits: 0 = a hardware queue of its own (2 / 3: as a stream of the lowest / highest
 * priority, whose queues the runtime keeps apart from the plain streams' four), 1 = it shares the analysis stream's queue, -1 = wherever the
 * runtime put it (small contexts, probe off) */
int dsvg_ctx_copy_queue(const dsvg_ctx *ctx);
/* The first coding hipStream_t (operator-style callers: dsvg_download_recon and the host-output dsvg_pack_recons run on it).  ORDERING: work put on
 * the handle after this call runs behind everything the context has enqueued so far, including a device-output packing pass that dsvg_pack_recons
 * placed on the second coding stream (round 5): the call itself makes the first stream wait for that pass.  A handle fetched BEFORE a later
 * dsvg_pack_recons says nothing about that later pass -- ask again after it (cheap), or use dsvg_ctx_join.  NULL on error. */
void *dsvg_ctx_stream(dsvg_ctx *ctx);
/* make `stream` (a hipStream_t of the caller's on the context's device; NULL or the first coding stream itself: only the join below) wait for
 * everything the context has enqueued so far on its first coding stream and for a pending device-output packing pass: what a consumer of
 * dsvg_pack_recons(.., out_on_device=1) calls before it reads yuv_out in stream order, without a whole-context dsvg_ctx_sync. */
int dsvg_ctx_join(dsvg_ctx *ctx, void *stream);
/* Sparse P pictures: tiles of the fused inverse transform (128x64 pixels) counted since the previous call --
 * out[0], out[1] = tiles that took the general path (luma, chroma), out[2], out[3] = tiles found empty (no detail symbol,
 * LL3 zero: reconstruction = prediction, nothing computed).  Counting is off until a call with enable != 0 and stops
 * again with enable = 0 (one atomic per tile).  Syncs the context and clears the counters.  bench.py uses it to price
 * the kernel at the bytes it really moved. */
int dsvg_ctx_tile_stats(dsvg_ctx *ctx, unsigned long long out[4], int enable);
/* the same plus what the symbol fetches of the sparse inverse amount to (round 4: bench.py prices the kernels at ALL the bytes they
 * must move): out[4] = 8x8 luma patches of computed tiles whose flag was up (their 96 bytes of level-1 symbols were fetched by
 * k_inv_p_tile), out[5] = chroma patches with a flag (k_inv_patch_c fetched their 126 bytes of symbols of the three levels),
 * out[6] = chroma patches without a flag that were still rewritten (non-zero LL3 residual, or prediction not in place: 64 bytes
 * in, 64 out), out[7] = bytes of reconstruction border written by the fused inverse kernels (round 6; tallied on the host from the jobs' extents). */
int dsvg_ctx_tile_stats2(dsvg_ctx *ctx, unsigned long long out[8], int enable);

/* device memory helpers for callers that keep the raw clip in HBM (bench.py) */
int dsvg_dev_alloc(dsvg_ctx *ctx, void **dptr, size_t bytes);
int dsvg_dev_free(dsvg_ctx *ctx, void *dptr);
int dsvg_dev_upload(dsvg_ctx *ctx, void *dptr, const void *src, size_t bytes);
int dsvg_dev_download(dsvg_ctx *ctx, void *dst, const void *dptr, size_t bytes);   /* synchronous */
/* Host-resident input (dsv_main.c:394-421 reads each frame from the .yuv into host memory).  dsvg_host_alloc gives
 * pinned memory; dsvg_ingest_begin starts the upload of `bytes` of packed frames on a copy stream of its own into one
 * of two device buffers owned by the context and returns that buffer: a following dsvg_load_frames_map on it waits for
 * the copy on the device, not on the host.  Asynchronous for pinned memory (the caller keeps yuv_host unchanged until
 * that load has run: after a dsvg_get_luma_sums / dsvg_analyse / dsvg_ctx_sync that follows it); pageable memory works
 * and is staged by the runtime inside the call.  At most two ingests may be outstanding. */
int dsvg_host_alloc(dsvg_ctx *ctx, void **hptr, size_t bytes);
int dsvg_host_free(dsvg_ctx *ctx, void *hptr);
/* the same without a context (a buffer that outlives the context it was allocated through: the decoder's pinned frame pool) */
int dsvg_host_free_on(int device, void *hptr);
/* the raw allocation of reconstruction slot `recon_slot` -- the reference's frame layout, borders as the device left them, dsvg_geom.frame_alloc_bytes
 * bytes -- into host memory (pinned: one asynchronous copy) behind the decoding work on the coding stream; waits for the copy, for nothing else */
int dsvg_download_recon_frame(dsvg_ctx *ctx, int recon_slot, void *raw_out, size_t bytes);
int dsvg_ingest_begin(dsvg_ctx *ctx, const void *yuv_host, size_t bytes, void **dptr);
/* The same for a clip that arrives piece by piece (dsv_enc takes a frame per call): dsvg_ingest_open reserves the next of the
 * two buffers for `bytes` bytes and returns it; dsvg_ingest_part queues the upload of one piece (host memory, pinned for an
 * asynchronous copy) to dptr + offset as soon as the caller has it.  A load from the buffer waits, on the device, for the
 * parts queued before it. */
int dsvg_ingest_open(dsvg_ctx *ctx, size_t bytes, void **dptr);
int dsvg_ingest_part(dsvg_ctx *ctx, void *dptr, size_t offset, const void *host, size_t bytes);

/* Tightly packed planar frames -> resident source slots [first_slot, first_slot+n):
 * copy into the bordered reference layout, replicate borders (dsv_clone_frame/dsv_extend_frame),
 * build the luma pyramid (mk_pyramid dsv_encoder.c:194-217) and the smallest level's mean luma
 * (check_scene_change dsv_encoder.c:538-554).  yuv may be a host or a device pointer.  Async. */
int dsvg_load_frames(dsvg_ctx *ctx, int first_slot, int n, const void *yuv, int yuv_on_device, int with_pyramid);
/* same, frame i read from yuv + i*frame_pitch bytes (device pointer only) */
int dsvg_load_frames_strided(dsvg_ctx *ctx, int first_slot, int n, const void *yuv_dev, size_t frame_pitch, int with_pyramid);
/* same, frame i (at yuv_dev + i*frame_pitch) goes to source slot slots[i]: one launch set for a whole batch.
 * Luma sums: a load with the pyramid replaces the sums (dsvg_get_luma_sums / dsvg_get_avg_luma) of the slots it loads -- a second
 * load of a slot does not add to the first.  The mapped loads (this call and dsvg_load_frames_map_ex) clear the sums of ALL the
 * context's slots first, not only of the slots they load: after one, the sum of a slot the call did not name reads 0.  The
 * contiguous loads above touch the sums of their own slots alone. */
int dsvg_load_frames_map(dsvg_ctx *ctx, int n, const int *slots, const void *yuv_dev, size_t frame_pitch, int with_pyramid);
/* same with chroma_in_place (one flag per frame, or NULL): a flagged frame's chroma planes are not copied -- the forward
 * transform and the motion search's chroma test read them from the caller's clip; only its luma gets the bordered copy and
 * the pyramid (what a frame needs as a motion search REFERENCE; frame.c:122-164,240-327, hme.c:667-681).  The clip must stay
 * unchanged until the pictures coded from those slots have been fetched AND the frame that follows each of them in its stream
 * has been analysed.  Needs even chroma planes a multiple of 8 wide and a 16-byte aligned clip; otherwise (or with
 * DSV1_NO_CHROMA_IN_PLACE) the frames are copied whole.  dsvg_ctx_chroma_in_place_frames: how many frames took it (tests).
 * Round 5, luma in place: where the geometry allows (luma a multiple of 16 wide and 4 high, two or more pyramid levels, a picture
 * wider and taller than twice the ring below + 64) a flagged frame's LUMA stays in the clip as well -- same contract, nothing
 * new for the caller.  The forward transforms read it there, and so does the level-0 motion search for every block that cannot
 * leave the picture; of the bordered copy only a ring is written (a block + twice the search's reach in from each edge, plus
 * the border), which blocks near an edge read.  The pyramid levels are built as ever.  DSV1_NO_LUMA_IN_PLACE switches it
 * off; dsvg_ctx_luma_in_place_frames counts the frames that took it. */
int dsvg_load_frames_map_ex(dsvg_ctx *ctx, int n, const int *slots, const void *yuv_dev, size_t frame_pitch, int with_pyramid,
                            const unsigned char *chroma_in_place);
long dsvg_ctx_chroma_in_place_frames(const dsvg_ctx *ctx);
long dsvg_ctx_luma_in_place_frames(const dsvg_ctx *ctx);
int dsvg_get_luma_sums(dsvg_ctx *ctx, int first_slot, int n, unsigned *sums_out);   /* raw sums, syncs */
int dsvg_get_avg_luma(dsvg_ctx *ctx, int first_slot, int n, int *avg_out);           /* syncs */

/* Hierarchical motion estimation for npairs (current, reference) source-slot pairs
 * (motion_est dsv_encoder.c:219-254 -> dsv_hme).  mvs_out: npairs * nblocks dsvg_mv on the host. Syncs. */
int dsvg_analyse(dsvg_ctx *ctx, int npairs, const int *cur_slots, const int *ref_slots, dsvg_mv *mvs_out);

typedef struct {
    int src_slot;            /* source frame to code */
    int ref_recon_slot;      /* reconstruction used for prediction, -1 for an I picture */
    int recon_slot;          /* where to keep this picture's reconstruction, -1 = do not keep.  May equal ref_recon_slot
                              * (updated in place through a separate prediction frame); a DIFFERENT slot is faster: the
                              * prediction is then written straight into it and only tiles with a residual are touched again */
    int quant;               /* frame quantiser (quality2quant dsv_encoder.c:165) */
    const dsvg_mv *mvs;      /* host, nblocks entries (P pictures) */
    const unsigned char *stable_blocks; /* host, nblocks entries (encode_stable_blocks output) */
    int out_slot;            /* where the packed planes wait for dsvg_fetch_pictures */
    int no_intra_blocks;     /* P pictures: 1 = the caller knows that no block of mvs has mode != 0 (saves a scan) */
    int has_reach;           /* P pictures: 1 = mv_reach holds min(mv.x >> 1), max(mv.x >> 1), min(mv.y >> 1), max(mv.y >> 1) over the
                              * inter blocks of mvs, each taken with 0 (saves a pass over the vectors: see border_hint) */
    short mv_reach[4];
    int border_hint;         /* 1 = no picture coded by a LATER call predicts from this reconstruction (the caller knows the
                              * next picture of the stream: it is in this call, or it starts a GOP).  The replicated border
                              * (dsv_extend_frame) is then written only as far as the motion vectors of the pictures of this
                              * call that predict from it reach -- possibly not at all.  0 = unknown: if the slot is not
                              * rewritten within the call, the whole 64-pixel border is written */
} dsvg_pic_job;

typedef struct {
    int32_t dc[3];           /* unquantised DC (coefficient [0]) of each plane */
    uint32_t nruns[3];       /* number of (run,value) pairs */
    uint32_t nbytes[3];      /* payload length in bytes (bit count rounded up) */
    const uint8_t *payload[3]; /* host (pinned) pointers, valid until the next dsvg_fetch_pictures */
    int32_t rc_quant;        /* pictures coded by dsvg_code_batch_rc: the frame quantiser the device's rate control chose ... */
    uint32_t rc_pkt_len;     /* ... and the bytes of the picture packet as it computed them (0 / 0 for other pictures) */
} dsvg_pic_out;

/* Residual coding of njobs pictures in one batch: frame copy, dsv_sub_pred, then per plane
 * dsv_fwd_sbt / dsv_encode_plane (quantise+dequantise+pack) / dsv_inv_sbt, dsv_frame_add and the
 * extended reconstruction (encode_one_frame dsv_encoder.c:657-674, encode_picture :518-526).
 * Enqueues only; results are collected by dsvg_fetch_pictures (which syncs). */
int dsvg_code_pictures(dsvg_ctx *ctx, int njobs, const dsvg_pic_job *jobs);
/* nsteps consecutive frame steps of njobs pictures each (jobs[step*njobs + j]) in one call: one upload of
 * all tables, kernel chains back to back; step k+1 may predict from the reconstructions of step k.  The out
 * slots of the call must form one contiguous block.  With several coding streams (dsvg_ctx_code_streams) the jobs of a
 * step are shared out by position; a call in which a reconstruction slot would be written and read (or written twice) by
 * jobs of different shares is run on one stream instead -- always correct, fastest when stream s keeps position s. */
int dsvg_code_batch(dsvg_ctx *ctx, int nsteps, int njobs, const dsvg_pic_job *jobs);
/* Device-resident average-bitrate rate control (round 4; quality2quant dsv_encoder.c:70-168 + the statistics of dsv_enc
 * :816-848 as include/dsvg_rc.h, run by k_rc on the device): the same as dsvg_code_batch for streams whose every quantiser
 * depends on the size of the packet before -- jobs[].quant is ignored, rc[step*njobs + j] says which stream's state
 * (rc_slot, < max(n_recon_slots, max_jobs)) picture j of a step belongs to, how many bytes of its packet precede the quantiser
 * field (prefix_len: header + side information, known before the picture is coded) and quality2quant's forced_intra.  A stream
 * keeps its position j from step to step.  The state lives on the device from call to call: dsvg_rc_upload seeds it (once, or when
 * the caller changed the stream's parameters), dsvg_rc_download reads it back (syncs).  dsvg_pic_out.rc_quant / rc_pkt_len return
 * what the device chose and computed for every picture. */
typedef struct { int rc_slot; int prefix_len; int forced_intra; } dsvg_rc_job;
struct dsvg_rc_state;
int dsvg_code_batch_rc(dsvg_ctx *ctx, int nsteps, int njobs, const dsvg_pic_job *jobs, const dsvg_rc_job *rc);
int dsvg_rc_upload(dsvg_ctx *ctx, int first_slot, int n, const struct dsvg_rc_state *states);
int dsvg_rc_download(dsvg_ctx *ctx, int first_slot, int n, struct dsvg_rc_state *states);
/* the PARAMETER fields of the streams' state only (bitrate, frame rate, nudge, max_q_step, quality bounds: everything from
 * dsvg_rc_state.bitrate on) -- what a caller may change between calls (the reference reads them per frame, dsv_encoder.c:84-165);
 * ordered on the coding stream: pictures enqueued before keep the old parameters, pictures enqueued after see the new ones */
int dsvg_rc_set_params(dsvg_ctx *ctx, int first_slot, int n, const struct dsvg_rc_state *states);
int dsvg_fetch_pictures(dsvg_ctx *ctx, int n, const int *out_slots, dsvg_pic_out *outs);
/* The same with the device-to-host copy cut into `nchunks` pieces that end on multiples of `align` pictures: as soon as a
 * piece has arrived, cb(arg, first, count) is called for its pictures (outs[first .. first+count) are valid then) while the
 * later pieces are still being copied -- the caller's packet assembly overlaps the link. */
typedef void (*dsvg_fetch_cb)(void *arg, int first, int count);
int dsvg_fetch_pictures_cb(dsvg_ctx *ctx, int n, const int *out_slots, dsvg_pic_out *outs, int nchunks, int align, dsvg_fetch_cb cb, void *arg);
/* Quality measurement (opt-in, encoder): with it on, every picture coded by a dsvg_code_batch / dsvg_code_batch_rc /
 * dsvg_code_pictures call that STARTS afterwards also gets, on the device, the sum of squared errors between its source and its
 * reconstruction -- what a decoder will show -- per plane over the picture area (borders excluded; chroma at its subsampled
 * size): SSE[p] = sum (src - recon)^2, exact.  Pictures nobody predicts from are reconstructed for it in a work frame (the
 * packets stay byte-identical).  With it off nothing of this runs.  PSNR = 10 log10(255^2 N / SSE), +inf for SSE 0.
 * dsvg_fetch_sse: sse_out[3 i + p] for out_slots[i] -- valid after dsvg_fetch_pictures of those slots and until they are coded
 * again; DSVG_ERR_ARG for a slot whose picture was coded with the measurement off.  Waits for the calls that coded them. */
int dsvg_ctx_sse_enable(dsvg_ctx *ctx, int on);
int dsvg_fetch_sse(dsvg_ctx *ctx, int n, const int *out_slots, uint64_t *sse_out);
/* SSIM (opt-in, encoder, independent of the SSE): per picture and plane the sum over the 8x8 windows at stride 4 (top-left
 * (4i, 4j) with 4i <= w - 8, 4j <= h - 8; uniform weights, population statistics) of rint(s * DSVG_SSIM_ONE), s evaluated in
 * binary64 from the window's int32 sums exactly as k_quality.hip states it -- an exact int64, negative where the picture is.
 * Mean SSIM of a plane = SSIM_FX / (DSVG_SSIM_ONE * nwin), nwin = ((w - 8) / 4 + 1) * ((h - 8) / 4 + 1) (0 below 8 x 8).
 * Same scope and timing as the SSE pair: dsvg_fetch_ssim gives ssim_out[3 i + p] for out_slots[i]; DSVG_ERR_ARG for a slot
 * whose picture was coded with SSIM off.  With SSE and SSIM both on, one pass over the pictures makes both. */
#define DSVG_SSIM_ONE 4294967296LL   /* 2^32: the fixed-point scale of one window's SSIM */
int dsvg_ctx_ssim_enable(dsvg_ctx *ctx, int on);
int dsvg_fetch_ssim(dsvg_ctx *ctx, int n, const int *out_slots, int64_t *ssim_out);
/* Source-resolution quality (opt-in, encoder; resolution ladders, dsv1_resladder_src_quality_enable): every picture of a call that
 * starts afterwards is, for each out slot given a reference frame with dsvg_ctx_xres_refs before that call, upscaled on the device
 * from its reconstruction to the reference geometry ref_w x ref_h (the same format; at least the picture's size on every axis of
 * every plane, at most 8 times it) with the dsv1_resample_* tables of `filter`, and compared with that frame: per plane the SSE over
 * the reference plane and the SSIM_FX over its windows, with the definitions of the two pairs above.  Independent of them.  Off
 * (sse_on = ssim_on = 0) nothing of it runs.  A change of geometry or filter rebuilds the tables and forgets the frames set.
 * dsvg_ctx_xres_refs: out slot out_slots[i] of the next call that codes it is measured against the packed planar frame
 * ref_clip + frames[i] * (reference frame bytes), device memory the caller keeps unchanged until that call's pictures are fetched;
 * the call takes the setting (a slot not set again is not measured next time).  Fetch as dsvg_fetch_sse / _ssim; DSVG_ERR_ARG for
 * a slot whose picture was not measured. */
int dsvg_ctx_xres_enable(dsvg_ctx *ctx, int sse_on, int ssim_on, int ref_w, int ref_h, int filter);
int dsvg_ctx_xres_refs(dsvg_ctx *ctx, const void *ref_clip, int n, const int *out_slots, const int *frames);
int dsvg_fetch_xres_sse(dsvg_ctx *ctx, int n, const int *out_slots, uint64_t *sse_out);
int dsvg_fetch_xres_ssim(dsvg_ctx *ctx, int n, const int *out_slots, int64_t *ssim_out);
/* The four figures by kind: dsvg_fetch_quality(kind) is the fetch above of that kind, the SSIM_FX sums as their two's complement. */
enum { DSVG_Q_SSE, DSVG_Q_SSIM, DSVG_Q_XSSE, DSVG_Q_XSSIM, DSVG_Q_KINDS };
int dsvg_fetch_quality(dsvg_ctx *ctx, int kind, int n, const int *out_slots, uint64_t *out);
int dsvg_download_recon(dsvg_ctx *ctx, int recon_slot, uint8_t *yuv_out);            /* syncs */
/* the first `bytes` bytes of the slot's whole frame allocation in the reference layout (dsv_mk_frame frame.c:63-120:
 * Y,U,V back to back, 64-px replicated borders): what the next picture's motion compensation reads.  Syncs. */
int dsvg_download_recon_raw(dsvg_ctx *ctx, int recon_slot, uint8_t *raw_out, size_t bytes);
/* The encoder writes a reconstruction's border only as far as the pictures that predict from it read it (dsv_pic_job.border_hint,
 * dsvg_code_batch).  dsvg_recon_border: the extents the slot's last encoder job wrote -- pixels left, right, rows above, below
 * the picture, luma [0..3] and chroma [4..7] (columns are written in units of 16, rows in units of 8, at most 64).
 * dsvg_download_recon_asis: the allocation as it is (dsvg_download_recon_raw completes the border first).
 * dsvg_extend_recon: complete the border of a slot now (asynchronous, coding stream). */
int dsvg_recon_border(dsvg_ctx *ctx, int recon_slot, short ext_out[8]);
int dsvg_download_recon_asis(dsvg_ctx *ctx, int recon_slot, uint8_t *raw_out, size_t bytes);
int dsvg_extend_recon(dsvg_ctx *ctx, int recon_slot);
/* The same view of a SOURCE slot (tests): the first `bytes` bytes of source slot `src_slot` at pyramid level `level` (0 = the frame
 * itself, 1 .. the context's pyramid levels), exactly as the device holds them, in the reference frame layout of that level's
 * dimensions (rsu(width, level) x rsu(height, level): Y,U,V allocations back to back, 64-px borders).  Levels above 0 carry luma
 * only: their chroma allocations are never written.  Of a frame loaded with its chroma (or luma) in place, the slot holds what
 * earlier loads left in those planes (in the luma interior inside the ring).  Waits for the loads enqueued so far; completes
 * nothing and changes nothing. */
int dsvg_download_source_raw(dsvg_ctx *ctx, int src_slot, int level, uint8_t *raw_out, size_t bytes);
/* a frame allocation in the reference layout (as dsvg_download_recon_raw returns it) into a reconstruction slot: how a decoder
 * carries its reference picture over when the stream changes its block size and a new context is needed.  Syncs. */
int dsvg_upload_recon_raw(dsvg_ctx *ctx, int recon_slot, const uint8_t *raw, size_t bytes);
/* n reconstruction slots -> tightly packed planar frames, frame i at yuv_out + i*out_pitch.  Device output: enqueued
 * without a sync: on the first coding stream, or -- n >= 4, decoder contexts -- on the second one beside the next call's entropy decoding.
 * Before reading it: dsvg_ctx_sync, or order the consumer behind the pass with dsvg_ctx_join(ctx, consumer_stream) / a dsvg_ctx_stream()
 * handle fetched AFTER this call.  Host output: copied back and synchronised. */
int dsvg_pack_recons(dsvg_ctx *ctx, int n, const int *recon_slots, void *yuv_out, size_t out_pitch, int out_on_device);
/* An output pixel format resolved for one geometry (the session layer works it out: include/dsv1_api.h, decoder output formats).  A
 * SEGMENT is one output plane and the planes of the decoded frame (0 Y, 1 U, 2 V) that feed it, in the order their samples appear:
 * PLAIN one plane, sample for sample; PAIR two planes interleaved; YUYV / UYVY all three as 4:2:2 macro-pixels.  hd / vd: the chroma
 * planes are halved horizontally / vertically on the way, o = (a + b + 1) >> 1 with the last column / row repeated, horizontally
 * first.  wide: a sample v is written as the little-endian 16-bit word v << shift.  A segment's width and rows are those of the
 * output, after the halving or the doubling (hu / vu below). */
enum { DSVG_PIXOUT_PLAIN, DSVG_PIXOUT_PAIR, DSVG_PIXOUT_YUYV, DSVG_PIXOUT_UYVY, DSVG_PIXOUT_RGB };
typedef struct {
    int kind, nin, in_plane[3];
    int rows;                /* of the output plane */
    int width;               /* samples per row of the first input plane as they arrive (chroma: after the halving) */
    int cwidth;              /* YUYV / UYVY: macro-pixels per row */
    size_t off, pitch;       /* the output plane inside an output frame */
} dsvg_pixout_seg;
/* RGB output (csrc/k_rgb.hip; include/dsv1_api.h, RGB): on != 0 makes the format an RGB one.  Its segments are the RGB planes (kind
 * DSVG_PIXOUT_RGB, one for the packed orders, three for the planar ones; rows = h, width = w); hs / vs are the chroma shifts of the
 * decoded frames, which the pass upsamples (linear != 0: centre-sited linear, else replication) before the Q14 inverse matrix
 * inv = IY, RV, GU, GV, BU with luma offset oy. */
typedef struct { int on, order, linear, hs, vs, oy; int32_t inv[5]; } dsvg_rgbout;
typedef struct {
    int nseg, wide, shift, hd, vd;
    size_t frame_bytes;      /* what one output frame occupies: the least distance from frame to frame */
    size_t planes_bytes;     /* where its last plane ends */
    dsvg_pixout_seg seg[3];
    dsvg_rgbout rgb;
    int hu, vu, linear;      /* the chroma planes are doubled horizontally / vertically on the way, vertically first: centre-sited linear
                                (linear != 0; include/dsv1_api.h, chroma resampling) or by replication */
} dsvg_pixout;
/* dsvg_pack_recons for an output format: slot recon_slots[i] -> frame out_index[i] (NULL: i) at out + out_index[i] * out_pitch, in
 * ONE pass over the bordered reconstructions (csrc/k_pixout.hip) that writes only the bytes of samples -- never the padding behind a
 * row, behind the planes or between frames.  Stream placement, ordering and the second pass of a flagged decoder call exactly as
 * dsvg_pack_recons.  Host output: staged on the device and copied back with one copy where the frames are dense (no padding, every
 * frame written); else the caller's buffer goes up first so that what the pass does not write comes back as it was. */
int dsvg_export_recons(dsvg_ctx *ctx, int n, const int *recon_slots, const int *out_index, void *out, size_t out_pitch,
                       int out_on_device, const dsvg_pixout *fmt);
/* the same pass over n tightly packed planar frames, frame_bytes apart on the output side; device pointers, or host memory that is
 * staged (the destination goes up first, as above).  Any w, h >= 1.  Synchronous. */
int dsvg_export_planar(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsvg_pixout *fmt, int on_device);

/* Debug overlay of decoded pictures (csrc/k_drawinfo.hip; include/dsv1_api.h, debug overlays).  dsvg_ctx_draw_info: with mode != 0 (bits
 * 1 / 2 / 4: stability dashes, motion vectors, intra dots; any non-zero value: the block grid) every picture with a reference of the
 * dsvg_decode_pictures calls that follow is copied, behind its reconstruction and on the same stream, to a scratch frame of the context
 * (one per job of a call, allocated when first needed) and drawn on there from the call's own block tables.  Until the next decoder
 * call dsvg_pack_recons / dsvg_export_recons / dsvg_download_recon / dsvg_download_recon_frame of that slot read the scratch frame; the
 * slot itself -- what later pictures predict from, dsvg_download_recon_raw -- stays clean.  Mode 0: no allocation, copy or launch.
 * dsvg_draw_info_planar: the overlay on n tightly packed planar frames in place, frame i from mvs / stable + i * nblocks (host tables;
 * stable: bit 0); blk 16 .. 64, mode 1 .. 7.  Synchronous. */
int dsvg_ctx_draw_info(dsvg_ctx *ctx, int mode);
/* Output scale of decoded pictures (csrc/k_scale.hip, k_scale_slots; include/dsv1_api.h, decoder output scale).  With a size set,
 * dsvg_pack_recons / dsvg_export_recons hand out every picture resampled to out_w x out_h at the context's subsampling: each plane on
 * its own with the tables of dsv1_resample_weights (filter: DSV1_SCALE_TENT / _CUBIC), read from the reconstruction -- or from the
 * overlay's scratch frame where dsvg_ctx_draw_info drew -- with its indices clamped to the plane, never from the border.
 * dsvg_pack_recons then writes packed planar frames of the scaled geometry (out_pitch at least such a frame) in its one pass;
 * dsvg_export_recons takes a dsvg_pixout resolved for the scaled geometry, and its pass reads the scaled frames from a scratch of the
 * context (allocated when first needed).  Stream placement, ordering and the second pass of a flagged decoder call as before.
 * 0, 0 switches it off; off is the default and allocates, copies and launches nothing.  DSVG_ERR_ARG, the setting in force unchanged:
 * a plane's axis outside 1/8 <= source / output <= 8, an unknown filter, a size that is not positive.  A pending decoder call is
 * settled first.  dsvg_download_recon* and the references are not scaled. */
int dsvg_ctx_output_scale(dsvg_ctx *ctx, int out_w, int out_h, int filter);
int dsvg_draw_info_planar(int device, void *clip, int w, int h, int subsamp, int n, int blk_w, int blk_h, const dsvg_mv *mvs,
                          const unsigned char *stable, int mode, int on_device);

/* Decoder side: coefficient (run,value) pairs parsed on the host are scattered + dequantised,
 * inverse transformed and motion compensated on the device (dsv_dec dsv_decoder.c:379-436). */
typedef struct {
    int ref_recon_slot;      /* -1 for an I picture */
    int recon_slot;          /* output picture slot */
    int quant;
    const dsvg_mv *mvs;
    const unsigned char *stable_blocks;
    const uint8_t *plane_data[3];   /* host: bytes following the 32-bit plane length */
    uint32_t plane_len[3];
} dsvg_dec_job;
int dsvg_decode_pictures(dsvg_ctx *ctx, int njobs, const dsvg_dec_job *jobs);
/* P pictures are decoded through int16 symbol planes (the encoder's fused inverse).  A picture those cannot hold exactly -- a
 * symbol beyond int16 (not producible from 8-bit video, but parsable), or a cell shared by two scan regions that must keep
 * the earlier region's value (hzcc.c:295-435) -- is detected on the device and its call decoded again from int32 coefficients
 * before anything reads or predicts from the result (the next decode call, dsvg_ctx_sync, the downloads, a host-side pack).
 * dsvg_ctx_decoder_redone: how many calls took that second pass (tests). */
long dsvg_ctx_decoder_redone(const dsvg_ctx *ctx);

/* Kernel timing hook for bench.py: every launch of the kernels selected by `kernel_mask` (bit i =
 * kernel id i, names from dsvg_prof_kernel_name) is bracketed by HIP events on the pipeline stream.
 * dsvg_prof_get returns the summed event time (ms), launch count and the ALGORITHMIC bytes those
 * launches moved (compulsory traffic: each input read once, each output written once; the per-sample
 * figures are listed in DESIGN.md) since the last reset. */
/* two marks on the first coding stream and the GPU-side time between them (HIP events): dsvg_ctx_mark(ctx, 0) when a timed region
 * starts, dsvg_ctx_mark(ctx, 1) behind its last enqueued coding work; dsvg_ctx_mark_ms after a sync.  bench.py prints it beside its
 * host clock so that the headline can be corroborated from the device side. */
int dsvg_ctx_mark(dsvg_ctx *ctx, int which);
int dsvg_ctx_mark_ms(dsvg_ctx *ctx, float *ms);
/* Where a step's time goes, from the pipeline's own streams (round 6): dsvg_ctx_timeline(ctx, 1) starts collecting timing marks at the boundaries of
 * clip upload / frame load + pyramid / motion search / table uploads / coding (both coding streams) / fetch (one HIP event per mark, ten per batch;
 * 0 stops and clears).  dsvg_ctx_timeline_get (context synchronised) sums them: out[0] = coding phases seen, [1] = device ms first mark .. last mark,
 * [2] upload, [3] load, [4] motion search, [5] table uploads, [6] coding on the first stream, [7] on the second, [8] fetch (gather + copies) --
 * device ms summed over the phases --, [9] = ms during which none of load / search / tables / coding was in flight (the chip waits for the host),
 * [10] = the same inside [first coding start, last coding end], [11] = ms of coding overlapped by a load / search phase. */
int dsvg_ctx_timeline(dsvg_ctx *ctx, int on);
int dsvg_ctx_timeline_get(dsvg_ctx *ctx, double out[12]);
/* the host's side of dsvg_fetch_pictures(_cb) per call since the last reset: out[0] = ms waiting for the coding calls behind the slots, [1] = ms for
 * the plane summaries (a small device-to-host round trip), [2] = ms for gather + the copy in pieces + the callback's work, [3] = bytes copied, [4] = calls */
int dsvg_ctx_fetch_prof(dsvg_ctx *ctx, double out[5], int reset);
int dsvg_prof_kernels(void);
const char *dsvg_prof_kernel_name(int kid);
int dsvg_prof_enable(dsvg_ctx *ctx, unsigned long long kernel_mask);
int dsvg_prof_reset(dsvg_ctx *ctx);
int dsvg_prof_get(dsvg_ctx *ctx, int kid, double *ms, long *launches, double *alg_bytes);

/* Which branch the encoder's forward launchers take (tests): read-only, host side, no effect on coding.
 * fwd[g]: the general kernel (k_fwd_mc_pix) of a P picture's plane group g (0 luma, 1 the chroma pair) -- a mask of DSVG_FWD_*:
 * the facts (WHOLE, or the strips TOP / BOTTOM / LEFT / RIGHT that can hold patches the lean kernel leaves) and the shape of the
 * grid (ROW1 / COL1: one row / one column of thread blocks, which a strip pair collapses to); -1: not decided (no P picture yet,
 * or motion compensation not fused).  hme[l] = {NKBF of the register body or 0, fullx, fully, mask of the PARTs launched (bit p =
 * PART p)} of motion-search level l; csum: 0 = k_hme_csum not launched, 1 = launched, 2 = launched and every workgroup returns
 * at once for reasons the host knows (fullx > 64, chroma block width not a multiple of 16), -1: not decided.
 * tail_threads / scan_threads: the workgroup size of the last k_tail_q / k_hz_scan launch (1024 for few jobs per launch, else 256).
 * dsvg_dispatch_last: what the last forward plan of a P plane group, the last motion-search plan, the last k_tail_q step and the
 * scan launch said in this process (the plans' executors, launch_fwd_plan / launch_hme_plan, fill it in; fusable: whether the last
 * P plane group took the fused kernels).
 * dsvg_dispatch_plan: the same figures for an encoder context of this geometry, without a device -- read from the plans themselves
 * (fwd_sbt_plan, hme_plan: see dsvg_fwd_plan / dsvg_hme_plan below) on the geometry tables of dsvg_ctx_create (one set-up, shared
 * with the context; the GPU tests still compare both queries on a live context); tail_threads / scan_threads = -1 (they depend on
 * the jobs per launch). */
#define DSVG_FWD_WHOLE  1
#define DSVG_FWD_TOP    2
#define DSVG_FWD_BOTTOM 4
#define DSVG_FWD_LEFT   8
#define DSVG_FWD_RIGHT  16
#define DSVG_FWD_ROW1   32
#define DSVG_FWD_COL1   64
typedef struct dsvg_dispatch {
    int blk_w, blk_h;
    int fusable;                              /* mc_fusable: P pictures take k_fwd_mc_fast + k_fwd_mc_pix */
    int fwd[2];
    int hme_levels;                           /* the pyramid's levels above level 0 */
    int hme[DSVG_MAX_PYRAMID + 1][4];
    int csum;
    int tail_threads, scan_threads;
} dsvg_dispatch;
int dsvg_dispatch_last(dsvg_dispatch *out);
int dsvg_dispatch_plan(int width, int height, int subsamp, dsvg_dispatch *out);

/* The launches of the inverse transform (tests): what the launcher of the inverse kernels (launch_inv_sbt) does for one plane group of
 * njobs pictures of an encoder context of this geometry, without a device -- the launcher's own plan (inv_sbt_plan: the launcher runs
 * its steps and decides nothing), on the geometry tables of dsvg_ctx_create.  group: 0 luma, 1 the chroma pair; isP, with_tail
 * (bit 0: the LDS tail first, bit 1: levels 5..4 were done for all planes in one launch), insym (details from the symbol planes),
 * patch_kernel (sparse P pictures: flags and prediction given) and fuse_border (the caller lets the chroma patch kernel write the
 * reconstruction's borders where it can) as the callers pass them; switches: a mask of DSVG_INV_NO_* for the A/B switches of the
 * same names (DSV1_NO_*), whatever the environment says.  Writes the first min(steps, cap) steps in launch order and *fb (1: the
 * chroma patch kernel writes the borders of all three planes; fb may be null) and returns the number of steps, or a negative
 * DSVG_ERR_* for a geometry dsvg_ctx_create refuses.
 * A step: kernel = the index of dsvg_prof_kernel_name; the grid (xcd != 0: launched in one dimension, 8 * ceil(x * y * z / 8) workgroups
 * that decode the logical grid, 1: in XCD order, 2: in the hardware's order, DSVG_INV_NO_XCD_ORDER); args = the kernel's trailing integer arguments (k_inv_haar_tile: first tile column of the
 * strips, -(first tile row) - 1, or 0, 0 for its whole grid; k_inv_p_tile: the edge tile column / row it also takes or -1;
 * k_inv_patch_c: imax, jmax, jpart, fb); bytes = the algorithmic bytes the profiler books; cover = the level-3 cells of every plane
 * of the group whose pixels the step writes: NONE, the WHOLE plane, the RECTangle of cells [0, cx) x [0, cy), or every tile FROM
 * tile column cx or tile row cy on (tiles of 16 x 8 cells). */
#define DSVG_INV_NO_PATCH_PART   1
#define DSVG_INV_NO_EDGE_TILES   2
#define DSVG_INV_NO_FUSED_BORDER 4
#define DSVG_INV_NO_XCD_ORDER    8
#define DSVG_INV_COVER_NONE  0
#define DSVG_INV_COVER_WHOLE 1
#define DSVG_INV_COVER_RECT  2
#define DSVG_INV_COVER_FROM  3
typedef struct dsvg_inv_step {
    int kernel;
    int grid[3], xcd;
    int args[4];
    double bytes;
    int cover, cx, cy;
} dsvg_inv_step;
int dsvg_inv_plan(int width, int height, int subsamp, int group, int isP, int with_tail, int insym, int patch_kernel, int fuse_border,
                  unsigned switches, int njobs, dsvg_inv_step *steps, int cap, int *fb);

/* The launches of the forward transform and of the motion search (tests), without a device: the plans the encoder's launchers run
 * step by step (fwd_sbt_plan / fwd_step_plan -> launch_fwd_plan, hme_plan -> launch_hme_plan: the executors decide nothing), on the
 * geometry tables of dsvg_ctx_create.
 * dsvg_fwd_plan: group 0 luma, 1 the chroma pair of njobs pictures (isP: all P, else all I) as the frame step of dsvg_code_batch asks
 * for them -- quantised, motion compensation fused where the geometry allows, general_whole = 0: no picture has an intra block --, or
 * group DSVG_FWD_GROUP_STEP: what the step launches once for all planes of its njobs pictures (levels 4..5, then k_tail_q, or
 * k_fwd_tail with DSVG_FWD_NO_LLQ).  switches: DSVG_FWD_NO_* for DSV1_NO_XCD_ORDER, DSV1_NO_MC_FUSION, DSV1_NO_LLQ, whatever the
 * environment says.  *mask (may be null): the DSVG_FWD_* mask of a P plane group, or -1.  A step: kernel, grid, xcd and bytes as in
 * dsvg_inv_step; block, dynamic LDS bytes; args = the kernel's trailing integers (k_fwd_mc_pix: bxofs, byofs, bxstep, bystep -- thread
 * block (x, y) of the launch works on block (bxofs + x * bxstep, byofs + y * bystep) of the full grid; k_fwd_b4t / k_fwd_haar_pix:
 * from_src; k_fwd_haar_mid<4>: 1 = with the LL quantiser).  k_tail_q's variant is its block size.
 * dsvg_hme_plan: the motion search of npairs pairs (csum_table: with the chroma table, as a context has it): k_hme_csum if any, the
 * launches of every level from the top down, k_hme_detail.  A step: kernel; l0, nkbf, part = the k_hme_level<L0, NKBF, PART>
 * instance; level; count = the level's blocks per pair in this launch; fullx, fully; inv_per, inv_row = min(floor(2^32 / d),
 * 2^32 - 1) of count and of the row length the block index is split by; grid (k_hme_level: grid[0] workgroups, launched rounded up
 * to a multiple of 8), block; bytes (0 where cont); cont = 1: the launch has no profiler bracket of its own, it continues the previous step's.
 * Both write the first min(steps, cap) steps in launch order and return the number of steps, or a negative DSVG_ERR_*. */
#define DSVG_FWD_GROUP_STEP   2
#define DSVG_FWD_NO_XCD_ORDER 1
#define DSVG_FWD_NO_MC_FUSION 2
#define DSVG_FWD_NO_LLQ       4
typedef struct dsvg_fwd_step {
    int kernel;
    int grid[3], xcd;
    int block[2];
    unsigned lds;
    int args[4];
    double bytes;
} dsvg_fwd_step;
int dsvg_fwd_plan(int width, int height, int subsamp, int group, int isP, int general_whole, unsigned switches, int njobs,
                  dsvg_fwd_step *steps, int cap, int *mask);
typedef struct dsvg_hme_step {
    int kernel;
    int l0, nkbf, part;
    int level, count, fullx, fully;
    unsigned inv_per, inv_row;
    int grid[2], block;
    double bytes;
    int cont;
} dsvg_hme_step;
int dsvg_hme_plan(int width, int height, int subsamp, int csum_table, int npairs, dsvg_hme_step *steps, int cap);

/* The plan of a coding call (tests): what dsvg_code_batch / dsvg_code_batch_rc (rc != NULL) decide on the host for these jobs in an
 * encoder context created with these arguments, without a device -- the call's own plan (plan_code_batch, csrc/dsvg_batch_plan.h: the
 * call commits it and enqueues from it), on the geometry tables of dsvg_ctx_create.  code_streams as dsvg_ctx_code_streams sets it;
 * switches: a mask of DSVG_BATCH_* for the A/B switches DSV1_NO_SMALL_SPLIT, DSV1_NO_PAR_ENQUEUE, DSV1_NO_LAZY_BORDER, DSV1_NO_MC_FUSION,
 * whatever the environment says, and PROFILED for a context with kernel timing on (dsvg_prof_enable).  Returns DSVG_OK, a negative
 * DSVG_ERR_* for a geometry dsvg_ctx_create refuses, the code and text the call itself answers for jobs it refuses, or DSVG_ERR_ARG
 * for arrays that are missing or too small (the scalars are filled in then).
 * Device job d = t * njobs + k is the picture at position k of frame step t in device order (I pictures first); sg = ng * t + g is
 * coding stream g's share of step t, device positions [gk[g], gk[g + 1]).  The caller sets the arrays and their capacities:
 *   cap_steps:  nI[t], the I pictures of step t;
 *   cap_jobs:   order[d] = the caller's index inside its step of device job d; mvu[d] / stu[d] = index of the job's vector / flag table
 *               among the call's tables (jobs that pass one pointer share one), mvcp[d] / stcp[d] = 1: this job's host table is the one
 *               uploaded; ext[8 d + i] = how far the job's reconstruction gets its border written (as dsvg_recon_border); rc_next[d] =
 *               base + the device job of the same rate-controlled stream's next picture (-1: none, or no rc);
 *   cap_groups: ioff[sg] / icnt[sg] = the share's intra blocks in ilist, entries (position among the share's P pictures) * nblk +
 *               block; noint[sg] = 1: icnt says all there is to know (0: motion compensation is not fused, the blocks were not listed);
 *               keeps[sg] = 1: a picture of the share keeps its reconstruction;
 *   cap_ilist:  ilist, iln entries.
 * Append-only: later versions add fields at the end. */
#define DSVG_BATCH_NO_SMALL_SPLIT  1
#define DSVG_BATCH_NO_PAR_ENQUEUE  2
#define DSVG_BATCH_NO_LAZY_BORDER  4
#define DSVG_BATCH_NO_MC_FUSION    8
#define DSVG_BATCH_PROFILED        16
typedef struct dsvg_batch_plan {
    int cap_steps, cap_jobs, cap_groups, cap_ilist;
    int *nI;
    int *order, *mvu, *stu;
    unsigned char *mvcp, *stcp;
    short *ext;
    int *rc_next;
    int *ioff, *icnt;
    unsigned char *noint, *keeps;
    int *ilist;
    int nblk, mc_fused;            /* of the geometry: blocks per picture, motion compensation fused into the forward transform */
    int base, total, ng, gk[5];    /* first out slot, pictures, coding streams and their split of a step */
    int iln, nmv, nst, mv_contig;  /* intra-list entries; vector / flag tables uploaded; nmv == total */
    int par_enqueue;               /* every coding stream is enqueued by a thread of its own */
} dsvg_batch_plan;
int dsvg_code_batch_plan(int width, int height, int subsamp, int n_recon_slots, int n_src_slots, int max_jobs, int out_slots, int code_streams,
                         unsigned switches, int nsteps, int njobs, const dsvg_pic_job *jobs, const dsvg_rc_job *rc, dsvg_batch_plan *out);

/* The plan of a decoder call (tests): what dsvg_decode_pictures decides on the host for these jobs in a context created with these
 * arguments (the encoder's own block size), without a device -- the call's own plan (plan_decode, csrc/dsvg_dec_plan.h: the call commits
 * it and enqueues from it), on the geometry tables of dsvg_ctx_create.  switches: a mask of DSVG_DEC_* for the A/B switches
 * DSV1_NO_DEC_SYM, DSV1_NO_DEC_SYM_I, DSV1_DEC_ONE_STREAM, DSV1_NO_MC_PATCH, DSV1_NO_INPLACE_PRED, DSV1_NO_DEC_SYM_OV, DSV1_NO_MC_FUSION,
 * whatever the environment says, and PROFILED for a context with kernel timing on.  force32: the repeat of a flagged call on int32
 * coefficients; draw_mode as dsvg_ctx_draw_info sets it.  Returns DSVG_OK, a negative DSVG_ERR_* for a geometry dsvg_ctx_create
 * refuses, the code and text the call itself answers for jobs it refuses, or DSVG_ERR_ARG for arrays that are missing or too small
 * (the scalars are filled in then).  The jobs' payloads are read (each plane's header).
 * Device job d is the picture at position d in device order (I pictures first).  The caller sets the arrays and their capacities:
 *   cap_jobs:  order[d] = the caller's index of device job d; path[d] = 0 int32 coefficients, 1 an I picture, 2 a P picture on the int16
 *              symbol planes; wide[d] = 1: lim[1] holds the job's limits, else lim[0]; inplace[d] = 1: the prediction is written
 *              into the reconstruction slot; per plane at [3 d + p]: dec_sym (the plane takes symbols), dc, runs, len (the plane
 *              header and the payload's bytes), bitpos (first bit of the code chain), blob_off (bytes, in the call's payload blob),
 *              meta_off (in the call's parse records);
 *   cap_ilist: ilist, iln entries: per P picture the blocks k_mc takes by list beside k_mc_patch, (position among the P pictures) *
 *              nblk + block (mc == 2 only).
 * Append-only: later versions add fields at the end. */
#define DSVG_DEC_NO_SYM           1
#define DSVG_DEC_NO_SYM_I         2
#define DSVG_DEC_ONE_STREAM       4
#define DSVG_DEC_NO_MC_PATCH      8
#define DSVG_DEC_NO_INPLACE_PRED  16
#define DSVG_DEC_NO_SYM_OV        32
#define DSVG_DEC_NO_MC_FUSION     64
#define DSVG_DEC_PROFILED         128
typedef struct dsvg_dec_plan {
    int cap_jobs, cap_ilist;
    int *order, *path, *dec_sym;
    unsigned char *wide, *inplace;
    int *dc, *runs, *len;
    long long *bitpos, *blob_off, *meta_off;
    int *ilist;
    /* of the geometry: blocks per picture and per row, patch motion compensation possible, luma / chroma planes that can take symbols
     * and that have cells shared between scan regions, a second coding stream exists, scan chunks per plane */
    int nblk, nbh, mc_patch, sym_ok[2], ov[2], second_stream, nchunks[3];
    int lim[2][16];                /* the sixteen per-level limits: [0] a P picture's ranges, [1] wide */
    int nI;                        /* I pictures of the call */
    long long blob, nmeta;         /* bytes of the payload blob, parse records */
    int max_entries, max_chunks;   /* the parse / scatter grids */
    int insym, f0, anysym;         /* enqueue_recon's insym; first job that may raise a flag; some plane is on the symbol path */
    int scatter_one, resolve, fork;  /* one scatter launch (else three); k_hz_dec_resolve runs; motion compensation on the second stream */
    int mc, ex0, ey0, iln;         /* 0 no P picture, 1 k_mc, 2 k_mc_patch plus k_mc by list; ragged 8x8 patches from block (ex0, ey0) on */
    int draw0, draw1;              /* device jobs [draw0, draw1) get the debug overlay */
} dsvg_dec_plan;
int dsvg_decode_plan(int width, int height, int subsamp, int n_recon_slots, int max_jobs, unsigned switches, int force32, int draw_mode,
                     int njobs, const dsvg_dec_job *jobs, dsvg_dec_plan *out);

/* The plan of a source load (tests): what dsvg_load_frames / _strided / _map / _map_ex decide on the host for n frames in a context of
 * this geometry, without a device -- the load's own plan (plan_load, csrc/dsvg_load_plan.h: the load launches from it and decides
 * nothing itself).  pyramid_levels as dsvg_ctx_create takes it (0: the encoder's own); src_mod16, pitch_mod16: the source pointer and
 * the distance between two frames modulo 16 (dsvg_load_frames: 0 and the bytes of a packed frame modulo 16); switches: a mask of
 * DSVG_LOAD_NO_* for the A/B switches DSV1_NO_UNPACK_SIDES, DSV1_NO_LEVEL_SIDES, DSV1_NO_FUSE_LEVEL2, whatever the environment says;
 * n_chroma_in_place / n_luma_in_place: the frames of the call that took dsvg_load_frames_map_ex's flag (the second only where
 * luma_in_place_ok).  Returns DSVG_OK or a negative DSVG_ERR_* for a geometry dsvg_ctx_create refuses.
 *   sides: k_unpack writes the side borders of the picture rows of all three planes; fuse1 / fuse2: it writes pyramid level 1 / levels 1
 *   and 2 as well; sides1 / sides2: with those levels' side borders.  body[p]: the body of k_unpack plane p of the call's first frame
 *   takes, DSVG_UNPACK_* (every frame's where pitch_mod16 is 0, else a later frame takes the scalar or the 16-byte body as its own address falls; NONE: no frame of the call copies its chroma); grid_planes: the
 *   launch's planes.  level[l], l = 0 .. levels (level 0 alone without the pyramid): the luma plane; border = the kernel that writes the
 *   level's border, tb_only = only the rows above and below; ds2x = k_ds2x writes the level, with the side borders (ds2x_sides), with a
 *   last dword of a row that is not whole (ds2x_tail), from a level of odd width / height, whose last column / row of means reads a
 *   border pixel (src_odd_w / src_odd_h).  luma_sum: k_luma_sum runs, on the top level; luma_sum_dword: four samples per load.
 *   ring_x16, ring_y4: of a luma-in-place frame's bordered copy only the border and the picture's outer ring_x16 x 16 columns and
 *   ring_y4 x 4 rows are written.  chroma_in_place_ok / luma_in_place_ok: the geometry allows the flag's two effects (the context also
 *   asks DSV1_NO_CHROMA_IN_PLACE, DSV1_NO_LUMA_IN_PLACE and DSV1_NO_FUSE_LEVEL2).  launches[k], bytes[k]: the launches and the
 *   algorithmic bytes the profiler books for kernel id k = k_unpack, k_extend, k_extend16, k_ds2x, k_luma_sum (ids 0..4).
 * Append-only: later versions add fields at the end. */
#define DSVG_LOAD_NO_UNPACK_SIDES 1
#define DSVG_LOAD_NO_LEVEL_SIDES  2
#define DSVG_LOAD_NO_FUSE_LEVEL2  4
enum { DSVG_UNPACK_NONE, DSVG_UNPACK_SCALAR, DSVG_UNPACK_V16, DSVG_UNPACK_FUSED1, DSVG_UNPACK_FUSED2 };
enum { DSVG_BORDER_NONE, DSVG_BORDER_EXTEND, DSVG_BORDER_EXTEND16 };
typedef struct dsvg_load_level {
    int w, h;
    int border, tb_only;
    int ds2x, ds2x_sides, ds2x_tail, src_odd_w, src_odd_h;
} dsvg_load_level;
typedef struct dsvg_load_plan_out {
    int levels;
    int sides, fuse1, fuse2, sides1, sides2;
    int body[3], grid_planes;
    dsvg_load_level level[DSVG_MAX_PYRAMID + 1];
    int luma_sum, luma_sum_dword;
    int ring_x16, ring_y4;
    int chroma_in_place_ok, luma_in_place_ok;
    int launches[5];
    double bytes[5];
} dsvg_load_plan_out;
int dsvg_load_plan(int width, int height, int subsamp, int pyramid_levels, int with_pyramid, int src_mod16, int pitch_mod16, unsigned switches,
                   int n, int n_chroma_in_place, int n_luma_in_place, dsvg_load_plan_out *out);

/* The plan of a packet fetch (tests): what dsvg_fetch_pictures(_cb) decides on the host, without a device or a context -- the call's own
 * two plans (plan_fetch_wait, plan_fetch_layout, csrc/dsvg_fetch_plan.h: the call waits, grows, copies and calls back as they say) on
 * what they read of a context, as plain arrays.  ctx_out_slots: the context's out slots; slot_ev[ctx_out_slots]: per out slot the index
 * in the ring of nring coding events of the call that coded it last (-1: none); slot_isP[n_isP]: it holds a P picture (n_isP may be
 * smaller than ctx_out_slots, 0 on a context that has coded nothing); ncalls: coding calls made; has_cb: a callback is given; switches:
 * a mask of DSVG_FETCH_* for the A/B switch DSV1_NO_FETCH_FAST, whatever the environment says; bits[7]: the packed bits of a job
 * (bytes per job, the three planes' offsets, the three planes' capacities); total_bits[3 i + p], overflow[3 i + p]: the plane
 * summaries of out_slots[i] as they come back; nchunks, align: as dsvg_fetch_pictures_cb takes them.  Returns DSVG_OK, the code and
 * text the call itself answers for arguments or an overflowed plane, or DSVG_ERR_ARG for arrays that are missing or too small.
 *   few: the one-round-trip path (at most 4 pictures, no callback, every slot coded by the newest call or never, no I picture, switch
 *   unset); stream_wait: the coding events wait[0 .. nwait) -- each once, in first-appearance order -- are waited for in the fetch stream,
 *   else on the host; grow_few: what that path asks of the payload pair (elements, the `few` rule of dsvg_ctx_mem_grow) and copies[9 n]:
 *   its copies per picture and plane (source byte in the packed bits, destination byte, bytes); fits: every plane lies within them.
 *   general: the general path runs (not few, or few and not fits): the plane summaries of out slots lo .. hi come back in one copy,
 *   rows[9 n] is the gather table (source byte, destination byte, bytes), total the bytes gathered, grow what it asks of the payload
 *   pair, and the copy is made in nchunks pieces: pictures piece[2 j] .. piece[2 j + 1] - 1, bytes piece_bytes[2 j] .. piece_bytes[2 j + 1] - 1,
 *   the callback called once per piece in this order.  nbytes[3 n], pay[3 n]: every payload's bytes and where it starts in the pinned
 *   buffer, on the path that delivers.  A refused call reports no growth -- except that an overflowed plane found on the few path is
 *   found after grow_few was taken.
 * Append-only: later versions add fields at the end. */
#define DSVG_FETCH_NO_FAST 1
typedef struct dsvg_fetch_plan_out {
    int cap_pics, cap_pieces;                /* in: pictures / pieces the caller's arrays hold */
    int *wait;                               /* cap_pics */
    unsigned long long *copies, *rows;       /* 9 * cap_pics each */
    unsigned *nbytes;                        /* 3 * cap_pics */
    unsigned long long *pay;                 /* 3 * cap_pics */
    int *piece;                              /* 2 * cap_pieces */
    unsigned long long *piece_bytes;         /* 2 * cap_pieces */
    int few, stream_wait, nwait, lo, hi, fits, general, nchunks;
    unsigned long long grow_few, total, grow;
} dsvg_fetch_plan_out;
int dsvg_fetch_plan(int ctx_out_slots, int n, const int *out_slots, const int *slot_ev, int n_isP, const unsigned char *slot_isP, int nring,
                    long long ncalls, int has_cb, unsigned switches, const unsigned long long bits[7], const unsigned long long *total_bits,
                    const int *overflow, int nchunks, int align, dsvg_fetch_plan_out *out);

/* A context's memory (csrc/dsvg_ctx_mem.h).  Every buffer a context owns has an id, 0 .. DSVG_CTX_MEM_IDS - 1, and a short name
 * (dsvg_ctx_mem_name).  dsvg_ctx_mem_plan: the buffers dsvg_ctx_create_blk allocates for these arguments, in the order it allocates
 * them, without a device -- the same argument and geometry checks with the same codes; at most `cap` rows are written, the number of
 * rows is returned (>= 0), totals[DSVG_MEM_DEVICE] = device bytes (slabs among them), totals[DSVG_MEM_PINNED] = pinned host bytes.
 * Buffers allocated on first use are not in the plan: dsvg_ctx_mem_grow gives the bytes such a buffer takes in a context of these
 * arguments when it holds `cap` elements and `need` are asked for (few: the fetch of a few pictures, gath_d / gath_h), 0 = not such an id.
 * dsvg_ctx_mem_live: the bytes the context holds now, per id (n <= DSVG_CTX_MEM_IDS entries).  dsvg_mem_outstanding: device and pinned
 * bytes held by all live contexts of the process.  dsvg_debug_fail_alloc_at (tests): the n-th allocation of a context from now on
 * fails as out of memory, without a HIP call (0 = off). */
#define DSVG_CTX_MEM_IDS 84
enum { DSVG_MEM_DEVICE, DSVG_MEM_PINNED, DSVG_MEM_SLAB };
typedef struct dsvg_ctx_mem_row {
    int id, kind, zeroed;
    size_t count, size, pad, bytes;          /* bytes = count * size + pad */
} dsvg_ctx_mem_row;
const char *dsvg_ctx_mem_name(int id);
int dsvg_ctx_mem_plan(int width, int height, int subsamp, int pyramid_levels, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots,
                      int blk_w, int blk_h, dsvg_ctx_mem_row *rows, int cap, size_t totals[2]);
size_t dsvg_ctx_mem_grow(int width, int height, int subsamp, int pyramid_levels, int n_src_slots, int n_recon_slots, int max_jobs, int out_slots,
                         int blk_w, int blk_h, int id, size_t need, size_t cap, int few);
int dsvg_ctx_mem_live(const dsvg_ctx *ctx, size_t *bytes_by_id, int n);
void dsvg_mem_outstanding(size_t out[2]);
void dsvg_debug_fail_alloc_at(int n);

#ifdef __cplusplus
}
#endif
#endif
