/*
 * dsv1_api.h -- session-level C API of libdsv1_mi355x.so: the drop-in surface behind dsv_main.c.
 *
 * Every symbol the reference CLI binds (dsv_main.c:440-557,652-717) is exported with the same name,
 * argument meaning, ownership and return codes, and the structs callers poke (DSV_ENCODER,
 * DSV_DECODER, DSV_META, DSV_FRAME, DSV_BUF) keep the reference's field order and sizes
 * (dsv.h:86-198, dsv_encoder.h:58-110, dsv_decoder.h:27-43).  The per-frame arithmetic runs in the HIP
 * kernels behind include/dsvg.h; this layer (plain C) keeps GOP / scene-change / rate-control /
 * stability logic, side-info coding and packet framing on the host.
 *
 * Extensions (names of our own): dsv1_batch_* encodes many independent closed GOPs per call with
 * frames resident in HBM -- the throughput path used by bench.py and by GOP sharding across GPUs.
 */
#ifndef DSV1_API_H
#define DSV1_API_H

#include <limits.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include "dsvg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* packet types (dsv.h:34-43) */
#define DSV_PT_META 0x00
#define DSV_PT_PIC  0x04
#define DSV_PT_EOS  0x10
#define DSV_PACKET_HDR_SIZE 14
#define DSV_PACKET_TYPE_OFFSET 5
#define DSV_PACKET_PREV_OFFSET 6
#define DSV_PACKET_NEXT_OFFSET 10

#define DSV_SUBSAMP_444 0x0
#define DSV_SUBSAMP_422 0x4
#define DSV_SUBSAMP_420 0x5
#define DSV_SUBSAMP_411 0x8

#define DSV_MAX_QUALITY 2047
#define DSV_QUALITY_PERCENT(p) (DSV_MAX_QUALITY * (p) / 100)
#define DSV_GOP_INTRA 0
#define DSV_GOP_INF INT_MAX
#define DSV_ENC_NUM_BUFS 0x03
#define DSV_ENC_FINISHED 0x04
#define DSV_RATE_CONTROL_CRF 0
#define DSV_RATE_CONTROL_ABR 1
#define DSV_MAX_PYRAMID_LEVELS 5

typedef uint32_t DSV_FNUM;
typedef dsvg_meta   DSV_META;
typedef dsvg_plane  DSV_PLANE;
typedef dsvg_frame  DSV_FRAME;
typedef dsvg_mv     DSV_MV;
typedef dsvg_params DSV_PARAMS;
typedef struct { unsigned char *data; unsigned len; } DSV_BUF;

typedef struct {                 /* same fields, order and sizes as dsv_encoder.h:58-110 */
    int quality;
    int gop;
    int do_scd;
    int rc_mode;
    int rc_high_motion_nudge;
    unsigned bitrate;
    int max_q_step;
    int min_quality;
    int max_quality;
    int min_I_frame_quality;
    int intra_pct_thresh;
    int scene_change_delta;
    unsigned stable_refresh;
    int pyramid_levels;
    /* internal state (kept in the public struct by the reference, so kept here) */
    unsigned rc_quant;
    unsigned bpf_total;
    unsigned bpf_reset;
    int bpf_avg;
    int total_P_frame_q;
    int avg_P_frame_q;
    int last_P_frame_over;
    int back_into_range;
    DSV_FNUM next_fnum;
    void *ref;                   /* reference: DSV_ENCDATA*; here: opaque device session handle */
    DSV_META vidmeta;
    int prev_link;
    int force_metadata;
    struct DSV_STAB_ACC { signed x : 16; signed y : 16; } *stability;
    unsigned refresh_ctr;
    unsigned char *stable_blocks;
    DSV_FNUM prev_gop;
    int prev_avg_luma;
} DSV_ENCODER;

typedef struct {                 /* dsv_decoder.h:35-43 */
    DSV_META vidmeta;
    void *ref;                   /* reference: DSV_IMAGE*; here: opaque device session handle */
    int draw_info;               /* set by the user: DSV_DRAW_* bits, drawn on the GPU (debug overlays, below) */
    int got_metadata;
} DSV_DECODER;

#define DSV_DEC_OK        0
#define DSV_DEC_ERROR     1
#define DSV_DEC_EOS       2
#define DSV_DEC_GOT_META  3
#define DSV_DEC_NEED_NEXT 4

/* ---- encoder (dsv_encoder.h:112-121) ---- */
void dsv_enc_init(DSV_ENCODER *enc);
void dsv_enc_free(DSV_ENCODER *enc);
void dsv_enc_set_metadata(DSV_ENCODER *enc, DSV_META *md);
void dsv_enc_force_metadata(DSV_ENCODER *enc);
void dsv_enc_start(DSV_ENCODER *enc);
/* dsv_enc takes ownership of frame (its pixels are copied before the call returns).  CRF streams are coded with a LOOKAHEAD
 * (DSV1_ENC_LOOKAHEAD frames, default 16 GOPs): the call returns 0 buffers while the lookahead fills, then up to two packets
 * per call (metadata + picture, as the reference), always whole packets in stream order; dsv_enc_end_of_stream returns every
 * packet still owed followed by the EOS packet in bufs[0] (ONE buffer holding several packets: a caller that needs one
 * packet per DSV_BUF splits it on the packets' next-link words, or sets DSV1_ENC_PIPELINE=0 for the frame-synchronous
 * behaviour: one picture per call, same bytes).  Changes to the encoder's public fields between calls (quality, bitrate,
 * min_ / max_quality, min_I_frame_quality, max_q_step, rc_high_motion_nudge, dsv_enc_force_metadata) apply from the frame of
 * the NEXT call on, exactly as in the reference (it reads them when it codes a frame, dsv_encoder.c:84-165,794-803): the frames
 * gathered before the change are sent to the device as a short batch first (round 5).  dsv_enc_free without
 * dsv_enc_end_of_stream drops the frames still buffered (and logs it).  ABR streams (their pictures are coded one after the
 * other: every packet's size feeds the next quantiser) gather 32 frames (DSV1_ENC_LOOKAHEAD) for a common analysis pass: the same
 * contract with a shorter lookahead, the same bytes as the frame-synchronous encoder.
 * THE REFERENCE'S PACKET CONTRACT (dsv_encoder.c:766-810: one packet per DSV_BUF, at most two per dsv_enc call, exactly one EOS
 * packet from dsv_enc_end_of_stream) for a library caller that cannot split a buffer: before dsv_enc_end_of_stream, call
 *     while ((n = dsv_enc(enc, NULL, bufs)) > 0) { ...write bufs[0 .. n-1]... }
 * -- a FLUSH CALL (frame == NULL, an extension: the reference would crash on it).  The first one codes and collects everything
 * the session still holds; each returns up to two whole packets, one per DSV_BUF, in stream order; 0 = drained.
 * dsv_enc_end_of_stream then returns the 14-byte EOS packet alone.
 * OR ask for the reference's contract outright: dsv1_enc_set_strict_packets(enc, 1) after dsv_enc_init / dsv_enc_start and BEFORE the first
 * dsv_enc (an extension, round 6; an error once the session exists): the session then runs frame-synchronously -- every dsv_enc call codes its
 * frame and returns that frame's packets (metadata + picture, one per DSV_BUF), dsv_enc_end_of_stream returns the EOS packet alone, exactly
 * dsv_encoder.c:766-810 -- at the frame-at-a-time rate instead of the lookahead's. */
int  dsv1_enc_set_strict_packets(DSV_ENCODER *enc, int on);
int  dsv_enc(DSV_ENCODER *enc, DSV_FRAME *frame, DSV_BUF *bufs);
void dsv_enc_end_of_stream(DSV_ENCODER *enc, DSV_BUF *bufs);

/* ---- decoder (dsv_decoder.h:51-59) ---- */
int  dsv_dec(DSV_DECODER *d, DSV_BUF *buf, DSV_FRAME **out, DSV_FNUM *fn); /* frees buf */
DSV_META *dsv_get_metadata(DSV_DECODER *d);
void dsv_dec_free(DSV_DECODER *d);

/* ---- frames, buffers, allocator, logging, file helpers (dsv.h:160-247, util.h:31-34) ---- */
DSV_FRAME *dsv_mk_frame(int format, int width, int height, int border);
DSV_FRAME *dsv_load_planar_frame(int format, void *data, int width, int height);
DSV_FRAME *dsv_frame_ref_inc(DSV_FRAME *frame);
void dsv_frame_ref_dec(DSV_FRAME *frame);
void dsv_mk_buf(DSV_BUF *buf, int size);
void dsv_buf_free(DSV_BUF *buf);
void *dsv_alloc(int size);
/* Extension: while an encoder batch / session is open, dsv_free keeps blocks of 256 KB .. 64 MB (a batch's packet buffers) for the next
 * dsv_alloc instead of returning their pages to the system -- at most DSV1_RECYCLE_MAX_MB (default 1024) megabytes, DSV1_NO_RECYCLE=1:
 * never.  The parked blocks go back to the system when the last batch / session closes (and a block freed after that is freed for good);
 * dsv1_release_parked gives them back at once, dsv1_parked_bytes says how much is parked.  dsv1_recycle_hold(+1 / -1) is the count
 * behind that (a caller that wants parking without an open batch may hold it itself). */
void dsv1_release_parked(void);
size_t dsv1_parked_bytes(void);
int dsv1_recycle_hold(int delta);
/* host phases of dsv1_batch_submit / _collect (round 6): dsv1_host_prof_enable(1) clears and starts the sums, dsv1_host_prof_get returns the
 * number of phases and fills ms per submitted batch for the first n of them (dsv1_host_prof_name(k) says what phase k is); process-wide. */
/* threads (the calling one included) the session layer's parallel loops use in this process: DSV1_HOST_THREADS, else by the cores the process may
 * run on -- affinity mask, the container's CPU quota, the node's ranks (csrc/host/dsv1_util.c: dsv1_host_threads_rule) */
int dsv1_host_threads(void);
void dsv1_host_prof_enable(int on);
int dsv1_host_prof_get(double *ms_per_batch, int n, long *batches);
const char *dsv1_host_prof_name(int k);
void dsv1_debug_fail_alloc_at(int n);        /* tests: the n-th host allocation of the next dsv1_batch_open / dsv1_stream_open fails (0 = off) */
void dsv_free(void *ptr);
void dsv_memory_report(void);
void dsv_set_log_level(int level);
int  dsv_get_log_level(void);
int  dsv_yuv_write(FILE *out, int fno, DSV_PLANE *planes);
int  dsv_yuv_read(FILE *in, int fno, uint8_t *o, int w, int h, int subsamp);
void dsv_movec_pred(DSV_MV *vecs, DSV_PARAMS *p, int x, int y, int *px, int *py);
unsigned estimate_bitrate(int quality, int gop, DSV_META *md);
void conv444to422(DSV_PLANE *srcf, DSV_PLANE *dstf);
void conv422to420(DSV_PLANE *srcf, DSV_PLANE *dstf);

/* ---- extensions: device selection + batched closed-GOP encoding ---- */
void dsv1_set_device(int device);            /* HIP device used by sessions opened afterwards */

typedef struct dsv1_batch dsv1_batch;
/* cfg: a DSV_ENCODER filled like dsv_main.c:463-489 would (dsv_enc_init + fields + vidmeta);
 * nstreams independent streams, frames_per_call frames each per call. */
int  dsv1_batch_open(dsv1_batch **out, const DSV_ENCODER *cfg, int device, int nstreams, int frames_per_call);
/* ONE stream, GOP-parallel (the always-exact scheme): every call takes frames_per_call CONSECUTIVE frames of
 * the stream (yuv: [frame]; a last, shorter call is not supported here -- dsv_enc does that) and codes the chains of pictures
 * between I pictures side by side, max_chains at a time, after replaying the encoder's serial decisions (GOP starts,
 * scene changes, forced-intra pictures, stability flags: all functions of source pixels) on the host.  The stream equals
 * the frame-serial encoder's for every CRF configuration (dsv_encoder.c:345-399,538-552,624-653); ABR is refused.  Used
 * with dsv1_batch_encode / submit / collect / eos / close like a batch of one stream. */
int  dsv1_stream_open(dsv1_batch **out, const DSV_ENCODER *cfg, int device, int frames_per_call, int max_chains);
/* QUALITY LADDER: nsources sources, each coded at nrungs rate settings (rungs[r], 1 <= nrungs <= DSV1_MAX_RUNGS) from ONE upload
 * and ONE analysis.  Output stream k = s * nrungs + r is byte for byte the stream the reference encoder writes for source s with
 * rungs[r].  The rungs must agree on everything the source-only analysis reads -- vidmeta, gop, do_scd, scene_change_delta,
 * intra_pct_thresh, stable_refresh, pyramid_levels, rc_mode -- else DSVG_ERR_ARG before any device work; they may differ in the
 * rate-control fields (quality, bitrate, max_q_step, min_ / max_quality, min_I_frame_quality, rc_high_motion_nudge).  Every
 * dsv1_batch_* call works on a ladder: input (encode / submit / stage, every input form) is [source][frame], nsources x
 * frames_per_call frames; output buffers, eos, recon_slot, get_sse / get_ssim (sse[(k * frames_per_call + t) * 3 + p]) and
 * dsv1_batch_encoder are per output stream k.  dsv_enc_force_metadata on any rung starts a GOP on every rung of that source;
 * dsv1_batch_set_fnum(b, k, n) renumbers every rung of k's source.  A plain batch is a ladder of one rung. */
#define DSV1_MAX_RUNGS 16
int  dsv1_ladder_open(dsv1_batch **out, const DSV_ENCODER *rungs, int nrungs, int device, int nsources, int frames_per_call);
int  dsv1_batch_rungs(const dsv1_batch *b);   /* rungs per source: 1 for a plain batch */
void dsv1_batch_close(dsv1_batch *b);
void dsv1_batch_set_fnum(dsv1_batch *b, int stream, DSV_FNUM next_fnum);
/* Round 5: reference pictures nobody predicts from are coded without their reconstruction (no inverse transform; the packets are the
 * same -- the reference encoder builds that picture and never reads it, dsv_encoder.c:665-708).  Known exactly inside a call; for a call's
 * last picture when the next frame number starts a GOP, and if dsv1_batch_set_fnum then turns that GOP start into a P picture the next
 * submit codes the dropped picture again with its reconstruction kept (remedied) before it goes on.  Returns how many reconstructions
 * were dropped so far.  DSV1_RECON_ALL=1: every reference picture is reconstructed. */
long dsv1_batch_dropped_recons(const dsv1_batch *b, long *remedied);
/* the same switch as a call (between batches: nothing in flight): on != 0 reconstructs every reference picture from the next submit on */
int  dsv1_batch_recon_all(dsv1_batch *b, int on);
/* Quality measurement (opt-in): with it on, the device also sums, for every picture of the batches submitted afterwards, the squared
 * errors between the source and the reconstruction (what a decoder shows: DSV1 is closed-loop) per plane over the picture area,
 * borders excluded, chroma at its subsampled size -- an exact uint64_t, computed inside the frame steps (dsvg_ctx_sse_enable); the
 * packets are the same with it on or off.  PSNR = 10 log10(255^2 N / SSE) per plane, +inf for SSE 0; over the picture: sum SSE /
 * sum N.  Batch and chain mode (dsv1_stream_open), CRF and ABR, every input form.  dsv1_batch_sse_enable: only between batches
 * (nothing in flight, as dsv1_batch_recon_all), else DSVG_ERR_ARG.  dsv1_batch_get_sse: the sums of the batch returned by the
 * last dsv1_batch_collect / dsv1_batch_encode, sse[(s * frames_per_call + t) * 3 + p] for stream s (chain mode: one stream), frame t
 * in submitted order, plane p; n = room in values (>= nstreams * frames_per_call * 3); DSVG_ERR_ARG when that batch was not
 * measured or none has been collected.  Not offered: the drop-in dsv_enc and the decoders. */
int  dsv1_batch_sse_enable(dsv1_batch *b, int on);
int  dsv1_batch_get_sse(const dsv1_batch *b, uint64_t *sse, size_t n);
/* SSIM of the same pictures (opt-in, independent of the SSE: any combination): per picture and plane the fixed-point sum of
 * the 8x8 windows' SSIM at stride 4 (dsvg_ctx_ssim_enable, DSVG_SSIM_ONE) -- an exact int64; mean SSIM = ssim_fx /
 * (DSVG_SSIM_ONE * nwin[p]), over the picture sum ssim_fx / (DSVG_SSIM_ONE * sum nwin).  The packets are the same with it on
 * or off.  Same contract as the SSE pair: ssim_fx[(s * frames_per_call + t) * 3 + p]; enable only between batches; DSVG_ERR_ARG
 * when the batch collected last was not measured, none has been collected, or n is short. */
int  dsv1_batch_ssim_enable(dsv1_batch *b, int on);
int  dsv1_batch_get_ssim(const dsv1_batch *b, int64_t *ssim_fx, size_t n);
/* stream s's encoder struct (the batch owns it).  Its public parameter fields -- quality, bitrate, min_ / max_quality,
 * min_I_frame_quality, max_q_step, rc_high_motion_nudge; dsv_enc_force_metadata -- may be changed between submits, as a caller of
 * the reference changes them between dsv_enc calls; geometry, GOP structure and rate-control mode may not. */
DSV_ENCODER *dsv1_batch_encoder(dsv1_batch *b, int stream);
/* Encode frames_per_call frames of every stream.  yuv: [stream][frame] tightly packed planar frames,
 * host (yuv_on_device = 0) or device memory (1).  The call has finished with the clip when it returns (a device clip's chroma
 * planes are read in place by the coding kernels, dsvg_load_frames_map_ex, only luma is copied -- and the call returns after
 * the batch has been collected).  For each stream s the packets are appended to out[s] (a growing buffer the
 * caller owns: data = NULL / len = 0 to start; freed with dsv_free).  Returns 0 or a DSVG_ERR_*. */
int  dsv1_batch_encode(dsv1_batch *b, const void *yuv, int yuv_on_device, DSV_BUF *out);
/* Pipelined form (CRF): submit enqueues a batch and returns while its residual coding still runs on
 * the device; collect fetches + assembles the OLDEST submitted batch.  At most two batches may be in
 * flight, so the steady state is  submit(i+1); collect(i);  -- the analysis of batch i+1 (frame load,
 * pyramid, motion estimation: source pixels only) then overlaps the residual coding of batch i on a
 * second HIP stream, and the host packet assembly overlaps both.  ABR streams pipeline the same way since round 4: every
 * quantiser still follows from the size of the packet before, but that chain runs on the device (k_rc, include/dsvg_rc.h) and
 * the streams' rate-control state stays there from call to call; the session layer replays it on the host when it assembles the
 * packets (the encoder structs stay in step) and fails the batch (DSVG_ERR_RC) if the two ever disagree.  The rate-control
 * PARAMETERS (bitrate, quality bounds, max_q_step, rc_high_motion_nudge) are read from every stream's encoder struct
 * (dsv1_batch_encoder) at each submit: a change applies to every picture of the batches submitted after it -- the reference
 * reads them per frame (dsv_encoder.c:84-165), a batch is the unit here; batches already in flight keep what they were
 * submitted with, and so does their host-side replay.  DSV1_ABR_SERIAL=1: rounds 1-3's path -- submit codes frame by frame, assembles into out, and collect
 * only releases the slot. */
/* yuv_on_device for dsv1_batch_submit: 0 = host memory, 1 = device memory, copied whole -- submit has finished with the clip
 * when it returns; DSV1_CLIP_HELD = device memory that the caller keeps UNCHANGED until dsv1_batch_collect of this batch has
 * returned: chroma is then read in place by the coding kernels and only luma is copied (what bench.py times: 21 % less traffic
 * in the load stage).  Opt-in since round 4: a caller that reuses its clip right after submit gets correct streams with 1. */
#define DSV1_CLIP_HELD 2
int  dsv1_batch_submit(dsv1_batch *b, const void *yuv, int yuv_on_device, DSV_BUF *out);
int  dsv1_batch_collect(dsv1_batch *b, DSV_BUF *out);
/* Host-resident input (the .yuv reader of dsv_main.c:394-421): announce the host clip of a coming submit.  Its
 * upload is queued at once on a copy stream and runs under whatever the device is doing; up to two clips may be
 * staged, and dsv1_batch_submit(b, yuv_host, 0, ...) consumes the oldest one (it must be given the same pointer; a
 * submit with nothing staged starts the upload itself).  Asynchronous when yuv_host is pinned (dsvg_host_alloc): the
 * clip must stay unchanged until the collect of that batch returned.  Steady state, uploads back to back:
 *   stage(i+2); submit(i+1); collect(i). */
int  dsv1_batch_stage(dsv1_batch *b, const void *yuv_host);
/* append the end-of-stream packet of stream s */
int  dsv1_batch_eos(dsv1_batch *b, int stream, DSV_BUF *out);
/* Concatenate per-GOP streams (each encoded independently with fnum seeded to its position) into one
 * .dsv: rewrites the prev_link of every picture/EOS packet exactly as a serial encode would
 * (set_link_offsets dsv_encoder.c:171-192) and appends an EOS.  Returns dsv_alloc'd buffer. */
int  dsv1_concat_gops(const DSV_BUF *gops, int ngops, DSV_BUF *out);
void *dsv1_batch_ctx(dsv1_batch *b);          /* the dsvg_ctx* (profiling hooks) */
/* reconstruction slot that holds `stream`'s current reference picture (the encoder's recon_frame, dsv_encoder.c:663-674),
 * for dsvg_download_recon / dsvg_download_recon_raw; -1 if the stream has none yet */
int   dsv1_batch_recon_slot(const dsv1_batch *b, int stream);

/* ---- Submit plan (tests; csrc/host/dsv1_submit_plan.h; restated in tests/submit_plan.py) ----
 * What a submit decides, as plain tables: the session plans its call with the same pure functions, commits the state they return and
 * enqueues from their tables.  A call of nf frames of S sources x R rungs (output stream k = s * R + r), F frames per call at most;
 * the pictures lie [stream][F].
 *   dsv1_submit_src: a source's decision state (the encoder's fields; force_metadata OR-ed over the rungs).
 *   dsv1_submit_pic: a picture's decisions.  has_ref after the GOP / scene-change rules is a motion-search candidate; isP is final
 *     after the forced-intra rule (n_intra * 100 / nblk > intra_pct_thresh).  reach: min / max of the inter blocks' mv.x >> 1,
 *     mv.y >> 1, each taken with 0.  cur_slot / ref_slot: source slots (a ring of 2F + 1 rows of S); out_slot: where the packet waits.
 *   dsv1_submit_stream: an output stream's state.  rpar: which slot of its pair {k, k + N} holds the current reference; has_recon;
 *     border_skipped / recon_dropped: the call's last picture was coded with a short border / without a reconstruction because
 *     next_gop (the stream's next frame number starts a GOP) held.
 *   dsv1_submit_job: one device job in enqueue order: pic = index of its picture; remedy = the whole border, no reach.
 *   dsv1_submit_call: nsteps frame steps of njobs jobs each, jobs[first ..]. */
typedef struct { uint32_t next_fnum, prev_gop; int gop, force_metadata, do_scd, prev_avg_luma, scene_change_delta; } dsv1_submit_src;
typedef struct {
    uint32_t fnum;
    int gop_start, is_ref, has_ref, forced_intra, isP, n_intra;
    short reach[4];
    int cur_slot, ref_slot, out_slot;
} dsv1_submit_pic;
typedef struct { unsigned char rpar, has_recon, border_skipped, recon_dropped, next_gop; } dsv1_submit_stream;
typedef struct { int pic, ref_recon_slot, recon_slot, out_slot, border_hint, remedy; } dsv1_submit_job;
typedef struct { int nsteps, njobs, first; } dsv1_submit_call;
typedef struct {
    int S, R, F, nf;            /* nf < F needs S * R == 1 */
    int chains;                 /* 0: batch mode; else chain mode (S = R = 1), this many chains side by side */
    unsigned gcount;            /* frames per stream submitted before this call */
    int par;                    /* the half of the out slots this call uses: calls alternate 0, 1 */
    int npix_small;             /* pixels of the smallest pyramid level: luma sum / npix_small is the mean the scene-cut rule compares */
    int nblk, intra_pct_thresh;
    int abr, serial, keep_all;  /* ABR streams; their frame-by-frame host path; every reference picture reconstructed */
    int nf_prev;                /* frames of the call before (a remedy needs its pictures) */
    int carry[2];               /* chain mode, in and out: the pair / slot the open chain's newest reconstruction lives in (-1: none) */
    int npairs, next, nremedy, njobs, ncalls, dropped;      /* out: how much of each table was written */
} dsv1_submit_query;
/* the tables a plan writes, all the caller's */
typedef struct {
    dsv1_submit_pic *pics;              /* [S * R * F] */
    int *pair_cur, *pair_ref, *pair_pic;/* [S * F] each: the motion-search pairs (source slots, picture) */
    int *ext;                           /* [S * R] reconstruction slots to extend after all */
    int *remedy_streams;                /* [S * R] streams whose dropped reconstruction is needed after all ... */
    dsv1_submit_job *remedy;            /* [S * R] ... and the remedy call's jobs (pic: index into the call before's pictures) */
    dsv1_submit_job *jobs;              /* [S * R * F] in enqueue order */
    dsv1_submit_call *calls;            /* [F] (serial: one call per frame step) */
    int *scratch;                       /* [4 * (F + 1)] */
} dsv1_submit_tables;
/* One submit on plain arrays, no device.  In and out: q, src[S], st[S * R].  In: luma[(2F + 1) * S] raw sums by source slot (read with
 * do_scd), n_intra[S * R * F] for the lead rungs' motion-search candidates (in place of a motion search), prev[S * R * F] the pictures
 * of the call before (NULL: none).  Out: *tb.  DSVG_ERR_ARG for arguments a submit refuses, and for chain mode's P picture without a
 * reference picture. */
int   dsv1_submit_plan(dsv1_submit_query *q, dsv1_submit_src *src, dsv1_submit_stream *st, const unsigned *luma, const int *n_intra,
                       const dsv1_submit_pic *prev, const dsv1_submit_tables *tb);

/* ---- Rate control (tests; include/dsvg_rc.h as this layer compiles it; restated in tests/rc_model.py) ----
 * The functions of the average-bitrate chain on the caller's state, no device: the quantiser of the next picture (quality2quant
 * dsv_encoder.c:70-168), the statistics after a packet (dsv_encoder.c:816-848), the bits of a signed exp-Golomb code, the bytes of a
 * picture packet whose three planes carry dc[] and total_bits[] payload bits, and -- the host instantiation of what k_rc rewrites in a
 * job record -- the quantiser tables of a frame quantiser: out[76] = plane-major (qp, qp_h) of the ten scan regions of the three
 * planes, then hqp[16]. */
struct dsvg_rc_state;
int      dsv1_rc_pick(struct dsvg_rc_state *state, int isP, int forced_intra);
void     dsv1_rc_after(struct dsvg_rc_state *state, int isP, unsigned pkt_len);
unsigned dsv1_rc_seg_bits(int v);
unsigned dsv1_rc_packet_len(unsigned prefix_len, const int dc[3], const unsigned long long total_bits[3]);
void     dsv1_rc_job_tables(int quant, int isP, int out[76]);

/* ---- Source chain plan (tests; csrc/host/dsv1_srcchain_plan.h; restated in tests/srcchain_plan.py) ----
 * What the source side of a session (convert -> levels -> deinterlace or inverse telecine -> denoise -> orient -> reframe -> overlay)
 * decides, as plain data: the sessions answer every setter, reset and seek with dsv1_scp_set and enqueue every call from
 * dsv1_scp_call; the two queries below run the same functions on the caller's structs, with no device.
 *   dsv1_srcchain_state: the chain.  kind[p]: the pass at position p of the chain (DSV1_SC_NONE: none); the deinterlacer and the
 *     inverse telecine are the two occupants of position 2.  ov_clip[par]: the overlay pass's own clip of a call parity exists.
 *   dsv1_srcchain_req: one call.  valid: what the setting's own check said (dsv1_*_valid, the layout functions); identity: levels and
 *     reframe settings that change nothing (they clear the pass); mode: the converter's kind (1: RGB, 2: the HDR import), the deinterlacer's mode, the
 *     orientation's code (0 clears); busy: batches in flight or clips staged (a batch), calls in flight (a resolution ladder).
 *   dsv1_srcchain_geom: what follows from a state.  w x h raw (the frames that come in), mw x mh oriented, ow x oh canvas, with
 *     their packed planar frame bytes; conv_frames: frames per source the converter's and the levels' clips hold; frames_in /
 *     frame_in_bytes / bytes_in: what a call brings; lane: the chain holds a lane.
 *   dsv1_srcchain_set_plan: the answer to a request.  text: row of the refusal table (dsv1_srcchain_plan_text; 0: none).  noop: no
 *     pass before, none now.  Per position: alloc = bytes of each of its two clips to allocate, free_ = its clips go, reset = the
 *     pass's history or state goes (position 6: the picture counters start at 0).  All or nothing: a refusal changes nothing.
 *   dsv1_srcchain_call_plan: one call's clip through the chain.  src / dst of a step: DSV1_SC_CALLER (the clip as it came),
 *     DSV1_SC_UPLOAD (the lane's upload of it) or the position whose clip of the call's parity it is.  A step of kind DSV1_SC_NONE
 *     is the device-to-device copy (bytes; alloc: the clip is allocated first) of a caller's device clip that reaches the overlays
 *     untouched.  bypass: nothing is enqueued, the clip goes on as it came.  advance: every source's overlay counter moves by it. */
enum { DSV1_SC_NONE, DSV1_SC_CONVERT, DSV1_SC_LEVELS, DSV1_SC_DEINTERLACE, DSV1_SC_IVTC, DSV1_SC_DENOISE, DSV1_SC_ORIENT, DSV1_SC_REFRAME,
       DSV1_SC_OVERLAY, DSV1_SC_KINDS };
enum { DSV1_SC_SLOTS = 7, DSV1_SC_MAX_STEPS = 8 };
enum { DSV1_SC_OP_SET, DSV1_SC_OP_RESET, DSV1_SC_OP_SEEK };
enum { DSV1_SC_CALLER = -1, DSV1_SC_UPLOAD = -2 };
typedef struct {
    int nsrc, F, subsamp, keep_lane, ow, oh;
    int kind[DSV1_SC_SLOTS];
    int conv_rgb;                       /* the converter's kind: 0 the re-packing one, 1 the RGB import, 2 the HDR import */
    size_t conv_fb;                     /* bytes of a frame of the converter's source format */
    int deint_mode, orient;
    int in_w, in_h;                     /* the reframe's input */
    int ov_clip[2];
} dsv1_srcchain_state;
typedef struct { int op, kind, set, valid, identity, busy, mode, w, h, out_w, out_h, source; size_t frame_bytes; } dsv1_srcchain_req;
typedef struct { int w, h, mw, mh, ow, oh, conv_frames, frames_in, lane; size_t fb, mfb, ofb, frame_in_bytes, bytes_in; } dsv1_srcchain_geom;
typedef struct {
    int rc, text, noop;
    dsv1_srcchain_state next;
    dsv1_srcchain_geom g;               /* of next */
    size_t alloc[DSV1_SC_SLOTS];
    int free_[DSV1_SC_SLOTS], reset[DSV1_SC_SLOTS];
} dsv1_srcchain_set_plan;
typedef struct { int kind, pos, nframes, src, dst; size_t bytes, alloc; } dsv1_srcchain_step;
typedef struct {
    int rc, bypass, nsteps, out, advance;
    size_t upload;
    dsv1_srcchain_step step[DSV1_SC_MAX_STEPS];
} dsv1_srcchain_call_plan;
/* One request / one call (form: 0 host memory, 1 a plain device clip, DSV1_CLIP_HELD; active: the overlays blend something in this
 * call; par: the call's parity) on plain structs, no device.  They return out->rc: DSVG_ERR_ARG for what the session refuses (and,
 * with *out as it was, for what is no request: a kind that is no pass, a reset of a pass that keeps nothing, a seek of another). */
int   dsv1_srcchain_plan_set(const dsv1_srcchain_state *s, const dsv1_srcchain_req *q, dsv1_srcchain_set_plan *out);
int   dsv1_srcchain_plan_call(const dsv1_srcchain_state *s, int form, int active, int par, dsv1_srcchain_call_plan *out);
const char *dsv1_srcchain_plan_text(int row);       /* the refusal table's row (NULL past its end; row 0 is empty) */
/* what a call of the session must bring, straight from its chain: in[0] frames per source, in[1] x in[2] the raw picture;
 * *frame_bytes: bytes from frame to frame */
int   dsv1_batch_source_input(const dsv1_batch *b, int in[3], size_t *frame_bytes);

/* ---- extension: the resampler of resolution ladders (csrc/k_scale.hip; stated in numpy in tests/_scale.py) ----
 * Downscale or identity: on each axis of each plane 1 <= S / D <= 8 (S source length, D destination length); every plane is scaled
 * on its own, from the source's chroma dims to the destination's (rshift_up); the format is kept.  Centre-aligned sample grids;
 * chroma siting is not modelled.  Filters, stretched by S / D (anti-aliasing): DSV1_SCALE_TENT (linear, support 1) and
 * DSV1_SCALE_CUBIC (Catmull-Rom, a = -0.5, support 2).  Weight table of one axis: output sample i reads the T = 2 ceil(support S / D)
 * + 2 source samples start[i] .. start[i] + T - 1 (clamped to [0, S - 1]) with the integer weights q[i * T + t], which sum to 16384;
 * built in binary64 in a fixed order, no contraction (dsv1_scale.c).  Arithmetic, horizontal pass first: H = sum qh P (int32),
 * Hs = (H + 128) >> 8; V = sum qv Hs (int32); out = clamp((V + 2^19) >> 20, 0, 255).  S == D is the identity for both filters. */
#define DSV1_SCALE_TENT  0
#define DSV1_SCALE_CUBIC 1
int  dsv1_scale_taps(int S, int D, int filter);              /* T of an axis, or DSVG_ERR_ARG outside the limits */
int  dsv1_scale_weights(int S, int D, int filter, int32_t *start, int16_t *q, int T);   /* start[D], q[D * T]; host only */
/* n packed planar frames sw x sh -> dw x dh (any sizes within the ratio limits, odd ones included), host or device memory
 * (on_device: src and dst are device pointers).  Synchronous: the frames are in dst when it returns. */
int  dsv1_scale_clip(int device, const void *src, int sw, int sh, int subsamp, int n, void *dst, int dw, int dh, int filter,
                     int on_device);
/* The same resampler in both directions: on each axis of each plane 1/8 <= S / D <= 8, anamorphic included (an axis may go up while
 * the other goes down).  The kernel is stretched only to downscale: inv = min(1, D / S), r = ceil(support max(1, S / D)),
 * T = 2r + 2, taps floor(c) - r .. floor(c) + r + 1 with c = ((2i+1) S - D) / (2D), w = K(|j - c| inv); the same binary64 build,
 * rint and remainder rule, clamped source indices and two-pass integer arithmetic as above.  Where S >= D the tables ARE
 * dsv1_scale_weights', bit for bit; S == D is the identity.  Stated in numpy in tests/_resample.py.  dsv1_scale_* keep refusing
 * S < D. */
int  dsv1_resample_taps(int S, int D, int filter);           /* T of an axis, or DSVG_ERR_ARG outside the limits */
int  dsv1_resample_weights(int S, int D, int filter, int32_t *start, int16_t *q, int T);   /* start[D], q[D * T]; host only */
int  dsv1_resample_clip(int device, const void *src, int sw, int sh, int subsamp, int n, void *dst, int dw, int dh, int filter,
                        int on_device);               /* as dsv1_scale_clip, every axis of every plane either way */

/* RESOLUTION LADDER: nsources sources of geometry *src, each coded at ngeoms (1..DSV1_MAX_GEOMS) geometries, at every rate rung of
 * that geometry.  rungs[g]: width x height (the format of the source) and nrates (1..DSV1_MAX_RUNGS) DSV_ENCODER rate rungs whose
 * vidmeta is that geometry, with the agreement rules of dsv1_ladder_open among them.  Built as one quality ladder per geometry
 * (dsv1_resladder_batch: every dsv1_batch_* call works on it); the source crosses the link once per call, each geometry's scale
 * (filter: DSV1_SCALE_*) is ordered on the device before that geometry's frame load, and the scaled clips are held by the resladder
 * (double-buffered) until that geometry's collect.  A geometry of the source's size is not scaled.  Output stream
 * k = s * Ntot + off[g] + rate, Ntot = sum of nrates, off[g] = sum of nrates of the geometries before g; output buffers, eos, encoder(k)
 * and get_sse / get_ssim (sse[(k * frames_per_call + t) * 3 + p], against the SCALED source that stream's encoder saw) are per k.
 * Input: [source][frame], nsources x frames_per_call frames of the source geometry, the three forms of dsv1_batch_submit.
 * Refused before any device allocation: a rung larger than the source or below 1 / 8 of it on an axis of a plane, another format,
 * a bad filter, ngeoms outside 1..16, an empty rate list (DSVG_ERR_ARG); a geometry dsv1_batch_open would not accept (its code).
 * Not offered: stage, chain mode, the drop-in dsv_enc, the decoders, rungs larger than the source.  (Upscaling as such:
 * dsv1_resample_clip; measuring rungs at the source resolution: dsv1_resladder_src_quality_enable below.) */
#define DSV1_MAX_GEOMS 16
typedef struct {
    int width, height;
    int nrates;
    const DSV_ENCODER *rates;
} dsv1_res_rung;
typedef struct dsv1_resladder dsv1_resladder;
/* what a call of the ladder must bring, straight from its source chain (as dsv1_batch_source_input) */
int  dsv1_resladder_source_input(const dsv1_resladder *r, int in[3], size_t *frame_bytes);
int  dsv1_resladder_open(dsv1_resladder **out, const DSV_META *src, const dsv1_res_rung *rungs, int ngeoms, int device, int nsources,
                         int frames_per_call, int filter);
void dsv1_resladder_close(dsv1_resladder *r);
int  dsv1_resladder_nstreams(const dsv1_resladder *r);       /* nsources * Ntot */
dsv1_batch *dsv1_resladder_batch(dsv1_resladder *r, int g);  /* geometry g's quality ladder (its streams: s * nrates[g] + rate) */
DSV_ENCODER *dsv1_resladder_encoder(dsv1_resladder *r, int k);
int  dsv1_resladder_encode(dsv1_resladder *r, const void *yuv, int yuv_on_device, DSV_BUF *out);
int  dsv1_resladder_submit(dsv1_resladder *r, const void *yuv, int yuv_on_device, DSV_BUF *out);   /* at most two in flight */
int  dsv1_resladder_collect(dsv1_resladder *r, DSV_BUF *out);
int  dsv1_resladder_eos(dsv1_resladder *r, int k, DSV_BUF *out);
int  dsv1_resladder_sse_enable(dsv1_resladder *r, int on);
int  dsv1_resladder_ssim_enable(dsv1_resladder *r, int on);
int  dsv1_resladder_get_sse(const dsv1_resladder *r, uint64_t *sse, size_t n);
int  dsv1_resladder_get_ssim(const dsv1_resladder *r, int64_t *ssim_fx, size_t n);
/* host-to-device bytes the resladder uploaded itself so far (host input: one source clip per call, whatever ngeoms is) and calls */
int  dsv1_resladder_uploads(const dsv1_resladder *r, uint64_t *bytes, long *calls);
/* Rungs measured at the SOURCE resolution (opt-in, off after open; the packets are the same with it on or off): every picture's
 * reconstruction upscaled to the source's plane dims with the dsv1_resample_* tables of `filter` (DSV1_SCALE_*; a geometry of the
 * source's size goes through the identity tables) and compared with the ORIGINAL source frame of its (source, frame), on the GPU
 * right behind the picture's reconstruction (k_xres_quality, one pass): per plane the SSE over the source plane area (uint64) and
 * SSIM_FX over the 8x8 windows at stride 4 of the source plane dims (the definition of dsv1_batch_get_ssim), so the figures of
 * every geometry are comparable.  Independent of the rung-resolution get_sse / get_ssim: any combination may be on.
 * src_quality_enable: only between calls (nothing in flight), else DSVG_ERR_ARG; DSVG_ERR_ARG for a bad filter.  get_src_*: the
 * figures of the call collected last, [(k * frames_per_call + t) * 3 + p]; DSVG_ERR_ARG when that call was not measured or n is
 * short.  The source is read until the call's collect: host input from the resladder's upload buffer, a DSV1_CLIP_HELD clip in
 * place (the caller's promise); a plain device clip (yuv_on_device = 1) is the caller's again when submit returns, so with the
 * measurement on submit first copies it device to device into the resladder's buffer of the call's parity (one clip's bytes of
 * HBM traffic each way per call; off, nothing is copied). */
int  dsv1_resladder_src_quality_enable(dsv1_resladder *r, int sse_on, int ssim_on, int filter);
int  dsv1_resladder_get_src_sse(const dsv1_resladder *r, uint64_t *sse, size_t n);
int  dsv1_resladder_get_src_ssim(const dsv1_resladder *r, int64_t *ssim_fx, size_t n);

/* ---- extension: pixel formats, in (csrc/k_pixfmt.hip; stated in numpy in tests/_pixfmt.py) and out (csrc/k_pixout.hip;
 * tests/_pixout.py) ----
 * What a decoder- or capture-fed caller has: NV12 / NV16 / NV21 / NV61, P010 / P210, planar 10 / 12 / 16 bits, YUY2 / UYVY, with row
 * pitches and a frame stride.  Converted on the device to the tightly packed planar 8-bit frames every other entry point reads; the
 * subsampling is kept.  With cw x ch the chroma dims (rshift_up):
 *   planar:      Y w x h, U and V cw x ch samples;
 *   semi-planar: Y w x h, then ONE plane of ch rows of cw (U, V) pairs -- or (V, U) pairs;
 *   packed:      h rows of cw macro-pixels Y0 U Y1 V (YUYV) or U Y0 V Y1 (UYVY); the second luma of the last macro-pixel of an
 *                odd-width row is padding.
 * A sample of depth 8 is its byte.  A sample word x (little-endian 16 bits) of depth d > 8: v = msb_aligned ? x >> (16 - d) :
 * x & (2^d - 1), output min(255, (v + 2^(d-9)) >> (d - 8)) -- round half up, clamp; one rule, no dither.
 * Valid: planar with any subsampling and depth; semi-planar with 4:2:0 or 4:2:2, any depth; packed with 4:2:2 and depth 8.  A pitch
 * below a row's bytes, a frame_bytes below the planes, an unknown layout or depth, msb_aligned outside 0 / 1 at a depth above 8, or
 * any other combination is invalid: dsv1_pix_frame_bytes returns 0 and every entry point DSVG_ERR_ARG before any device work.
 * Padding bytes (pitch beyond the row, frame stride beyond the planes, the unused luma of an odd packed row) never reach the output.
 * The same dsv1_pix_format describes what the batched decoder and dsv1_export_clip WRITE (below: decoder output formats), with an
 * output subsampling beside it. */
#define DSV1_PIX_PLANAR        0
#define DSV1_PIX_SEMIPLANAR_UV 1     /* NV12 / NV16 / P010 / P210 */
#define DSV1_PIX_SEMIPLANAR_VU 2     /* NV21 / NV61 */
#define DSV1_PIX_PACKED_YUYV   3     /* YUY2 */
#define DSV1_PIX_PACKED_UYVY   4
typedef struct {
    int layout;        /* DSV1_PIX_* */
    int depth;         /* 8, 10, 12 or 16 significant bits; > 8: little-endian 16-bit words */
    int msb_aligned;   /* depth > 8 only: 1 = value in the upper bits (P010), 0 = in the lower bits (yuv420p10le) */
    int pitch[3];      /* bytes from row to row of plane 0 / 1 / 2; 0 = tight.  Semi-planar: pitch[1] is the UV plane's, pitch[2]
                          unused.  Packed: pitch[0] only */
    size_t frame_bytes;/* bytes from frame to frame; 0 = tight (the planes back to back, each pitch x rows) */
} dsv1_pix_format;
size_t dsv1_pix_frame_bytes(const dsv1_pix_format *pf, int w, int h, int subsamp);   /* 0 = invalid combination */
/* n frames of format *pf, frame_bytes apart -> n tightly packed planar 8-bit frames in dst; host or device memory (on_device: src
 * and dst are device pointers).  Any w, h >= 1.  Synchronous: the frames are in dst when it returns.  The last frame's frame_bytes
 * is the end of the source buffer: nothing beyond it is read. */
int  dsv1_convert_clip(int device, const void *src, const dsv1_pix_format *pf, int w, int h, int subsamp, int n, void *dst,
                       int on_device);
/* From the next submit on, dsv1_batch_encode / submit take clips of format *pf ([stream or source][frame], frame_bytes apart); only
 * between batches (nothing in flight, no clip staged), else DSVG_ERR_ARG.  NULL, or planar / 8 bits / tight, switches back.  Host
 * input is uploaded raw and converted on the device, with no host synchronisation between upload, conversion and frame load; a
 * plain device clip (yuv_on_device = 1) is the caller's again when submit returns (submit waits for the conversion); a
 * DSV1_CLIP_HELD clip stays unchanged until that batch's collect and submit does not wait.  The converted clip lives in buffers
 * the batch owns (one per call parity) and goes on as a held clip.  Plain batches, quality ladders (per source) and chain mode.
 * dsv1_batch_stage returns DSVG_ERR_ARG while a format is set.  Not offered: the drop-in dsv_enc and dsv_dec (it returns a host
 * DSV_FRAME).  Another subsampling than the stream's, in and out: chroma resampling, below.  RGB, in and out: the extension at the
 * end of this file. */
int  dsv1_batch_set_source_format(dsv1_batch *b, const dsv1_pix_format *pf);
/* dsv1_resladder_open for sources of format *pf (NULL or the default: dsv1_resladder_open itself).  The conversion runs on the
 * scaler's stream in front of the scales; a geometry of the source's size and dsv1_resladder_src_quality_enable read the CONVERTED
 * clip, which the resladder holds (per call parity) until collect -- get_src_sse / get_src_ssim measure against the 8-bit source
 * the encoders saw.  dsv1_resladder_uploads counts the raw bytes that crossed the link, once per call. */
int  dsv1_resladder_open_src(dsv1_resladder **out, const DSV_META *src, const dsv1_pix_format *pf, const dsv1_res_rung *rungs,
                             int ngeoms, int device, int nsources, int frames_per_call, int filter);

/* ---- extension: batched decoding (dsv_dec decodes one picture per call, dsv_decoder.c:286-472) ----
 * nstreams independent streams of one geometry; every call takes ONE packet per stream (packets[s]: not freed, not
 * modified) and decodes all picture packets among them as one device batch.  status[s] = DSV_DEC_OK (a frame was
 * written), DSV_DEC_GOT_META, DSV_DEC_EOS or DSV_DEC_ERROR; fnum[s] = frame number (-1 if none).  The decoded frame
 * of stream s is written tightly packed planar (Y, U, V) at yuv_out + s*out_pitch (out_pitch 0 = frame size), in
 * device memory (asynchronous: dsvg_ctx_sync(dsv1_decbatch_ctx(d)) before reading) or host memory (synchronised).
 * Reference pictures stay resident on the device.  Returns 0 or a DSVG_ERR_*.
 *
 * DECODER OUTPUT FORMATS (csrc/k_pixout.hip; stated in numpy in tests/_pixout.py).  With a format set, ONE pass reads the decoded
 * pictures and writes frames of dsv1_pix_format *pf (layouts, pitches and frame stride as for sources) at subsampling out_subsamp,
 * in the place of the packed planar pass.  out_subsamp: the streams' own; 4:2:2 from 4:4:4 streams; 4:2:0 from 4:4:4 or 4:2:2 streams
 * (the reference CLI's -out420p, on the device); every other pair -- anything from 4:1:1, any upsampling -- is DSVG_ERR_ARG, and so
 * is a layout that is not valid at out_subsamp (dsv1_pix_frame_bytes(pf, w, h, out_subsamp) == 0).  Luma is untouched; with cw x ch a
 * chroma plane of the stream, horizontal halving is o[y][i] = (c[y][2i] + c[y][min(2i+1, cw-1)] + 1) >> 1 for i < (cw+1)/2, vertical
 * halving o[j][x] = (c[2j][x] + c[min(2j+1, ch-1)][x] + 1) >> 1 for j < (ch+1)/2, 4:4:4 -> 4:2:0 the horizontal step, rounded to 8
 * bits, then the vertical one (conv444to422 / conv422to420, in the order dsv_main.c applies them).  A sample v of depth 8 is its
 * byte; of depth d > 8 the little-endian word v << (d - 8), moved up by 16 - d when msb_aligned (v << 8: P010), every other bit
 * zero -- so dsv1_convert_clip of the output gives the planar frames back.  Never written: the bytes between a row's end and its
 * pitch, between the planes' end and frame_bytes, beyond the last frame's planes; the second luma byte of the last macro-pixel of
 * an odd-width packed row repeats the row's last luma sample.
 * dsv1_decbatch_set_output_format: between calls; from the next decode call on.  pf == NULL, or planar / 8 bits / tight with the
 * streams' own subsampling, switches back to the packed planar pass.  An invalid combination is DSVG_ERR_ARG and leaves the
 * setting in force as it was.  The setting outlives the context the batch rebuilds on a change of block size.
 * dsv1_decbatch_out_frame_bytes: what one output frame occupies under the setting in force -- out_pitch when 0 is passed;
 * a smaller out_pitch is DSVG_ERR_ARG.  Frame s at yuv_out + s * out_pitch; streams without a picture in a call keep their frame.
 * dsv1_export_clip: the standalone twin of dsv1_convert_clip: n tightly packed planar 8-bit frames (w x h at subsamp) -> n frames
 * of *pf at out_subsamp, frame_bytes apart, host or device memory (on_device: both), any w, h >= 1, synchronous; the last frame
 * ends with its planes. */
typedef struct dsv1_decbatch dsv1_decbatch;
int  dsv1_decbatch_open(dsv1_decbatch **out, int device, const DSV_META *meta, int nstreams);
int  dsv1_decbatch_decode(dsv1_decbatch *d, const DSV_BUF *packets, void *yuv_out, size_t out_pitch, int out_on_device,
                          int *status, DSV_FNUM *fnum);
void dsv1_decbatch_close(dsv1_decbatch *d);
int  dsv1_decbatch_set_output_format(dsv1_decbatch *d, const dsv1_pix_format *pf, int out_subsamp);
size_t dsv1_decbatch_out_frame_bytes(const dsv1_decbatch *d);
int  dsv1_export_clip(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsv1_pix_format *pf, int out_subsamp,
                      int on_device);
void *dsv1_decbatch_ctx(dsv1_decbatch *d);      /* (ask again after every decode call: the batch builds a new context when its streams
                                                  * announce another block size while none of them holds a reference picture) */

/* ---- extension: chroma resampling in the source and output passes (csrc/k_pixfmt.hip, csrc/k_pixout.hip; stated in numpy in
 * tests/_chroma.py) ----
 * The entry points above keep the subsampling (sources) or halve it (output) and refuse everything else; these take the other
 * subsampling beside the format.  In both directions a pair with 4:1:1 on one side only is DSVG_ERR_ARG.
 * IN, halving: a source of format *pf at src_subsamp into frames at `subsamp`.  Pairs: 4:4:4 -> 4:2:2 or 4:2:0, 4:2:2 -> 4:2:0; equal
 * subsamplings are the pass above; upsampling on the way in is DSVG_ERR_ARG.  Every layout that is valid at src_subsamp
 * (dsv1_pix_frame_bytes(pf, w, h, src_subsamp) != 0) is taken: planar for all three pairs, NV16 / NV61 / P210 and YUYV / UYVY for 4:2:2
 * -> 4:2:0.  Every sample is reduced to 8 bits first (the depth rule above); the 8-bit chroma planes are then halved as the decoder
 * output pass halves them -- the horizontal step, rounded to 8 bits, then the vertical one, the last column and the last row
 * repeated -- in the same launch, with no intermediate plane:
 *   dsv1_convert_clip_sub(buf, pf, src_subsamp -> subsamp) == dsv1_export_clip(dsv1_convert_clip(buf, pf, src_subsamp), planar 8-bit
 *   tight, src_subsamp -> subsamp),
 * the composition the RGB import follows.  Not offered: halving at the source depth before the reduction, dither.
 * dsv1_batch_set_source_format_sub: dsv1_batch_set_source_format with its contract (ownership, staging, in flight, plain batches,
 * quality ladders, chain mode) for clips at src_subsamp; the target is the batch's vidmeta.subsamp.  pf == NULL: tight planar 8-bit
 * at src_subsamp.  The source setters replace each other.  The deinterlacer and the noise filter run behind the converter, at the
 * batch's subsampling.  dsv1_resladder_open_src_sub: dsv1_resladder_open_src for such sources; the converted clip at src->subsamp
 * stands for the source (scales, a geometry of the source's size, get_src_sse / get_src_ssim); dsv1_resladder_uploads counts the raw
 * bytes.
 * OUT, upsampling: frames decoded at `subsamp` written at out_subsamp.  dsv1_export_clip_up and dsv1_decbatch_set_output_format_up
 * take every pair the calls above take and 4:2:0 -> 4:2:2, 4:2:0 -> 4:4:4, 4:2:2 -> 4:4:4; the layout must be valid at out_subsamp (4:2:2:
 * planar, NV16 / NV61, P210, YUYV / UYVY; 4:4:4: planar).  `upsample` is DSV1_CHROMA_REPLICATE or DSV1_CHROMA_LINEAR (RGB, below),
 * validated always and read only where something goes up.  The chroma planes are brought to the output's chroma dims ocw x och
 * (rshift_up of w x h at out_subsamp) as the RGB output pass brings them to the luma grid.  REPLICATE: c[y >> dv][x >> dh], dv / dh 1
 * where the vertical / horizontal shift drops.  LINEAR, centre-sited: vertically first where the vertical shift drops, o[2j] =
 * (3 c[j] + c[max(j - 1, 0)] + 2) >> 2, o[2j+1] = (3 c[j] + c[min(j + 1, ch - 1)] + 2) >> 2, rows at or beyond och dropped; then the same
 * over columns, on that 8-bit result, where the horizontal shift drops, columns at or beyond ocw dropped.  Each sample is then
 * written by the output rule above (depth, msb_aligned, padding never written, the odd-width packed row).  So
 * dsv1_rgb_export_clip(x at 4:2:0, rf) == dsv1_rgb_export_clip(dsv1_export_clip_up(x, planar 8-bit tight, 4:4:4, rf->upsample), rf).
 * dsv1_decbatch_set_output_format_up: the contract of dsv1_decbatch_set_output_format (one pass in the place of the packing pass;
 * dsv1_decbatch_out_frame_bytes follows; the int32 second pass writes its frames again; the setting outlives a rebuilt context; an
 * invalid call leaves the setting in force as it was).  The three output setters replace each other.
 * Not offered: chroma siting other than centre, the drop-in dsv_enc / dsv_dec. */
int  dsv1_convert_clip_sub(int device, const void *src, const dsv1_pix_format *pf, int w, int h, int src_subsamp, int subsamp, int n,
                           void *dst, int on_device);
int  dsv1_batch_set_source_format_sub(dsv1_batch *b, const dsv1_pix_format *pf, int src_subsamp);
int  dsv1_resladder_open_src_sub(dsv1_resladder **out, const DSV_META *src, const dsv1_pix_format *pf, int src_subsamp,
                                 const dsv1_res_rung *rungs, int ngeoms, int device, int nsources, int frames_per_call, int filter);
int  dsv1_export_clip_up(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsv1_pix_format *pf,
                         int out_subsamp, int upsample, int on_device);
int  dsv1_decbatch_set_output_format_up(dsv1_decbatch *d, const dsv1_pix_format *pf, int out_subsamp, int upsample);

/* ---- extension: RGB, in and out (csrc/k_rgb.hip; stated in numpy in tests/_rgb.py) ----
 * What renderers, capture and displays hold: 8-bit RGB, packed or planar.  Unlike the pixel formats above this is no re-packing: a
 * matrix, a range, chroma downsampling on the way in and upsampling on the way out.  Exact integers, no floating point at run time.
 * LAYOUTS.  RGB24 / BGR24: 3 bytes per pixel, one plane.  RGBA / BGRA / ARGB / ABGR: 4 bytes per pixel; the A byte is ignored on input
 * and written as 255 on output.  PLANAR_RGB / PLANAR_GBR: three planes of w x h bytes in that order.  pitch[p]: bytes from row to row
 * of plane p, 0 = tight (packed orders: pitch[0] only); frame_bytes: frame to frame, 0 = tight.  Any w, h >= 1.  Padding bytes (a
 * pitch beyond the row, a stride beyond the planes, everything beyond the last frame's planes) are never read into a result and
 * never written.  A pitch below a row's bytes, a frame_bytes below the planes, an unknown order, matrix or upsampling mode, or
 * full_range outside 0 / 1: dsv1_rgb_frame_bytes returns 0 and every entry point DSVG_ERR_ARG before any device work.  4:1:1 with RGB
 * is DSVG_ERR_ARG in both directions.
 * MATRIX AND RANGE.  BT.601 (Kr 0.299, Kb 0.114), BT.709 (0.2126, 0.0722), BT.2020 non-constant-luminance (0.2627, 0.0593); Kg = 1 -
 * Kr - Kb.  full_range 0: sy = 219/255, sc = 224/255, oy = 16; 1: sy = sc = 1, oy = 0.  r() rounds an exact rational half up.
 * Forward, Q16: the Y row (R, G, B) is r(65536 sy Kr), the remainder of r(65536 sy), r(65536 sy Kb); with hf = r(65536 sc / 2) the Cb
 * row is -r(65536 sc Kr / (2 (1 - Kb))), -(hf + that), hf and the Cr row hf, -(hf + the B coefficient), -r(65536 sc Kb / (2 (1 - Kr))).
 * Inverse, Q14: IY = r(16384 / sy), RV = r(16384 * 2 (1 - Kr) / sc), GU = -r(16384 * 2 (1 - Kb) Kb / (Kg sc)), GV = -r(16384 * 2 (1 -
 * Kr) Kr / (Kg sc)), BU = r(16384 * 2 (1 - Kb) / sc).  dsv1_rgb_tables returns the literals the library holds: fwd = the three rows,
 * inv = IY, RV, GU, GV, BU.
 * IN.  Per pixel, int32, >> arithmetic: Y = clamp((Yrow . (R, G, B) + (oy << 16) + 32768) >> 16), Cb / Cr = clamp((row . (R, G, B) +
 * (128 << 16) + 32768) >> 16), clamp to 0..255 (it binds: full-range pure blue and red give 256).  The 8-bit 4:4:4 chroma planes are
 * then halved as the decoder output pass halves (conv444to422 / conv422to420: (a + b + 1) >> 1 over column pairs, the last column
 * repeated, rounded to 8 bits, then over row pairs), so import(rgb, S) == dsv1_export_clip(import(rgb, 4:4:4), 4:4:4 -> S).
 * OUT.  Chroma is brought to the luma grid first (hs / vs the streams' chroma shifts).  DSV1_CHROMA_REPLICATE: c[y >> vs][x >> hs].
 * DSV1_CHROMA_LINEAR, centre-sited, the mirror of the halving: vertically first where vs = 1, o[2j] = (3 c[j] + c[max(j - 1, 0)] + 2)
 * >> 2, o[2j+1] = (3 c[j] + c[min(j + 1, ch - 1)] + 2) >> 2, rows at or beyond h dropped; then the same over columns, on that 8-bit
 * result, where hs = 1.  With y = Y - oy, u = Cb - 128, v = Cr - 128: R = clamp((IY y + RV v + 8192) >> 14), G = clamp((IY y + GU u +
 * GV v + 8192) >> 14), B = clamp((IY y + BU u + 8192) >> 14).  `upsample` is read on output only (but validated always).
 * Not offered: chroma siting other than centre, dither, float RGB and deeper RGB frames (deep YCbCr with a PQ or HLG transfer: HDR
 * sources, below), constant-luminance BT.2020, transfer functions on 8-bit RGB (the PQ and HLG curves of deep sources: HDR sources). */
#define DSV1_RGB_RGB24      0
#define DSV1_RGB_BGR24      1
#define DSV1_RGB_RGBA       2
#define DSV1_RGB_BGRA       3
#define DSV1_RGB_ARGB       4
#define DSV1_RGB_ABGR       5
#define DSV1_RGB_PLANAR_RGB 6
#define DSV1_RGB_PLANAR_GBR 7
#define DSV1_MATRIX_BT601   0
#define DSV1_MATRIX_BT709   1
#define DSV1_MATRIX_BT2020  2        /* non-constant luminance */
#define DSV1_CHROMA_REPLICATE 0
#define DSV1_CHROMA_LINEAR    1
typedef struct { int order, matrix, full_range, upsample; int pitch[3]; size_t frame_bytes; } dsv1_rgb_format;
size_t dsv1_rgb_frame_bytes(const dsv1_rgb_format *rf, int w, int h);                 /* 0 = invalid */
int  dsv1_rgb_tables(int matrix, int full_range, int32_t fwd[9], int32_t inv[5]);      /* host only */
/* n RGB frames -> n tightly packed planar 8-bit frames at `subsamp` (4:4:4, 4:2:2, 4:2:0) and back; host or device memory
 * (on_device: src and dst are device pointers), synchronous; the last RGB frame ends with its planes. */
int  dsv1_rgb_import_clip(int device, const void *src, const dsv1_rgb_format *rf, int w, int h, int subsamp, int n, void *dst,
                          int on_device);
int  dsv1_rgb_export_clip(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsv1_rgb_format *rf,
                          int on_device);
/* dsv1_batch_set_source_format for RGB clips, with its contract (between batches only; host input uploaded raw and converted on the
 * converter's stream with no host wait; a plain device clip is the caller's again when submit returns; a DSV1_CLIP_HELD clip stays
 * unchanged until collect; dsv1_batch_stage is refused while set; plain batches, quality ladders, chain mode).  The target
 * subsampling is the batch's vidmeta.subsamp.  The two setters replace each other; NULL switches back to packed planar.  An invalid
 * format leaves the setting in force as it was. */
int  dsv1_batch_set_source_rgb(dsv1_batch *b, const dsv1_rgb_format *rf);
/* dsv1_resladder_open_src with the RGB converter in its place: the converted clip stands for the source (scales, a geometry of the
 * source's size, get_src_sse / get_src_ssim); dsv1_resladder_uploads counts the raw RGB bytes. */
int  dsv1_resladder_open_rgb(dsv1_resladder **out, const DSV_META *src, const dsv1_rgb_format *rf, const dsv1_res_rung *rungs,
                             int ngeoms, int device, int nsources, int frames_per_call, int filter);
/* dsv1_decbatch_set_output_format for RGB frames, with its contract (ONE pass over the bordered reconstructions in the place of the
 * packing pass; dsv1_decbatch_out_frame_bytes follows; a smaller out_pitch is refused; streams without a picture keep their frame;
 * the int32 second pass writes its frames again in the format; the setting outlives a rebuilt context).  The two output setters
 * replace each other; NULL switches back to packed planar. */
int  dsv1_decbatch_set_output_rgb(dsv1_decbatch *d, const dsv1_rgb_format *rf);

/* ---- extension: HDR sources, tone-mapped to SDR (csrc/k_hdr.hip; stated in numpy in tests/_hdr.py) ----
 * What comes in deep today is mostly HDR: PQ or HLG, BT.2020.  Cut to 8 bits by the depth rule and shown as BT.709 it is grey and
 * washed out.  The HDR import converts frames of a dsv1_pix_format of depth 10, 12 or 16 (planar or semi-planar) on the device to the
 * tightly packed planar 8-bit SDR frames every other entry point reads, at the session's subsampling.  Two layers.
 * SETTINGS -> TABLES (host only, binary64).  dsv1_hdr: transfer (DSV1_TRANSFER_*); matrix (DSV1_MATRIX_*) and full_range of the
 * source signal; gamut: 1 converts BT.2020 primaries to BT.709, 0 keeps them; curve (DSV1_TONEMAP_*); peak_nits 100..10000, the
 * source's peak; white_nits 48..min(peak_nits, 1000), the HDR level that becomes SDR 1.0, 0 = 203; out_matrix, out_full_range: the
 * SDR signal.  dsv1_hdr_valid says 1 for such settings; dsv1_hdr_build fills a dsv1_hdr_tables (DSVG_ERR_ARG for invalid ones):
 *   ycc[5]      IY, RV, GU, GV, BU in Q14 from the 10-bit signal to a 0..4095 index: the inverse rows of the RGB section times
 *               4095 / (4 * 255) (limited: IY = r(16384 * 4095 / 876), RV = r(16384 * 2 (1 - Kr) * 4095 / 896), ...; full: / 1023)
 *   in_oy, in_oc  64 (limited) or 0, and 512
 *   eotf[4096]  linear light of E' = i / 4095 in Q20, 2^20 = peak_nits.  PQ: min(ST 2084 nits, peak) / peak.  HLG: the inverse OETF
 *               of BT.2100 (scene light, 0..1)
 *   gamut[9]    Q14 rows over linear R, G, B; identity (16384 on the diagonal) when gamut == 0, else the BT.2087 matrix 1.6605 -0.5876
 *               -0.0728 / -0.1246 1.1329 -0.0083 / -0.0182 -0.1006 1.1187: off-diagonals -r(16384 |m|), the diagonal the remainder,
 *               so every row sums to 16384 exactly
 *   gain[3329]  Q16, by bucket (cidx below) of m = max(R, G, B) with representative R: r(65536 * T(R / 2^20 * peak) / (R / 2^20)),
 *               at R = 0 r(65536 * peak / white).  HLG: the 1.2 OOTF is folded in on max-RGB, T(peak * (R / 2^20)^1.2) / (R / 2^20), 0 at
 *               R = 0 -- a stated approximation: the true OOTF works on luminance
 *   oetf[3329]  E' in 0..4095 by bucket of the SDR linear value (2^20 = 1.0): r(4095 * (R / 2^20)^(1 / 2.4)), a pure 2.4 gamma
 *   fwd[9], ybias, cbias  Q20 rows Y, Cb, Cr from E' 0..4095 to the 8-bit signal: the forward rules of the RGB section with 65536 -> 2^20
 *               and sy = 219 / 4095, sc = 224 / 4095 (limited) or 255 / 4095 (full); ybias = (oy << 20) + 2^19, cbias = (128 << 20) + 2^19
 * CURVES on m in nits, T in [0, 1].  CLIP: min(m / white, 1).  REINHARD: x = m / white, L = peak / white, min(x (1 + x / L^2) / (1 + x),
 * 1).  BT2390: the EETF of BT.2390 5.4.1 in the PQ domain, source peak peak_nits, target peak white_nits, no black lift: E1 = PQ(m) /
 * PQ(peak), maxLum = PQ(white) / PQ(peak), KS = 1.5 maxLum - 0.5, E2 = E1 below KS, else with t = (E1 - KS) / (1 - KS) the spline
 * (2t^3 - 3t^2 + 1) KS + (t^3 - 2t^2 + t)(1 - KS) + (-2t^3 + 3t^2) maxLum; back to nits, divided by white, at most 1.
 * TABLES -> PIXELS (device, exact integers; a caller may edit the tables, as with dsv1_levels: every device entry point takes the
 * tables, not the settings).  dsv1_hdr_tables_valid bounds them so that nothing on the pixel path overflows: |ycc[i]| <= 2^19 and in_oy,
 * in_oc in 0..1023 (step c stays inside int32: 3 * 2^19 * 1023 + 8192 < 2^31); eotf[i] <= 2^20; |gamut[i]| <= 2^18 (step e: 3 * 2^18 * 2^20
 * in int64); gain: any uint32 (step f: 2^20 * 2^32 in int64); oetf[i] <= 4095; |fwd[i]| <= 2^16 and |ybias|, |cbias| <= 2^30 (step h stays
 * inside int32: 3 * 2^16 * 4095 + 2^30 < 2^31).  Per pixel, >> arithmetic:
 *   a. sample    v as the pixel formats section defines it; s = d == 10 ? v : min(1023, (v + 2^(d-11)) >> (d - 10))
 *   b. chroma to the luma grid at 10 bits, src_subsamp -> 4:4:4: DSV1_CHROMA_REPLICATE or DSV1_CHROMA_LINEAR, the formulas of the RGB
 *                output section unchanged, on the 10-bit samples
 *   c. index     y = Y - in_oy, u = Cb - in_oc, v = Cr - in_oc; R: clamp((IY y + RV v + 8192) >> 14, 0, 4095), G: IY y + GU u + GV v,
 *                B: IY y + BU u
 *   d. linear    lin = eotf[idx], per channel
 *   e. gamut     clamp((row . lin + 8192) >> 14, 0, 2^20), int64
 *   f. tone map  m = max of the three, g = gain[cidx(m)], out = min((c g + 32768) >> 16, 2^20), int64
 *   g. OETF      E = oetf[cidx(out)]
 *   h. signal    Y = clamp((fwdY . E + ybias) >> 20, 0, 255), Cb and Cr with cbias
 *   i. halve     the 8-bit 4:4:4 chroma is halved to `subsamp` exactly as the RGB import halves:
 *                hdr_import(x, S) == dsv1_export_clip(hdr_import(x, 4:4:4), 4:4:4 -> S)
 * cidx(v), v <= 2^20: v below 256; else with e = floor(log2 v), ((e - 7) << 8) | ((v >> (e - 8)) & 255): 3329 buckets of 8 significant
 * bits.  A bucket's representative: the value itself below 256, else lower + width / 2, at most 2^20.
 * Valid: src_subsamp -> subsamp equal or halving among 4:4:4, 4:2:2 and 4:2:0, planar or semi-planar layouts valid at src_subsamp.
 * Depth 8, packed layouts, 4:1:1, upsampling on the way in, an upsample mode that is none, invalid tables: DSVG_ERR_ARG before any
 * device work.  Pitches, frame stride and padding as for every pixel format: padding is never read into a result.
 * dsv1_hdr_import_clip: n frames -> n packed planar 8-bit frames at `subsamp`; host or device memory (on_device: both pointers),
 * synchronous; the last frame ends with its planes.  dsv1_batch_set_source_hdr: the contract of dsv1_batch_set_source_format_sub
 * (between batches only; ownership of the clips; dsv1_batch_stage refused while set; plain batches, quality ladders, chain mode); the
 * tables are copied.  The three source setters replace each other; NULL tables clear it; an invalid call leaves the setting in force
 * as it was.  dsv1_resladder_open_hdr: dsv1_resladder_open_src_sub with the HDR import in the converter's place: the converted clip
 * stands for the source, dsv1_resladder_uploads counts the raw bytes.
 * Not offered: dither, left-sited chroma, constant-luminance BT.2020, HDR output from the decoders, the reframed / oriented
 * resladder constructors with HDR (batches combine them through the setters), dynamic metadata. */
#define DSV1_TRANSFER_PQ      0
#define DSV1_TRANSFER_HLG     1
#define DSV1_TONEMAP_CLIP     0
#define DSV1_TONEMAP_REINHARD 1
#define DSV1_TONEMAP_BT2390   2
#define DSV1_HDR_ONE          (1u << 20)
#define DSV1_HDR_NBUCKETS     3329
typedef struct { int transfer, matrix, full_range, gamut, curve, peak_nits, white_nits, out_matrix, out_full_range; } dsv1_hdr;
typedef struct {
    int32_t  ycc[5];
    int32_t  in_oy, in_oc;
    uint32_t eotf[4096];
    int32_t  gamut[9];
    uint32_t gain[DSV1_HDR_NBUCKETS];
    uint16_t oetf[DSV1_HDR_NBUCKETS];
    int32_t  fwd[9];
    int32_t  ybias, cbias;
} dsv1_hdr_tables;
/* one text for host, kernel and tools (the kernel's file defines DSV1_HDR_FN with its device qualifiers before it includes this) */
#ifndef DSV1_HDR_FN
#define DSV1_HDR_FN static inline
#endif
DSV1_HDR_FN int dsv1_hdr_cidx(uint32_t v)
{
    int e;
    if (v < 256) return (int)v;
    e = 31 - __builtin_clz(v);
    return ((e - 7) << 8) | (int)((v >> (e - 8)) & 255);
}
int  dsv1_hdr_valid(const dsv1_hdr *hd);                                      /* host only */
int  dsv1_hdr_build(const dsv1_hdr *hd, dsv1_hdr_tables *t);                  /* host only */
int  dsv1_hdr_tables_valid(const dsv1_hdr_tables *t);                         /* 1 or 0; host only */
int  dsv1_hdr_cidx_of(uint32_t v);                                            /* dsv1_hdr_cidx for callers without a C compiler; -1 above 2^20 */
int  dsv1_hdr_import_clip(int device, const void *src, const dsv1_pix_format *pf, int w, int h, int src_subsamp, int subsamp, int n,
                          void *dst, const dsv1_hdr_tables *tables, int upsample, int on_device);
int  dsv1_batch_set_source_hdr(dsv1_batch *b, const dsv1_pix_format *pf, int src_subsamp, const dsv1_hdr_tables *tables, int upsample);
int  dsv1_resladder_open_hdr(dsv1_resladder **out, const DSV_META *src, const dsv1_pix_format *pf, int src_subsamp,
                             const dsv1_hdr_tables *tables, int upsample, const dsv1_res_rung *rungs, int ngeoms, int device, int nsources,
                             int frames_per_call, int filter);

/* ---- extension: deinterlacing (csrc/k_deint.hip; stated in numpy in tests/_deint.py) ----
 * DSV1 has no interlaced coding tools; an interlaced source (1080i, 576i, 480i) is deinterlaced in front of the encoder: motion-
 * adaptive, edge-directed, in exact integers.  Input and output are the tightly packed planar 8-bit frames every other entry point
 * reads.  Each plane is treated on its own at its own dimensions W x H (the chroma planes of 4:2:0 alternate fields line by line
 * like luma).  Line y of a plane belongs to field y & 1 (0 = top); tff (0 / 1) says which field of a frame is earlier in time; the
 * first field's parity is p = tff ? 0 : 1.  cur is frame t of a stream, prv frame t - 1 of the same stream, or absent.
 * An output picture keeps the lines of one parity q and makes the others.  DSV1_DEINT_FRAME (n frames in, n out): output t keeps
 * q = p.  DSV1_DEINT_FIELD (n in, 2n out): output 2t keeps q = p (first-field output), output 2t + 1 keeps q = 1 - p (second-field
 * output).  A plane with H == 1 is copied to every output.  Otherwise, for every x:
 *   kept line ((y & 1) == q): out[y][x] = cur[y][x].
 *   made line: up = y - 1 >= 0 ? y - 1 : y + 1; dn = y + 1 <= H - 1 ? y + 1 : y - 1; cx(i) = clamp(i, 0, W - 1);
 *     c[i] = cur[up][cx(i)], e[i] = cur[dn][cx(i)].
 *   spatial value, j = -2 .. 2: S(j) = sum over k = -1, 0, 1 of |c[x + k + j] - e[x + k - j]|, P(j) = (c[x + j] + e[x - j]) >> 1.
 *     best = S(0) - 1, sp = P(0).  If S(-1) < best: best = S(-1), sp = P(-1), and only then, if S(-2) < best: S(-2) / P(-2).  Then,
 *     against the best reached so far: if S(1) < best: S(1) / P(1), and only then, if S(2) < best: S(2) / P(2).
 *   temporal value and motion bound.  First-field output: A = prv[y][x], B = cur[y][x], tp = (A + B) >> 1, td0 = |A - B| >> 1.
 *     Second-field output: tp = cur[y][x], td0 = |cur[y][x] - prv[y][x]| >> 1.  Both: td1 = (|prv[up][x] - c[x]| + |prv[dn][x] -
 *     e[x]|) >> 1, d = max(td0, td1).  prv absent: tp = cur[y][x], d = 255 (the result is sp).
 *   out[y][x] = min(max(sp, tp - d), tp + d).
 * A picture needs its own frame and the one before it; nothing looks ahead, so the result of a stream does not depend on how it is
 * cut into calls, and a static stream is woven exactly (d = 0) from its second frame on.
 * SESSIONS.  The deinterlacer runs on the device behind the source converter or the RGB import when one is set (and with neither),
 * in front of the frame load and, in a resolution ladder, in front of the scales, with no host synchronisation of its own.  Clip
 * ownership is dsv1_batch_set_source_format's: a plain device clip is the caller's again when submit returns, a DSV1_CLIP_HELD clip
 * stays unchanged until collect, dsv1_batch_stage is refused while set.  The deinterlaced clip lives in session-owned buffers per call
 * parity and goes on as a held clip; the session keeps each source's last input frame (after conversion) as the next call's prv.
 * Setting, changing or clearing the mode forgets the history of every source, _reset that of one source (-1: every source) -- a
 * discontinuity; both only with nothing in flight (DSVG_ERR_ARG otherwise; _reset with no deinterlacer set too).  frames_per_call
 * counts coded pictures: in FIELD mode a call takes frames_per_call / 2 input frames per source, and an odd frames_per_call is
 * DSVG_ERR_ARG at the setter.  The frame rate in vidmeta is the caller's statement.  In a resolution ladder the deinterlaced clip
 * stands for the source everywhere: the scales, a geometry of the source's size, get_src_sse / get_src_ssim.  An invalid mode or tff
 * is DSVG_ERR_ARG before any device work and leaves the setting as it was.
 * Not offered: the drop-in dsv_enc, any lookahead.  (Inverse telecine and field order detection: the next section.) */
#define DSV1_DEINT_FRAME 0
#define DSV1_DEINT_FIELD 1
typedef struct { int mode; int tff; } dsv1_deint;
int  dsv1_deint_out_frames(const dsv1_deint *di, int n);      /* n or 2n; DSVG_ERR_ARG for an invalid *di or n < 0; host only */
/* n frames of one stream -> dsv1_deint_out_frames(di, n) pictures.  prev: one frame that precedes src[0], or NULL for none.  Host or
 * device memory (on_device: all three pointers are device pointers); any w, h >= 1 and every subsampling the library knows;
 * synchronous; nothing outside the frames is read or written. */
int  dsv1_deinterlace_clip(int device, const void *src, int w, int h, int subsamp, int n, const void *prev, void *dst,
                           const dsv1_deint *di, int on_device);
int  dsv1_batch_set_source_deinterlace(dsv1_batch *b, const dsv1_deint *di);          /* NULL = off; batches, ladders, chain mode */
int  dsv1_batch_deinterlace_reset(dsv1_batch *b, int source);                         /* -1 = every source */
int  dsv1_resladder_set_deinterlace(dsv1_resladder *r, const dsv1_deint *di);
int  dsv1_resladder_deinterlace_reset(dsv1_resladder *r, int source);

/* ---- extension: inverse telecine and field order detection (csrc/k_ivtc.hip; stated in numpy in tests/_ivtc.py) ----
 * Much 29.97i material is film that was 3:2 pulled down: film frames A B C D arrive as the frames (At,Ab) (Bt,Bb) (Bt,Cb) (Ct,Db)
 * (Dt,Db) -- three progressive, two combed, one field sent twice.  Deinterlacing it throws away half the vertical detail of pictures
 * that are all there.  This pass weaves the four film frames back exactly and drops the fifth: 5n frames in, 4n out, tightly packed
 * planar 8-bit frames as everywhere.  Causal, no lookahead, every decision made on the device.
 * All decisions read luma only, W x H.  Line y belongs to field y & 1; p = tff ? 0 : 1 is the parity of the field that is first in
 * time; cur is frame t of a stream, prv frame t - 1, or absent.
 * COMB.  Kept lines of parity q from frame K, the lines of parity 1 - q from frame O: over every y with (y & 1) == 1 - q, y - 1 >= 0,
 *   y + 1 <= H - 1 (border lines without two neighbours are left out) and every x, a = K[y-1][x], b = K[y+1][x], o = O[y][x],
 *   e = max(min(a, b) - o, o - max(a, b), 0); comb(K, q, O) = the sum of e over the samples where e > nt.
 * FIELD METRICS of frame t, four uint32_t: mc[q] = comb(cur, q, cur), mp[q] = comb(cur, q, prv), q = 0, 1; mp = 0 where prv is absent.
 *   Stored as mc0 mc1 mp0 mp1.  A sum is at most 255 * W * ceil(H / 2); the calls below take a luma of at most 16843008 samples
 *   (255 * W * H < 2^32 - 1: exact in uint32_t for every size the library encodes, 4K and beyond) and refuse anything larger.
 * MATCH.  match[t] = P (1) if prv is present and mp[p] < mc[p], else C (0).  Keeping the first field in time makes P and C enough: a
 *   film frame covers at least two consecutive fields, so the kept field's partner is the opposite field just before it (prv's) or
 *   just after it (cur's own).
 * WOVEN PICTURE V_t, every plane at its own dimensions (the chroma planes alternate fields line by line, as in the deinterlacer):
 *   lines of parity p from cur, the others from prv if the match is P, else from cur.  A plane with one line is cur's.
 * DECIMATION.  Input is grouped in cycles of 5 from the start of the stream.  D_t = the luma SAD of V_t against V_(t-1), UINT32_MAX for
 *   the first picture of a stream.  In each cycle the picture with the smallest D is dropped (drop[c] = 0 .. 4, on ties the earliest);
 *   the other four go out in order.  n must be a multiple of 5.
 * STATE a stream carries between calls, dsv1_ivtc_state_bytes: its last input frame (frame_bytes), then the luma of its last woven
 *   picture (w * h), which may be one that was dropped.  Calls take whole cycles, so the output of a stream does not depend on how it is
 *   cut into calls.
 * FIELD ORDER from the same metrics (dsv1_field_order_from_metrics, host only): every frame that has a prv (t >= 1, and t = 0 where
 *   first_has_prev) votes tff if mp[0] < mp[1] and bff if mp[1] < mp[0]: mp[0] weaves the top field of t with the bottom field of t - 1,
 *   one field time apart under tff, three under bff.  1 (tff) if tff_votes > 2 * bff_votes, 0 (bff) if bff_votes > 2 * tff_votes, -1
 *   otherwise.  The vote is for material that moves and is smooth against its motion: texture that decorrelates within one field's
 *   motion does not separate the orders, telecined film decides only three votes of five, and on static material mp equals mc, so a
 *   frame's vote there compares the vertical detail of its own two fields (no vote at all where there is none) and says nothing
 *   about time.
 * dsv1_ivtc_match / dsv1_ivtc_pick (host only) are the two decision rules the kernels run, compiled from the same header
 *   (csrc/dsvg_ivtc_rules.h): match [n] from metrics [n][4]; drop [n / 5] from D [n].
 *   dsv1_detect_field_order_clip does both steps over a clip with no prev and answers 1 / 0 / -1 or an error below -1: DSVG_ERR_ARG
 *   and its kin; since -1 is an answer, a HIP runtime failure comes back as DSVG_ERR_NODEVICE (dsvg_last_error has the text).
 * dsv1_field_metrics_clip: src and prev (one frame, or NULL) host or device memory (on_device), the metrics always to host memory.
 * dsv1_ivtc_clip: n frames of one stream -> 4n / 5 pictures.  state_in: what the call before left, or NULL: the stream starts here;
 *   state_out: receives the state, or NULL; it may be state_in.  src, states and dst host or device memory (on_device); match_out [n]
 *   and drop_out [n / 5] always host memory, either may be NULL.  dst must not overlap src.  Synchronous; any w, h >= 1 within the bound
 *   above and every subsampling the library knows; nothing outside the frames and the states is read or written.
 * SESSIONS.  The pass takes the deinterlacer's place in the source chain: convert -> levels -> inverse telecine -> denoise -> orient -> reframe.  It is
 * exclusive with the deinterlacer: setting either while the other is set is DSVG_ERR_ARG with the settings left as they were.  Setting,
 * changing or clearing it forgets its own state and the noise filter's (the pictures change meaning); _reset forgets the state of one
 * source (-1: every source): its next picture is a first picture.  The setters and _reset only with nothing in flight (DSVG_ERR_ARG
 * otherwise; _reset with no inverse telecine set too).  frames_per_call counts coded pictures: a call takes 5 * frames_per_call / 4
 * input frames per source, and frames_per_call % 4 != 0 is DSVG_ERR_ARG at the setter.  Like the other passes it is set after a
 * reframe, never before.  Clip ownership is dsv1_batch_set_source_format's; dsv1_batch_stage is refused while it is set.  The frame
 * rate in vidmeta stays the caller's statement.  An invalid dsv1_ivtc is DSVG_ERR_ARG before any device work.
 * Not offered: the drop-in dsv_enc; lookahead or n-matches; mixed or hybrid content handling, and post-processing of frames that stay
 * combed; cadences other than cycle 5; reading the decisions back from a session; automatic application of a detected order. */
#define DSV1_IVTC_C 0
#define DSV1_IVTC_P 1
typedef struct { int tff; int nt; int reserved[2]; } dsv1_ivtc;   /* tff 0 / 1, nt 0 .. 254, reserved 0; else DSVG_ERR_ARG */
int    dsv1_ivtc_out_frames(const dsv1_ivtc *iv, int n);          /* 4n / 5; DSVG_ERR_ARG unless n >= 0 and n % 5 == 0; host only */
size_t dsv1_ivtc_state_bytes(int w, int h, int subsamp);          /* frame_bytes + w * h; 0 for w, h < 1 or an unknown subsampling; host only */
int    dsv1_field_metrics_clip(int device, const void *src, int w, int h, int subsamp, int n, const void *prev, int nt,
                               uint32_t *metrics /* [n][4]: mc0 mc1 mp0 mp1, host */, int on_device);
int    dsv1_field_order_from_metrics(const uint32_t *metrics, int n, int first_has_prev);   /* 1 / 0 / -1; DSVG_ERR_ARG for NULL or n < 1 */
int    dsv1_detect_field_order_clip(int device, const void *src, int w, int h, int subsamp, int n, int nt, int on_device);
int    dsv1_ivtc_match(const uint32_t *metrics, int n, int first_has_prev, int tff, uint8_t *match);
int    dsv1_ivtc_pick(const uint32_t *D, int n, uint8_t *drop /* [n / 5] */);
int    dsv1_ivtc_clip(int device, const void *src, int w, int h, int subsamp, int n, const void *state_in, void *state_out,
                      void *dst, const dsv1_ivtc *iv, uint8_t *match_out /* [n] or NULL */, uint8_t *drop_out /* [n / 5] or NULL */,
                      int on_device);
int    dsv1_batch_set_source_ivtc(dsv1_batch *b, const dsv1_ivtc *iv);     /* NULL = off; batches, quality ladders, chain mode */
int    dsv1_batch_ivtc_reset(dsv1_batch *b, int source);                   /* -1 = every source */
int    dsv1_resladder_set_ivtc(dsv1_resladder *r, const dsv1_ivtc *iv);
int    dsv1_resladder_ivtc_reset(dsv1_resladder *r, int source);

/* ---- extension: temporal noise reduction (csrc/k_denoise.hip; stated in numpy in tests/_denoise.py) ----
 * Camera and film noise is uncorrelated from picture to picture: motion compensation cannot predict it and every P picture codes it
 * again.  This is a motion-adaptive, recursive temporal filter in exact integers in front of the encoder: causal, no lookahead.  Input
 * and output are the tightly packed planar 8-bit frames every other entry point reads, n pictures in and n out.  Every plane is treated
 * on its own at its own dimensions W x H; the strength T is `luma` for plane 0 and `chroma` for planes 1 and 2; a plane with T == 0 is
 * copied and keeps no state.  Per plane and stream the filter carries from picture to picture pin, the previous INPUT picture of the
 * plane (uint8), and S, the filter state (uint16: the filtered value times 16, always within 0 .. 4080).  For picture t, with
 * c = cur[y][x], for every sample:
 *   first picture of a stream (no history): S' = 16 c.
 *   otherwise: cl(a, y, x) = a[clamp(y, 0, H - 1)][clamp(x, 0, W - 1)];
 *     m0   = sum over dy, dx in {-1, 0, 1} of |cl(cur, y + dy, x + dx) - cl(pin, y + dy, x + dx)|      (3x3 SAD of the inputs)
 *     pout = (S + 8) >> 4
 *     m    = max(m0, 3 |c - pout|)
 *     k    = 4 if m <= T;  16 if m >= 2 T;  4 + (12 (m - T) + T / 2) / T otherwise      (integer division, both operands >= 0; 4 .. 16)
 *     S'   = S + (((16 c - S) k + 8) >> 4)                                               (arithmetic shift: floor)
 *   out = (S' + 8) >> 4;  pin' = cur;  S <- S'.
 * Consequences: a noiseless static stream passes through unchanged (m = 0, S = 16 c stays); a sample in motion (m >= 2 T) is the input
 * sample and its state restarts from it (k = 16: S' = 16 c); S never leaves 0 .. 4080 (S' lies between S and 16 c); nothing looks
 * ahead and the state is all a picture needs of the past, so the result of a stream does not depend on how it is cut into calls.
 * A stream's STATE is 3 * frame_bytes bytes: pin in the frame's layout, then S in the frame's layout as little-endian uint16; the
 * state of a plane with T == 0 is written as zeros and ignored when read.
 * SESSIONS.  The filter runs on the device behind the source converter or the RGB import and behind the deinterlacer when those are
 * set (and with none of them) -- in DSV1_DEINT_FIELD mode it filters the 2n deinterlaced pictures --, in front of the frame load and,
 * in a resolution ladder, in front of the scales, with no host synchronisation of its own.  Clip ownership is
 * dsv1_batch_set_source_format's: a plain device clip is the caller's again when submit returns, a DSV1_CLIP_HELD clip stays unchanged
 * until collect, dsv1_batch_stage is refused while set.  The filtered clip lives in session-owned buffers per call parity and goes on
 * as a held clip; the session keeps each source's state (pin of the last picture the filter saw, and S).  Setting, changing or clearing
 * the filter forgets the state of every source, and so does setting, changing or clearing the deinterlacer underneath it (the pictures
 * change meaning); _reset forgets that of one source (-1: every source) -- a discontinuity: its next picture is a first picture.  The
 * setters and _reset only with nothing in flight (DSVG_ERR_ARG otherwise; _reset with no filter set too).  An invalid dsv1_denoise is
 * DSVG_ERR_ARG before any device work and leaves the setting as it was.  In a resolution ladder the filtered clip stands for the
 * source everywhere: the scales, a geometry of the source's size, get_src_sse / get_src_ssim.
 * Not offered: the drop-in dsv_enc, spatial filtering (a 3x3 threshold-average stage was tried and lost PSNR), motion-compensated
 * filtering, noise-level estimation, any lookahead. */
#define DSV1_DENOISE_MAX 512
typedef struct { int luma; int chroma; } dsv1_denoise;      /* each 0 .. DSV1_DENOISE_MAX; both 0, or anything outside: DSVG_ERR_ARG */
size_t dsv1_denoise_state_bytes(int w, int h, int subsamp);  /* 3 * frame_bytes; 0 for w, h < 1 or an unknown subsampling; host only */
/* n pictures of one stream -> n pictures.  state_in: the state the call before left, or NULL: the stream starts here.  state_out: receives
 * the state the clip leaves, or NULL: discarded; it may be state_in.  Host or device memory (on_device: all four pointers are device
 * pointers); dst must not overlap src; any w, h >= 1 and every subsampling the library knows; synchronous; nothing outside the frames
 * and the states is read or written. */
int  dsv1_denoise_clip(int device, const void *src, int w, int h, int subsamp, int n, const void *state_in, void *state_out, void *dst,
                       const dsv1_denoise *dn, int on_device);
int  dsv1_batch_set_source_denoise(dsv1_batch *b, const dsv1_denoise *dn);            /* NULL = off; batches, ladders, chain mode */
int  dsv1_batch_denoise_reset(dsv1_batch *b, int source);                             /* -1 = every source */
int  dsv1_resladder_set_denoise(dsv1_resladder *r, const dsv1_denoise *dn);
int  dsv1_resladder_denoise_reset(dsv1_resladder *r, int source);

/* ---- extension: reframe -- crop, pad, letterbox, pillarbox -- and bar detection (csrc/k_reframe.hip; stated in numpy in
 * tests/_reframe.py) ----
 * The picture's frame: film sources with black bars, decoder surfaces with junk rows (1920x1088), a 4:3 or 2.39:1 source inside a 16:9
 * ladder, captures with dirty edge columns.  A dsv1_pix_format cannot express a window (its planes lie back to back at pitch x rows),
 * so this is a pass of its own: a window of the incoming picture placed on a canvas of the coded size, a fill colour elsewhere.
 * Input and output are the tightly packed planar 8-bit frames every other entry point reads, n in and n out.
 * INDEXING.  Every plane p on its own, with its shifts (hs_p, vs_p): 0 for luma, the subsampling's for chroma.  X0 = x >> hs_p,
 * W = rshift_up(w, hs_p), DX = dst_x >> hs_p; Y0, H, DY likewise with vs_p.  out_p[Y][X] = in_p[Y - DY + Y0][X - DX + X0] where
 * DX <= X < DX + W and DY <= Y < DY + H, and fill[p] elsewhere.
 * VALID (dsv1_reframe_valid, host only, 1 / 0): every size >= 1; 0 <= x, x + w <= in_w, 0 <= y, y + h <= in_h; 0 <= dst_x, dst_x + w <=
 * out_w, 0 <= dst_y, dst_y + h <= out_h; x and dst_x multiples of 1 << hs, y and dst_y of 1 << vs (w and h need not be); reserved == 0;
 * the subsampling one the library knows (4:4:4, 4:2:2, 4:2:0, 4:1:1).  The chroma window then lies inside both chroma planes: with
 * x = X0 << hs, X0 + W = X0 + ceil(w / 2^hs) = ceil((x + w) / 2^hs) <= ceil(in_w / 2^hs), the input chroma plane's width, and with
 * dst_x = DX << hs in the same way DX + W <= ceil(out_w / 2^hs); rows likewise.  Anything else is DSVG_ERR_ARG before any device work.
 * LINE SUMS, on luma only: row_sum[t][r] the sum of row r of frame t, col_sum[t][c] the sum of column c; uint32_t, exact for every size
 * the library takes.  dsv1_line_sums_clip: src host or device memory (on_device), the sums always to host memory; synchronous.
 * BARS (dsv1_bars_from_sums, host only): ffmpeg cropdetect's rule -- a line's mean against a limit, the union taken over the frames.
 * Row r is content if in any frame row_sum[t][r] > (uint64_t)thresh * w, a column likewise with h.  x0, x1 the first and last content
 * columns, y0, y1 the first and last content rows; the rectangle is rounded INWARD to align: x = roundup(x0, align), w =
 * rounddown(x1 + 1, align) - x, y and h likewise.  Returns 1 with rect = {x, y, w, h} when both sizes are positive; 0 with rect all zero
 * when nothing is content or the rounding leaves nothing; DSVG_ERR_ARG for thresh outside 0 .. 254 or align not a power of two in
 * 1 .. 64.  Known consequence of the rule: a column's mean includes the rows of horizontal bars (and a row's the columns of vertical
 * ones), so a letterboxed picture needs more light in a column to count than the limit says.  dsv1_detect_bars_clip does both steps.
 * SESSIONS.  The reframe is the LAST pass of the source chain: convert -> levels -> deinterlace -> denoise -> orient -> reframe, then the scales of a
 * resolution ladder or the frame load.  The passes in front of it run at in_w x in_h; denoising rows that are then cut away is accepted
 * waste.  dsv1_batch_set_source_reframe (plain batches, quality ladders, chain mode): out_w x out_h must be the batch's geometry.  It
 * changes the geometry the other passes are built for, so it may be set, changed or cleared only with nothing in flight, nothing
 * staged, and no source format, RGB format, deinterlacer or noise filter set -- else DSVG_ERR_ARG with the setting left as it was (an
 * invalid struct too).  Formats and passes set AFTER it resolve at in_w x in_h; clips are then in_w x in_h.  NULL clears it, and so does
 * the identity (window = input = canvas at 0, 0): no pass, no copy, no lane.  Clip ownership is dsv1_batch_set_source_format's;
 * dsv1_batch_stage is refused while it is set.
 * dsv1_resladder_open_reframed: src is the geometry handed in and must equal rf->in_w x in_h; at most one of pf (at src_subsamp) / rgb;
 * rf == NULL behaves as the existing opens.  The CANVAS takes the source's place everywhere behind the chain: the scaler's source
 * geometry, the 1 .. 8 ratio check of the rungs (a rung larger than the canvas is refused although it is smaller than the input), a
 * geometry "of the source's size", the clip get_src_sse / get_src_ssim measure against.  dsv1_resladder_set_deinterlace / _set_denoise
 * act in front of the reframe.
 * Not offered: the drop-in dsv_enc; one window per source; windows that move from call to call (pan and scan); bar detection inside a
 * session (the coded size depends on it, so it runs before open); a crop in the decoders' output pass; fusing the window into the
 * frame load. */
typedef struct {
    int in_w, in_h;     /* the frames that come in (after conversion / deinterlacing / noise filter) */
    int x, y, w, h;     /* the window of them that is kept */
    int out_w, out_h;   /* the canvas: the frames that go on */
    int dst_x, dst_y;   /* where the window's top left lands on the canvas */
    uint8_t fill[3];    /* Y, U, V of every canvas sample outside the window */
    uint8_t reserved;   /* 0 */
} dsv1_reframe;
int  dsv1_reframe_valid(const dsv1_reframe *rf, int subsamp);
int  dsv1_reframe_clip(int device, const void *src, int n, void *dst, const dsv1_reframe *rf, int subsamp, int on_device);
int  dsv1_line_sums_clip(int device, const void *src, int w, int h, int subsamp, int n, uint32_t *row_sum /* [n][h] */,
                         uint32_t *col_sum /* [n][w] */, int on_device);
int  dsv1_bars_from_sums(const uint32_t *row_sum, const uint32_t *col_sum, int w, int h, int n, int thresh, int align,
                         int rect[4] /* x, y, w, h */);
int  dsv1_detect_bars_clip(int device, const void *src, int w, int h, int subsamp, int n, int thresh, int align, int rect[4],
                           int on_device);
int  dsv1_batch_set_source_reframe(dsv1_batch *b, const dsv1_reframe *rf);            /* NULL or the identity = off */
int  dsv1_resladder_open_reframed(dsv1_resladder **out, const DSV_META *src, const dsv1_reframe *rf, const dsv1_pix_format *pf,
                                  int src_subsamp, const dsv1_rgb_format *rgb, const dsv1_res_rung *rungs, int ngeoms, int device,
                                  int nsources, int frames_per_call, int filter);

/* ---- extension: orientation -- rotate, flip, transpose: the eight orientations (csrc/k_orient.hip; stated in numpy in
 * tests/_orient.py) ----
 * Phone and tablet footage stored in sensor order beside a rotation tag or display matrix, mirrored or upside-down captures, portrait
 * video that is stood upright before it is pillarboxed into a 16:9 ladder.  A dsv1_pix_format has only positive pitches and a
 * dsv1_reframe keeps rows as rows, so this is a pass of its own.  Input and output are the tightly packed planar 8-bit frames every
 * other entry point reads, n in and n out.
 * DEFINITION.  Every plane on its own, at its own dimensions: input plane I of IH rows of IW samples, output plane O.
 *   0 NONE        O[y][x] = I[y][x]              IW x IH        4 TRANSPOSE   O[y][x] = I[x][y]              IH x IW
 *   1 HFLIP       O[y][x] = I[y][IW-1-x]         IW x IH        5 ROT90       O[y][x] = I[IH-1-x][y]         IH x IW   (clockwise)
 *   2 VFLIP       O[y][x] = I[IH-1-y][x]         IW x IH        6 ROT270      O[y][x] = I[x][IW-1-y]         IH x IW   (90 counter-clockwise)
 *   3 ROT180      O[y][x] = I[IH-1-y][IW-1-x]    IW x IH        7 TRANSVERSE  O[y][x] = I[IH-1-x][IW-1-y]    IH x IW
 * The code is a bit set: bit 2 transposes first, bit 0 then mirrors the columns of the result, bit 1 then its rows.  The luma geometry
 * going out is w x h for codes 0-3 and h x w for codes 4-7 (dsv1_orient_dims).
 * VALID (dsv1_orient_valid, host only, 1 / 0): the code in 0 .. 7, the subsampling one the library knows, and for codes 4-7 equal
 * horizontal and vertical chroma shifts -- 4:4:4 and 4:2:0.  With hs == vs the transposed chroma plane of rshift_up(h) x rshift_up(w)
 * samples is exactly the chroma plane of the h x w output, odd sizes included; at 4:2:2 or 4:1:1 it would be a plane of no subsampling
 * the codec has: DSVG_ERR_ARG before any device work.  A 4:2:2 source reaches a rotation through the converter's 4:2:2 -> 4:2:0 halving
 * (dsv1_batch_set_source_format_sub), which runs in front of this pass.  Any w, h >= 1.
 * CHROMA SITING.  Planes are mirrored independently.  With an odd luma size under subsampling the last chroma sample covers one luma
 * sample, not two, so a mirror moves the chroma siting by half a chroma sample along that axis.  This is accepted.
 * HOST HELPERS (no device): dsv1_orient_compose(a, b) is the one code equal to applying a and then b; dsv1_orient_inverse;
 * dsv1_orient_from_exif maps EXIF orientation tags 1 .. 8 to codes 0, 1, 3, 2, 4, 5, 7, 6; dsv1_orient_from_matrix reads an MP4 /
 * QuickTime track display matrix, 16.16 fixed point, a = m[0], b = m[1], c = m[3], d = m[4] (m[2], m[5], m[8] and the translation m[6],
 * m[7] are ignored): the source sample at column p, row q is shown at column a p + c q, row b p + d q.  With b == c == 0, a and d each
 * +-65536: (+,+) NONE, (-,+) HFLIP, (+,-) VFLIP, (-,-) ROT180.  With a == d == 0, b and c each +-65536, as (b, c): (+,+) TRANSPOSE,
 * (+,-) ROT90, (-,+) ROT270, (-,-) TRANSVERSE.  Scale, shear and other angles -- and every argument out of range -- are DSVG_ERR_ARG.
 * dsv1_orient_clip: src and dst host or device memory (on_device), w x h the frames that come in; synchronous; code 0 copies.
 * SESSIONS.  The pass sits between the noise filter and the reframe: convert -> levels -> deinterlace or inverse telecine -> denoise -> orient ->
 * reframe.  The deinterlacer has to see rows as fields, so it comes first; the reframe's window is chosen on the upright picture, so it
 * comes after.  dsv1_batch_set_source_orient (plain batches, quality ladders, chain mode): the ORIENTED geometry is the reframe's input,
 * or the batch's geometry without one; clips then come in at the RAW geometry, dsv1_orient_dims(dsv1_orient_inverse(orient), ...) of
 * it, and formats and passes set afterwards resolve there.  It changes the geometry those passes are built for, so it may be set,
 * changed or cleared only with nothing in flight, nothing staged, and no source format, RGB format, deinterlacer, inverse telecine or
 * noise filter set -- else, and for a code that is not valid at the batch's subsampling, DSVG_ERR_ARG with the setting left as it was.
 * A reframe is set BEFORE the orientation: dsv1_batch_set_source_reframe is refused while an orientation is set.  Code 0 clears it: no
 * pass, no copy, no lane.  Clip ownership is dsv1_batch_set_source_format's; dsv1_batch_stage is refused while it is set.
 * dsv1_resladder_open_oriented is dsv1_resladder_open_reframed with the code: src is the raw geometry handed in; with a reframe,
 * rf->in_w x in_h must be the oriented geometry; without one the oriented picture stands for the source everywhere behind the chain
 * (the scaler's source, the ratio check, a geometry "of the source's size", the clip get_src_sse / get_src_ssim measure against).
 * orient == 0 behaves as dsv1_resladder_open_reframed.
 * Not offered: the drop-in dsv_enc; orientation in the decoders' output pass; arbitrary angles; transposing 4:2:2 or 4:1:1; one
 * orientation per source of a batch; an orientation that changes between calls; fusing the pass into the reframe or the frame load. */
enum { DSV1_ORIENT_NONE, DSV1_ORIENT_HFLIP, DSV1_ORIENT_VFLIP, DSV1_ORIENT_ROT180, DSV1_ORIENT_TRANSPOSE, DSV1_ORIENT_ROT90,
       DSV1_ORIENT_ROT270, DSV1_ORIENT_TRANSVERSE };
int  dsv1_orient_valid(int orient, int subsamp);
int  dsv1_orient_dims(int orient, int w, int h, int *ow, int *oh);
int  dsv1_orient_compose(int a, int b);
int  dsv1_orient_inverse(int a);
int  dsv1_orient_from_exif(int tag);
int  dsv1_orient_from_matrix(const int32_t m[9]);
int  dsv1_orient_clip(int device, const void *src, int w, int h, int subsamp, int n, void *dst, int orient, int on_device);
int  dsv1_batch_set_source_orient(dsv1_batch *b, int orient);                          /* 0 = off */
int  dsv1_resladder_open_oriented(dsv1_resladder **out, const DSV_META *src, int orient, const dsv1_reframe *rf, const dsv1_pix_format *pf,
                                  int src_subsamp, const dsv1_rgb_format *rgb, const dsv1_res_rung *rungs, int ngeoms, int device,
                                  int nsources, int frames_per_call, int filter);

/* ---- extension: levels -- range conversion and per-plane tables; histograms (csrc/k_levels.hip; stated in numpy in tests/_levels.py) ----
 * Phone, webcam and MJPEG sources are full-range YCbCr; coded as they are they play back with crushed blacks and clipped whites.  Black
 * and white point correction and a saturation trim are the same kind of work: pointwise per plane.  One definition covers them, three
 * 256-entry tables, one per plane (Y, U, V); every content is valid.
 * DEFINITION.  out_p[i] = lut[p][in_p[i]] for every sample i of plane p.  Frames are the tightly packed planar 8-bit frames every other
 * entry point reads, n in and n out at the same geometry; every subsampling the library knows, any w, h >= 1.  The identity
 * (lut[p][v] == v everywhere) means "off".
 * BUILDERS (host only; exact integers, no floating point, nothing depends on a libm).  r(a / b) rounds the exact rational half up:
 * floor((2 a + b) / (2 b)) with a true floor for negative a, the r() of the RGB section.  clamp() is to 0 .. 255.
 *   dsv1_levels_identity(lv)                    lut[p][v] = v.
 *   dsv1_levels_range(lv, src_full, dst_full)   equal flags: the identity.
 *       full -> limited (1, 0):  Y = 16 + r(v * 219 / 255)               C = 128 + r((v - 128) * 224 / 255)
 *       limited -> full (0, 1):  Y = clamp(r((v - 16) * 255 / 219))      C = clamp(128 + r((v - 128) * 255 / 224))
 *     Full to limited maps 0 and 255 to 16 and 235 (luma), 16 and 240 (chroma).  Limited to full: THE CLAMP BINDS -- luma below 16
 *     and above 235 saturates, chroma 240 gives 255, and chroma 16 gives 1 (128 - 127.5 rounded half up), not 0.  Flags outside
 *     0 / 1: DSVG_ERR_ARG.
 *   dsv1_levels_adjust(lv, in_black, in_white, out_black, out_white, sat_q8)
 *       luma:   v <= in_black gives out_black; v >= in_white gives out_white; else
 *               out_black + r((v - in_black) * (out_white - out_black) / (in_white - in_black))
 *       chroma: clamp(128 + r((v - 128) * sat_q8 / 256))                  (sat_q8 256: unchanged; 0: grey)
 *     Valid: 0 <= in_black < in_white <= 255, 0 <= out_black <= out_white <= 255, 0 <= sat_q8 <= 1024.
 *   dsv1_levels_compose(a, b, out)              out[p][v] = b[p][a[p][v]]: a first.  out may be a or b.
 *   dsv1_levels_is_identity(lv)                 1 / 0.
 * Every builder returns DSVG_ERR_ARG for an invalid argument (NULL included) and leaves *lv untouched then.  Gamma and other curves
 * are the caller's tables: no builder is offered for them.
 * HISTOGRAM.  hist[t][p][v] is the number of samples of plane p of frame t with value v: uint32_t [n][3][256], exact for every size
 * the library takes.  dsv1_histogram_clip computes it on the GPU; hist is always host memory and the call is synchronous.
 *   dsv1_range_from_histogram(hist, n, ppm, &full), host only: outside = the luma samples < 16 or > 235 plus the chroma samples < 16
 *     or > 240, total = every sample, both summed over the n frames; full = outside * 1000000 > (uint64_t)ppm * total.  ppm outside
 *     0 .. 1000000 or n < 1: DSVG_ERR_ARG.  Returns DSVG_OK.
 *   dsv1_points_from_histogram(hist, n, low_ppm, high_ppm, &black, &white), host only, luma only, summed over the frames: black is the
 *     largest b with count(Y < b) * 1e6 <= low_ppm * total_Y, white the smallest w with count(Y > w) * 1e6 <= high_ppm * total_Y,
 *     both in 0 .. 255.
 *     Returns 1 when black < white, else 0 with both zero; ppm outside 0 .. 1000000, n < 1 or NULL: DSVG_ERR_ARG.
 *   dsv1_detect_range_clip is dsv1_histogram_clip and then dsv1_range_from_histogram.
 * dsv1_levels_clip: src and dst host or device memory (on_device); synchronous; dst may equal src, any other overlap is the caller's
 * error; a plane whose table is the identity is still copied.  Invalid arguments -- w, h < 1, an unknown subsampling, NULL pointers,
 * n < 1 -- are DSVG_ERR_ARG before any device work.
 * SESSIONS.  The pass sits directly behind the converter or the RGB import and in front of the deinterlacer or the inverse telecine, so
 * their thresholds and the noise filter's see standard-range pictures: convert -> levels -> deinterlace or inverse telecine ->
 * denoise -> orient -> reframe.  It runs at the raw geometry over the frames a call brings.  dsv1_batch_set_source_levels (plain
 * batches, quality ladders, chain mode) and dsv1_resladder_set_levels: NULL or the identity clears the pass -- no pass, no copy, and no
 * lane if nothing else needs one.  It is set AFTER the reframe and the orientation (dsv1_batch_set_source_reframe and _orient are
 * refused while levels are set), otherwise in any order relative to the format, the deinterlacer, the inverse telecine and the noise
 * filter.  Setting, changing or clearing it forgets the deinterlacer's history, the inverse telecine's state and the noise filter's
 * state of every source: the pictures change meaning.  Only with nothing in flight (and nothing staged), else DSVG_ERR_ARG with the
 * setting left as it was.  dsv1_batch_stage is refused while it is set; clip ownership is dsv1_batch_set_source_format's.  In a
 * resolution ladder the levelled clip stands for the source everywhere behind it, get_src_sse / get_src_ssim included.
 * Not offered: the drop-in dsv_enc; levels in the decoders' output pass; hue rotation or any operation that mixes planes; tables
 * that change from picture to picture inside one call's clip; a histogram or auto-levels inside a session; fusing the tables into the
 * converter's launch. */
typedef struct { uint8_t lut[3][256]; } dsv1_levels;     /* Y, U, V; every content is valid */
int  dsv1_levels_identity(dsv1_levels *lv);
int  dsv1_levels_range(dsv1_levels *lv, int src_full, int dst_full);
int  dsv1_levels_adjust(dsv1_levels *lv, int in_black, int in_white, int out_black, int out_white, int sat_q8);
int  dsv1_levels_compose(const dsv1_levels *a, const dsv1_levels *b, dsv1_levels *out);
int  dsv1_levels_is_identity(const dsv1_levels *lv);
int  dsv1_range_from_histogram(const uint32_t *hist, int n, int ppm, int *full);
int  dsv1_points_from_histogram(const uint32_t *hist, int n, int low_ppm, int high_ppm, int *black, int *white);
int  dsv1_levels_clip(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsv1_levels *lv, int on_device);
int  dsv1_histogram_clip(int device, const void *src, int w, int h, int subsamp, int n, uint32_t *hist, int on_device);
int  dsv1_detect_range_clip(int device, const void *src, int w, int h, int subsamp, int n, int ppm, int *full, int on_device);
int  dsv1_batch_set_source_levels(dsv1_batch *b, const dsv1_levels *lv);               /* NULL or the identity = off */
int  dsv1_resladder_set_levels(dsv1_resladder *r, const dsv1_levels *lv);

/* ---- extension: overlays -- logos, watermarks, bitmap subtitles and slates burned into the sources (csrc/k_overlay.hip; the plan:
 * csrc/dsvg_overlay_plan.h; stated in numpy in tests/_overlay.py) ----
 * Alpha compositing of a list of timed bitmaps, with fades, as the LAST source pass.  Exact integers; nothing here rounds in floating
 * point.  (The decoders' draw_info below is a different thing: debug drawing on decoded pictures.)
 * DEFINITION.  A BITMAP is four 8-bit planes, tightly packed in this order: Y (w x h), U and V (cw x ch, cw = rshift_up(w, hs), ch =
 * rshift_up(h, vs) at the session's subsampling), A (w x h, straight alpha, not premultiplied).  A PLACEMENT (dsv1_overlay) puts it with
 * its top left at x, y of the canvas -- the coded geometry, behind the reframe -- on pictures t0 .. t0 + dur - 1 (dur 0: for ever) of
 * source `source` (-1: every source), at `opacity` 0 .. 256, fading in over fade_in pictures and out over fade_out.
 *   The opacity of picture t (dsv1_overlay_opacity_at, host only): 0 for t < t0 and, with dur > 0, for t >= t0 + dur; otherwise
 *     a = min(t - t0 + 1, fade_in + 1),  b = fade_out + 1 with dur == 0, else min(t0 + dur - t, fade_out + 1),
 *     op = r(opacity * a * b / ((fade_in + 1) * (fade_out + 1))), r() the round-half-up of the levels section, in 64-bit arithmetic.
 *   Chroma alpha: A_c[Y][X] = r(sum / count) over the bitmap's own alpha samples that chroma sample covers -- 1, 2 or 4 at 4:2:0,
 *     1 .. 4 in a row at 4:1:1, fewer where an odd w or h ends inside the sample.  (Not weighted by anything but the count.)
 *   The blend, for every plane and every sample the bitmap covers, alpha = A (luma) or A_c (chroma):
 *     k = alpha * op (0 .. 65280),  out = (in * (65280 - k) + ov * k + 32640) / 65280, the division a floor -- 65280 = 256 * 255: a
 *     shift, then an exact division by 255.  k == 0 gives in; alpha == 255 with op == 256 gives ov; the numerator stays below 2^24.
 *     Samples outside every overlay keep their bytes.
 *   Order: overlays composite in list order, later on top; each blend reads the result of the one before.
 * VALID (dsv1_overlay_valid, host only, 1 / 0): w, h >= 1; 0 <= x, x + w <= W, 0 <= y, y + h <= H; x a multiple of 1 << hs and y of
 * 1 << vs (w and h need not be); opacity in 0 .. 256; source in -1 .. S - 1; a subsampling the library knows (4:4:4, 4:2:2, 4:2:0,
 * 4:1:1); reserved == 0; planes not NULL.  (fade_in and fade_out are 0 .. 65535 by their type.)  Anything else is DSVG_ERR_ARG before
 * any device work.
 * THE PLAN (dsv1_overlay_plan, host only, no device): the items (overlay, source, frame in call, op) with op > 0 of a call of F frames
 * of S sources whose first pictures are counters[s], in the order source, frame, overlay, each with a layer: 1 + the largest layer of an
 * earlier item of the same source and frame whose luma rectangle intersects it, 1 where there is none.  Items of one layer never touch
 * the same byte; the pass is one launch per layer over every plane, source and frame of the call, sized by the items' area, and nothing
 * at all -- no launch, no upload, no copy -- for a call in which nothing is active.  Returns the number of items (the first `room` are
 * written; NULL / 0 counts) or DSVG_ERR_ARG; *nlayers is written when everything fitted.
 * dsv1_overlay_clip: in place and synchronous, on host or device memory (on_device); frame i is picture t_first + i of source 0 (the
 * list is valid for S == 1: source 0 or -1).
 * dsv1_overlay_from_rgba (host only): an RGBA image of `pitch` bytes a row (0: tight) in one of the 4-byte or 3-byte packed orders
 * (DSV1_RGB_*; planar orders: three tight planes of pitch bytes a row one after the other) -> the four planes into out_planes
 * (dsv1_overlay_bytes(w, h, subsamp) bytes).  Y, U, V are the RGB import's: r() of the forward table, the chroma halved horizontally
 * first and then vertically, (a + b + 1) >> 1 with the last column / row repeated -- at 4:1:1 horizontally twice; A is the alpha bytes,
 * 255 for orders without alpha.
 * SESSIONS.  The pass is the LAST of the source chain: convert -> levels -> deinterlace or inverse telecine -> denoise -> orient ->
 * reframe -> overlay, then the scales of a resolution ladder or the frame load.  It changes no geometry, so it may be set, replaced or
 * cleared in any order relative to the other passes -- but only with nothing in flight and nothing staged, else DSVG_ERR_ARG with the
 * setting left as it was; one invalid item refuses the whole list the same way.  dsv1_batch_set_source_overlays (plain batches, quality
 * ladders, chain mode): n in 0 .. DSV1_MAX_OVERLAYS; NULL or 0 clears -- no pass, and no lane if nothing else needs one.  The bitmaps are
 * copied: the caller's memory is free on return.  Every source keeps a picture counter: 0 when a list is set, advanced by
 * frames_per_call by every call, across calls as the noise filter's state is; dsv1_batch_overlay_seek(b, source or -1, t) sets it
 * (DSVG_ERR_ARG where no list is set).  The clip: where it reaches the pass in memory of the chain's own (another pass's output, or the
 * upload of a host clip) it is blended where it lies; a caller's device clip (plain or held) is first copied device-to-device into a
 * clip of the pass, and is never written.  A call in which nothing is active, with no other pass set, takes the path of a batch with
 * nothing set.  dsv1_batch_stage is refused while a list is set.  dsv1_resladder_set_overlays / _overlay_seek: the pass runs on the
 * canvas in front of the scales, and the overlaid clip stands for the source everywhere behind it, get_src_sse / get_src_ssim included.
 * Not offered: the drop-in dsv_enc; overlays in the decoders' output pass; overlays that move or scale; text rendering; premultiplied
 * alpha; bitmaps partly off the canvas; replacing the list with batches in flight; alpha-weighted chroma. */
#define DSV1_MAX_OVERLAYS 4096
typedef struct {
    const uint8_t *planes;      /* Y, U, V, A */
    int w, h;
    int x, y;                   /* top left on the canvas */
    int source;                 /* -1: every source */
    int opacity;                /* 0 .. 256 */
    int64_t t0;                 /* the first picture */
    uint32_t dur;               /* pictures; 0: for ever */
    uint16_t fade_in, fade_out; /* pictures */
    int reserved;               /* 0 */
} dsv1_overlay;
typedef struct { int overlay, source, frame, op, layer; } dsv1_overlay_item;
size_t dsv1_overlay_bytes(int w, int h, int subsamp);           /* of a bitmap's four planes; 0 for invalid arguments */
int  dsv1_overlay_valid(const dsv1_overlay *ov, int W, int H, int subsamp, int S);
int  dsv1_overlay_opacity_at(const dsv1_overlay *ov, int64_t t);
long long dsv1_overlay_plan(const dsv1_overlay *list, int n, int S, int F, const int64_t *counters, int W, int H, int subsamp,
                            dsv1_overlay_item *items, long long room, int *nlayers);
int  dsv1_overlay_from_rgba(const void *rgba, int pitch, int w, int h, int order, int matrix, int full_range, int subsamp, uint8_t *out_planes);
int  dsv1_overlay_clip(int device, void *clip, int w, int h, int subsamp, int n, const dsv1_overlay *list, int count, int64_t t_first,
                       int on_device);
int  dsv1_batch_set_source_overlays(dsv1_batch *b, const dsv1_overlay *list, int n);   /* NULL or 0 = off */
int  dsv1_batch_overlay_seek(dsv1_batch *b, int source, int64_t t);
int  dsv1_resladder_set_overlays(dsv1_resladder *r, const dsv1_overlay *list, int n);
int  dsv1_resladder_overlay_seek(dsv1_resladder *r, int source, int64_t t);

/* ---- extension: debug overlays (csrc/k_drawinfo.hip; stated in Python in tests/_drawinfo.py) ----
 * The reference decoder's -drawinfo (draw_info dsv_decoder.c:147-243), drawn on the device ahead of the output pass: what an encoder
 * decided, on the decoded luma of every picture that has a reference (P pictures; I pictures and chroma are untouched, and so are the
 * pictures later ones predict from -- the overlay goes onto a copy).  Blocks are walked in raster order, block (i, j) at x = i blk_w,
 * y = j blk_h, and a later writer of a pixel wins:
 *   grid     any non-zero mode: luma row y is 0 (once per block row, before its blocks), then column x, rows y .. min(y + blk_h, h) - 1;
 *   dash     DSV_DRAW_STABHQ, blocks whose stability flag has bit 0: (x + blk_w/2 + k, y + blk_h/2), k = -(blk_w/4) .. blk_w/4, is 255
 *            for odd k, 0 for even k;
 *   vector   DSV_DRAW_MOVECS, inter blocks: the walk of csrc/dsvg_drawvec.h from the block's centre (x + blk_w/2, y + blk_h/2) towards the
 *            centre + (mv.x, mv.y), the vector raw, as pixels: every point up to, not including, the end is 0 (a zero vector: the centre);
 *   dots     DSV_DRAW_IBLOCK, intra blocks: 255 at (x + blk_w (1 + 2a) / 4, y + blk_h (1 + 2b) / 4) for every set submask bit a + 2b.
 * Everything is clipped to the luma plane.  DEVIATION: the reference does not bounds-check its dots, so with a dimension that is no
 * multiple of the block size the dots of its edge blocks land outside the luma plane, in chroma; here such a dot is not drawn.  On
 * block-multiple geometries the result is the reference's, byte for byte.
 * dsv_dec honours DSV_DECODER.draw_info as the reference does (any non-zero value: the grid; bits 1, 2, 4 the rest; others ignored).
 * dsv1_decbatch_set_draw_info: mode 0 .. 7 (else DSVG_ERR_ARG) for every later call and every output setting -- the overlay is on the
 * decoded luma before the one output pass, so a frame is export(overlay(plain decode)); it outlives a rebuilt context.  With mode 0
 * nothing is allocated, copied or launched.
 * dsv1_packet_blockinfo (host only): the side information of one picture packet of a w x h stream as the decoders parse it: the block
 * size, whether the picture has a reference and one dsv1_blockinfo per block in raster order (n: room in `out`, at least
 * ceil(w / blk_w) * ceil(h / blk_h)).  Without a reference only `stable` is filled.  DSVG_ERR_ARG for anything but a well-formed
 * picture packet, or too small an n.
 * dsv1_draw_info_clip: the same overlay on n tightly packed planar frames in place (host or device memory; synchronous), frame i from
 * the table info + i * ceil(w / blk_w) * ceil(h / blk_h); block sizes 16 .. 64, mode 1 .. 7, a subsampling the library knows.
 * Not offered: overlays on the encoder's reconstructions, drawing into chroma, the reference's out-of-plane dots, colours or labels. */
#define DSV_DRAW_STABHQ 1        /* dsv_decoder.h:38-40 */
#define DSV_DRAW_MOVECS 2
#define DSV_DRAW_IBLOCK 4
typedef struct {
    int16_t mvx, mvy;            /* inter blocks */
    uint8_t mode;                /* 0 inter, 1 intra */
    uint8_t submask;             /* intra blocks: DSV_MASK_INTRA* bits */
    uint8_t stable;              /* bit 0 of the stream's stability flag */
    uint8_t reserved;
} dsv1_blockinfo;
int  dsv1_decbatch_set_draw_info(dsv1_decbatch *d, int mode);

/* ---- extension: decoder output scale (csrc/k_scale.hip, k_scale_slots; stated in numpy in tests/_resample.py) ----
 * dsv1_decbatch_set_output_scale: the batched decoder hands out its pictures at out_w x out_h in the place of the streams' size --
 * proxies, thumbnails, a fixed display size -- resampled inside its one output pass, so the full-size frames never leave the
 * reconstruction slots.  The definition is dsv1_resample_clip's: every plane on its own, at the streams' subsampling (chroma planes
 * of rshift_up(out_w) x rshift_up(out_h)), exact integers, filter DSV1_SCALE_TENT or DSV1_SCALE_CUBIC; any ratio with
 * 1/8 <= source / output <= 8 on every axis of every plane, up or down, each axis on its own.
 * Order of the pass: the debug overlay at the streams' resolution, then the scale at the streams' subsampling, then the output
 * format's chroma halving or doubling, depth, packing or RGB matrix: a frame is export(resample(overlay(plain decode))).
 * SCALE FIRST, FORMAT SECOND.  The call drops whatever output format is in force: output is packed planar frames of the scaled
 * geometry again.  dsv1_decbatch_set_output_format, _format_up and _set_output_rgb called after it resolve for the scaled geometry
 * (a dsv1_pix_format with explicit pitches has to fit it).  0, 0 switches the scale off, and drops the format as well.
 * DSVG_ERR_ARG -- a ratio out of range, an unknown filter, a size that is not positive, d == NULL -- leaves scale and format in
 * force as they were.  Between calls; from the next decode call on; the setting outlives a rebuilt context.  The reference pictures
 * stay at full size.  dsv1_decbatch_out_frame_bytes follows (packed planar: the scaled frame); a smaller out_pitch is DSVG_ERR_ARG.
 * dsv1_decbatch_out_dims: the luma size of the frames handed out under the setting in force (the streams' own with the scale off).
 * Not offered: a scale in the frame-at-a-time dsv_dec (a DSV_FRAME has the stream's geometry), one size per stream. */
int  dsv1_decbatch_set_output_scale(dsv1_decbatch *d, int out_w, int out_h, int filter);   /* 0, 0: off; filter: DSV1_SCALE_* */
int  dsv1_decbatch_out_dims(const dsv1_decbatch *d, int *w, int *h);
int  dsv1_packet_blockinfo(const uint8_t *data, size_t len, int w, int h, int *blk_w, int *blk_h, int *has_ref, dsv1_blockinfo *out, size_t n);
int  dsv1_draw_info_clip(int device, void *clip, int w, int h, int subsamp, int n, int blk_w, int blk_h, const dsv1_blockinfo *info, int mode,
                         int on_device);

#ifdef __cplusplus
}
#endif
#endif
