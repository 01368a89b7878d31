/* dsvg_pixfmt.h -- private: the layout a source pixel format (include/dsv1_api.h, dsv1_pix_format) works out to for one geometry, and
 * the device side of the source passes (dsvg_lane.hip, k_pixfmt.hip, k_rgb.hip, k_hdr.hip, k_deint.hip, k_ivtc.hip, k_denoise.hip, k_reframe.hip, k_orient.hip, k_levels.hip, k_overlay.hip).  Read by the C session layer and by the HIP plumbing. */
#ifndef DSVG_PIXFMT_H
#define DSVG_PIXFMT_H

#include "../../include/dsv1_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a SEGMENT is one source plane and the output planes it feeds */
enum { DSV1_PIXSEG_PLAIN, DSV1_PIXSEG_PAIR, DSV1_PIXSEG_YUYV, DSV1_PIXSEG_UYVY };
typedef struct {
    int kind;                   /* PLAIN: one sample -> one byte of one plane; PAIR: interleaved (a, b) samples -> two planes; YUYV / UYVY:
                                   macro-pixels -> Y, U, V */
    int rows;
    int width;                  /* output bytes per row of the first output plane (PLAIN / PAIR: samples / pairs per row; packed: w) */
    int cwidth;                 /* packed: macro-pixels per row = bytes per row of the U and V planes */
    int nout;
    int dpitch[3];              /* output planes: row pitch (tight) and offset inside the packed planar frame */
    size_t doff[3];
    size_t soff, spitch;        /* the source plane inside a source frame */
} dsv1_pix_seg;
typedef struct {
    int nseg;
    int wide;                   /* 16-bit words */
    int shift;                  /* wide: (x >> shift) & 0x1ff are the sample's 9 leading significant bits t; output min(255, (t + 1) >> 1) */
    size_t frame_bytes;         /* source frame to frame */
    size_t planes_bytes;        /* what a source frame holds: the last frame need not be longer */
    size_t out_frame_bytes;
    dsv1_pix_seg seg[3];
    /* chroma halved on the way (include/dsv1_api.h, chroma resampling): horizontally / vertically, o = (a + b + 1) >> 1 on the 8-bit
     * samples, the last column / row repeated, horizontally first; scw x sch are the chroma dims of the source.  The chroma outputs of
     * a segment then have the halved dims (PLAIN / PAIR: rows and width; packed: cwidth, and a chroma row for every two of `rows`). */
    int hd, vd, scw, sch;
} dsv1_pix_layout;
/* the layout of *pf at src_subsamp for frames at `subsamp` (the same, or one that halves: 4:4:4 -> 4:2:2 / 4:2:0, 4:2:2 -> 4:2:0).
 * DSVG_OK, or DSVG_ERR_ARG for every combination include/dsv1_api.h calls invalid; no device is looked at */
int dsv1_pix_layout_of(const dsv1_pix_format *pf, int w, int h, int src_subsamp, int subsamp, dsv1_pix_layout *L);
int dsv1_pix_is_default(const dsv1_pix_format *pf, int w, int h, int subsamp);      /* NULL, or planar / 8 bits / tight */
/* The other direction (decoder output formats, k_pixout.hip): format *pf at subsampling out_subsamp for frames decoded at `subsamp`,
 * resolved for the output pass.  DSVG_ERR_ARG for an invalid format and for every pair but: the same subsampling, 4:4:4 -> 4:2:2,
 * 4:4:4 or 4:2:2 -> 4:2:0, and -- upsample a DSV1_CHROMA_* mode, not DSV1_CHROMA_NONE -- 4:2:0 -> 4:2:2 / 4:4:4, 4:2:2 -> 4:4:4. */
#define DSV1_CHROMA_NONE (-1)
int dsv1_pixout_of(const dsv1_pix_format *pf, int w, int h, int subsamp, int out_subsamp, int upsample, dsvg_pixout *F);

/* ---- the lane: where a session's source-side work is enqueued (dsvg_lane.hip) ----
 * One non-blocking stream, one event, two raw upload buffers (per call parity, grown on demand) and the device memory handed out.
 * The passes below own none of that: they take the stream to launch on.  _upload / _copy_in put host / device bytes into upload
 * buffer `buf` on the stream, behind the pass that read it last; _download is the copy and the wait; _order records everything
 * enqueued so far and makes a context's frame-load stream wait for it, on the device; _free waits for the stream and gives one
 * allocation back; _destroy waits for the stream and frees everything. */
typedef struct dsvg_lane dsvg_lane;
int  dsvg_lane_create(dsvg_lane **out, int device);
void dsvg_lane_destroy(dsvg_lane *l);
int  dsvg_lane_alloc(dsvg_lane *l, void **dptr, size_t bytes);
int  dsvg_lane_free(dsvg_lane *l, void *dptr);
int  dsvg_lane_upload(dsvg_lane *l, int buf, const void *host, size_t bytes, void **dptr);
int  dsvg_lane_copy_in(dsvg_lane *l, int buf, const void *dev, size_t bytes, void **dptr);
int  dsvg_lane_copy_dd(dsvg_lane *l, void *dst_dev, const void *src_dev, size_t bytes);       /* device to device on the stream */
int  dsvg_lane_download(dsvg_lane *l, void *host, const void *dptr, size_t bytes);
int  dsvg_lane_order(dsvg_lane *l, dsvg_ctx *ctx);
int  dsvg_lane_sync(dsvg_lane *l);
void *dsvg_lane_stream(dsvg_lane *l);

/* The passes: parameters, their own device state, per-source validity.  _run enqueues on `stream` and returns.  _destroy frees memory
 * the pass's kernels may still read: the caller waits for the lane they ran on first (dsvg_lane_sync). */

/* A converter of one (geometry, subsampling, format): nframes source frames -> tightly packed planar frames (device pointers). */
typedef struct dsvg_pixconv dsvg_pixconv;
int  dsvg_pixconv_create(dsvg_pixconv **out, int device, const dsv1_pix_layout *L);
void dsvg_pixconv_destroy(dsvg_pixconv *c);
int  dsvg_pixconv_run(dsvg_pixconv *c, void *stream, const void *src_dev, int nframes, void *dst_dev);


/* ---- RGB (include/dsv1_api.h, RGB; k_rgb.hip; host side: host/dsv1_rgb.c) ----
 * An RGB format resolved for one geometry and one subsampling of the YCbCr side: the planes, the position of R, G and B in memory
 * order, the tables.  One layout serves both directions. */
typedef struct {
    int w, h, hs, vs, cw, ch;
    int nplanes;                /* 1: packed (bpp 3 or 4); 3: planar (bpp 1) */
    int bpp;
    int first;                  /* 4-byte orders: the byte of the pixel that holds the first colour component (0 or 1) */
    int comp[3];                /* memory position k (byte after `first` / plane k) holds 0 R, 1 G, 2 B */
    int linear;                 /* output: DSV1_CHROMA_LINEAR */
    int oy;
    int32_t fwd[9], inv[5];
    size_t off[3], pitch[3];
    size_t frame_bytes;         /* RGB frame to frame */
    size_t planes_bytes;        /* what an RGB frame holds */
    size_t yuv_frame_bytes;     /* the tightly packed planar frame */
} dsv1_rgb_layout;
/* DSVG_OK, or DSVG_ERR_ARG for whatever include/dsv1_api.h calls invalid (4:1:1 included); no device is looked at */
int dsv1_rgb_layout_of(const dsv1_rgb_format *rf, int w, int h, int subsamp, dsv1_rgb_layout *L);
/* the output pass's view of it: frames decoded at `subsamp` -> RGB frames */
int dsv1_rgbout_of(const dsv1_rgb_format *rf, int w, int h, int subsamp, dsvg_pixout *F);
/* a dsvg_pixconv whose pass is the RGB import (k_rgb.hip) instead of a re-packing */
int  dsvg_pixconv_create_rgb(dsvg_pixconv **out, int device, const dsv1_rgb_layout *L);
/* the pass itself, on a stream of the caller's: nframes RGB frames of layout *L -> tightly packed planar frames (device pointers) */
int  dsvg_rgb_import_run(void *stream, const dsv1_rgb_layout *L, const void *src_dev, int nframes, void *dst_dev);

/* ---- HDR sources (include/dsv1_api.h, HDR sources; k_hdr.hip; host side: host/dsv1_hdr.c) ----
 * A deep pixel format resolved for one geometry and one pair of subsamplings: the source planes (semi: 0 planar, 1 interleaved
 * (U, V), 2 (V, U); the chroma planes' offsets and pitches in [1] and [2], the same plane twice where interleaved), the sample rule
 * (word >> vshift) & vmask then min(1023, (v + rnd) >> rs), and the dims of the chroma planes on both sides. */
typedef struct {
    int w, h;
    int shs, svs, scw, sch;     /* the source's chroma shifts and dims */
    int dhs, dvs, ocw, och;     /* the output's */
    int semi;
    int vshift, vmask, rs, rnd;
    size_t off[3], pitch[3];
    size_t frame_bytes;         /* source frame to frame */
    size_t planes_bytes;        /* what a source frame holds */
    size_t out_frame_bytes;     /* the tightly packed planar frame */
} dsv1_hdr_layout;
/* DSVG_OK, or DSVG_ERR_ARG for whatever include/dsv1_api.h calls invalid; no device is looked at */
int  dsv1_hdr_layout_of(const dsv1_pix_format *pf, int w, int h, int src_subsamp, int subsamp, dsv1_hdr_layout *L);
/* a dsvg_pixconv whose pass is the HDR import (k_hdr.hip); it owns the tables' device copy.  upsample: DSV1_CHROMA_* */
int  dsvg_pixconv_create_hdr(dsvg_pixconv **out, int device, const dsv1_hdr_layout *L, const dsv1_hdr_tables *tables, int upsample);
/* the pass itself, on a stream of the caller's: nframes frames of layout *L -> tightly packed planar frames (device pointers).
 * tab_dev: DSVG_HDR_TAB_WORDS dwords in device memory as dsvg_hdr_tab_pack lays the three lookup tables out; rows: the small tables,
 * which travel as kernel arguments (dsvg_hdr_rows_of); cus: the device's CUs -- the launch is as many workgroups as are resident at
 * once, each of which stages the lookup tables once and walks items of the whole call */
#define DSVG_HDR_TAB_WORDS (4096 + DSV1_HDR_NBUCKETS + (DSV1_HDR_NBUCKETS + 1) / 2)
typedef struct { int32_t ycc[5], in_oy, in_oc, gamut[9], fwd[9], ybias, cbias; } dsvg_hdr_rows;
void dsvg_hdr_tab_pack(const dsv1_hdr_tables *tables, uint32_t *words);
void dsvg_hdr_rows_of(const dsv1_hdr_tables *tables, dsvg_hdr_rows *rows);
int  dsvg_hdr_import_run(void *stream, const dsv1_hdr_layout *L, const dsvg_hdr_rows *rows, const uint32_t *tab_dev, int upsample, int cus,
                         const void *src_dev, int nframes, void *dst_dev);


/* ---- deinterlacing (include/dsv1_api.h, Deinterlacing; k_deint.hip; host side: host/dsv1_deint.c) ----
 * A deinterlacer of one (geometry, subsampling, mode, field order) for nsrc sources and -- with_history -- each source's last input
 * frame, which is the next call's prv.  _run deinterlaces a call's clip ([source][nin frames] -> [source][nin or 2 nin pictures]);
 * _reset forgets one source's history (-1: all).  _clip is the standalone pass with an explicit prev and no history. */
int  dsv1_deint_valid(const dsv1_deint *di);            /* 1: mode and tff are ones include/dsv1_api.h knows */
typedef struct dsvg_deint dsvg_deint;
int  dsvg_deint_create(dsvg_deint **out, int device, int w, int h, int subsamp, const dsv1_deint *di, int nsrc, int with_history);
void dsvg_deint_destroy(dsvg_deint *d);
int  dsvg_deint_run(dsvg_deint *d, void *stream, const void *src_dev, int nin, void *dst_dev);
int  dsvg_deint_clip(dsvg_deint *d, void *stream, const void *src_dev, int n, const void *prev_dev, void *dst_dev);
int  dsvg_deint_reset(dsvg_deint *d, int source);

/* ---- inverse telecine and field metrics (include/dsv1_api.h, Inverse telecine; k_ivtc.hip; host side: host/dsv1_ivtc.c; the two
 * decision rules: dsvg_ivtc_rules.h) ----
 * An inverse telecine of one (geometry, subsampling, field order, nt) for nsrc sources, nin frames per source and call (a multiple of
 * 5), its decision tables in device memory and -- with_state -- each source's state.  _run takes a call's clip ([source][nin frames] ->
 * [source][4 nin / 5 pictures]) and refreshes the states; _reset forgets one source's (-1: all).  _clip is the standalone pass of one
 * stream (nsrc == 1) with explicit states (frame bytes + w * h each, device memory, either may be NULL, they may be the same) and none
 * kept; _tables: where the last call's match [nsrc][nin] and drop [nsrc][nin / 5] lie in device memory.  The field metrics of n frames
 * of one stream: [n][4] uint32 in device memory (zeroed on the stream first). */
int  dsv1_ivtc_valid(const dsv1_ivtc *iv);              /* 1: tff 0 / 1, nt 0 .. 254, reserved 0 */
typedef struct dsvg_ivtc dsvg_ivtc;
int  dsvg_ivtc_create(dsvg_ivtc **out, int device, int w, int h, int subsamp, const dsv1_ivtc *iv, int nsrc, int nin, int with_state);
void dsvg_ivtc_destroy(dsvg_ivtc *d);
int  dsvg_ivtc_run(dsvg_ivtc *d, void *stream, const void *src_dev, void *dst_dev);
int  dsvg_ivtc_clip(dsvg_ivtc *d, void *stream, const void *src_dev, const void *state_in_dev, void *state_out_dev, void *dst_dev);
void dsvg_ivtc_tables(const dsvg_ivtc *d, const void **match_dev, const void **drop_dev);
int  dsvg_ivtc_reset(dsvg_ivtc *d, int source);
int  dsvg_field_metrics_run(int device, void *stream, const void *src_dev, int w, int h, int subsamp, int n, const void *prev_dev, int nt,
                            void *metrics_dev);

/* ---- temporal noise reduction (include/dsv1_api.h, Temporal noise reduction; k_denoise.hip; host side: host/dsv1_denoise.c) ----
 * A noise filter of one (geometry, subsampling, strengths) for nsrc sources and -- with_state -- each source's state in device memory:
 * pin, the last input picture (two buffers, read from one and written to the other), and S.  _run filters a call's clip ([source][n
 * pictures] -> the same); _reset forgets one source's state (-1: all).  _clip is the standalone pass with explicit states (3 frames'
 * bytes each, device memory, either may be NULL, they may be the same) and none kept. */
int  dsv1_denoise_valid(const dsv1_denoise *dn);        /* 1: both strengths in 0 .. 512 and not both 0 */
typedef struct dsvg_denoise dsvg_denoise;
int  dsvg_denoise_create(dsvg_denoise **out, int device, int w, int h, int subsamp, const dsv1_denoise *dn, int nsrc, int with_state);
void dsvg_denoise_destroy(dsvg_denoise *d);
int  dsvg_denoise_run(dsvg_denoise *d, void *stream, const void *src_dev, int n, void *dst_dev);
int  dsvg_denoise_clip(dsvg_denoise *d, void *stream, const void *src_dev, int n, const void *state_in_dev, void *state_out_dev, void *dst_dev);
int  dsvg_denoise_reset(dsvg_denoise *d, int source);

/* ---- reframe and line sums (include/dsv1_api.h, Reframe; k_reframe.hip; host side: host/dsv1_reframe.c) ----
 * A reframe of one (dsv1_reframe, subsampling): nframes frames of in_w x in_h -> nframes frames of out_w x out_h; it keeps no state
 * and owns no device memory.  The line sums of one geometry: nframes frames -> row sums [nframes][h] and column sums [nframes][w] of
 * the luma, uint32 in device memory (the column sums are zeroed on the stream first). */
typedef struct dsvg_reframe dsvg_reframe;
int  dsvg_reframe_create(dsvg_reframe **out, int device, const dsv1_reframe *rf, int subsamp);
void dsvg_reframe_destroy(dsvg_reframe *r);
int  dsvg_reframe_run(dsvg_reframe *r, void *stream, const void *src_dev, int nframes, void *dst_dev);
/* ---- orientation (include/dsv1_api.h, Orientation; k_orient.hip; host side: host/dsv1_orient.c) ----
 * One code for frames that come in at w x h: nframes frames -> nframes frames of dsv1_orient_dims(orient, w, h); it keeps no state
 * and owns no device memory.  Code 0 is a device-to-device copy on the stream (the standalone call's; a session sets no pass for it). */
typedef struct dsvg_orient dsvg_orient;
int  dsvg_orient_create(dsvg_orient **out, int device, int orient, int w, int h, int subsamp);
void dsvg_orient_destroy(dsvg_orient *o);
int  dsvg_orient_run(dsvg_orient *o, void *stream, const void *src_dev, int nframes, void *dst_dev);
/* ---- levels and the histogram (include/dsv1_api.h, Levels; k_levels.hip; host side: host/dsv1_levels.c) ----
 * Three tables for frames of w x h: nframes frames -> nframes frames, out_p[i] = lut[p][in_p[i]], dst == src allowed (the pass is
 * pointwise); it keeps no state and owns 1 KiB of device memory, the tables.  In a session it runs directly behind the converter:
 * convert -> levels -> deinterlace or inverse telecine -> denoise -> orient -> reframe.  The histogram: nframes frames ->
 * uint32 [nframes][3][256] in device memory, zeroed on the stream first. */
typedef struct dsvg_levels dsvg_levels;
int  dsvg_levels_create(dsvg_levels **out, int device, const dsv1_levels *lv, int w, int h, int subsamp);
void dsvg_levels_destroy(dsvg_levels *l);
int  dsvg_levels_run(dsvg_levels *l, void *stream, const void *src_dev, int nframes, void *dst_dev);
int  dsvg_levels_set_replicas(dsvg_levels *l, int rep);   /* measurements: the copies of the table in LDS, 32 (default) or 1 */
typedef struct dsvg_histogram dsvg_histogram;
int  dsvg_histogram_create(dsvg_histogram **out, int device, int w, int h, int subsamp);
void dsvg_histogram_destroy(dsvg_histogram *g);
int  dsvg_histogram_run(dsvg_histogram *g, void *stream, const void *src_dev, int nframes, void *hist_dev);
/* ---- overlays (include/dsv1_api.h, Overlays; k_overlay.hip; the plan: dsvg_overlay_plan.h; host side: host/dsv1_overlay.c) ----
 * A list of n valid placements on frames of w x h for nsrc sources: the bitmaps (and their chroma alpha planes) are packed into device
 * memory at create, the caller's are free on return.  _run blends IN PLACE a call's clip, [source][nframes] frames, counters[s] the
 * picture source s's first frame is: the call is planned (dsvg_overlay_plan), the table goes up on the stream into the buffer of call
 * parity `par`, one launch per layer follows; nothing active: nothing is enqueued.  _active: the items such a call would blend (pure).
 * In a session it is the LAST pass: ... -> orient -> reframe -> overlay. */
typedef struct dsvg_overlay dsvg_overlay;
int  dsvg_overlay_create(dsvg_overlay **out, int device, const dsv1_overlay *list, int n, int w, int h, int subsamp, int nsrc);
void dsvg_overlay_destroy(dsvg_overlay *o);
long long dsvg_overlay_active(const dsvg_overlay *o, int nframes, const int64_t *counters);
int  dsvg_overlay_run(dsvg_overlay *o, void *stream, int par, void *clip_dev, int nframes, const int64_t *counters);
typedef struct dsvg_linesums dsvg_linesums;
int  dsvg_linesums_create(dsvg_linesums **out, int device, int w, int h, int subsamp);
void dsvg_linesums_destroy(dsvg_linesums *s);
int  dsvg_linesums_run(dsvg_linesums *s, void *stream, const void *src_dev, int nframes, void *row_dev, void *col_dev);

#ifdef __cplusplus
}
#endif
#endif
