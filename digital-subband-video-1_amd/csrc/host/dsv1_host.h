/* dsv1_host.h -- private helpers of the C session layer: MSB-first bit writer/reader with the
 * interleaved exp-Golomb codes (bs.c:28-267 semantics: the writer ORs into a zeroed buffer) and a
 * growable output buffer.  Host-only scalar code for headers and side information; the coefficient
 * payloads themselves are packed on the GPU. */
#ifndef DSV1_HOST_H
#define DSV1_HOST_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../../include/dsv1_api.h"
#include "../dsvg_pixfmt.h"       /* source pixel formats: the layout of a format; the lane and the passes in front of the encoder */

/* `end` bounds the READER (bits): past it every bit reads as 1 -- which ends any exp-Golomb prefix -- and `over` is set,
 * so a truncated or hostile packet can neither run the reader off its buffer nor loop; the writer ignores it */
typedef struct { uint8_t *p; unsigned pos, end; int over; } bitw;

static inline void bw_init(bitw *b, uint8_t *buf) { b->p = buf; b->pos = 0; b->end = ~0u; b->over = 0; }
static inline void br_init(bitw *b, uint8_t *buf, unsigned nbytes) { b->p = buf; b->pos = 0; b->end = nbytes > 0x1fffffffu ? ~0u : nbytes * 8u; b->over = 0; }
static inline void bw_align(bitw *b) { b->pos = (b->pos + 7u) & ~7u; }
static inline unsigned bw_bytes(const bitw *b) { return b->pos >> 3; }
static inline void bw_bit(bitw *b, unsigned one)
{
    if (one) b->p[b->pos >> 3] |= (uint8_t)(0x80u >> (b->pos & 7));
    b->pos++;
}
static inline void bw_bits(bitw *b, int n, unsigned v) { while (n--) bw_bit(b, (v >> n) & 1u); }
static inline void bw_ueg(bitw *b, unsigned v)
{
    const unsigned m = v + 1;
    int k = 31 - __builtin_clz(m);
    while (k-- > 0) { b->pos++; bw_bit(b, (m >> k) & 1u); }
    bw_bit(b, 1);
}
static inline void bw_seg(bitw *b, int v)
{
    const unsigned m = v < 0 ? (unsigned)-v : (unsigned)v;
    bw_ueg(b, m);
    if (m) bw_bit(b, v < 0);
}
static inline void bw_bytes_in(bitw *b, const uint8_t *src, unsigned n)
{
    memcpy(b->p + (b->pos >> 3), src, n);
    b->pos += n * 8u;
}

static inline unsigned br_bit(bitw *b)
{
    unsigned v;
    if (b->pos >= b->end) { b->over = 1; return 1u; }
    v = (b->p[b->pos >> 3] >> (7 - (b->pos & 7))) & 1u;
    b->pos++;
    return v;
}
static inline unsigned br_bits(bitw *b, int n) { unsigned v = 0; while (n--) v = (v << 1) | br_bit(b); return v; }
static inline unsigned br_ueg(bitw *b) { unsigned m = 1; int k = 0; while (!br_bit(b) && k++ < 32) m = (m << 1) | br_bit(b); return m - 1; }
static inline int br_seg(bitw *b) { int v = (int)br_ueg(b); return (v && br_bit(b)) ? -v : v; }

/* zero-bit run-length coder (bs.c:222-267) */
typedef struct { bitw b; int nz; } zrle;
static inline void zr_init(zrle *z, uint8_t *buf) { bw_init(&z->b, buf); z->nz = 0; }
static inline void zr_init_rd(zrle *z, uint8_t *buf, unsigned nbytes) { br_init(&z->b, buf, nbytes); z->nz = 0; }
static inline void zr_put(zrle *z, int bit) { if (bit) { bw_ueg(&z->b, (unsigned)z->nz); z->nz = 0; } else z->nz++; }
static inline int zr_end(zrle *z) { bw_ueg(&z->b, (unsigned)z->nz); z->nz = 0; bw_align(&z->b); return (int)bw_bytes(&z->b); }
static inline int zr_get(zrle *z)
{
    if (z->nz == 0) z->nz = (int)br_ueg(&z->b); else z->nz--;
    return z->nz == 0;
}

static inline void put_be32(uint8_t *p, unsigned v)
{
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
static inline unsigned get_be32(const uint8_t *p)
{
    return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3];
}

/* append n bytes to a dsv_alloc-backed growing DSV_BUF (capacity kept in a hidden word before data) */
int  dsv1_buf_append(DSV_BUF *b, const uint8_t *src, unsigned n);
int  dsv1_buf_reserve(DSV_BUF *b, unsigned n);
/* dsv_alloc without the zeroing (a buffer the library fills itself); freed with dsv_free like any other */
void *dsv1_alloc_raw(int size);
/* the decoder's pinned output frames (dsv1_util.c) */
#define DSV1_POOL_FRAMES 6
typedef struct dsv1_frame_pool dsv1_frame_pool;
dsv1_frame_pool *dsv1_pool_new(dsvg_ctx *ctx, int device, size_t bytes, int n);
void dsv1_pool_unref(dsv1_frame_pool *pl);
DSV_FRAME *dsv1_pool_frame(dsv1_frame_pool *pl, int format, int width, int height);
int dsv1_recycle_hold(int delta);       /* dsv1_util.c: +1 a batch opens, -1 it closes (the last one out releases the parked blocks) */
void dsv1_log(int level, const char *fmt, ...);
extern int dsv1_device;
/* parallel loop over S independent items on a persistent worker pool: fn(ctx, s, worker) for every s; DSV1_HOST_THREADS workers (default min(12,
 * half of this process's share of the cores)) */
typedef void (*dsv1_par_fn)(void *ctx, int s, int tid);
void dsv1_par_for(int S, dsv1_par_fn fn, void *ctx);
void dsv1_par_for_long(int S, dsv1_par_fn fn, void *ctx);      /* the same for a few long items (two already run in parallel) */
/* ONE background loop beside the foreground ones (round 6): begin returns at once, idle workers take the items (foreground loops go first), end joins
 * with the caller's help; a second begin joins the first.  fn / ctx must stay valid until the end call. */
void dsv1_par_bg_begin(int S, dsv1_par_fn fn, void *ctx);
void dsv1_par_bg_end(void);
int dsv1_par_bg_pending(void);
/* the default size of that pool as a function of the host (dsv1_util.c); exported so that the rule can be tested without the host it is for */
int dsv1_host_threads_rule(long online, long allowed, long ranks, int pinned_by_launcher);

/* dsv1_enc.c: the fields every rung of a quality ladder must agree on (dsv1_ladder_open) */
int dsv1_ladder_rungs_agree(const DSV_ENCODER *a, const DSV_ENCODER *b);
/* dsvg_pipe.hip: what dsvg_ctx_create would answer for the geometry, without a device (DSVG_OK, DSVG_ERR_ARG, DSVG_ERR_UNSUPPORTED) */
int dsvg_geom_check(int width, int height, int subsamp);
/* k_scale.hip: the device side of the resampler.  A scaler holds the weight tables of ngeom destination geometries of one source
 * geometry (uploaded once); _run scales a clip to geometry g on a stream of the caller's (a lane's, dsvg_pixfmt.h).  _destroy frees the
 * tables its kernels read: the caller waits for that lane first. */
typedef struct dsvg_scaler dsvg_scaler;
int  dsvg_scaler_create(dsvg_scaler **out, int device, int sw, int sh, int subsamp, int ngeom, const int *dw, const int *dh, int filter);
void dsvg_scaler_destroy(dsvg_scaler *s);
int  dsvg_scaler_run(dsvg_scaler *s, void *stream, int g, const void *src_dev, int nframes, void *dst_dev);

/* dsv1_srcchain.c: the source side of a session -- a lane, whichever of convert -> levels -> deinterlace or inverse telecine ->
 * denoise -> orient -> reframe -> overlay are set, and each pass's output clip per call parity (a batch of that parity reads the last
 * one as a held clip until its collect).  WHAT IS TAKEN AND REFUSED, the three geometries, the clips' sizes, what a setter forgets
 * behind it and when the lane exists are dsv1_srcchain_plan.h's (which also holds dsv1_frame_bytes): this file resolves a request's
 * arguments, asks the plan, and commits or enqueues what it says.  st is the plan's state of the chain, g what follows from it
 * (g.w x g.h: the frames that come in; g.ow x g.oh: the clip handed on).  On an error the chain is as it was (dsv1_srcchain_request
 * says what that means for a history). */
#include "dsv1_srcchain_plan.h"
enum { DSV1_SRC_CONVERT = DSV1_SC_CONVERT, DSV1_SRC_LEVELS, DSV1_SRC_DEINTERLACE, DSV1_SRC_IVTC, DSV1_SRC_DENOISE, DSV1_SRC_ORIENT, DSV1_SRC_REFRAME,
       DSV1_SRC_OVERLAY, DSV1_SRC_SCALE };             /* chain order; SCALE: the standalone clip call's only */
typedef struct {
    int device;
    dsv1_srcchain_state st;
    dsv1_srcchain_geom g;
    dsvg_lane *lane;
    void *pass[DSV1_SC_SLOTS];          /* the pass at each position (its kind: st.kind) */
    void *clip[DSV1_SC_SLOTS][2];       /* its output clip per call parity; the overlays': see dsv1_scp_call */
    int64_t *ov_t;                      /* [nsrc] the overlays' picture counters */
} dsv1_srcchain;
void dsv1_srcchain_init(dsv1_srcchain *c, int device, int w, int h, int subsamp, int nsrc, int F, int keep_lane);
void dsv1_srcchain_close(dsv1_srcchain *c);            /* waits for the lane; frees everything */
int  dsv1_srcchain_lane(dsv1_srcchain *c);             /* creates the lane where there is none yet */
/* ONE SETTER PATH for both sessions: resolve arg (NULL: clear the pass) with the kind's own check, dsv1_scp_set, on a refusal one
 * log line "who: text", else create the pass and commit.  arg by kind: CONVERT dsv1_src_format; LEVELS dsv1_levels; DEINTERLACE
 * dsv1_deint; IVTC dsv1_ivtc; DENOISE dsv1_denoise; ORIENT int; REFRAME dsv1_reframe; OVERLAY dsv1_src_overlays.  busy: the
 * session's (batches in flight or clips staged; calls in flight).
 * _signal: a reset (op DSV1_SC_OP_RESET: a discontinuity in `source`, -1 every source) or the overlays' seek (DSV1_SC_OP_SEEK: the
 * next picture of `source` is t), by the same plan and log line. */
/* pf, or rgb, or hdr (the tables of an HDR import of *pf at src_subsamp, chroma brought up by `upsample`), or none of them: no converter */
typedef struct { const dsv1_pix_format *pf; int src_subsamp; const dsv1_rgb_format *rgb; const dsv1_hdr_tables *hdr; int upsample; } dsv1_src_format;
typedef struct { const dsv1_overlay *list; int n; } dsv1_src_overlays;
int  dsv1_srcchain_request(dsv1_srcchain *c, const char *who, int busy, int kind, const void *arg);
int  dsv1_srcchain_signal(dsv1_srcchain *c, const char *who, int busy, int op, int kind, int source, int64_t t);
int  dsv1_reframe_is_identity(const dsv1_reframe *rf);  /* dsv1_reframe.c: window = input = canvas at 0, 0 */
static inline int dsv1_srcchain_any(const dsv1_srcchain *c)       /* a pass is set */
{
    int p, any = 0;
    for (p = 0; p < DSV1_SC_SLOTS; p++) any |= c->st.kind[p];
    return any;
}
/* a call's clip (host memory: uploaded into the buffer of the parity first) through the passes set, enqueued on the lane as
 * dsv1_scp_call says; *out: the device clip that stands for the source from there on (the input itself where nothing was enqueued) */
int  dsv1_srcchain_run(dsv1_srcchain *c, int par, const void *clip, int on_device, const void **out);
/* the standalone clip calls: one pass (DSV1_SRC_*; SCALE: a scaler's geometry 0) over n frames on a lane of the call's own.  in[0] the
 * clip, in[1] an optional second input (the deinterlacer's prev, the filter's state_in); out[0] the result, out[1] the filter's
 * state_out.  Host memory is uploaded / allocated / downloaded, device memory used in place; the call waits for the pass. */
typedef struct { const void *in[2]; size_t in_bytes[2]; void *out[2]; size_t out_bytes[2]; } dsv1_clip_io;
int  dsv1_pass_clip(int device, int kind, void *pass, int n, const dsv1_clip_io *io, int on_device);
/* dsv1_enc.c: whether the batch's source chain holds a lane right now (tests: a chain with no pass set holds none) */
int dsv1_batch_has_source_lane(const dsv1_batch *b);
/* dsv1_enc.c: source-resolution figures of a batch (dsvg_ctx_xres_enable; resolution ladders): stream k = s * R + r, frame t of a
 * call is measured against frame s * frames_per_call + t of the reference clip named for the next submit (device memory, kept until
 * that batch's collect); the figures of the batch collected last, [(k * F + t) * 3 + p].  Enable only between batches. */
int  dsv1_batch_xres_enable(dsv1_batch *b, int sse_on, int ssim_on, int ref_w, int ref_h, int filter);
int  dsv1_batch_xres_source(dsv1_batch *b, const void *ref_clip_dev);
int  dsv1_batch_get_xres_sse(const dsv1_batch *b, uint64_t *sse, size_t n);
int  dsv1_batch_get_xres_ssim(const dsv1_batch *b, int64_t *ssim_fx, size_t n);
/* the record of one kind of figure (DSVG_Q_*) that a batch, and a resolution ladder over its batches, keeps: the switch, and the
 * batch collected last: [streams][frames][3], the SSIM_FX sums as their two's complement; n values, 0 = not measured (or nothing
 * collected).  dsv1_batch_quality: the batch's own (NULL for no batch or no such kind), for the resolution ladder to gather from;
 * what it points to holds until the batch's next collect or close. */
typedef struct { int on; uint64_t *v; size_t n; } dsv1_quality;
const dsv1_quality *dsv1_batch_quality(const dsv1_batch *b, int kind);

#define CLAMPI(v, lo, hi) ((v) < (lo) ? (lo) : ((v) > (hi) ? (hi) : (v)))

#endif
