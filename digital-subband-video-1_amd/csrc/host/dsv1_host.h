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

/* the tightly packed planar frame */
static inline size_t dsv1_frame_bytes(int w, int h, int subsamp)
{
    const int hs = (subsamp >> 2) & 3, vs = subsamp & 3;
    return (size_t)w * h + 2 * (size_t)((w + (1 << hs) - 1) >> hs) * (size_t)((h + (1 << vs) - 1) >> vs);
}

/* dsv1_srcchain.c: the source side of a session -- a lane, the optional converter, levels, deinterlacer, noise filter, orientation, reframe and overlays with their
 * settings, and each pass's output clip per call parity (a batch of that parity reads the last one as a held clip until its collect).
 * A chain with no pass set holds no lane -- no stream, no device memory -- unless the session keeps it (keep_lane: a resolution
 * ladder uploads and scales on it).  The setters replace or (NULL) clear one pass; on an error the chain is as it was.  The session
 * checks that nothing is in flight, and its arguments, before it calls one.
 * THREE GEOMETRIES.  RAW, w x h (fb), is what convert, levels, deinterlace and denoise are built for: the frames that come in.  ORIENTED,
 * mw x mh (mfb), is what the orientation leaves and the reframe reads.  CANVAS, ow x oh (ofb), is the clip the chain hands on: the
 * session's geometry.  Raw and oriented differ only while a transposing orientation is set, oriented and canvas only while a reframe
 * -- the LAST pass -- is set.  The reframe may be set, changed or cleared only while no other pass is set, the orientation only while
 * none but the reframe is (the session checks); the passes set after them resolve at w x h. */
enum { DSV1_SRC_CONVERT, DSV1_SRC_DEINTERLACE, DSV1_SRC_DENOISE, DSV1_SRC_ORIENT, DSV1_SRC_REFRAME, DSV1_SRC_LEVELS, DSV1_SRC_OVERLAY,
       DSV1_SRC_SCALE,
       DSV1_SRC_IVTC };                 /* (the inverse telecine: exclusive with the deinterlacer, whose place and clips it takes) */
typedef struct {
    int device, w, h, subsamp, nsrc, F, keep_lane;
    int mw, mh;                         /* the oriented geometry: the reframe's input */
    int ow, oh;                         /* the geometry handed on (the session's) */
    size_t fb, raw_fb, mfb, ofb;        /* the packed planar frame that comes in; the converter's source frame; the oriented frame; the frame handed on */
    dsvg_lane *lane;
    dsvg_pixconv *pc;
    dsvg_deint *dd;
    dsv1_deint dd_set;
    dsvg_ivtc *iv;                      /* the inverse telecine, in the deinterlacer's place (never both) */
    dsv1_ivtc iv_set;
    int conv_frames;                    /* frames per source the converter's clips, and the levels', hold */
    dsvg_levels *lv;                    /* directly behind the converter; its clips are sized as the converter's */
    dsvg_denoise *dn;
    dsv1_denoise dn_set;
    dsvg_orient *orn;
    int orient;                         /* the code set (0: no pass) */
    dsvg_reframe *rf;
    /* the overlays: the LAST pass, on the canvas, IN PLACE on whatever clip of the chain's own reaches it; its two clips exist only
     * once a caller's device clip reached it with no other pass set (copied there first).  ov_t[s]: source s's picture counter */
    dsvg_overlay *ov;
    int64_t *ov_t;
    void *clip[7][2];
} dsv1_srcchain;
void dsv1_srcchain_init(dsv1_srcchain *c, int device, int w, int h, int subsamp, int nsrc, int F, int keep_lane);
void dsv1_srcchain_close(dsv1_srcchain *c);            /* waits for the lane; frees everything */
int  dsv1_srcchain_lane(dsv1_srcchain *c);             /* creates the lane where there is none yet */
int  dsv1_srcchain_set_format(dsv1_srcchain *c, const dsv1_pix_layout *L, const dsv1_rgb_layout *R);      /* one of them, or neither: no converter */
int  dsv1_srcchain_set_deinterlace(dsv1_srcchain *c, const dsv1_deint *di);         /* (resets the noise filter's state) */
int  dsv1_srcchain_set_denoise(dsv1_srcchain *c, const dsv1_denoise *dn);
/* the inverse telecine (resets the noise filter's state).  A call then brings 5 F / 4 frames per source: the converter's clips are
 * allocated again for them, and again for F when it is cleared; on an error the chain is as it was.  The session checks that F is a
 * multiple of 4 and that no deinterlacer is set (and no inverse telecine when it sets a deinterlacer). */
int  dsv1_srcchain_set_ivtc(dsv1_srcchain *c, const dsv1_ivtc *iv);
int  dsv1_srcchain_ivtc_reset(dsv1_srcchain *c, int source);                        /* DSVG_ERR_ARG where the pass is not set */
/* a valid reframe whose canvas is ow x oh, or NULL / the identity: none.  DSVG_ERR_ARG, chain as it was, while another pass is set */
int  dsv1_srcchain_set_reframe(dsv1_srcchain *c, const dsv1_reframe *rf);
/* a code valid at the chain's subsampling; 0: none.  The oriented geometry stays, the raw one becomes what the inverse code makes of
 * it.  DSVG_ERR_ARG, chain as it was, while a pass other than the reframe is set */
int  dsv1_srcchain_set_orient(dsv1_srcchain *c, int orient);
/* tables, or NULL / the identity: none.  Forgets the deinterlacer's history, the inverse telecine's and the noise filter's state */
int  dsv1_srcchain_set_levels(dsv1_srcchain *c, const dsv1_levels *lv);
int  dsv1_reframe_is_identity(const dsv1_reframe *rf);  /* dsv1_reframe.c: window = input = canvas at 0, 0 */
int  dsv1_srcchain_deinterlace_reset(dsv1_srcchain *c, int source);                 /* DSVG_ERR_ARG where the pass is not set */
int  dsv1_srcchain_denoise_reset(dsv1_srcchain *c, int source);
/* a list of n valid placements on the canvas (the bitmaps are copied), or NULL / 0: none.  The counters start at 0.  It changes no
 * geometry: any order relative to the other setters.  _seek: source s's (-1: every source's) next picture is t; DSVG_ERR_ARG where no
 * list is set */
int  dsv1_srcchain_set_overlays(dsv1_srcchain *c, const dsv1_overlay *list, int n);
int  dsv1_srcchain_overlay_seek(dsv1_srcchain *c, int source, int64_t t);
/* the passes that write a clip of their own (everything but the overlays) */
static inline int dsv1_srcchain_writes(const dsv1_srcchain *c) { return c->pc || c->lv || c->dd || c->iv || c->dn || c->orn || c->rf; }
static inline int dsv1_srcchain_any(const dsv1_srcchain *c) { return dsv1_srcchain_writes(c) || c->ov; }
int  dsv1_srcchain_frames_in(const dsv1_srcchain *c);  /* frames per source and call that come in: F, F / 2 at field rate, 5 F / 4 in front of the inverse telecine */
size_t dsv1_srcchain_bytes_in(const dsv1_srcchain *c); /* ... and the bytes of a call's clip */
/* a call's clip (host memory: uploaded into the buffer of the parity first) through whichever of convert -> levels -> deinterlace -> denoise ->
 * orient -> reframe -> overlay are set, enqueued on the lane; *out: the device clip that stands for the source from there on (the input itself where
 * nothing ran: no pass set, or overlays alone with none active in the call -- then host memory comes back as host memory unless the session keeps the lane) */
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
