/* dsv1_scale.c -- the resampler's weight tables, the standalone scaler and resolution ladders (include/dsv1_api.h).
 *
 * The weight tables are the definition of the scaler (tests/_scale.py states the same in numpy): binary64, the order written
 * below, no contraction -- the Makefile compiles this file with -ffp-contract=off (gcc does not implement the STDC FP_CONTRACT
 * pragma), and tests/test_scale_host.py checks the object for fused multiply-adds and the tables against numpy.
 *
 * A resolution ladder is one quality ladder (dsv1_ladder_open) per geometry plus a source chain (dsv1_srcchain.c) and a scaler
 * (k_scale.hip).  A call uploads the source clip once on the chain's lane, scales it there for every geometry whose size differs
 * from the source's, and makes each geometry's frame-load stream wait for that on the device (dsvg_lane_order) before the geometry's
 * submit; the scaled clips go to the ladders as held device clips (DSV1_CLIP_HELD), one buffer per geometry and call parity, which
 * the next submit of the same parity -- after that geometry's collect -- overwrites.
 *
 * A source of another pixel format (dsv1_resladder_open_src), a deinterlacer, a noise filter: the raw clip is what crosses the link;
 * the chain's passes run on the lane in front of the scales, and the clip they leave, which the chain holds per call parity, stands
 * for the source from there on (scales, a geometry of the source's size, the source-resolution figures). */
#include <math.h>
#include "dsv1_host.h"

int dsv1_scale_taps(int S, int D, int filter)
{
    if (D < 1 || S < D) return DSVG_ERR_ARG;
    return dsv1_resample_taps(S, D, filter);
}

/* either direction, 1/8 <= S / D <= 8: r = ceil(support max(1, S / D)), T = 2r + 2 (for S >= D what dsv1_scale_taps always gave) */
int dsv1_resample_taps(int S, int D, int filter)
{
    const long long sup = filter == DSV1_SCALE_TENT ? 1 : filter == DSV1_SCALE_CUBIC ? 2 : 0;
    if (!sup || D < 1 || S < 1 || (long long)S > 8LL * D || (long long)D > 8LL * S) return DSVG_ERR_ARG;
    return (int)(2 * (S >= D ? (sup * S + D - 1) / D : sup) + 2);
}

static double scale_kernel(double x, int filter)
{
    if (filter == DSV1_SCALE_TENT) return x < 1.0 ? 1.0 - x : 0.0;       /* max(0, 1 - x) */
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
}

/* one axis's table in either direction (T checked by the caller): inv = min(1, D / S) -- the kernel is stretched only to downscale */
static void resample_table(int S, int D, int filter, int32_t *start, int16_t *q, int T)
{
    double w[2 * (2 * 8 + 1) + 2];                                      /* T <= 2 ceil(2 * 8) + 2 = 34 */
    int i, t;
    for (i = 0; i < D; i++) {
        const double c = (double)((2LL * i + 1) * S - D) / (double)(2LL * D);
        const double inv = S >= D ? (double)D / (double)S : 1.0;
        const long long j0 = (long long)floor(c) - (T - 2) / 2;
        double sum = 0.0;
        int s = 0, best = 0;
        for (t = 0; t < T; t++) {
            const double x = fabs(((double)(j0 + t) - c) * inv);
            w[t] = scale_kernel(x, filter);
            sum += w[t];
        }
        for (t = 0; t < T; t++) {
            const int v = (int)rint(w[t] * 16384.0 / sum);             /* round half to even (the default rounding mode) */
            q[(size_t)i * T + t] = (int16_t)v;
            s += v;
            if (v > q[(size_t)i * T + best]) best = t;
        }
        q[(size_t)i * T + best] = (int16_t)(q[(size_t)i * T + best] + 16384 - s);
        start[i] = (int32_t)j0;
    }
}

int dsv1_scale_weights(int S, int D, int filter, int32_t *start, int16_t *q, int T)
{
    const int Tn = dsv1_scale_taps(S, D, filter);
    if (Tn < 0 || T != Tn || !start || !q) return DSVG_ERR_ARG;
    resample_table(S, D, filter, start, q, T);
    return DSVG_OK;
}

int dsv1_resample_weights(int S, int D, int filter, int32_t *start, int16_t *q, int T)
{
    const int Tn = dsv1_resample_taps(S, D, filter);
    if (Tn < 0 || T != Tn || !start || !q) return DSVG_ERR_ARG;
    resample_table(S, D, filter, start, q, T);
    return DSVG_OK;
}

/* every axis of every plane within the ratio limits (taps: dsv1_scale_taps, downscale only, or dsv1_resample_taps): DSVG_OK or
 * DSVG_ERR_ARG */
static int dims_ok(int (*taps)(int, int, int), int sw, int sh, int fmt, int dw, int dh, int filter)
{
    const int hs = (fmt >> 2) & 3, vs = fmt & 3;
    if (fmt != DSV_SUBSAMP_444 && fmt != DSV_SUBSAMP_422 && fmt != DSV_SUBSAMP_420 && fmt != DSV_SUBSAMP_411) return DSVG_ERR_ARG;
    if (taps(sw, dw, filter) < 0 || taps(sh, dh, filter) < 0) return DSVG_ERR_ARG;
    if (taps((sw + (1 << hs) - 1) >> hs, (dw + (1 << hs) - 1) >> hs, filter) < 0) return DSVG_ERR_ARG;
    if (taps((sh + (1 << vs) - 1) >> vs, (dh + (1 << vs) - 1) >> vs, filter) < 0) return DSVG_ERR_ARG;
    return DSVG_OK;
}
static int scale_dims_ok(int sw, int sh, int fmt, int dw, int dh, int filter) { return dims_ok(dsv1_scale_taps, sw, sh, fmt, dw, dh, filter); }
static int resample_dims_ok(int sw, int sh, int fmt, int dw, int dh, int filter) { return dims_ok(dsv1_resample_taps, sw, sh, fmt, dw, dh, filter); }

/* the standalone clip call of both directions (the scaler's tables are dsv1_resample_weights, which are dsv1_scale_weights where
 * S >= D); the caller has checked the dims against its own limits */
static int resample_clip_impl(int device, const void *src, int sw, int sh, int subsamp, int n, void *dst, int dw, int dh, int filter,
                              int on_device)
{
    dsvg_scaler *sc = NULL;
    const dsv1_clip_io io = {{src, NULL}, {dsv1_frame_bytes(sw, sh, subsamp) * (size_t)n, 0}, {dst, NULL}, {dsv1_frame_bytes(dw, dh, subsamp) * (size_t)n, 0}};
    int rc;
    if ((rc = dsvg_scaler_create(&sc, device, sw, sh, subsamp, 1, &dw, &dh, filter))) return rc;
    rc = dsv1_pass_clip(device, DSV1_SRC_SCALE, sc, n, &io, on_device);
    dsvg_scaler_destroy(sc);
    return rc;
}

int dsv1_scale_clip(int device, const void *src, int sw, int sh, int subsamp, int n, void *dst, int dw, int dh, int filter, int on_device)
{
    int rc;
    if (!src || !dst || n < 1 || device < 0 || sw < 1 || sh < 1) return DSVG_ERR_ARG;
    if ((rc = scale_dims_ok(sw, sh, subsamp, dw, dh, filter))) return rc;
    return resample_clip_impl(device, src, sw, sh, subsamp, n, dst, dw, dh, filter, on_device);
}

int dsv1_resample_clip(int device, const void *src, int sw, int sh, int subsamp, int n, void *dst, int dw, int dh, int filter, int on_device)
{
    int rc;
    if (!src || !dst || n < 1 || device < 0 || sw < 1 || sh < 1) return DSVG_ERR_ARG;
    if ((rc = resample_dims_ok(sw, sh, subsamp, dw, dh, filter))) return rc;
    return resample_clip_impl(device, src, sw, sh, subsamp, n, dst, dw, dh, filter, on_device);
}

/* ---- resolution ladders ------------------------------------------------------------------------------------------------- */
struct dsv1_resladder {
    int ngeom, nsrc, F, ntot;
    int w[DSV1_MAX_GEOMS], h[DSV1_MAX_GEOMS], nr[DSV1_MAX_GEOMS], off[DSV1_MAX_GEOMS + 1];
    int same[DSV1_MAX_GEOMS];           /* geometry of the source's size: fed the source itself, no scale */
    size_t gfb[DSV1_MAX_GEOMS];
    dsv1_batch *lad[DSV1_MAX_GEOMS];
    dsvg_scaler *sc;
    int scale_idx[DSV1_MAX_GEOMS];      /* the scaler's table of geometry g (-1: same size) */
    void *clip[DSV1_MAX_GEOMS][2];      /* scaled clips, per call parity */
    int parity, pending[2];
    DSV_BUF *tmp;                       /* [max nsrc * nrates]: a geometry's view of the caller's output buffers */
    uint64_t up_bytes;
    long up_calls;
    /* the figures of the call collected last, per kind (DSVG_Q_*), gathered from the geometries' ladders.  `on` is kept for the two
     * source-resolution kinds only (dsv1_resladder_src_quality_enable: every geometry's ladder measures against the source clip, which
     * submit must hold for them); the switches of the rungs' own two live in the ladders alone, and their `on` here stays 0 */
    dsv1_quality q[DSVG_Q_KINDS];
    int sw, sh;
    /* the lane everything in front of the ladders runs on (kept while the resladder lives: uploads, scales), and the passes in front
     * of the scales: the source pixel format (dsv1_resladder_open_src), dsv1_resladder_set_deinterlace, dsv1_resladder_set_denoise */
    dsv1_srcchain src;
};

void dsv1_resladder_close(dsv1_resladder *r)
{
    int g;
    if (!r) return;
    for (g = 0; g < r->ngeom; g++) dsv1_batch_close(r->lad[g]);
    if (r->src.lane) (void)dsvg_lane_sync(r->src.lane); /* (the scales read the tables) */
    dsvg_scaler_destroy(r->sc);
    dsv1_srcchain_close(&r->src);                       /* (and the scaled clips and upload buffers of its lane) */
    free(r->tmp);
    for (g = 0; g < DSVG_Q_KINDS; g++) free(r->q[g].v);
    free(r);
}

int dsv1_resladder_open(dsv1_resladder **out, const DSV_META *src, const dsv1_res_rung *rungs, int ngeoms, int device, int nsources,
                        int frames_per_call, int filter)
{
    return dsv1_resladder_open_src(out, src, NULL, rungs, ngeoms, device, nsources, frames_per_call, filter);
}

static int resladder_open_fmt(dsv1_resladder **out, const DSV_META *src, int orient, const dsv1_reframe *frm, const dsv1_pix_format *pf,
                              int src_subsamp, const dsv1_rgb_format *rf, const dsv1_hdr_tables *ht, int upsample, const dsv1_res_rung *rungs,
                              int ngeoms, int device, int nsources, int frames_per_call, int filter);

int dsv1_resladder_open_src(dsv1_resladder **out, const DSV_META *src, const dsv1_pix_format *pf, const dsv1_res_rung *rungs, int ngeoms,
                            int device, int nsources, int frames_per_call, int filter)
{
    return resladder_open_fmt(out, src, 0, NULL, pf, src ? src->subsamp : 0, NULL, NULL, 0, rungs, ngeoms, device, nsources, frames_per_call, filter);
}

/* sources at src_subsamp: the converter halves their chroma to src->subsamp on the way */
int dsv1_resladder_open_src_sub(dsv1_resladder **out, const DSV_META *src, const dsv1_pix_format *pf, int src_subsamp, const dsv1_res_rung *rungs,
                                int ngeoms, int device, int nsources, int frames_per_call, int filter)
{
    static const dsv1_pix_format planar8 = {DSV1_PIX_PLANAR, 8, 0, {0, 0, 0}, 0};
    if (!pf && src && src_subsamp != src->subsamp) pf = &planar8;
    return resladder_open_fmt(out, src, 0, NULL, pf, src_subsamp, NULL, NULL, 0, rungs, ngeoms, device, nsources, frames_per_call, filter);
}

/* RGB sources: the RGB import pass (k_rgb.hip) in the converter's place, everything else as dsv1_resladder_open_src */
int dsv1_resladder_open_rgb(dsv1_resladder **out, const DSV_META *src, const dsv1_rgb_format *rf, const dsv1_res_rung *rungs, int ngeoms,
                            int device, int nsources, int frames_per_call, int filter)
{
    if (out) *out = NULL;
    if (!rf) return DSVG_ERR_ARG;
    return resladder_open_fmt(out, src, 0, NULL, NULL, src ? src->subsamp : 0, rf, NULL, 0, rungs, ngeoms, device, nsources, frames_per_call, filter);
}

/* sources of geometry *src = the reframe's input, reframed behind the other passes: the CANVAS stands for the source from the scales on */
int dsv1_resladder_open_reframed(dsv1_resladder **out, const DSV_META *src, const dsv1_reframe *rf, const dsv1_pix_format *pf, int src_subsamp,
                                 const dsv1_rgb_format *rgb, const dsv1_res_rung *rungs, int ngeoms, int device, int nsources, int frames_per_call,
                                 int filter)
{
    return dsv1_resladder_open_oriented(out, src, DSV1_ORIENT_NONE, rf, pf, src_subsamp, rgb, rungs, ngeoms, device, nsources, frames_per_call, filter);
}

/* sources of the RAW geometry *src, oriented behind the other passes and in front of the reframe: the reframe's input is the oriented
 * geometry, and without a reframe the oriented picture stands for the source from the scales on */
int dsv1_resladder_open_oriented(dsv1_resladder **out, const DSV_META *src, int orient, const dsv1_reframe *rf, const dsv1_pix_format *pf,
                                 int src_subsamp, const dsv1_rgb_format *rgb, const dsv1_res_rung *rungs, int ngeoms, int device, int nsources,
                                 int frames_per_call, int filter)
{
    static const dsv1_pix_format planar8 = {DSV1_PIX_PLANAR, 8, 0, {0, 0, 0}, 0};
    int mw, mh;
    if (out) *out = NULL;
    if (!src || (pf && rgb)) return DSVG_ERR_ARG;
    if (!dsv1_orient_valid(orient, src->subsamp) || dsv1_orient_dims(orient, src->width, src->height, &mw, &mh)) {
        dsv1_log(1, "dsv1_resladder_open_oriented: %d is not an orientation of %dx%d sources of subsampling 0x%x", orient, src->width, src->height, src->subsamp);
        return DSVG_ERR_ARG;
    }
    if (rf && (!dsv1_reframe_valid(rf, src->subsamp) || rf->in_w != mw || rf->in_h != mh)) {
        dsv1_log(1, "dsv1_resladder_open: not a valid reframe of %dx%d pictures (the sources, oriented) of subsampling 0x%x", mw, mh, src->subsamp);
        return DSVG_ERR_ARG;
    }
    if (rgb) src_subsamp = src->subsamp;
    else if (!pf && src_subsamp != src->subsamp) pf = &planar8;
    return resladder_open_fmt(out, src, orient, rf, pf, src_subsamp, rgb, NULL, 0, rungs, ngeoms, device, nsources, frames_per_call, filter);
}

/* HDR sources: the HDR import pass (k_hdr.hip) of *pf at src_subsamp in the converter's place, everything else as dsv1_resladder_open_src_sub */
int dsv1_resladder_open_hdr(dsv1_resladder **out, const DSV_META *src, const dsv1_pix_format *pf, int src_subsamp, const dsv1_hdr_tables *tables,
                            int upsample, const dsv1_res_rung *rungs, int ngeoms, int device, int nsources, int frames_per_call, int filter)
{
    if (out) *out = NULL;
    if (!pf || !tables) return DSVG_ERR_ARG;
    return resladder_open_fmt(out, src, 0, NULL, pf, src_subsamp, NULL, tables, upsample, rungs, ngeoms, device, nsources, frames_per_call, filter);
}

/* ht: the tables of an HDR import of *pf (then the pixel format is never "the default") */
static int resladder_open_fmt(dsv1_resladder **out, const DSV_META *src, int orient, const dsv1_reframe *frm, const dsv1_pix_format *pf,
                              int src_subsamp, const dsv1_rgb_format *rf, const dsv1_hdr_tables *ht, int upsample, const dsv1_res_rung *rungs,
                              int ngeoms, int device, int nsources, int frames_per_call, int filter)
{
    /* cw x ch: what stands for the source behind the chain -- the reframe's canvas, or the source itself, oriented (the callers pass a
     * valid code); the passes in front of the orientation and the caller's clips are src->width x src->height */
    const int tr = orient & 4;
    const int cw = frm && src ? frm->out_w : src ? (tr ? src->height : src->width) : 0, ch = frm && src ? frm->out_h : src ? (tr ? src->width : src->height) : 0;
    dsv1_resladder *r;
    dsv1_pix_layout pl;
    dsv1_rgb_layout rl;
    dsv1_hdr_layout hl;
    dsv1_src_format fmt;
    int g, k, rc, ntot = 0, nscaled = 0, maxr = 0, dw[DSV1_MAX_GEOMS], dh[DSV1_MAX_GEOMS];
    if (out) *out = NULL;
    /* arguments first: nothing below touches a device until every geometry has passed */
    if (!out || !src || !rungs || ngeoms < 1 || ngeoms > DSV1_MAX_GEOMS || nsources < 1 || frames_per_call < 1) return DSVG_ERR_ARG;
    if (filter != DSV1_SCALE_TENT && filter != DSV1_SCALE_CUBIC) return DSVG_ERR_ARG;
    if (src->width < 1 || src->height < 1) return DSVG_ERR_ARG;
    if (ht && ((upsample != DSV1_CHROMA_REPLICATE && upsample != DSV1_CHROMA_LINEAR) || !dsv1_hdr_tables_valid(ht) ||
               dsv1_hdr_layout_of(pf, src->width, src->height, src_subsamp, src->subsamp, &hl))) {
        dsv1_log(1, "dsv1_resladder_open_hdr: not a valid HDR source for %dx%d sources of subsampling 0x%x into 0x%x", src->width, src->height,
                 src_subsamp, src->subsamp);
        return DSVG_ERR_ARG;
    }
    if (pf && dsv1_pix_layout_of(pf, src->width, src->height, src_subsamp, src->subsamp, &pl)) {
        dsv1_log(1, "dsv1_resladder_open_src: not a valid pixel format for %dx%d sources of subsampling 0x%x into 0x%x", src->width, src->height,
                 src_subsamp, src->subsamp);
        return DSVG_ERR_ARG;
    }
    if (pf && !ht && src_subsamp == src->subsamp && dsv1_pix_is_default(pf, src->width, src->height, src->subsamp)) pf = NULL;
    if (rf && dsv1_rgb_layout_of(rf, src->width, src->height, src->subsamp, &rl)) {
        dsv1_log(1, "dsv1_resladder_open_rgb: not a valid RGB format for %dx%d sources of subsampling 0x%x", src->width, src->height, src->subsamp);
        return DSVG_ERR_ARG;
    }
    for (g = 0; g < ngeoms; g++) {
        const dsv1_res_rung *G = &rungs[g];
        if (!G->rates || G->nrates < 1 || G->nrates > DSV1_MAX_RUNGS) {
            dsv1_log(1, "dsv1_resladder_open: geometry %d needs 1 to %d rate rungs", g, DSV1_MAX_RUNGS);
            return DSVG_ERR_ARG;
        }
        if (scale_dims_ok(cw, ch, src->subsamp, G->width, G->height, filter)) {
            dsv1_log(1, "dsv1_resladder_open: geometry %d (%dx%d) is not a downscale of %dx%d by at most 8 on every axis and plane", g, G->width,
                     G->height, cw, ch);
            return DSVG_ERR_ARG;
        }
        for (k = 0; k < G->nrates; k++) {
            const DSV_META *m = &G->rates[k].vidmeta;
            if (m->width != G->width || m->height != G->height || m->subsamp != src->subsamp) {
                dsv1_log(1, "dsv1_resladder_open: rate rung %d of geometry %d is not %dx%d in the source's format", k, g, G->width, G->height);
                return DSVG_ERR_ARG;
            }
            if (k && !dsv1_ladder_rungs_agree(&G->rates[0], &G->rates[k])) {
                dsv1_log(1, "dsv1_resladder_open: rate rung %d of geometry %d differs from its rung 0 in a field the analysis reads", k, g);
                return DSVG_ERR_ARG;
            }
        }
        ntot += G->nrates;
        if (G->nrates > maxr) maxr = G->nrates;
    }
    if (nsources > INT_MAX / ntot / frames_per_call / 3) return DSVG_ERR_ARG;
    for (g = 0; g < ngeoms; g++)
        if ((rc = dsvg_geom_check(rungs[g].width, rungs[g].height, src->subsamp))) {
            dsv1_log(1, "dsv1_resladder_open: geometry %d (%dx%d) is one the encoder does not take", g, rungs[g].width, rungs[g].height);
            return rc;
        }
    r = (dsv1_resladder *)calloc(1, sizeof(*r));
    if (!r) return DSVG_ERR_NOMEM;
    r->ngeom = ngeoms; r->nsrc = nsources; r->F = frames_per_call; r->ntot = ntot;
    r->sw = cw; r->sh = ch;
    dsv1_srcchain_init(&r->src, device, cw, ch, src->subsamp, nsources, frames_per_call, 1);
    r->tmp = (DSV_BUF *)calloc((size_t)nsources * maxr, sizeof(DSV_BUF));
    r->q[DSVG_Q_SSE].v = (uint64_t *)calloc((size_t)3 * nsources * ntot * frames_per_call, sizeof(uint64_t));
    r->q[DSVG_Q_SSIM].v = (uint64_t *)calloc((size_t)3 * nsources * ntot * frames_per_call, sizeof(uint64_t));
    if (!r->tmp || !r->q[DSVG_Q_SSE].v || !r->q[DSVG_Q_SSIM].v) { dsv1_resladder_close(r); return DSVG_ERR_NOMEM; }
    for (g = 0; g < ngeoms; g++) {
        r->w[g] = rungs[g].width; r->h[g] = rungs[g].height; r->nr[g] = rungs[g].nrates;
        r->off[g + 1] = r->off[g] + rungs[g].nrates;
        r->gfb[g] = dsv1_frame_bytes(r->w[g], r->h[g], src->subsamp);
        r->same[g] = r->w[g] == cw && r->h[g] == ch;
        r->scale_idx[g] = -1;
        if (!r->same[g]) { r->scale_idx[g] = nscaled; dw[nscaled] = r->w[g]; dh[nscaled] = r->h[g]; nscaled++; }
    }
    /* the lane exists even when no geometry is scaled: host input is uploaded through it */
    fmt.pf = pf; fmt.src_subsamp = src_subsamp; fmt.rgb = rf; fmt.hdr = ht; fmt.upsample = upsample;
    if ((rc = dsvg_scaler_create(&r->sc, device, cw, ch, src->subsamp, nscaled, dw, dh, filter)) ||
        (rc = dsv1_srcchain_lane(&r->src)) || (rc = dsv1_srcchain_request(&r->src, "dsv1_resladder_open", 0, DSV1_SRC_REFRAME, frm)) ||
        (rc = dsv1_srcchain_request(&r->src, "dsv1_resladder_open", 0, DSV1_SRC_ORIENT, &orient)) ||
        (rc = dsv1_srcchain_request(&r->src, "dsv1_resladder_open", 0, DSV1_SRC_CONVERT, &fmt))) { dsv1_resladder_close(r); return rc; }
    for (g = 0; g < ngeoms; g++) {
        if ((rc = dsv1_ladder_open(&r->lad[g], rungs[g].rates, rungs[g].nrates, device, nsources, frames_per_call))) break;
        r->ngeom = g + 1;
        if (!r->same[g])
            for (k = 0; k < 2 && !rc; k++) rc = dsvg_lane_alloc(r->src.lane, &r->clip[g][k], r->gfb[g] * (size_t)nsources * frames_per_call);
        if (rc) break;
    }
    if (rc) { r->ngeom = g + (g < ngeoms && r->lad[g] ? 1 : 0); dsv1_resladder_close(r); return rc; }
    *out = r;
    return DSVG_OK;
}

int dsv1_resladder_nstreams(const dsv1_resladder *r) { return r ? r->nsrc * r->ntot : DSVG_ERR_ARG; }
dsv1_batch *dsv1_resladder_batch(dsv1_resladder *r, int g) { return r && g >= 0 && g < r->ngeom ? r->lad[g] : NULL; }

/* output stream k -> (geometry, that ladder's stream) */
static int res_split(const dsv1_resladder *r, int k, int *kg)
{
    int s, o, g;
    if (!r || k < 0 || k >= r->nsrc * r->ntot) return -1;
    s = k / r->ntot; o = k % r->ntot;
    for (g = 0; o >= r->off[g + 1]; g++) ;
    *kg = s * r->nr[g] + (o - r->off[g]);
    return g;
}

DSV_ENCODER *dsv1_resladder_encoder(dsv1_resladder *r, int k)
{
    int kg, g = res_split(r, k, &kg);
    return g < 0 ? NULL : dsv1_batch_encoder(r->lad[g], kg);
}

int dsv1_resladder_eos(dsv1_resladder *r, int k, DSV_BUF *out)
{
    int kg, g = res_split(r, k, &kg);
    if (g < 0 || !out) return DSVG_ERR_ARG;
    return dsv1_batch_eos(r->lad[g], kg, out);
}

/* geometry g's view of the caller's buffers (out[s * Ntot + off[g] + rate]) into r->tmp, and back */
static void view_in(dsv1_resladder *r, int g, DSV_BUF *out)
{
    int s, q;
    for (s = 0; s < r->nsrc; s++)
        for (q = 0; q < r->nr[g]; q++) r->tmp[s * r->nr[g] + q] = out[s * r->ntot + r->off[g] + q];
}
static void view_out(dsv1_resladder *r, int g, DSV_BUF *out)
{
    int s, q;
    for (s = 0; s < r->nsrc; s++)
        for (q = 0; q < r->nr[g]; q++) out[s * r->ntot + r->off[g] + q] = r->tmp[s * r->nr[g] + q];
}

int dsv1_resladder_submit(dsv1_resladder *r, const void *yuv, int yuv_on_device, DSV_BUF *out)
{
    const void *dsrc;
    const int plain_dev = yuv_on_device == 1;
    int g, rc, par;
    if (!r || !yuv || !out || yuv_on_device < 0 || yuv_on_device > DSV1_CLIP_HELD) return DSVG_ERR_ARG;
    par = r->parity;
    if (r->pending[par]) { dsv1_log(1, "resolution ladder submitted twice without collect"); return DSVG_ERR_ARG; }
    if (plain_dev && (r->q[DSVG_Q_XSSE].on || r->q[DSVG_Q_XSSIM].on) && !dsv1_srcchain_any(&r->src)) {
        /* the source-resolution figures read the source until collect, and a plain device clip is the caller's again when submit
         * returns: a device-to-device copy into the buffer of the call's parity, which from here on stands for the clip */
        void *d;
        if ((rc = dsvg_lane_copy_in(r->src.lane, par, yuv, r->src.g.bytes_in, &d))) return rc;
        dsrc = d;
    } else {
        /* the RAW clip crosses the link once (host input), into the lane's buffer of this call's parity, which is held until this
         * call's collect (a geometry of the source's size reads it in place); the chain's passes write clips of this call's parity,
         * and what they leave stands for the source from here on */
        if ((rc = dsv1_srcchain_run(&r->src, par, yuv, yuv_on_device, &dsrc))) return rc;
        if (!yuv_on_device) { r->up_bytes += r->src.g.bytes_in; r->up_calls++; }
    }
    if (dsrc == yuv && plain_dev && (r->q[DSVG_Q_XSSE].on || r->q[DSVG_Q_XSSIM].on)) {
        /* (overlays alone and none active in this call: the clip came back as it went in; the figures read it until collect) */
        void *d;
        if ((rc = dsvg_lane_copy_in(r->src.lane, par, yuv, r->src.g.bytes_in, &d))) return rc;
        dsrc = d;
    }
    /* the resladder's own memory is held until collect (a plain device clip: the sync at the end waits for whatever read it) */
    if (dsrc != yuv) yuv_on_device = DSV1_CLIP_HELD;
    for (g = 0; g < r->ngeom; g++) {
        const void *clip = dsrc;
        int form = yuv_on_device;
        if ((r->q[DSVG_Q_XSSE].on || r->q[DSVG_Q_XSSIM].on) && (rc = dsv1_batch_xres_source(r->lad[g], dsrc))) return rc;
        if (!r->same[g]) {
            if ((rc = dsvg_scaler_run(r->sc, dsvg_lane_stream(r->src.lane), r->scale_idx[g], dsrc, r->nsrc * r->F, r->clip[g][par]))) return rc;
            clip = r->clip[g][par];
            form = DSV1_CLIP_HELD;
        }
        if ((rc = dsvg_lane_order(r->src.lane, (dsvg_ctx *)dsv1_batch_ctx(r->lad[g])))) return rc;
        view_in(r, g, out);
        rc = dsv1_batch_submit(r->lad[g], clip, form, r->tmp);
        view_out(r, g, out);
        if (rc) return rc;
    }
    /* a plain device clip is the caller's again when submit returns: the passes, scales or the copy that read it must have run */
    if (plain_dev && (rc = dsvg_lane_sync(r->src.lane))) return rc;
    r->pending[par] = 1;
    r->parity ^= 1;
    return DSVG_OK;
}

/* ---- the source side between calls: the chain's one request path (dsv1_srcchain_request), as a batch's setters; busy: calls in
 * flight.  What the chain leaves stands for the source everywhere behind it: the scales read it, and so do the source-resolution
 * figures. ---- */
#define RES_BUSY(r) ((r)->pending[0] || (r)->pending[1])
int dsv1_resladder_set_deinterlace(dsv1_resladder *r, const dsv1_deint *di)
{
    return r ? dsv1_srcchain_request(&r->src, "dsv1_resladder_set_deinterlace", RES_BUSY(r), DSV1_SRC_DEINTERLACE, di) : DSVG_ERR_ARG;
}
int dsv1_resladder_set_ivtc(dsv1_resladder *r, const dsv1_ivtc *iv)
{
    return r ? dsv1_srcchain_request(&r->src, "dsv1_resladder_set_ivtc", RES_BUSY(r), DSV1_SRC_IVTC, iv) : DSVG_ERR_ARG;
}
int dsv1_resladder_set_levels(dsv1_resladder *r, const dsv1_levels *lv)
{
    return r ? dsv1_srcchain_request(&r->src, "dsv1_resladder_set_levels", RES_BUSY(r), DSV1_SRC_LEVELS, lv) : DSVG_ERR_ARG;
}
int dsv1_resladder_set_denoise(dsv1_resladder *r, const dsv1_denoise *dn)
{
    return r ? dsv1_srcchain_request(&r->src, "dsv1_resladder_set_denoise", RES_BUSY(r), DSV1_SRC_DENOISE, dn) : DSVG_ERR_ARG;
}
int dsv1_resladder_set_overlays(dsv1_resladder *r, const dsv1_overlay *list, int n)
{
    dsv1_src_overlays o = {list, n};
    return r ? dsv1_srcchain_request(&r->src, "dsv1_resladder_set_overlays", RES_BUSY(r), DSV1_SRC_OVERLAY, &o) : DSVG_ERR_ARG;
}
int dsv1_resladder_deinterlace_reset(dsv1_resladder *r, int source)
{
    return r ? dsv1_srcchain_signal(&r->src, "dsv1_resladder_deinterlace_reset", RES_BUSY(r), DSV1_SC_OP_RESET, DSV1_SRC_DEINTERLACE, source, 0) : DSVG_ERR_ARG;
}
int dsv1_resladder_ivtc_reset(dsv1_resladder *r, int source)
{
    return r ? dsv1_srcchain_signal(&r->src, "dsv1_resladder_ivtc_reset", RES_BUSY(r), DSV1_SC_OP_RESET, DSV1_SRC_IVTC, source, 0) : DSVG_ERR_ARG;
}
int dsv1_resladder_denoise_reset(dsv1_resladder *r, int source)
{
    return r ? dsv1_srcchain_signal(&r->src, "dsv1_resladder_denoise_reset", RES_BUSY(r), DSV1_SC_OP_RESET, DSV1_SRC_DENOISE, source, 0) : DSVG_ERR_ARG;
}
int dsv1_resladder_overlay_seek(dsv1_resladder *r, int source, int64_t t)
{
    return r ? dsv1_srcchain_signal(&r->src, "dsv1_resladder_overlay_seek", 0, DSV1_SC_OP_SEEK, DSV1_SRC_OVERLAY, source, t) : DSVG_ERR_ARG;
}
int dsv1_resladder_source_input(const dsv1_resladder *r, int in[3], size_t *frame_bytes)
{
    if (!r || !in || !frame_bytes) return DSVG_ERR_ARG;
    in[0] = r->src.g.frames_in; in[1] = r->src.g.w; in[2] = r->src.g.h;
    *frame_bytes = r->src.g.frame_in_bytes;
    return DSVG_OK;
}

int dsv1_resladder_collect(dsv1_resladder *r, DSV_BUF *out)
{
    int g, par, s, q, k, rc, have[DSVG_Q_KINDS];
    if (!r || !out) return DSVG_ERR_ARG;
    par = r->pending[r->parity] ? r->parity : (r->parity ^ 1);      /* oldest first */
    if (!r->pending[par]) { dsv1_log(1, "nothing to collect"); return DSVG_ERR_ARG; }
    r->pending[par] = 0;
    for (k = 0; k < DSVG_Q_KINDS; k++) { r->q[k].n = 0; have[k] = r->q[k].v != NULL; }
    for (g = 0; g < r->ngeom; g++) {
        const size_t per = (size_t)3 * r->F;
        view_in(r, g, out);
        rc = dsv1_batch_collect(r->lad[g], r->tmp);
        view_out(r, g, out);
        if (rc) return rc;
        /* the geometry's figures [s * nr + q][t][p] go to [s * Ntot + off + q][t][p], straight from its ladder's record; a kind is
         * present only if every geometry delivered it (a ladder measured ... or not) */
        for (k = 0; k < DSVG_Q_KINDS; k++) {
            const dsv1_quality *from = dsv1_batch_quality(r->lad[g], k);
            if (!from || !from->n || from->n > (size_t)r->nsrc * r->nr[g] * per) have[k] = 0;
            if (!have[k]) continue;
            for (s = 0; s < r->nsrc; s++)
                for (q = 0; q < r->nr[g]; q++)
                    memcpy(r->q[k].v + (size_t)(s * r->ntot + r->off[g] + q) * per, from->v + (size_t)(s * r->nr[g] + q) * per, sizeof(uint64_t) * per);
        }
    }
    for (k = 0; k < DSVG_Q_KINDS; k++) if (have[k]) r->q[k].n = (size_t)3 * r->nsrc * r->ntot * r->F;
    return DSVG_OK;
}

int dsv1_resladder_encode(dsv1_resladder *r, const void *yuv, int yuv_on_device, DSV_BUF *out)
{
    int rc;
    if (!r || !out) return DSVG_ERR_ARG;
    if (r->pending[0] || r->pending[1]) { dsv1_log(1, "dsv1_resladder_encode with calls in flight"); return DSVG_ERR_ARG; }
    if ((rc = dsv1_resladder_submit(r, yuv, yuv_on_device, out))) return rc;
    return dsv1_resladder_collect(r, out);
}

int dsv1_resladder_sse_enable(dsv1_resladder *r, int on)
{
    int g, rc;
    if (!r) return DSVG_ERR_ARG;
    for (g = 0; g < r->ngeom; g++)
        if ((rc = dsv1_batch_sse_enable(r->lad[g], on))) return rc;
    return DSVG_OK;
}
int dsv1_resladder_ssim_enable(dsv1_resladder *r, int on)
{
    int g, rc;
    if (!r) return DSVG_ERR_ARG;
    for (g = 0; g < r->ngeom; g++)
        if ((rc = dsv1_batch_ssim_enable(r->lad[g], on))) return rc;
    return DSVG_OK;
}
static int resladder_get(const dsv1_resladder *r, int kind, const char *fn, void *out, size_t n)
{
    if (!r || !out || !r->q[kind].n || n < r->q[kind].n) { dsv1_log(1, "%s: nothing measured, or no room", fn); return DSVG_ERR_ARG; }
    memcpy(out, r->q[kind].v, sizeof(uint64_t) * r->q[kind].n);
    return DSVG_OK;
}
int dsv1_resladder_get_sse(const dsv1_resladder *r, uint64_t *sse, size_t n) { return resladder_get(r, DSVG_Q_SSE, "dsv1_resladder_get_sse", sse, n); }
int dsv1_resladder_get_ssim(const dsv1_resladder *r, int64_t *ssim_fx, size_t n) { return resladder_get(r, DSVG_Q_SSIM, "dsv1_resladder_get_ssim", ssim_fx, n); }
int dsv1_resladder_get_src_sse(const dsv1_resladder *r, uint64_t *sse, size_t n) { return resladder_get(r, DSVG_Q_XSSE, "dsv1_resladder_get_src_sse", sse, n); }
int dsv1_resladder_get_src_ssim(const dsv1_resladder *r, int64_t *ssim_fx, size_t n) { return resladder_get(r, DSVG_Q_XSSIM, "dsv1_resladder_get_src_ssim", ssim_fx, n); }
/* every geometry's ladder measures its pictures upscaled to the source's dims against the source clip (dsv1_batch_xres_*) */
int dsv1_resladder_src_quality_enable(dsv1_resladder *r, int sse_on, int ssim_on, int filter)
{
    int g, rc;
    const size_t n = r ? (size_t)3 * r->nsrc * r->ntot * r->F : 0;
    if (!r) return DSVG_ERR_ARG;
    if (r->pending[0] || r->pending[1]) { dsv1_log(1, "dsv1_resladder_src_quality_enable with calls in flight"); return DSVG_ERR_ARG; }
    if (filter != DSV1_SCALE_TENT && filter != DSV1_SCALE_CUBIC) { dsv1_log(1, "dsv1_resladder_src_quality_enable: bad filter %d", filter); return DSVG_ERR_ARG; }
    if (sse_on && !r->q[DSVG_Q_XSSE].v && !(r->q[DSVG_Q_XSSE].v = (uint64_t *)calloc(n, sizeof(uint64_t)))) return DSVG_ERR_NOMEM;
    if (ssim_on && !r->q[DSVG_Q_XSSIM].v && !(r->q[DSVG_Q_XSSIM].v = (uint64_t *)calloc(n, sizeof(uint64_t)))) return DSVG_ERR_NOMEM;
    for (g = 0; g < r->ngeom; g++)
        if ((rc = dsv1_batch_xres_enable(r->lad[g], sse_on, ssim_on, r->sw, r->sh, filter))) return rc;
    r->q[DSVG_Q_XSSE].on = sse_on != 0;
    r->q[DSVG_Q_XSSIM].on = ssim_on != 0;
    return DSVG_OK;
}
int dsv1_resladder_uploads(const dsv1_resladder *r, uint64_t *bytes, long *calls)
{
    if (!r) return DSVG_ERR_ARG;
    if (bytes) *bytes = r->up_bytes;
    if (calls) *calls = r->up_calls;
    return DSVG_OK;
}
