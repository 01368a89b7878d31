/* dsv1_levels.c -- levels and histograms (include/dsv1_api.h, Levels): the host-only table builders, the range and point rules on a
 * histogram, and the standalone calls.  The definitions are stated in numpy in tests/_levels.py; the kernels and their device
 * plumbing: k_levels.hip; the sessions: dsv1_srcchain.c, dsv1_enc.c, dsv1_scale.c.
 * Everything here is exact integer arithmetic: r(a / b) = floor((2 a + b) / (2 b)), b > 0, with a true floor for negative a. */
#include "dsv1_host.h"

static int subsamp_known(int subsamp)
{
    return subsamp == DSV_SUBSAMP_444 || subsamp == DSV_SUBSAMP_422 || subsamp == DSV_SUBSAMP_420 || subsamp == DSV_SUBSAMP_411;
}

static int rdiv(int a, int b)
{
    const int n = 2 * a + b, d = 2 * b;
    return n >= 0 ? n / d : -((-n + d - 1) / d);
}
static uint8_t clamp8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

int dsv1_levels_identity(dsv1_levels *lv)
{
    int p, v;
    if (!lv) return DSVG_ERR_ARG;
    for (p = 0; p < 3; p++)
        for (v = 0; v < 256; v++) lv->lut[p][v] = (uint8_t)v;
    return DSVG_OK;
}

int dsv1_levels_is_identity(const dsv1_levels *lv)
{
    int p, v;
    if (!lv) return 0;
    for (p = 0; p < 3; p++)
        for (v = 0; v < 256; v++)
            if (lv->lut[p][v] != v) return 0;
    return 1;
}

int dsv1_levels_range(dsv1_levels *lv, int src_full, int dst_full)
{
    int p, v;
    if (!lv || src_full < 0 || src_full > 1 || dst_full < 0 || dst_full > 1) return DSVG_ERR_ARG;
    if (src_full == dst_full) return dsv1_levels_identity(lv);
    for (v = 0; v < 256; v++) {
        uint8_t y, c;
        if (src_full) { y = (uint8_t)(16 + rdiv(v * 219, 255)); c = (uint8_t)(128 + rdiv((v - 128) * 224, 255)); }
        else { y = clamp8(rdiv((v - 16) * 255, 219)); c = clamp8(128 + rdiv((v - 128) * 255, 224)); }
        lv->lut[0][v] = y;
        for (p = 1; p < 3; p++) lv->lut[p][v] = c;
    }
    return DSVG_OK;
}

int dsv1_levels_adjust(dsv1_levels *lv, int in_black, int in_white, int out_black, int out_white, int sat_q8)
{
    int v;
    if (!lv || in_black < 0 || in_black >= in_white || in_white > 255 || out_black < 0 || out_black > out_white || out_white > 255 ||
        sat_q8 < 0 || sat_q8 > 1024) return DSVG_ERR_ARG;
    for (v = 0; v < 256; v++) {
        lv->lut[0][v] = (uint8_t)(v <= in_black ? out_black : v >= in_white ? out_white :
                                  out_black + rdiv((v - in_black) * (out_white - out_black), in_white - in_black));
        lv->lut[1][v] = lv->lut[2][v] = clamp8(128 + rdiv((v - 128) * sat_q8, 256));
    }
    return DSVG_OK;
}

int dsv1_levels_compose(const dsv1_levels *a, const dsv1_levels *b, dsv1_levels *out)
{
    dsv1_levels t;
    int p, v;
    if (!a || !b || !out) return DSVG_ERR_ARG;
    for (p = 0; p < 3; p++)
        for (v = 0; v < 256; v++) t.lut[p][v] = b->lut[p][a->lut[p][v]];
    *out = t;                                           /* (out may be a or b) */
    return DSVG_OK;
}

int dsv1_range_from_histogram(const uint32_t *hist, int n, int ppm, int *full)
{
    uint64_t outside = 0, total = 0;
    int t, p, v;
    if (!hist || !full || n < 1 || ppm < 0 || ppm > 1000000) return DSVG_ERR_ARG;
    for (t = 0; t < n; t++)
        for (p = 0; p < 3; p++) {
            const uint32_t *h = hist + ((size_t)t * 3 + p) * 256;
            const int top = p ? 240 : 235;
            for (v = 0; v < 256; v++) {
                total += h[v];
                if (v < 16 || v > top) outside += h[v];
            }
        }
    /* (a clip of 2^44 samples and more would overflow the product; no clip the library takes comes near) */
    *full = outside * 1000000u > (uint64_t)ppm * total;
    return DSVG_OK;
}

int dsv1_points_from_histogram(const uint32_t *hist, int n, int low_ppm, int high_ppm, int *black, int *white)
{
    uint64_t y[256], total = 0, below, above;
    int t, v, b, w;
    if (black) *black = 0;
    if (white) *white = 0;
    if (!hist || !black || !white || n < 1 || low_ppm < 0 || low_ppm > 1000000 || high_ppm < 0 || high_ppm > 1000000) return DSVG_ERR_ARG;
    memset(y, 0, sizeof(y));
    for (t = 0; t < n; t++)
        for (v = 0; v < 256; v++) { y[v] += hist[(size_t)t * 768 + v]; total += hist[(size_t)t * 768 + v]; }
    /* count(Y < b) grows with b: the largest b that still passes (b = 0 always does) */
    for (b = 0, below = 0; b < 255 && (below + y[b]) * 1000000u <= (uint64_t)low_ppm * total; b++) below += y[b];
    /* count(Y > w) shrinks as w grows: the smallest w that passes (w = 255 always does) */
    for (w = 255, above = 0; w > 0 && (above + y[w]) * 1000000u <= (uint64_t)high_ppm * total; w--) above += y[w];
    if (b >= w) return 0;
    *black = b; *white = w;
    return 1;
}

int dsv1_levels_clip(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsv1_levels *lv, int on_device)
{
    dsvg_levels *l = NULL;
    size_t bytes;
    int rc;
    if (!src || !dst || !lv || n < 1 || device < 0 || w < 1 || h < 1 || !subsamp_known(subsamp)) return DSVG_ERR_ARG;
    bytes = dsv1_frame_bytes(w, h, subsamp) * (size_t)n;
    if ((rc = dsvg_levels_create(&l, device, lv, w, h, subsamp))) return rc;
    {
        const dsv1_clip_io io = {{src, NULL}, {bytes, 0}, {dst, NULL}, {bytes, 0}};
        rc = dsv1_pass_clip(device, DSV1_SRC_LEVELS, l, n, &io, on_device);
    }
    dsvg_levels_destroy(l);
    return rc;
}

int dsv1_histogram_clip(int device, const void *src, int w, int h, int subsamp, int n, uint32_t *hist, int on_device)
{
    dsvg_histogram *g = NULL;
    dsvg_lane *l = NULL;
    void *d, *dh = NULL;
    size_t hb;
    int rc;
    if (!src || !hist || n < 1 || device < 0 || w < 1 || h < 1 || !subsamp_known(subsamp)) return DSVG_ERR_ARG;
    hb = sizeof(uint32_t) * 768 * (size_t)n;
    if ((rc = dsvg_histogram_create(&g, device, w, h, subsamp))) return rc;
    if (!(rc = dsvg_lane_create(&l, device))) {
        if (!on_device && !(rc = dsvg_lane_upload(l, 0, src, dsv1_frame_bytes(w, h, subsamp) * (size_t)n, &d))) src = d;
        if (!rc) rc = dsvg_lane_alloc(l, &dh, hb);
        if (!rc) rc = dsvg_histogram_run(g, dsvg_lane_stream(l), src, n, dh);
        if (!rc) rc = dsvg_lane_download(l, hist, dh, hb);
        if (!rc) rc = dsvg_lane_sync(l);
        dsvg_lane_destroy(l);                           /* (waits for the stream; frees what the call allocated) */
    }
    dsvg_histogram_destroy(g);
    return rc;
}

int dsv1_detect_range_clip(int device, const void *src, int w, int h, int subsamp, int n, int ppm, int *full, int on_device)
{
    uint32_t *hist;
    int rc;
    if (!src || !full || n < 1 || device < 0 || w < 1 || h < 1 || !subsamp_known(subsamp) || ppm < 0 || ppm > 1000000) return DSVG_ERR_ARG;
    if ((size_t)n > SIZE_MAX / (sizeof(uint32_t) * 768)) return DSVG_ERR_ARG;
    hist = (uint32_t *)malloc(sizeof(uint32_t) * 768 * (size_t)n);
    if (!hist) return DSVG_ERR_NOMEM;
    rc = dsv1_histogram_clip(device, src, w, h, subsamp, n, hist, on_device);
    if (!rc) rc = dsv1_range_from_histogram(hist, n, ppm, full);
    free(hist);
    return rc;
}
