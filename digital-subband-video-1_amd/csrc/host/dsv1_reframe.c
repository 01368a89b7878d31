/* dsv1_reframe.c -- reframe and bar detection (include/dsv1_api.h, Reframe): validation, the bars rule and the standalone calls.  The
 * definitions are stated in numpy in tests/_reframe.py; the kernels and their device plumbing: k_reframe.hip; the sessions:
 * dsv1_srcchain.c, dsv1_enc.c, dsv1_scale.c. */
#include "dsv1_host.h"

static int subsamp_known(int subsamp)
{
    return subsamp == DSV_SUBSAMP_444 || subsamp == DSV_SUBSAMP_422 || subsamp == DSV_SUBSAMP_420 || subsamp == DSV_SUBSAMP_411;
}

int dsv1_reframe_valid(const dsv1_reframe *rf, int subsamp)
{
    int mx, my;
    if (!rf || !subsamp_known(subsamp) || rf->reserved) return 0;
    mx = (1 << ((subsamp >> 2) & 3)) - 1; my = (1 << (subsamp & 3)) - 1;
    if (rf->in_w < 1 || rf->in_h < 1 || rf->w < 1 || rf->h < 1 || rf->out_w < 1 || rf->out_h < 1) return 0;
    /* (written so that no sum overflows: every term is at least 0 and at most its bound when it is compared) */
    if (rf->x < 0 || rf->x > rf->in_w || rf->w > rf->in_w - rf->x || rf->y < 0 || rf->y > rf->in_h || rf->h > rf->in_h - rf->y) return 0;
    if (rf->dst_x < 0 || rf->dst_x > rf->out_w || rf->w > rf->out_w - rf->dst_x) return 0;
    if (rf->dst_y < 0 || rf->dst_y > rf->out_h || rf->h > rf->out_h - rf->dst_y) return 0;
    if ((rf->x & mx) || (rf->dst_x & mx) || (rf->y & my) || (rf->dst_y & my)) return 0;
    return 1;
}

int dsv1_reframe_is_identity(const dsv1_reframe *rf)
{
    return rf->x == 0 && rf->y == 0 && rf->dst_x == 0 && rf->dst_y == 0 && rf->w == rf->in_w && rf->h == rf->in_h && rf->out_w == rf->in_w &&
           rf->out_h == rf->in_h;
}

int dsv1_reframe_clip(int device, const void *src, int n, void *dst, const dsv1_reframe *rf, int subsamp, int on_device)
{
    dsvg_reframe *r = NULL;
    int rc;
    if (!src || !dst || n < 1 || device < 0 || !dsv1_reframe_valid(rf, subsamp)) return DSVG_ERR_ARG;
    if ((rc = dsvg_reframe_create(&r, device, rf, subsamp))) return rc;
    {
        const dsv1_clip_io io = {{src, NULL}, {dsv1_frame_bytes(rf->in_w, rf->in_h, subsamp) * (size_t)n, 0}, {dst, NULL},
                                 {dsv1_frame_bytes(rf->out_w, rf->out_h, subsamp) * (size_t)n, 0}};
        rc = dsv1_pass_clip(device, DSV1_SRC_REFRAME, r, n, &io, on_device);
    }
    dsvg_reframe_destroy(r);
    return rc;
}

int dsv1_line_sums_clip(int device, const void *src, int w, int h, int subsamp, int n, uint32_t *row_sum, uint32_t *col_sum, int on_device)
{
    dsvg_linesums *s = NULL;
    dsvg_lane *l = NULL;
    void *d, *drow = NULL, *dcol = NULL;
    const size_t rb = sizeof(uint32_t) * (size_t)(h > 0 ? h : 0) * (size_t)(n > 0 ? n : 0), cb = sizeof(uint32_t) * (size_t)(w > 0 ? w : 0) * (size_t)(n > 0 ? n : 0);
    int rc;
    if (!src || !row_sum || !col_sum || n < 1 || device < 0 || w < 1 || h < 1 || !subsamp_known(subsamp)) return DSVG_ERR_ARG;
    if ((rc = dsvg_linesums_create(&s, device, w, h, subsamp))) return rc;
    if (!(rc = dsvg_lane_create(&l, device))) {
        if (!on_device && !(rc = dsvg_lane_upload(l, 0, src, dsv1_frame_bytes(w, h, subsamp) * (size_t)n, &d))) src = d;
        if (!rc) rc = dsvg_lane_alloc(l, &drow, rb);
        if (!rc) rc = dsvg_lane_alloc(l, &dcol, cb);
        if (!rc) rc = dsvg_linesums_run(s, dsvg_lane_stream(l), src, n, drow, dcol);
        if (!rc) rc = dsvg_lane_download(l, row_sum, drow, rb);
        if (!rc) rc = dsvg_lane_download(l, col_sum, dcol, cb);
        if (!rc) rc = dsvg_lane_sync(l);
        dsvg_lane_destroy(l);                           /* (waits for the stream; frees what the call allocated) */
    }
    dsvg_linesums_destroy(s);
    return rc;
}

int dsv1_bars_from_sums(const uint32_t *row_sum, const uint32_t *col_sum, int w, int h, int n, int thresh, int align, int rect[4])
{
    int x0 = -1, x1 = -1, y0 = -1, y1 = -1, t, i, x, y, rw, rh;
    if (rect) rect[0] = rect[1] = rect[2] = rect[3] = 0;
    if (!row_sum || !col_sum || !rect || w < 1 || h < 1 || n < 1) return DSVG_ERR_ARG;
    if (thresh < 0 || thresh > 254 || align < 1 || align > 64 || (align & (align - 1))) return DSVG_ERR_ARG;
    for (t = 0; t < n; t++) {
        for (i = 0; i < h; i++)
            if (row_sum[(size_t)t * h + i] > (uint64_t)thresh * (uint64_t)w) { if (y0 < 0 || i < y0) y0 = i; if (i > y1) y1 = i; }
        for (i = 0; i < w; i++)
            if (col_sum[(size_t)t * w + i] > (uint64_t)thresh * (uint64_t)h) { if (x0 < 0 || i < x0) x0 = i; if (i > x1) x1 = i; }
    }
    if (x0 < 0 || y0 < 0) return 0;
    x = (x0 + align - 1) & ~(align - 1); rw = ((x1 + 1) & ~(align - 1)) - x;
    y = (y0 + align - 1) & ~(align - 1); rh = ((y1 + 1) & ~(align - 1)) - y;
    if (rw < 1 || rh < 1) return 0;
    rect[0] = x; rect[1] = y; rect[2] = rw; rect[3] = rh;
    return 1;
}

int dsv1_detect_bars_clip(int device, const void *src, int w, int h, int subsamp, int n, int thresh, int align, int rect[4], int on_device)
{
    uint32_t *sums;
    int rc;
    if (rect) rect[0] = rect[1] = rect[2] = rect[3] = 0;
    if (!src || !rect || n < 1 || device < 0 || w < 1 || h < 1 || !subsamp_known(subsamp)) return DSVG_ERR_ARG;
    if (thresh < 0 || thresh > 254 || align < 1 || align > 64 || (align & (align - 1))) return DSVG_ERR_ARG;
    if ((size_t)n > SIZE_MAX / sizeof(uint32_t) / ((size_t)w + (size_t)h)) return DSVG_ERR_ARG;
    sums = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)n * ((size_t)w + (size_t)h));
    if (!sums) return DSVG_ERR_NOMEM;
    rc = dsv1_line_sums_clip(device, src, w, h, subsamp, n, sums, sums + (size_t)n * h, on_device);
    if (!rc) rc = dsv1_bars_from_sums(sums, sums + (size_t)n * h, w, h, n, thresh, align, rect);
    free(sums);
    return rc;
}
