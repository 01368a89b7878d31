/* dsv1_overlay.c -- overlays (include/dsv1_api.h, Overlays): the host-only entry points -- validity, the opacity of a picture, the plan
 * of a call (all three are dsvg_overlay_plan.h's pure functions), the RGBA helper -- and the standalone call.  The definitions are
 * stated in numpy in tests/_overlay.py; the kernel and its device plumbing: k_overlay.hip; the sessions: dsv1_srcchain.c, dsv1_enc.c,
 * dsv1_scale.c. */
#include "dsv1_host.h"
#include "../dsvg_overlay_plan.h"

size_t dsv1_overlay_bytes(int w, int h, int subsamp)
{
    if (w < 1 || h < 1 || !dsvg_overlay_subsamp_known(subsamp)) return 0;
    return dsv1_frame_bytes(w, h, subsamp) + (size_t)w * h;
}

int dsv1_overlay_valid(const dsv1_overlay *ov, int W, int H, int subsamp, int S) { return dsvg_overlay_valid(ov, W, H, subsamp, S); }

int dsv1_overlay_opacity_at(const dsv1_overlay *ov, int64_t t) { return ov ? dsvg_overlay_opacity_at(ov, t) : 0; }

long long dsv1_overlay_plan(const dsv1_overlay *list, int n, int S, int F, const int64_t *counters, int W, int H, int subsamp,
                            dsv1_overlay_item *items, long long room, int *nlayers)
{
    int i;
    if (!list || n < 1 || n > DSV1_MAX_OVERLAYS || S < 1 || F < 1 || !counters || room < 0 || (room && !items)) return DSVG_ERR_ARG;
    for (i = 0; i < n; i++)
        if (!dsvg_overlay_valid(&list[i], W, H, subsamp, S)) return DSVG_ERR_ARG;
    return dsvg_overlay_plan(list, n, S, F, counters, items, room, nlayers);
}

/* o[i] = (c[2i] + c[min(2i + 1, n - 1)] + 1) >> 1 along a line of n samples `step` bytes apart; returns the new length */
static int halve_line(uint8_t *c, int n, size_t step)
{
    const int m = (n + 1) / 2;
    int i;
    for (i = 0; i < m; i++) {
        const int a = c[(size_t)(2 * i) * step], b = c[(size_t)(2 * i + 1 < n ? 2 * i + 1 : n - 1) * step];
        c[(size_t)i * step] = (uint8_t)((a + b + 1) >> 1);
    }
    return m;
}

int dsv1_overlay_from_rgba(const void *rgba, int pitch, int w, int h, int order, int matrix, int full_range, int subsamp, uint8_t *out_planes)
{
    /* memory position -> component (0 R, 1 G, 2 B), as the RGB import's */
    static const int comp_of[8][3] = {{0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {1, 2, 0}};
    const uint8_t *src = (const uint8_t *)rgba;
    int32_t fwd[9];
    uint8_t *Y, *U, *V, *A, *c444;
    int planar, bpp, first, apos, hs, vs, cw, ch, x, y, k, p;
    size_t rowb;
    if (!rgba || !out_planes || w < 1 || h < 1 || pitch < 0 || !dsvg_overlay_subsamp_known(subsamp)) return DSVG_ERR_ARG;
    if (order < DSV1_RGB_RGB24 || order > DSV1_RGB_PLANAR_GBR || dsv1_rgb_tables(matrix, full_range, fwd, NULL)) return DSVG_ERR_ARG;
    planar = order >= DSV1_RGB_PLANAR_RGB;
    bpp = planar ? 1 : order <= DSV1_RGB_BGR24 ? 3 : 4;
    first = order == DSV1_RGB_ARGB || order == DSV1_RGB_ABGR;
    apos = bpp == 4 ? (first ? 0 : 3) : -1;
    rowb = (size_t)w * bpp;
    if (pitch && (size_t)pitch < rowb) return DSVG_ERR_ARG;
    if (pitch) rowb = (size_t)pitch;
    hs = (subsamp >> 2) & 3; vs = subsamp & 3;
    cw = (w + (1 << hs) - 1) >> hs; ch = (h + (1 << vs) - 1) >> vs;
    Y = out_planes; U = Y + (size_t)w * h; V = U + (size_t)cw * ch; A = V + (size_t)cw * ch;
    if (!(c444 = (uint8_t *)malloc((size_t)w * h * 2))) return DSVG_ERR_NOMEM;
    for (y = 0; y < h; y++)
        for (x = 0; x < w; x++) {
            int c[3], v[3];
            for (k = 0; k < 3; k++)
                c[comp_of[order][k]] = planar ? src[(size_t)k * rowb * h + (size_t)y * rowb + x] : src[(size_t)y * rowb + (size_t)x * bpp + first + k];
            for (k = 0; k < 3; k++) {
                const int off = k ? 128 : full_range ? 0 : 16;
                v[k] = (fwd[3 * k] * c[0] + fwd[3 * k + 1] * c[1] + fwd[3 * k + 2] * c[2] + (off << 16) + 32768) >> 16;
                v[k] = CLAMPI(v[k], 0, 255);
            }
            Y[(size_t)y * w + x] = (uint8_t)v[0];
            c444[(size_t)y * w + x] = (uint8_t)v[1];
            c444[(size_t)w * h + (size_t)y * w + x] = (uint8_t)v[2];
            A[(size_t)y * w + x] = apos < 0 ? 255 : src[(size_t)y * rowb + (size_t)x * bpp + apos];
        }
    /* the chroma halving: rows first (each halving rounded to 8 bits), then columns; the planes stay at pitch w until they are copied out */
    for (p = 0; p < 2; p++) {
        uint8_t *c = c444 + (size_t)p * w * h, *o = p ? V : U;
        int n = w, m = h;
        for (k = 0; k < hs; k++) {
            int nn = n;
            for (y = 0; y < h; y++) nn = halve_line(c + (size_t)y * w, n, 1);
            n = nn;
        }
        for (k = 0; k < vs; k++) {
            int mm = m;
            for (x = 0; x < n; x++) mm = halve_line(c + x, m, (size_t)w);
            m = mm;
        }
        for (y = 0; y < ch; y++) memcpy(o + (size_t)y * cw, c + (size_t)y * w, (size_t)cw);
    }
    free(c444);
    return DSVG_OK;
}

int dsv1_overlay_clip(int device, void *clip, int w, int h, int subsamp, int n, const dsv1_overlay *list, int count, int64_t t_first, int on_device)
{
    dsvg_overlay *o = NULL;
    dsvg_lane *l = NULL;
    void *d = clip;
    size_t bytes;
    int rc, i;
    if (!clip || !list || n < 1 || count < 1 || count > DSV1_MAX_OVERLAYS || device < 0 || w < 1 || h < 1 || !dsvg_overlay_subsamp_known(subsamp)) return DSVG_ERR_ARG;
    for (i = 0; i < count; i++)
        if (!dsvg_overlay_valid(&list[i], w, h, subsamp, 1)) return DSVG_ERR_ARG;
    bytes = dsv1_frame_bytes(w, h, subsamp) * (size_t)n;
    if ((rc = dsvg_overlay_create(&o, device, list, count, w, h, subsamp, 1))) return rc;
    /* (nothing active in these n pictures: the clip stays as it is, and nothing crosses the link) */
    if (dsvg_overlay_active(o, n, &t_first) && !(rc = dsvg_lane_create(&l, device))) {
        if (!on_device) rc = dsvg_lane_upload(l, 0, clip, bytes, &d);
        if (!rc) rc = dsvg_overlay_run(o, dsvg_lane_stream(l), 0, d, n, &t_first);
        if (!rc && !on_device) rc = dsvg_lane_download(l, clip, d, bytes);
        if (!rc) rc = dsvg_lane_sync(l);
        dsvg_lane_destroy(l);                           /* (waits for the stream; frees what the call allocated) */
    }
    dsvg_overlay_destroy(o);
    return rc;
}
