/* dsv1_rgb.c -- RGB in and out (include/dsv1_api.h, RGB): the tables, what a dsv1_rgb_format works out to for one geometry -- the
 * definition tests/_rgb.py states in numpy -- and the standalone converters.  The kernels and their device plumbing: k_rgb.hip. */
#include "dsv1_host.h"

/* [matrix][full_range]: forward Q16 rows Y, Cb, Cr over (R, G, B); inverse Q14 IY, RV, GU, GV, BU.  Literals: tests/test_rgb_host.py
 * derives them again from Kr, Kb and the ranges in exact rationals. */
static const int32_t rgb_fwd[3][2][9] = {
    {{16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681}, {19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329}},
    {{11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639}, {13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005}},
    {{14786, 38160, 3338, -8038, -20746, 28784, 28784, -26469, -2315}, {17216, 44434, 3886, -9151, -23617, 32768, 32768, -30133, -2635}},
};
static const int32_t rgb_inv[3][2][5] = {
    {{19077, 26149, -6419, -13320, 33050}, {16384, 22970, -5638, -11700, 29032}},
    {{19077, 29372, -3494, -8731, 34610}, {16384, 25802, -3069, -7670, 30402}},
    {{19077, 27503, -3069, -10657, 35091}, {16384, 24160, -2696, -9361, 30825}},
};

int dsv1_rgb_tables(int matrix, int full_range, int32_t fwd[9], int32_t inv[5])
{
    if (matrix < DSV1_MATRIX_BT601 || matrix > DSV1_MATRIX_BT2020 || (full_range != 0 && full_range != 1)) return DSVG_ERR_ARG;
    if (fwd) memcpy(fwd, rgb_fwd[matrix][full_range], sizeof(rgb_fwd[0][0]));
    if (inv) memcpy(inv, rgb_inv[matrix][full_range], sizeof(rgb_inv[0][0]));
    return DSVG_OK;
}

int dsv1_rgb_layout_of(const dsv1_rgb_format *rf, int w, int h, int subsamp, dsv1_rgb_layout *L)
{
    /* memory position -> component (0 R, 1 G, 2 B) */
    static const int comp_of[8][3] = {{0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {1, 2, 0}};
    size_t rowb, off = 0;
    int p;
    if (!rf || !L || w < 1 || h < 1) return DSVG_ERR_ARG;
    if (subsamp != DSV_SUBSAMP_444 && subsamp != DSV_SUBSAMP_422 && subsamp != DSV_SUBSAMP_420) return DSVG_ERR_ARG;
    if (rf->order < DSV1_RGB_RGB24 || rf->order > DSV1_RGB_PLANAR_GBR) return DSVG_ERR_ARG;
    if (rf->upsample != DSV1_CHROMA_REPLICATE && rf->upsample != DSV1_CHROMA_LINEAR) return DSVG_ERR_ARG;
    memset(L, 0, sizeof(*L));
    if (dsv1_rgb_tables(rf->matrix, rf->full_range, L->fwd, L->inv)) return DSVG_ERR_ARG;
    L->w = w; L->h = h;
    L->hs = (subsamp >> 2) & 3; L->vs = subsamp & 3;
    L->cw = (w + (1 << L->hs) - 1) >> L->hs; L->ch = (h + (1 << L->vs) - 1) >> L->vs;
    L->nplanes = rf->order >= DSV1_RGB_PLANAR_RGB ? 3 : 1;
    L->bpp = L->nplanes == 3 ? 1 : rf->order <= DSV1_RGB_BGR24 ? 3 : 4;
    L->first = rf->order == DSV1_RGB_ARGB || rf->order == DSV1_RGB_ABGR;
    memcpy(L->comp, comp_of[rf->order], sizeof(L->comp));
    L->linear = rf->upsample == DSV1_CHROMA_LINEAR;
    L->oy = rf->full_range ? 0 : 16;
    rowb = (size_t)w * L->bpp;
    for (p = 0; p < L->nplanes; p++) {
        if (rf->pitch[p] < 0 || (rf->pitch[p] && (size_t)rf->pitch[p] < rowb)) return DSVG_ERR_ARG;
        L->pitch[p] = rf->pitch[p] ? (size_t)rf->pitch[p] : rowb;
        L->off[p] = off;
        off += L->pitch[p] * (size_t)h;
    }
    L->planes_bytes = off;
    if (rf->frame_bytes && rf->frame_bytes < off) return DSVG_ERR_ARG;
    L->frame_bytes = rf->frame_bytes ? rf->frame_bytes : off;
    L->yuv_frame_bytes = (size_t)w * h + 2 * (size_t)L->cw * L->ch;
    return DSVG_OK;
}

size_t dsv1_rgb_frame_bytes(const dsv1_rgb_format *rf, int w, int h)
{
    dsv1_rgb_layout L;
    return dsv1_rgb_layout_of(rf, w, h, DSV_SUBSAMP_444, &L) ? 0 : L.frame_bytes;
}

int dsv1_rgbout_of(const dsv1_rgb_format *rf, int w, int h, int subsamp, dsvg_pixout *F)
{
    dsv1_rgb_layout L;
    int p, rc;
    if (!F) return DSVG_ERR_ARG;
    if ((rc = dsv1_rgb_layout_of(rf, w, h, subsamp, &L))) return rc;
    memset(F, 0, sizeof(*F));
    F->nseg = L.nplanes;
    F->frame_bytes = L.frame_bytes;
    F->planes_bytes = L.planes_bytes;
    for (p = 0; p < L.nplanes; p++) {
        dsvg_pixout_seg *G = &F->seg[p];
        G->kind = DSVG_PIXOUT_RGB; G->nin = 3; G->in_plane[0] = 0; G->in_plane[1] = 1; G->in_plane[2] = 2;
        G->rows = h; G->width = w;
        G->off = L.off[p]; G->pitch = L.pitch[p];
    }
    F->rgb.on = 1; F->rgb.order = rf->order; F->rgb.linear = L.linear; F->rgb.hs = L.hs; F->rgb.vs = L.vs; F->rgb.oy = L.oy;
    memcpy(F->rgb.inv, L.inv, sizeof(L.inv));
    return DSVG_OK;
}

int dsv1_rgb_import_clip(int device, const void *src, const dsv1_rgb_format *rf, int w, int h, int subsamp, int n, void *dst, int on_device)
{
    dsv1_rgb_layout L;
    dsvg_pixconv *pc = NULL;
    int rc;
    if (!src || !dst || !rf || n < 1 || device < 0) return DSVG_ERR_ARG;
    if ((rc = dsv1_rgb_layout_of(rf, w, h, subsamp, &L))) return rc;
    if ((rc = dsvg_pixconv_create_rgb(&pc, device, &L))) return rc;
    {
        /* the last frame ends with its planes: a caller's buffer need not hold the stride's padding behind them */
        const dsv1_clip_io io = {{src, NULL}, {L.frame_bytes * (size_t)(n - 1) + L.planes_bytes, 0}, {dst, NULL}, {L.yuv_frame_bytes * (size_t)n, 0}};
        rc = dsv1_pass_clip(device, DSV1_SRC_CONVERT, pc, n, &io, on_device);
    }
    dsvg_pixconv_destroy(pc);
    return rc;
}

int dsv1_rgb_export_clip(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsv1_rgb_format *rf, int on_device)
{
    dsvg_pixout F;
    int rc;
    if (!src || !dst || !rf || n < 1 || device < 0) return DSVG_ERR_ARG;
    if ((rc = dsv1_rgbout_of(rf, w, h, subsamp, &F))) return rc;
    return dsvg_export_planar(device, src, w, h, subsamp, n, dst, &F, on_device);
}
