/* dsv1_pixfmt.c -- pixel formats (include/dsv1_api.h, dsv1_pix_format): what a format works out to for one geometry -- the
 * definition tests/_pixfmt.py states in numpy -- and the standalone converter; the kernel and its device plumbing: k_pixfmt.hip.
 * And the way back, decoder output formats (tests/_pixout.py, k_pixout.hip): the same layouts written, chroma halved on the way.
 * Both take a second subsampling (include/dsv1_api.h, chroma resampling; tests/_chroma.py): chroma halved on the way in, doubled on
 * the way out. */
#include "dsv1_host.h"

/* chroma is halved from subsampling a to b: 4:4:4 -> 4:2:2 / 4:2:0, 4:2:2 -> 4:2:0 */
static int halves(int a, int b)
{
    return (a == DSV_SUBSAMP_444 && (b == DSV_SUBSAMP_422 || b == DSV_SUBSAMP_420)) || (a == DSV_SUBSAMP_422 && b == DSV_SUBSAMP_420);
}

int dsv1_pix_layout_of(const dsv1_pix_format *pf, int w, int h, int src_subsamp, int out_subsamp, dsv1_pix_layout *L)
{
    const int subsamp = src_subsamp;     /* the source planes */
    int hs, vs, cw, ch, ocw, och, bps, p, nsp;
    size_t rowb[3], rows[3], off = 0;
    if (!pf || !L || w < 1 || h < 1) return DSVG_ERR_ARG;
    if (subsamp != DSV_SUBSAMP_444 && subsamp != DSV_SUBSAMP_422 && subsamp != DSV_SUBSAMP_420 && subsamp != DSV_SUBSAMP_411) return DSVG_ERR_ARG;
    if (out_subsamp != subsamp && !halves(subsamp, out_subsamp)) return DSVG_ERR_ARG;
    if (pf->depth != 8 && pf->depth != 10 && pf->depth != 12 && pf->depth != 16) return DSVG_ERR_ARG;
    if (pf->depth > 8 && pf->msb_aligned != 0 && pf->msb_aligned != 1) return DSVG_ERR_ARG;
    hs = (subsamp >> 2) & 3; vs = subsamp & 3;
    cw = (w + (1 << hs) - 1) >> hs; ch = (h + (1 << vs) - 1) >> vs;
    bps = pf->depth > 8 ? 2 : 1;
    memset(L, 0, sizeof(*L));
    L->hd = hs != ((out_subsamp >> 2) & 3); L->vd = vs != (out_subsamp & 3);
    L->scw = cw; L->sch = ch;
    ocw = (cw + L->hd) >> L->hd; och = (ch + L->vd) >> L->vd;
    L->wide = bps == 2;
    L->shift = !L->wide ? 0 : pf->msb_aligned ? 7 : pf->depth - 9;
    switch (pf->layout) {
    case DSV1_PIX_PLANAR:
        nsp = 3;
        rowb[0] = (size_t)w * bps; rowb[1] = rowb[2] = (size_t)cw * bps;
        rows[0] = (size_t)h; rows[1] = rows[2] = (size_t)ch;
        break;
    case DSV1_PIX_SEMIPLANAR_UV:
    case DSV1_PIX_SEMIPLANAR_VU:
        if (subsamp != DSV_SUBSAMP_420 && subsamp != DSV_SUBSAMP_422) return DSVG_ERR_ARG;
        nsp = 2;
        rowb[0] = (size_t)w * bps; rowb[1] = 2 * (size_t)cw * bps;
        rows[0] = (size_t)h; rows[1] = (size_t)ch;
        break;
    case DSV1_PIX_PACKED_YUYV:
    case DSV1_PIX_PACKED_UYVY:
        if (subsamp != DSV_SUBSAMP_422 || pf->depth != 8) return DSVG_ERR_ARG;
        nsp = 1;
        rowb[0] = 4 * (size_t)cw;
        rows[0] = (size_t)h;
        break;
    default:
        return DSVG_ERR_ARG;
    }
    L->nseg = nsp;
    for (p = 0; p < nsp; p++) {
        dsv1_pix_seg *S = &L->seg[p];
        if (pf->pitch[p] < 0 || (pf->pitch[p] && (size_t)pf->pitch[p] < rowb[p])) return DSVG_ERR_ARG;
        S->spitch = pf->pitch[p] ? (size_t)pf->pitch[p] : rowb[p];
        S->soff = off;
        S->rows = (int)rows[p];
        off += S->spitch * rows[p];
    }
    L->planes_bytes = off;
    if (pf->frame_bytes && pf->frame_bytes < off) return DSVG_ERR_ARG;
    L->frame_bytes = pf->frame_bytes ? pf->frame_bytes : off;
    cw = ocw; ch = och;                   /* from here on: the output's chroma planes */
    L->out_frame_bytes = (size_t)w * h + 2 * (size_t)cw * ch;
    {
        /* the output planes of the packed planar 8-bit frame */
        const size_t yo = 0, uo = (size_t)w * h, vo = uo + (size_t)cw * ch;
        dsv1_pix_seg *S = L->seg;
        if (nsp == 3) {
            for (p = 0; p < 3; p++) { S[p].kind = DSV1_PIXSEG_PLAIN; S[p].nout = 1; S[p].width = p ? cw : w; S[p].dpitch[0] = p ? cw : w; }
            S[1].rows = S[2].rows = ch;
            S[0].doff[0] = yo; S[1].doff[0] = uo; S[2].doff[0] = vo;
        } else if (nsp == 2) {
            const int vu = pf->layout == DSV1_PIX_SEMIPLANAR_VU;
            S[0].kind = DSV1_PIXSEG_PLAIN; S[0].nout = 1; S[0].width = w; S[0].dpitch[0] = w; S[0].doff[0] = yo;
            S[1].kind = DSV1_PIXSEG_PAIR; S[1].nout = 2; S[1].width = cw; S[1].dpitch[0] = S[1].dpitch[1] = cw; S[1].rows = ch;
            S[1].doff[0] = vu ? vo : uo; S[1].doff[1] = vu ? uo : vo;       /* the pair's first sample goes to doff[0] */
        } else {
            S[0].kind = pf->layout == DSV1_PIX_PACKED_YUYV ? DSV1_PIXSEG_YUYV : DSV1_PIXSEG_UYVY;
            S[0].nout = 3; S[0].width = w; S[0].cwidth = cw;
            S[0].dpitch[0] = w; S[0].dpitch[1] = S[0].dpitch[2] = cw;
            S[0].doff[0] = yo; S[0].doff[1] = uo; S[0].doff[2] = vo;
        }
    }
    return DSVG_OK;
}

size_t dsv1_pix_frame_bytes(const dsv1_pix_format *pf, int w, int h, int subsamp)
{
    dsv1_pix_layout L;
    return dsv1_pix_layout_of(pf, w, h, subsamp, subsamp, &L) ? 0 : L.frame_bytes;
}

int dsv1_pix_is_default(const dsv1_pix_format *pf, int w, int h, int subsamp)
{
    dsv1_pix_layout L;
    if (!pf) return 1;
    if (pf->layout != DSV1_PIX_PLANAR || pf->depth != 8 || dsv1_pix_layout_of(pf, w, h, subsamp, subsamp, &L)) return 0;
    return L.frame_bytes == L.out_frame_bytes && L.planes_bytes == L.out_frame_bytes;      /* every pitch a row, no stride beyond */
}

int dsv1_convert_clip(int device, const void *src, const dsv1_pix_format *pf, int w, int h, int subsamp, int n, void *dst, int on_device)
{
    return dsv1_convert_clip_sub(device, src, pf, w, h, subsamp, subsamp, n, dst, on_device);
}

/* ... into frames at `subsamp`, chroma halved on the way */
int dsv1_convert_clip_sub(int device, const void *src, const dsv1_pix_format *pf, int w, int h, int src_subsamp, int subsamp, int n, void *dst,
                          int on_device)
{
    dsv1_pix_layout L;
    dsvg_pixconv *pc = NULL;
    int rc;
    if (!src || !dst || !pf || n < 1 || device < 0) return DSVG_ERR_ARG;
    if ((rc = dsv1_pix_layout_of(pf, w, h, src_subsamp, subsamp, &L))) return rc;
    if ((rc = dsvg_pixconv_create(&pc, device, &L))) return rc;
    {
        /* the last frame ends with its planes: a caller's buffer need not hold the stride's padding behind them */
        const dsv1_clip_io io = {{src, NULL}, {L.frame_bytes * (size_t)(n - 1) + L.planes_bytes, 0}, {dst, NULL}, {L.out_frame_bytes * (size_t)n, 0}};
        rc = dsv1_pass_clip(device, DSV1_SRC_CONVERT, pc, n, &io, on_device);
    }
    dsvg_pixconv_destroy(pc);
    return rc;
}

/* ---- decoder output formats ---- */
int dsv1_pixout_of(const dsv1_pix_format *pf, int w, int h, int subsamp, int out_subsamp, int upsample, dsvg_pixout *F)
{
    dsv1_pix_layout L;
    int p, rc;
    const int up = upsample != DSV1_CHROMA_NONE && halves(out_subsamp, subsamp);
    if (!pf || !F) return DSVG_ERR_ARG;
    if (upsample != DSV1_CHROMA_NONE && upsample != DSV1_CHROMA_REPLICATE && upsample != DSV1_CHROMA_LINEAR) return DSVG_ERR_ARG;
    if (!(out_subsamp == subsamp || halves(subsamp, out_subsamp) || up)) return DSVG_ERR_ARG;
    if (subsamp != DSV_SUBSAMP_444 && subsamp != DSV_SUBSAMP_422 && subsamp != DSV_SUBSAMP_420 && subsamp != DSV_SUBSAMP_411) return DSVG_ERR_ARG;
    /* the format's planes at the output subsampling: the converter's source side is this pass's destination */
    if ((rc = dsv1_pix_layout_of(pf, w, h, out_subsamp, out_subsamp, &L))) return rc;
    memset(F, 0, sizeof(*F));
    F->nseg = L.nseg;
    F->wide = L.wide;
    F->shift = !L.wide ? 0 : pf->msb_aligned ? 8 : pf->depth - 8;       /* v << (d - 8) in the low bits, or moved up to bit 15: v << 8 */
    F->hd = !up && ((subsamp >> 2) & 3) != ((out_subsamp >> 2) & 3);
    F->vd = !up && (subsamp & 3) != (out_subsamp & 3);
    F->hu = up && ((subsamp >> 2) & 3) != ((out_subsamp >> 2) & 3);
    F->vu = up && (subsamp & 3) != (out_subsamp & 3);
    F->linear = up && upsample == DSV1_CHROMA_LINEAR;
    F->frame_bytes = L.frame_bytes;
    F->planes_bytes = L.planes_bytes;
    for (p = 0; p < L.nseg; p++) {
        const dsv1_pix_seg *S = &L.seg[p];
        dsvg_pixout_seg *G = &F->seg[p];
        G->rows = S->rows; G->width = S->width; G->cwidth = S->cwidth;
        G->off = S->soff; G->pitch = S->spitch;
        G->nin = S->nout;
        switch (S->kind) {
        case DSV1_PIXSEG_PLAIN: G->kind = DSVG_PIXOUT_PLAIN; G->in_plane[0] = L.nseg == 3 ? p : 0; break;
        case DSV1_PIXSEG_PAIR:  G->kind = DSVG_PIXOUT_PAIR; G->in_plane[0] = pf->layout == DSV1_PIX_SEMIPLANAR_VU ? 2 : 1; G->in_plane[1] = 3 - G->in_plane[0]; break;
        default:                G->kind = S->kind == DSV1_PIXSEG_YUYV ? DSVG_PIXOUT_YUYV : DSVG_PIXOUT_UYVY; G->in_plane[1] = 1; G->in_plane[2] = 2; break;
        }
    }
    return DSVG_OK;
}

static int export_clip(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsv1_pix_format *pf, int out_subsamp,
                       int upsample, int on_device)
{
    dsvg_pixout F;
    int rc;
    if (!src || !dst || !pf || n < 1 || device < 0) return DSVG_ERR_ARG;
    if ((rc = dsv1_pixout_of(pf, w, h, subsamp, out_subsamp, upsample, &F))) return rc;
    return dsvg_export_planar(device, src, w, h, subsamp, n, dst, &F, on_device);
}

int dsv1_export_clip(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsv1_pix_format *pf, int out_subsamp,
                     int on_device)
{
    return export_clip(device, src, w, h, subsamp, n, dst, pf, out_subsamp, DSV1_CHROMA_NONE, on_device);
}

int dsv1_export_clip_up(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsv1_pix_format *pf, int out_subsamp,
                        int upsample, int on_device)
{
    if (upsample != DSV1_CHROMA_REPLICATE && upsample != DSV1_CHROMA_LINEAR) return DSVG_ERR_ARG;
    return export_clip(device, src, w, h, subsamp, n, dst, pf, out_subsamp, upsample, on_device);
}
