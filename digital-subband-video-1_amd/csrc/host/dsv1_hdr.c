/* dsv1_hdr.c -- HDR sources (include/dsv1_api.h, HDR sources): settings -> tables in binary64 and exact rationals, the bounds that keep
 * the pixel path inside its integers, what a deep pixel format works out to for one geometry -- the definition tests/_hdr.py states in
 * numpy -- and the standalone converter.  The kernel and its device plumbing: k_hdr.hip, k_pixfmt.hip. */
#include <math.h>
#include "dsv1_host.h"

/* Kr, Kb in 1 / 10000 by DSV1_MATRIX_* */
static const int hdr_k[3][2] = {{2990, 1140}, {2126, 722}, {2627, 593}};

/* n / d rounded half up, n >= 0, d > 0 */
static int64_t rdiv(int64_t n, int64_t d) { return (2 * n + d) / (2 * d); }
static double rnd(double x) { return floor(x + 0.5); }

/* SMPTE ST 2084 */
#define PQ_M1 (2610.0 / 16384.0)
#define PQ_M2 (2523.0 / 4096.0 * 128.0)
#define PQ_C1 (3424.0 / 4096.0)
#define PQ_C2 (2413.0 / 4096.0 * 32.0)
#define PQ_C3 (2392.0 / 4096.0 * 32.0)
static double pq_nits(double e)
{
    const double p = pow(e, 1.0 / PQ_M2), num = p - PQ_C1 > 0.0 ? p - PQ_C1 : 0.0;
    return 10000.0 * pow(num / (PQ_C2 - PQ_C3 * p), 1.0 / PQ_M1);
}
static double pq_signal(double nits)
{
    const double yp = pow(nits / 10000.0, PQ_M1);
    return pow((PQ_C1 + PQ_C2 * yp) / (1.0 + PQ_C3 * yp), PQ_M2);
}
/* BT.2100 HLG inverse OETF: signal -> scene light 0..1 */
static double hlg_scene(double e)
{
    const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * log(4.0 * a);
    return e <= 0.5 ? e * e / 3.0 : (exp((e - c) / a) + b) / 12.0;
}

/* T: nits -> SDR linear 0..1 */
static double tonemap(const dsv1_hdr *hd, double white, double m)
{
    const double peak = (double)hd->peak_nits;
    double t;
    if (hd->curve == DSV1_TONEMAP_CLIP) t = m / white;
    else if (hd->curve == DSV1_TONEMAP_REINHARD) {
        const double x = m / white, l = peak / white;
        t = x * (1.0 + x / (l * l)) / (1.0 + x);
    } else {
        const double pw = pq_signal(peak), e1 = pq_signal(m) / pw, maxl = pq_signal(white) / pw, ks = 1.5 * maxl - 0.5;
        double e2 = e1;
        if (e1 >= ks && ks < 1.0) {
            const double s = (e1 - ks) / (1.0 - ks), s2 = s * s, s3 = s2 * s;
            e2 = (2.0 * s3 - 3.0 * s2 + 1.0) * ks + (s3 - 2.0 * s2 + s) * (1.0 - ks) + (-2.0 * s3 + 3.0 * s2) * maxl;
        }
        t = pq_nits(e2 * pw) / white;
    }
    return t < 1.0 ? t : 1.0;
}

static int white_of(const dsv1_hdr *hd) { return hd->white_nits ? hd->white_nits : 203; }

int dsv1_hdr_valid(const dsv1_hdr *hd)
{
    if (!hd) return 0;
    if (hd->transfer != DSV1_TRANSFER_PQ && hd->transfer != DSV1_TRANSFER_HLG) return 0;
    if (hd->matrix < DSV1_MATRIX_BT601 || hd->matrix > DSV1_MATRIX_BT2020 || hd->out_matrix < DSV1_MATRIX_BT601 || hd->out_matrix > DSV1_MATRIX_BT2020) return 0;
    if ((hd->full_range & ~1) || (hd->out_full_range & ~1) || (hd->gamut & ~1)) return 0;
    if (hd->curve < DSV1_TONEMAP_CLIP || hd->curve > DSV1_TONEMAP_BT2390) return 0;
    if (hd->peak_nits < 100 || hd->peak_nits > 10000) return 0;
    if (hd->white_nits && (hd->white_nits < 48 || hd->white_nits > 1000)) return 0;
    return white_of(hd) <= hd->peak_nits;
}

/* the representative of bucket i (dsv1_hdr_cidx): the value itself below 256, else the bucket's lower end + half its width, at most 2^20 */
static uint32_t bucket_rep(int i)
{
    const int e = (i >> 8) + 7;
    uint32_t r;
    if (i < 256) return (uint32_t)i;
    r = ((uint32_t)(256 + (i & 255)) << (e - 8)) + ((1u << (e - 8)) >> 1);
    return r < DSV1_HDR_ONE ? r : DSV1_HDR_ONE;
}

int dsv1_hdr_cidx_of(uint32_t v) { return v <= DSV1_HDR_ONE ? dsv1_hdr_cidx(v) : -1; }

int dsv1_hdr_build(const dsv1_hdr *hd, dsv1_hdr_tables *t)
{
    /* BT.2087: BT.2020 -> BT.709 primaries, in 1 / 10000 (the diagonal is the remainder of its row) */
    static const int g2087[3][3] = {{0, -5876, -728}, {-1246, 0, -83}, {-182, -1006, 0}};
    const double one = (double)DSV1_HDR_ONE;
    int64_t kr, kb, kg, ydiv, cdiv, syn, scn, yr, yb, hf, cbr, crb;
    double peak, white;
    int i, j;
    if (!t || !dsv1_hdr_valid(hd)) return DSVG_ERR_ARG;
    memset(t, 0, sizeof(*t));
    peak = (double)hd->peak_nits; white = (double)white_of(hd);
    /* the source signal at 10 bits -> an index 0..4095 */
    kr = hdr_k[hd->matrix][0]; kb = hdr_k[hd->matrix][1]; kg = 10000 - kr - kb;
    ydiv = hd->full_range ? 1023 : 876; cdiv = hd->full_range ? 1023 : 896;
    t->ycc[0] = (int32_t)rdiv(16384 * 4095, ydiv);
    t->ycc[1] = (int32_t)rdiv(16384 * 2 * (10000 - kr) * 4095, 10000 * cdiv);
    t->ycc[2] = -(int32_t)rdiv(16384 * 2 * (10000 - kb) * kb * 4095, 10000 * kg * cdiv);
    t->ycc[3] = -(int32_t)rdiv(16384 * 2 * (10000 - kr) * kr * 4095, 10000 * kg * cdiv);
    t->ycc[4] = (int32_t)rdiv(16384 * 2 * (10000 - kb) * 4095, 10000 * cdiv);
    t->in_oy = hd->full_range ? 0 : 64; t->in_oc = 512;
    for (i = 0; i < 4096; i++) {
        const double e = i / 4095.0;
        double v;
        if (hd->transfer == DSV1_TRANSFER_PQ) { v = pq_nits(e); v = (v < peak ? v : peak) / peak; }
        else v = hlg_scene(e);
        v = rnd(one * v);
        t->eotf[i] = v < one ? (uint32_t)v : DSV1_HDR_ONE;
    }
    for (i = 0; i < 3; i++) {
        int32_t sum = 0;
        for (j = 0; j < 3; j++)
            if (i != j) { t->gamut[3 * i + j] = hd->gamut ? -(int32_t)rdiv(16384 * (int64_t)-g2087[i][j], 10000) : 0; sum += t->gamut[3 * i + j]; }
        t->gamut[3 * i + i] = 16384 - sum;
    }
    for (i = 0; i < DSV1_HDR_NBUCKETS; i++) {
        const double f = bucket_rep(i) / one;
        double g;
        if (f == 0.0) g = hd->transfer == DSV1_TRANSFER_PQ ? rnd(65536.0 * peak / white) : 0.0;
        else g = rnd(65536.0 * tonemap(hd, white, hd->transfer == DSV1_TRANSFER_PQ ? f * peak : peak * pow(f, 1.2)) / f);
        t->gain[i] = g < 4294967295.0 ? (uint32_t)g : 4294967295u;
        t->oetf[i] = (uint16_t)rnd(4095.0 * pow(f, 1.0 / 2.4));
    }
    /* E' 0..4095 -> the SDR signal, Q20: the RGB section's forward rules with 4095 in the place of 255 */
    kr = hdr_k[hd->out_matrix][0]; kb = hdr_k[hd->out_matrix][1];
    syn = hd->out_full_range ? 255 : 219; scn = hd->out_full_range ? 255 : 224;
    yr = rdiv((1 << 20) * syn * kr, 4095 * 10000); yb = rdiv((1 << 20) * syn * kb, 4095 * 10000);
    hf = rdiv((1 << 20) * scn, 2 * 4095);
    cbr = -rdiv((1 << 20) * scn * kr, 4095 * 2 * (10000 - kb));
    crb = -rdiv((1 << 20) * scn * kb, 4095 * 2 * (10000 - kr));
    t->fwd[0] = (int32_t)yr; t->fwd[1] = (int32_t)(rdiv((1 << 20) * syn, 4095) - yr - yb); t->fwd[2] = (int32_t)yb;
    t->fwd[3] = (int32_t)cbr; t->fwd[4] = (int32_t)-(hf + cbr); t->fwd[5] = (int32_t)hf;
    t->fwd[6] = (int32_t)hf; t->fwd[7] = (int32_t)-(hf + crb); t->fwd[8] = (int32_t)crb;
    t->ybias = ((hd->out_full_range ? 0 : 16) << 20) + (1 << 19);
    t->cbias = (128 << 20) + (1 << 19);
    return DSVG_OK;
}

int dsv1_hdr_tables_valid(const dsv1_hdr_tables *t)
{
    int i;
    if (!t) return 0;
    for (i = 0; i < 5; i++) if (t->ycc[i] < -(1 << 19) || t->ycc[i] > (1 << 19)) return 0;
    if (t->in_oy < 0 || t->in_oy > 1023 || t->in_oc < 0 || t->in_oc > 1023) return 0;
    for (i = 0; i < 4096; i++) if (t->eotf[i] > DSV1_HDR_ONE) return 0;
    for (i = 0; i < 9; i++) if (t->gamut[i] < -(1 << 18) || t->gamut[i] > (1 << 18)) return 0;
    for (i = 0; i < DSV1_HDR_NBUCKETS; i++) if (t->oetf[i] > 4095) return 0;
    for (i = 0; i < 9; i++) if (t->fwd[i] < -(1 << 16) || t->fwd[i] > (1 << 16)) return 0;
    if (t->ybias < -(1 << 30) || t->ybias > (1 << 30) || t->cbias < -(1 << 30) || t->cbias > (1 << 30)) return 0;
    return 1;
}

int dsv1_hdr_layout_of(const dsv1_pix_format *pf, int w, int h, int src_subsamp, int subsamp, dsv1_hdr_layout *L)
{
    dsv1_pix_layout pl;
    int p;
    if (!pf || !L) return DSVG_ERR_ARG;
    if (pf->depth != 10 && pf->depth != 12 && pf->depth != 16) return DSVG_ERR_ARG;
    if (pf->layout != DSV1_PIX_PLANAR && pf->layout != DSV1_PIX_SEMIPLANAR_UV && pf->layout != DSV1_PIX_SEMIPLANAR_VU) return DSVG_ERR_ARG;
    if (src_subsamp == DSV_SUBSAMP_411 || subsamp == DSV_SUBSAMP_411) return DSVG_ERR_ARG;
    /* (the pair, the layout at src_subsamp, msb_aligned, the pitches and the stride: the pixel formats' own check) */
    if (dsv1_pix_layout_of(pf, w, h, src_subsamp, subsamp, &pl)) return DSVG_ERR_ARG;
    memset(L, 0, sizeof(*L));
    L->w = w; L->h = h;
    L->shs = (src_subsamp >> 2) & 3; L->svs = src_subsamp & 3; L->scw = pl.scw; L->sch = pl.sch;
    L->dhs = (subsamp >> 2) & 3; L->dvs = subsamp & 3;
    L->ocw = (w + (1 << L->dhs) - 1) >> L->dhs; L->och = (h + (1 << L->dvs) - 1) >> L->dvs;
    L->semi = pf->layout == DSV1_PIX_PLANAR ? 0 : pf->layout == DSV1_PIX_SEMIPLANAR_UV ? 1 : 2;
    for (p = 0; p < 3; p++) {
        const dsv1_pix_seg *S = &pl.seg[L->semi && p == 2 ? 1 : p];
        L->off[p] = S->soff; L->pitch[p] = S->spitch;
    }
    L->vshift = pf->msb_aligned ? 16 - pf->depth : 0; L->vmask = (1 << pf->depth) - 1;
    L->rs = pf->depth - 10; L->rnd = L->rs ? 1 << (L->rs - 1) : 0;
    L->frame_bytes = pl.frame_bytes; L->planes_bytes = pl.planes_bytes; L->out_frame_bytes = pl.out_frame_bytes;
    return DSVG_OK;
}

int dsv1_hdr_import_clip(int device, const void *src, const dsv1_pix_format *pf, int w, int h, int src_subsamp, int subsamp, int n, void *dst,
                         const dsv1_hdr_tables *tables, int upsample, int on_device)
{
    dsv1_hdr_layout L;
    dsvg_pixconv *pc = NULL;
    int rc;
    if (!src || !dst || !pf || !tables || n < 1 || device < 0) return DSVG_ERR_ARG;
    if (upsample != DSV1_CHROMA_REPLICATE && upsample != DSV1_CHROMA_LINEAR) return DSVG_ERR_ARG;
    if (!dsv1_hdr_tables_valid(tables)) return DSVG_ERR_ARG;
    if ((rc = dsv1_hdr_layout_of(pf, w, h, src_subsamp, subsamp, &L))) return rc;
    if ((rc = dsvg_pixconv_create_hdr(&pc, device, &L, tables, upsample))) return rc;
    {
        /* the last frame ends with its planes: a caller's buffer need not hold the stride's padding behind them */
        const dsv1_clip_io io = {{src, NULL}, {L.frame_bytes * (size_t)(n - 1) + L.planes_bytes, 0}, {dst, NULL}, {L.out_frame_bytes * (size_t)n, 0}};
        rc = dsv1_pass_clip(device, DSV1_SRC_CONVERT, pc, n, &io, on_device);
    }
    dsvg_pixconv_destroy(pc);
    return rc;
}
