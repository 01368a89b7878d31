/* dsv1_srcchain.c -- the source side of a session (dsv1_host.h): convert -> levels -> deinterlace or inverse telecine -> denoise -> orient -> reframe -> overlay on one lane (dsvg_pixfmt.h), for
 * batches (dsv1_enc.c) and resolution ladders (dsv1_scale.c), and the sequence the standalone clip calls share. */
#include "dsv1_host.h"

void dsv1_srcchain_init(dsv1_srcchain *c, int device, int w, int h, int subsamp, int nsrc, int F, int keep_lane)
{
    memset(c, 0, sizeof(*c));
    c->device = device; c->w = w; c->h = h; c->subsamp = subsamp; c->nsrc = nsrc; c->F = F; c->keep_lane = keep_lane;
    c->mw = c->ow = w; c->mh = c->oh = h;
    c->fb = c->mfb = c->ofb = dsv1_frame_bytes(w, h, subsamp);
}

int dsv1_srcchain_lane(dsv1_srcchain *c) { return c->lane ? DSVG_OK : dsvg_lane_create(&c->lane, c->device); }

/* no pass left: no lane (a session that keeps it for its own uploads and scales says so at init) */
static void chain_release(dsv1_srcchain *c)
{
    if (c->keep_lane || dsv1_srcchain_any(c)) return;
    dsvg_lane_destroy(c->lane);
    c->lane = NULL;
}

void dsv1_srcchain_close(dsv1_srcchain *c)
{
    if (c->lane) (void)dsvg_lane_sync(c->lane);        /* (the passes' kernels read the memory their destroy frees) */
    dsvg_pixconv_destroy(c->pc);
    dsvg_levels_destroy(c->lv);
    dsvg_deint_destroy(c->dd);
    dsvg_ivtc_destroy(c->iv);
    dsvg_denoise_destroy(c->dn);
    dsvg_orient_destroy(c->orn);
    dsvg_reframe_destroy(c->rf);
    dsvg_overlay_destroy(c->ov);
    free(c->ov_t);
    dsvg_lane_destroy(c->lane);                         /* (and the clips) */
    memset(c, 0, sizeof(*c));
}

/* the frames per source the converter and the levels write: what a call brings.  (Never fewer than F: a field-rate deinterlacer may be cleared
 * behind a converter that stays.) */
static int conv_frames_for(const dsv1_srcchain *c, int with_ivtc) { return with_ivtc ? c->F / 4 * 5 : c->F; }

/* pass p (NULL: none) takes slot k (DSV1_SRC_*): its two clips first, and only then does the pass set before go, with its clips.
 * The inverse telecine lives in the deinterlacer's slot; it changes what a call brings, so where a converter or the levels are
 * installed their two clips are allocated again for that many frames in the same step.  On an error the chain is as it was and p is still the caller's. */
static int chain_install(dsv1_srcchain *c, int k, void *p)
{
    const int slot = k == DSV1_SRC_IVTC ? DSV1_SRC_DEINTERLACE : k;
    const size_t fb = k == DSV1_SRC_REFRAME ? c->ofb : k == DSV1_SRC_ORIENT ? c->mfb : c->fb;
    const int cf = conv_frames_for(c, k == DSV1_SRC_IVTC ? p != NULL : c->iv != NULL);
    const int resize = k == DSV1_SRC_IVTC && cf != c->conv_frames;
    const int reconv = resize && c->pc, relev = resize && c->lv;
    void *clip[2] = {NULL, NULL}, *conv[2] = {NULL, NULL}, *lev[2] = {NULL, NULL};
    int rc, j;
    if (!p && !c->clip[slot][0]) return DSVG_OK;
    rc = dsv1_srcchain_lane(c);
    for (j = 0; p && j < 2 && !rc; j++) rc = dsvg_lane_alloc(c->lane, &clip[j], fb * (size_t)c->nsrc * (size_t)(k == DSV1_SRC_CONVERT || k == DSV1_SRC_LEVELS ? cf : c->F));
    for (j = 0; reconv && j < 2 && !rc; j++) rc = dsvg_lane_alloc(c->lane, &conv[j], fb * (size_t)c->nsrc * (size_t)cf);
    for (j = 0; relev && j < 2 && !rc; j++) rc = dsvg_lane_alloc(c->lane, &lev[j], fb * (size_t)c->nsrc * (size_t)cf);
    if (!rc) rc = dsvg_lane_sync(c->lane);
    if (rc) {
        if (c->lane) for (j = 0; j < 2; j++) { (void)dsvg_lane_free(c->lane, clip[j]); (void)dsvg_lane_free(c->lane, conv[j]); (void)dsvg_lane_free(c->lane, lev[j]); }
        chain_release(c);
        return rc;
    }
    switch (k) {
    case DSV1_SRC_CONVERT:     dsvg_pixconv_destroy(c->pc); c->pc = (dsvg_pixconv *)p; break;
    case DSV1_SRC_DEINTERLACE: dsvg_deint_destroy(c->dd); c->dd = (dsvg_deint *)p; break;
    case DSV1_SRC_IVTC:        dsvg_ivtc_destroy(c->iv); c->iv = (dsvg_ivtc *)p; break;
    case DSV1_SRC_LEVELS:      dsvg_levels_destroy(c->lv); c->lv = (dsvg_levels *)p; break;
    case DSV1_SRC_ORIENT:      dsvg_orient_destroy(c->orn); c->orn = (dsvg_orient *)p; break;
    case DSV1_SRC_REFRAME:     dsvg_reframe_destroy(c->rf); c->rf = (dsvg_reframe *)p; break;
    default:                   dsvg_denoise_destroy(c->dn); c->dn = (dsvg_denoise *)p; break;
    }
    for (j = 0; j < 2; j++) {
        (void)dsvg_lane_free(c->lane, c->clip[slot][j]);
        c->clip[slot][j] = clip[j];
        if (reconv) {
            (void)dsvg_lane_free(c->lane, c->clip[DSV1_SRC_CONVERT][j]);
            c->clip[DSV1_SRC_CONVERT][j] = conv[j];
        }
        if (relev) {
            (void)dsvg_lane_free(c->lane, c->clip[DSV1_SRC_LEVELS][j]);
            c->clip[DSV1_SRC_LEVELS][j] = lev[j];
        }
    }
    c->conv_frames = cf;
    chain_release(c);
    return DSVG_OK;
}

int dsv1_srcchain_set_format(dsv1_srcchain *c, const dsv1_pix_layout *L, const dsv1_rgb_layout *R)
{
    dsvg_pixconv *pc = NULL;
    int rc;
    if (L && (rc = dsvg_pixconv_create(&pc, c->device, L))) return rc;
    if (R && (rc = dsvg_pixconv_create_rgb(&pc, c->device, R))) return rc;
    if ((rc = chain_install(c, DSV1_SRC_CONVERT, pc))) { dsvg_pixconv_destroy(pc); return rc; }
    c->raw_fb = L ? L->frame_bytes : R ? R->frame_bytes : 0;
    return DSVG_OK;
}

/* directly behind the converter, at the raw geometry.  The pictures every pass behind it sees change meaning: their history and state
 * go (the sessions allow the call only with nothing in flight) */
int dsv1_srcchain_set_levels(dsv1_srcchain *c, const dsv1_levels *lv)
{
    dsvg_levels *l = NULL;
    int rc;
    if (lv && dsv1_levels_is_identity(lv)) lv = NULL;
    if (!lv && !c->lv) return DSVG_OK;                  /* (none before, none now: the pictures keep their meaning) */
    if (lv && (rc = dsvg_levels_create(&l, c->device, lv, c->w, c->h, c->subsamp))) return rc;
    if ((rc = chain_install(c, DSV1_SRC_LEVELS, l))) { dsvg_levels_destroy(l); return rc; }
    if (c->dd && (rc = dsvg_deint_reset(c->dd, -1))) return rc;
    if (c->iv && (rc = dsvg_ivtc_reset(c->iv, -1))) return rc;
    return c->dn ? dsvg_denoise_reset(c->dn, -1) : DSVG_OK;
}

int dsv1_srcchain_set_deinterlace(dsv1_srcchain *c, const dsv1_deint *di)
{
    dsvg_deint *dd = NULL;
    int rc;
    if (c->iv) return di ? DSVG_ERR_ARG : DSVG_OK;      /* (its slot is the inverse telecine's) */
    if (di && (rc = dsvg_deint_create(&dd, c->device, c->w, c->h, c->subsamp, di, c->nsrc, 1))) return rc;
    if ((rc = chain_install(c, DSV1_SRC_DEINTERLACE, dd))) { dsvg_deint_destroy(dd); return rc; }
    memset(&c->dd_set, 0, sizeof(c->dd_set));
    if (di) c->dd_set = *di;
    return c->dn ? dsvg_denoise_reset(c->dn, -1) : DSVG_OK;     /* the pictures the noise filter sees change meaning */
}

int dsv1_srcchain_set_ivtc(dsv1_srcchain *c, const dsv1_ivtc *iv)
{
    dsvg_ivtc *p = NULL;
    int rc;
    if (c->dd) return iv ? DSVG_ERR_ARG : DSVG_OK;      /* (its slot is the deinterlacer's) */
    if (iv && (c->F < 4 || c->F % 4)) return DSVG_ERR_ARG;
    if (!iv && !c->iv) return DSVG_OK;
    if (iv && (rc = dsvg_ivtc_create(&p, c->device, c->w, c->h, c->subsamp, iv, c->nsrc, c->F / 4 * 5, 1))) return rc;
    if ((rc = chain_install(c, DSV1_SRC_IVTC, p))) { dsvg_ivtc_destroy(p); return rc; }
    memset(&c->iv_set, 0, sizeof(c->iv_set));
    if (iv) c->iv_set = *iv;
    return c->dn ? dsvg_denoise_reset(c->dn, -1) : DSVG_OK;     /* the pictures the noise filter sees change meaning */
}

int dsv1_srcchain_set_denoise(dsv1_srcchain *c, const dsv1_denoise *dn)
{
    dsvg_denoise *nd = NULL;
    int rc;
    if (dn && (rc = dsvg_denoise_create(&nd, c->device, c->w, c->h, c->subsamp, dn, c->nsrc, 1))) return rc;
    if ((rc = chain_install(c, DSV1_SRC_DENOISE, nd))) { dsvg_denoise_destroy(nd); return rc; }
    memset(&c->dn_set, 0, sizeof(c->dn_set));
    if (dn) c->dn_set = *dn;
    return DSVG_OK;
}

/* the frames that come in take the reframe's input geometry (the session's own again without one): only while no other pass is set,
 * whose clips and state are sized for the geometry in force (the orientation is set behind it, and turns that geometry) */
int dsv1_srcchain_set_reframe(dsv1_srcchain *c, const dsv1_reframe *rf)
{
    dsvg_reframe *r = NULL;
    int rc;
    if (c->pc || c->lv || c->dd || c->iv || c->dn || c->orn) return DSVG_ERR_ARG;
    if (rf && (rf->out_w != c->ow || rf->out_h != c->oh)) return DSVG_ERR_ARG;
    if (rf && dsv1_reframe_is_identity(rf)) rf = NULL;
    if (rf && (rc = dsvg_reframe_create(&r, c->device, rf, c->subsamp))) return rc;
    if ((rc = chain_install(c, DSV1_SRC_REFRAME, r))) { dsvg_reframe_destroy(r); return rc; }
    c->w = c->mw = rf ? rf->in_w : c->ow; c->h = c->mh = rf ? rf->in_h : c->oh;
    c->fb = c->mfb = dsv1_frame_bytes(c->w, c->h, c->subsamp);
    return DSVG_OK;
}

/* the frames that come in are the oriented geometry (the reframe's input, or the session's own) turned back by the inverse code: only
 * while no pass in front of it is set, whose clips and state are sized for the raw geometry in force */
int dsv1_srcchain_set_orient(dsv1_srcchain *c, int orient)
{
    dsvg_orient *o = NULL;
    int rc, rw, rh;
    if (c->pc || c->lv || c->dd || c->iv || c->dn) return DSVG_ERR_ARG;
    if (!dsv1_orient_valid(orient, c->subsamp) || dsv1_orient_dims(dsv1_orient_inverse(orient), c->mw, c->mh, &rw, &rh)) return DSVG_ERR_ARG;
    if (orient && (rc = dsvg_orient_create(&o, c->device, orient, rw, rh, c->subsamp))) return rc;
    if ((rc = chain_install(c, DSV1_SRC_ORIENT, o))) { dsvg_orient_destroy(o); return rc; }
    c->orient = orient;
    c->w = rw; c->h = rh;
    c->fb = dsv1_frame_bytes(rw, rh, c->subsamp);
    return DSVG_OK;
}

/* the overlays: behind everything, on the canvas; no geometry changes, so no other pass minds.  The pass's own two clips are allocated by
 * the first call that needs them (dsv1_srcchain_run) and go with the list */
int dsv1_srcchain_set_overlays(dsv1_srcchain *c, const dsv1_overlay *list, int n)
{
    dsvg_overlay *o = NULL;
    int64_t *t = NULL;
    int rc, j;
    if (!list || n < 1) { list = NULL; n = 0; }
    if (!n && !c->ov) return DSVG_OK;
    if (n) {
        if (!(t = (int64_t *)calloc((size_t)c->nsrc, sizeof(*t)))) return DSVG_ERR_NOMEM;
        if ((rc = dsvg_overlay_create(&o, c->device, list, n, c->ow, c->oh, c->subsamp, c->nsrc)) || (rc = dsv1_srcchain_lane(c))) {
            dsvg_overlay_destroy(o);
            free(t);
            return rc;
        }
    }
    if (c->lane) (void)dsvg_lane_sync(c->lane);        /* (the old list's launches read its bitmaps) */
    dsvg_overlay_destroy(c->ov);
    free(c->ov_t);
    c->ov = o; c->ov_t = t;
    for (j = 0; j < 2 && !n; j++) {
        (void)dsvg_lane_free(c->lane, c->clip[DSV1_SRC_OVERLAY][j]);
        c->clip[DSV1_SRC_OVERLAY][j] = NULL;
    }
    chain_release(c);
    return DSVG_OK;
}

int dsv1_srcchain_overlay_seek(dsv1_srcchain *c, int source, int64_t t)
{
    int s;
    if (!c->ov || source < -1 || source >= c->nsrc) return DSVG_ERR_ARG;
    for (s = 0; s < c->nsrc; s++)
        if (source < 0 || source == s) c->ov_t[s] = t;
    return DSVG_OK;
}

int dsv1_srcchain_deinterlace_reset(dsv1_srcchain *c, int source) { return c->dd ? dsvg_deint_reset(c->dd, source) : DSVG_ERR_ARG; }
int dsv1_srcchain_ivtc_reset(dsv1_srcchain *c, int source) { return c->iv ? dsvg_ivtc_reset(c->iv, source) : DSVG_ERR_ARG; }
int dsv1_srcchain_denoise_reset(dsv1_srcchain *c, int source) { return c->dn ? dsvg_denoise_reset(c->dn, source) : DSVG_ERR_ARG; }

int dsv1_srcchain_frames_in(const dsv1_srcchain *c)
{
    if (c->iv) return c->F / 4 * 5;
    return c->dd && c->dd_set.mode == DSV1_DEINT_FIELD ? c->F / 2 : c->F;
}
size_t dsv1_srcchain_bytes_in(const dsv1_srcchain *c)
{
    return (c->pc ? c->raw_fb : c->fb) * (size_t)c->nsrc * (size_t)dsv1_srcchain_frames_in(c);
}

int dsv1_srcchain_run(dsv1_srcchain *c, int par, const void *clip, int on_device, const void **out)
{
    const int nin = dsv1_srcchain_frames_in(c);
    /* the items the overlays would blend in this call */
    const long long act = c->ov ? dsvg_overlay_active(c->ov, c->F, c->ov_t) : 0;
    void *st = dsvg_lane_stream(c->lane), *d;
    int rc, own = 0, s;                                 /* own: the clip lies in memory of the chain's */
    if (!c->lane || !clip || !out) return DSVG_ERR_ARG;
    if (!act && !dsv1_srcchain_writes(c) && (on_device || !c->keep_lane)) {
        /* overlays alone and none active: no upload, no copy, no launch -- the clip goes on as it came, only the pictures count */
        for (s = 0; c->ov && s < c->nsrc; s++) c->ov_t[s] += c->F;
        *out = clip;
        return DSVG_OK;
    }
    if (!on_device) {
        if ((rc = dsvg_lane_upload(c->lane, par, clip, dsv1_srcchain_bytes_in(c), &d))) return rc;
        clip = d;
        own = 1;
    }
    if (dsv1_srcchain_writes(c)) own = 1;
    if (c->pc) {
        if ((rc = dsvg_pixconv_run(c->pc, st, clip, c->nsrc * nin, c->clip[DSV1_SRC_CONVERT][par]))) return rc;
        clip = c->clip[DSV1_SRC_CONVERT][par];
    }
    if (c->lv) {
        if ((rc = dsvg_levels_run(c->lv, st, clip, c->nsrc * nin, c->clip[DSV1_SRC_LEVELS][par]))) return rc;
        clip = c->clip[DSV1_SRC_LEVELS][par];
    }
    if (c->dd) {
        if ((rc = dsvg_deint_run(c->dd, st, clip, nin, c->clip[DSV1_SRC_DEINTERLACE][par]))) return rc;
        clip = c->clip[DSV1_SRC_DEINTERLACE][par];
    }
    if (c->iv) {
        if ((rc = dsvg_ivtc_run(c->iv, st, clip, c->clip[DSV1_SRC_DEINTERLACE][par]))) return rc;
        clip = c->clip[DSV1_SRC_DEINTERLACE][par];
    }
    if (c->dn) {
        if ((rc = dsvg_denoise_run(c->dn, st, clip, c->F, c->clip[DSV1_SRC_DENOISE][par]))) return rc;
        clip = c->clip[DSV1_SRC_DENOISE][par];
    }
    if (c->orn) {
        if ((rc = dsvg_orient_run(c->orn, st, clip, c->nsrc * c->F, c->clip[DSV1_SRC_ORIENT][par]))) return rc;
        clip = c->clip[DSV1_SRC_ORIENT][par];
    }
    if (c->rf) {
        if ((rc = dsvg_reframe_run(c->rf, st, clip, c->nsrc * c->F, c->clip[DSV1_SRC_REFRAME][par]))) return rc;
        clip = c->clip[DSV1_SRC_REFRAME][par];
    }
    if (c->ov) {
        if (act) {
            if (!own) {
                /* the caller's device memory is never written: a copy into a clip of the pass first */
                const size_t bytes = c->ofb * (size_t)c->nsrc * (size_t)c->F;
                if (!c->clip[DSV1_SRC_OVERLAY][par] && (rc = dsvg_lane_alloc(c->lane, &c->clip[DSV1_SRC_OVERLAY][par], bytes))) return rc;
                if ((rc = dsvg_lane_copy_dd(c->lane, c->clip[DSV1_SRC_OVERLAY][par], clip, bytes))) return rc;
                clip = c->clip[DSV1_SRC_OVERLAY][par];
            }
            if ((rc = dsvg_overlay_run(c->ov, st, par, (void *)clip, c->F, c->ov_t))) return rc;
        }
        for (s = 0; s < c->nsrc; s++) c->ov_t[s] += c->F;
    }
    *out = clip;
    return DSVG_OK;
}

int dsv1_pass_clip(int device, int kind, void *pass, int n, const dsv1_clip_io *io, int on_device)
{
    dsvg_lane *l = NULL;
    const void *din[2] = {io->in[0], io->in[1]};
    void *dout[2] = {io->out[0], io->out[1]}, *st, *d;
    int rc, k;
    if ((rc = dsvg_lane_create(&l, device))) return rc;
    st = dsvg_lane_stream(l);
    for (k = 0; !on_device && k < 2 && !rc; k++) {
        if (io->in[k] && !(rc = dsvg_lane_upload(l, k, io->in[k], io->in_bytes[k], &d))) din[k] = d;
        if (io->out[k] && !rc) rc = dsvg_lane_alloc(l, &dout[k], io->out_bytes[k]);
    }
    if (!rc)
        switch (kind) {
        case DSV1_SRC_CONVERT:     rc = dsvg_pixconv_run((dsvg_pixconv *)pass, st, din[0], n, dout[0]); break;
        case DSV1_SRC_DEINTERLACE: rc = dsvg_deint_clip((dsvg_deint *)pass, st, din[0], n, din[1], dout[0]); break;
        case DSV1_SRC_DENOISE:     rc = dsvg_denoise_clip((dsvg_denoise *)pass, st, din[0], n, din[1], dout[1], dout[0]); break;
        case DSV1_SRC_LEVELS:      rc = dsvg_levels_run((dsvg_levels *)pass, st, din[0], n, dout[0]); break;
        case DSV1_SRC_ORIENT:      rc = dsvg_orient_run((dsvg_orient *)pass, st, din[0], n, dout[0]); break;
        case DSV1_SRC_REFRAME:     rc = dsvg_reframe_run((dsvg_reframe *)pass, st, din[0], n, dout[0]); break;
        default:                   rc = dsvg_scaler_run((dsvg_scaler *)pass, st, 0, din[0], n, dout[0]); break;
        }
    for (k = 0; !on_device && k < 2 && !rc; k++)
        if (io->out[k]) rc = dsvg_lane_download(l, io->out[k], dout[k], io->out_bytes[k]);
    if (!rc) rc = dsvg_lane_sync(l);
    dsvg_lane_destroy(l);                               /* (waits for the stream; frees what the call allocated) */
    return rc;
}
