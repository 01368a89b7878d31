/* dsv1_srcchain.c -- the source side of a session (dsv1_host.h): convert -> levels -> deinterlace or inverse telecine -> denoise -> orient -> reframe -> overlay on one lane (dsvg_pixfmt.h), for
 * batches (dsv1_enc.c) and resolution ladders (dsv1_scale.c), and the sequence the standalone clip calls share.  The decisions are
 * dsv1_srcchain_plan.h's; here is ONE table of what differs from pass to pass (how a request's argument is read, how the pass is
 * created, destroyed, reset and run), and loops over it that commit a setter's plan and enqueue a call's. */
#include "dsv1_host.h"

/* one launch of a pass: the chain's (dsv1_srcchain_run) and the standalone clip call's (dsv1_pass_clip: src2 / dst2 are its second
 * input and output) */
typedef struct { const void *src, *src2; void *dst, *dst2; int n, par; size_t bytes; dsvg_lane *lane; const int64_t *counters; } pass_io;

/* ---- per kind: the request's argument -> the plan's numbers (valid: the kind's own check) ---- */
static void convert_resolve(const dsv1_srcchain *c, const void *arg, dsv1_srcchain_req *q)
{
    const dsv1_src_format *f = (const dsv1_src_format *)arg;
    dsv1_pix_layout L;
    dsv1_rgb_layout R;
    dsv1_hdr_layout H;
    if (f->hdr) {
        q->mode = 2;
        q->valid = (f->upsample == DSV1_CHROMA_REPLICATE || f->upsample == DSV1_CHROMA_LINEAR) && dsv1_hdr_tables_valid(f->hdr) &&
                   !dsv1_hdr_layout_of(f->pf, c->g.w, c->g.h, f->src_subsamp, c->st.subsamp, &H);
        q->frame_bytes = q->valid ? H.frame_bytes : 0;
        return;
    }
    if (!f->pf && !f->rgb) { q->set = 0; return; }
    q->mode = f->rgb != NULL;
    /* (the frames that come in: the session's geometry, or the input of the reframe set before, turned back by the orientation) */
    if (f->rgb) { q->valid = !dsv1_rgb_layout_of(f->rgb, c->g.w, c->g.h, c->st.subsamp, &R); q->frame_bytes = q->valid ? R.frame_bytes : 0; }
    else { q->valid = !dsv1_pix_layout_of(f->pf, c->g.w, c->g.h, f->src_subsamp, c->st.subsamp, &L); q->frame_bytes = q->valid ? L.frame_bytes : 0; }
}
static void levels_resolve(const dsv1_srcchain *c, const void *arg, dsv1_srcchain_req *q) { (void)c; q->identity = dsv1_levels_is_identity((const dsv1_levels *)arg); }
static void deint_resolve(const dsv1_srcchain *c, const void *arg, dsv1_srcchain_req *q)
{
    (void)c;
    q->valid = dsv1_deint_valid((const dsv1_deint *)arg); q->mode = ((const dsv1_deint *)arg)->mode;
}
static void ivtc_resolve(const dsv1_srcchain *c, const void *arg, dsv1_srcchain_req *q) { (void)c; q->valid = dsv1_ivtc_valid((const dsv1_ivtc *)arg); }
static void denoise_resolve(const dsv1_srcchain *c, const void *arg, dsv1_srcchain_req *q) { (void)c; q->valid = dsv1_denoise_valid((const dsv1_denoise *)arg); }
static void orient_resolve(const dsv1_srcchain *c, const void *arg, dsv1_srcchain_req *q) { (void)c; q->mode = *(const int *)arg; }
static void reframe_resolve(const dsv1_srcchain *c, const void *arg, dsv1_srcchain_req *q)
{
    const dsv1_reframe *rf = (const dsv1_reframe *)arg;
    q->valid = dsv1_reframe_valid(rf, c->st.subsamp);
    q->identity = dsv1_reframe_is_identity(rf);
    q->w = rf->in_w; q->h = rf->in_h; q->out_w = rf->out_w; q->out_h = rf->out_h;
}
/* (the list is checked whole before anything changes; a count out of range is an invalid list, not an empty one) */
static void overlay_resolve(const dsv1_srcchain *c, const void *arg, dsv1_srcchain_req *q)
{
    const dsv1_src_overlays *o = (const dsv1_src_overlays *)arg;
    int i;
    q->valid = o->n >= 0 && o->n <= DSV1_MAX_OVERLAYS;
    q->set = !q->valid || (o->list && o->n >= 1);
    for (i = 0; q->valid && q->set && i < o->n; i++) q->valid = dsv1_overlay_valid(&o->list[i], c->st.ow, c->st.oh, c->st.subsamp, c->st.nsrc);
}

/* ---- per kind: the pass for a setting the plan took; g: the geometry it will run at ---- */
static int convert_create(const dsv1_srcchain *c, const dsv1_srcchain_geom *g, const void *arg, void **out)
{
    const dsv1_src_format *f = (const dsv1_src_format *)arg;
    dsv1_pix_layout L;
    dsv1_rgb_layout R;
    dsv1_hdr_layout H;
    if (f->hdr)
        return dsv1_hdr_layout_of(f->pf, g->w, g->h, f->src_subsamp, c->st.subsamp, &H) ? DSVG_ERR_ARG
                                                                                        : dsvg_pixconv_create_hdr((dsvg_pixconv **)out, c->device, &H, f->hdr, f->upsample);
    if (f->rgb) return dsv1_rgb_layout_of(f->rgb, g->w, g->h, c->st.subsamp, &R) ? DSVG_ERR_ARG : dsvg_pixconv_create_rgb((dsvg_pixconv **)out, c->device, &R);
    return dsv1_pix_layout_of(f->pf, g->w, g->h, f->src_subsamp, c->st.subsamp, &L) ? DSVG_ERR_ARG : dsvg_pixconv_create((dsvg_pixconv **)out, c->device, &L);
}
static int levels_create(const dsv1_srcchain *c, const dsv1_srcchain_geom *g, const void *arg, void **out)
{
    return dsvg_levels_create((dsvg_levels **)out, c->device, (const dsv1_levels *)arg, g->w, g->h, c->st.subsamp);
}
static int deint_create(const dsv1_srcchain *c, const dsv1_srcchain_geom *g, const void *arg, void **out)
{
    return dsvg_deint_create((dsvg_deint **)out, c->device, g->w, g->h, c->st.subsamp, (const dsv1_deint *)arg, c->st.nsrc, 1);
}
static int ivtc_create(const dsv1_srcchain *c, const dsv1_srcchain_geom *g, const void *arg, void **out)
{
    return dsvg_ivtc_create((dsvg_ivtc **)out, c->device, g->w, g->h, c->st.subsamp, (const dsv1_ivtc *)arg, c->st.nsrc, g->frames_in, 1);
}
static int denoise_create(const dsv1_srcchain *c, const dsv1_srcchain_geom *g, const void *arg, void **out)
{
    return dsvg_denoise_create((dsvg_denoise **)out, c->device, g->w, g->h, c->st.subsamp, (const dsv1_denoise *)arg, c->st.nsrc, 1);
}
static int orient_create(const dsv1_srcchain *c, const dsv1_srcchain_geom *g, const void *arg, void **out)
{
    return dsvg_orient_create((dsvg_orient **)out, c->device, *(const int *)arg, g->w, g->h, c->st.subsamp);
}
static int reframe_create(const dsv1_srcchain *c, const dsv1_srcchain_geom *g, const void *arg, void **out)
{
    (void)g;
    return dsvg_reframe_create((dsvg_reframe **)out, c->device, (const dsv1_reframe *)arg, c->st.subsamp);
}
static int overlay_create(const dsv1_srcchain *c, const dsv1_srcchain_geom *g, const void *arg, void **out)
{
    const dsv1_src_overlays *o = (const dsv1_src_overlays *)arg;
    return dsvg_overlay_create((dsvg_overlay **)out, c->device, o->list, o->n, g->ow, g->oh, c->st.subsamp, c->st.nsrc);
}

/* ---- per kind: thin adaptors over the passes' differing signatures (dsvg_pixfmt.h) ---- */
static void convert_destroy(void *p) { dsvg_pixconv_destroy((dsvg_pixconv *)p); }
static void levels_destroy(void *p) { dsvg_levels_destroy((dsvg_levels *)p); }
static void deint_destroy(void *p) { dsvg_deint_destroy((dsvg_deint *)p); }
static void ivtc_destroy(void *p) { dsvg_ivtc_destroy((dsvg_ivtc *)p); }
static void denoise_destroy(void *p) { dsvg_denoise_destroy((dsvg_denoise *)p); }
static void orient_destroy(void *p) { dsvg_orient_destroy((dsvg_orient *)p); }
static void reframe_destroy(void *p) { dsvg_reframe_destroy((dsvg_reframe *)p); }
static void overlay_destroy(void *p) { dsvg_overlay_destroy((dsvg_overlay *)p); }
static int deint_reset(void *p, int source) { return dsvg_deint_reset((dsvg_deint *)p, source); }
static int ivtc_reset(void *p, int source) { return dsvg_ivtc_reset((dsvg_ivtc *)p, source); }
static int denoise_reset(void *p, int source) { return dsvg_denoise_reset((dsvg_denoise *)p, source); }
static int copy_run(void *p, void *st, const pass_io *io) { (void)p; (void)st; return dsvg_lane_copy_dd(io->lane, io->dst, io->src, io->bytes); }
static int convert_run(void *p, void *st, const pass_io *io) { return dsvg_pixconv_run((dsvg_pixconv *)p, st, io->src, io->n, io->dst); }
static int levels_run(void *p, void *st, const pass_io *io) { return dsvg_levels_run((dsvg_levels *)p, st, io->src, io->n, io->dst); }
static int deint_run(void *p, void *st, const pass_io *io) { return dsvg_deint_run((dsvg_deint *)p, st, io->src, io->n, io->dst); }
static int deint_clip(void *p, void *st, const pass_io *io) { return dsvg_deint_clip((dsvg_deint *)p, st, io->src, io->n, io->src2, io->dst); }
static int ivtc_run(void *p, void *st, const pass_io *io) { return dsvg_ivtc_run((dsvg_ivtc *)p, st, io->src, io->dst); }
static int denoise_run(void *p, void *st, const pass_io *io) { return dsvg_denoise_run((dsvg_denoise *)p, st, io->src, io->n, io->dst); }
static int denoise_clip(void *p, void *st, const pass_io *io) { return dsvg_denoise_clip((dsvg_denoise *)p, st, io->src, io->n, io->src2, io->dst2, io->dst); }
static int orient_run(void *p, void *st, const pass_io *io) { return dsvg_orient_run((dsvg_orient *)p, st, io->src, io->n, io->dst); }
static int reframe_run(void *p, void *st, const pass_io *io) { return dsvg_reframe_run((dsvg_reframe *)p, st, io->src, io->n, io->dst); }
static int overlay_run(void *p, void *st, const pass_io *io) { return dsvg_overlay_run((dsvg_overlay *)p, st, io->par, io->dst, io->n, io->counters); }
static int scale_clip(void *p, void *st, const pass_io *io) { return dsvg_scaler_run((dsvg_scaler *)p, st, 0, io->src, io->n, io->dst); }

/* THE TABLE, by kind (DSV1_SRC_*; row 0: a call's device-to-device copy, dsv1_scp_call).  run: within a chain; clip: the standalone
 * clip call (NULL: there is none of this kind through dsv1_pass_clip) */
static const struct {
    void (*resolve)(const dsv1_srcchain *c, const void *arg, dsv1_srcchain_req *q);
    int  (*create)(const dsv1_srcchain *c, const dsv1_srcchain_geom *g, const void *arg, void **out);
    void (*destroy)(void *pass);
    int  (*reset)(void *pass, int source);
    int  (*run)(void *pass, void *stream, const pass_io *io);
    int  (*clip)(void *pass, void *stream, const pass_io *io);
} ops[DSV1_SRC_SCALE + 1] = {
    /* (copy)      */ {NULL, NULL, NULL, NULL, copy_run, NULL},
    /* CONVERT     */ {convert_resolve, convert_create, convert_destroy, NULL, convert_run, convert_run},
    /* LEVELS      */ {levels_resolve, levels_create, levels_destroy, NULL, levels_run, levels_run},
    /* DEINTERLACE */ {deint_resolve, deint_create, deint_destroy, deint_reset, deint_run, deint_clip},
    /* IVTC        */ {ivtc_resolve, ivtc_create, ivtc_destroy, ivtc_reset, ivtc_run, NULL},
    /* DENOISE     */ {denoise_resolve, denoise_create, denoise_destroy, denoise_reset, denoise_run, denoise_clip},
    /* ORIENT      */ {orient_resolve, orient_create, orient_destroy, NULL, orient_run, orient_run},
    /* REFRAME     */ {reframe_resolve, reframe_create, reframe_destroy, NULL, reframe_run, reframe_run},
    /* OVERLAY     */ {overlay_resolve, overlay_create, overlay_destroy, NULL, overlay_run, NULL},
    /* SCALE       */ {NULL, NULL, NULL, NULL, NULL, scale_clip},
};

void dsv1_srcchain_init(dsv1_srcchain *c, int device, int w, int h, int subsamp, int nsrc, int F, int keep_lane)
{
    memset(c, 0, sizeof(*c));
    c->device = device;
    c->st.ow = w; c->st.oh = h; c->st.subsamp = subsamp; c->st.nsrc = nsrc; c->st.F = F; c->st.keep_lane = keep_lane;
    c->g = dsv1_scp_geom(&c->st);
}

int dsv1_srcchain_lane(dsv1_srcchain *c) { return c->lane ? DSVG_OK : dsvg_lane_create(&c->lane, c->device); }

/* a lane the chain's state does not need goes */
static void chain_release(dsv1_srcchain *c)
{
    if (c->g.lane) return;
    dsvg_lane_destroy(c->lane);
    c->lane = NULL;
}

void dsv1_srcchain_close(dsv1_srcchain *c)
{
    int p;
    if (c->lane) (void)dsvg_lane_sync(c->lane);        /* (the passes' kernels read the memory their destroy frees) */
    for (p = 0; p < DSV1_SC_SLOTS; p++)
        if (c->pass[p]) ops[c->st.kind[p]].destroy(c->pass[p]);
    free(c->ov_t);
    dsvg_lane_destroy(c->lane);                         /* (and the clips) */
    memset(c, 0, sizeof(*c));
}

/* what the plan of a taken setter says, all or nothing: the new clips first, then the wait for the lane (the old pass's launches read
 * its memory), then the histories to forget, and only then the commit, which cannot fail: the pass at pos becomes `pass`, the clips
 * marked go, the new ones take their place.  On an error the passes, clips and geometries are as they were and `pass` is still the
 * caller's; a history forgotten before a later one failed stays forgotten (nothing is in flight that could tell), and a lane nothing
 * needs is released. */
static int chain_commit(dsv1_srcchain *c, const dsv1_srcchain_set_plan *P, int pos, void *pass)
{
    void *clip[DSV1_SC_SLOTS][2];
    int rc = DSVG_OK, p, j, work = !P->noop;
    memset(clip, 0, sizeof(clip));
    for (p = 0; p < DSV1_SC_SLOTS; p++) work |= P->reset[p];
    if (!work) return DSVG_OK;
    if (P->g.lane) rc = dsv1_srcchain_lane(c);
    for (p = 0; p < DSV1_SC_SLOTS; p++)
        for (j = 0; j < 2 && P->alloc[p] && !rc; j++) rc = dsvg_lane_alloc(c->lane, &clip[p][j], P->alloc[p]);
    if (!rc && P->reset[DSV1_SCP_OVERLAY] && !c->ov_t && !(c->ov_t = (int64_t *)calloc((size_t)c->st.nsrc, sizeof(*c->ov_t)))) rc = DSVG_ERR_NOMEM;
    if (!rc && c->lane) rc = dsvg_lane_sync(c->lane);
    for (p = 0; p < DSV1_SCP_OVERLAY && !rc; p++)
        if (P->reset[p]) rc = ops[c->st.kind[p]].reset(c->pass[p], -1);
    if (rc) {
        for (p = 0; c->lane && p < DSV1_SC_SLOTS; p++)
            for (j = 0; j < 2; j++) (void)dsvg_lane_free(c->lane, clip[p][j]);
        chain_release(c);
        return rc;
    }
    if (!P->noop) {
        if (c->pass[pos]) ops[c->st.kind[pos]].destroy(c->pass[pos]);
        c->pass[pos] = pass;
    }
    for (p = 0; p < DSV1_SC_SLOTS; p++)
        for (j = 0; j < 2 && (P->free_[p] || P->alloc[p]); j++) {
            (void)dsvg_lane_free(c->lane, c->clip[p][j]);
            c->clip[p][j] = clip[p][j];
        }
    if (P->reset[DSV1_SCP_OVERLAY]) memset(c->ov_t, 0, sizeof(*c->ov_t) * (size_t)c->st.nsrc);
    c->st = P->next;
    c->g = P->g;
    chain_release(c);
    return DSVG_OK;
}

static int chain_refused(const char *who, const dsv1_srcchain_set_plan *P)
{
    dsv1_log(1, "%s: %s", who, dsv1_scp_text(P->text));
    return P->rc;
}

int dsv1_srcchain_request(dsv1_srcchain *c, const char *who, int busy, int kind, const void *arg)
{
    dsv1_srcchain_req q;
    dsv1_srcchain_set_plan P;
    void *pass = NULL;
    int rc;
    memset(&q, 0, sizeof(q));
    q.op = DSV1_SC_OP_SET; q.kind = kind; q.busy = busy; q.set = arg != NULL; q.valid = 1;
    if (arg) ops[kind].resolve(c, arg, &q);
    P = dsv1_scp_set(&c->st, &q);
    if (P.rc) return chain_refused(who, &P);
    if (P.next.kind[dsv1_scp_pos(kind)] == kind && !P.noop && (rc = ops[kind].create(c, &P.g, arg, &pass))) return rc;
    if ((rc = chain_commit(c, &P, dsv1_scp_pos(kind), pass)) && pass) ops[kind].destroy(pass);
    return rc;
}

int dsv1_srcchain_signal(dsv1_srcchain *c, const char *who, int busy, int op, int kind, int source, int64_t t)
{
    dsv1_srcchain_req q;
    dsv1_srcchain_set_plan P;
    int s;
    memset(&q, 0, sizeof(q));
    q.op = op; q.kind = kind; q.busy = busy; q.source = source;
    P = dsv1_scp_set(&c->st, &q);
    if (P.rc) return chain_refused(who, &P);
    if (op == DSV1_SC_OP_RESET) return ops[kind].reset(c->pass[dsv1_scp_pos(kind)], source);
    for (s = 0; s < c->st.nsrc; s++)
        if (source < 0 || source == s) c->ov_t[s] = t;
    return DSVG_OK;
}

int dsv1_srcchain_run(dsv1_srcchain *c, int par, const void *clip, int on_device, const void **out)
{
    dsv1_srcchain_call_plan P;
    void *up = NULL, *st;
    int rc, i, s;
    if (!c->lane || !clip || !out) return DSVG_ERR_ARG;
    /* (active: the items the overlays would blend in this call) */
    P = dsv1_scp_call(&c->st, on_device, c->pass[DSV1_SCP_OVERLAY] && dsvg_overlay_active((dsvg_overlay *)c->pass[DSV1_SCP_OVERLAY], c->st.F, c->ov_t) != 0, par);
    if (P.rc) return P.rc;
    st = dsvg_lane_stream(c->lane);
    if (P.upload && (rc = dsvg_lane_upload(c->lane, par, clip, P.upload, &up))) return rc;
    for (i = 0; i < P.nsteps; i++) {
        const dsv1_srcchain_step *S = &P.step[i];
        pass_io io = {S->src == DSV1_SC_CALLER ? clip : S->src == DSV1_SC_UPLOAD ? up : c->clip[S->src][par], NULL, NULL, NULL, S->nframes, par, S->bytes, c->lane, c->ov_t};
        if (S->alloc) {
            if ((rc = dsvg_lane_alloc(c->lane, &c->clip[S->dst][par], S->alloc))) return rc;
            c->st.ov_clip[par] = 1;
        }
        io.dst = S->dst == DSV1_SC_UPLOAD ? up : c->clip[S->dst][par];
        if ((rc = ops[S->kind].run(c->pass[S->pos], st, &io))) return rc;
    }
    for (s = 0; s < c->st.nsrc && P.advance; s++) c->ov_t[s] += P.advance;
    *out = P.out == DSV1_SC_CALLER ? clip : P.out == DSV1_SC_UPLOAD ? up : c->clip[P.out][par];
    return DSVG_OK;
}

int dsv1_srcchain_plan_set(const dsv1_srcchain_state *s, const dsv1_srcchain_req *q, dsv1_srcchain_set_plan *out)
{
    if (!s || !q || !out || !dsv1_scp_req_ok(q)) return DSVG_ERR_ARG;
    *out = dsv1_scp_set(s, q);
    return out->rc;
}
int dsv1_srcchain_plan_call(const dsv1_srcchain_state *s, int form, int active, int par, dsv1_srcchain_call_plan *out)
{
    if (!s || !out || form < 0 || form > DSV1_CLIP_HELD) return DSVG_ERR_ARG;
    *out = dsv1_scp_call(s, form, active, par);
    return out->rc;
}
const char *dsv1_srcchain_plan_text(int row) { return dsv1_scp_text(row); }

int dsv1_pass_clip(int device, int kind, void *pass, int n, const dsv1_clip_io *io, int on_device)
{
    dsvg_lane *l = NULL;
    pass_io p = {io->in[0], io->in[1], io->out[0], io->out[1], n, 0, 0, NULL, NULL};
    void *st, *d;
    int rc, k;
    if (kind < 0 || kind > DSV1_SRC_SCALE || !ops[kind].clip) return DSVG_ERR_ARG;
    if ((rc = dsvg_lane_create(&l, device))) return rc;
    st = dsvg_lane_stream(l);
    for (k = 0; !on_device && k < 2 && !rc; k++) {
        if (io->in[k] && !(rc = dsvg_lane_upload(l, k, io->in[k], io->in_bytes[k], &d))) *(k ? &p.src2 : &p.src) = d;
        if (io->out[k] && !rc) rc = dsvg_lane_alloc(l, k ? &p.dst2 : &p.dst, io->out_bytes[k]);
    }
    if (!rc) rc = ops[kind].clip(pass, st, &p);
    for (k = 0; !on_device && k < 2 && !rc; k++)
        if (io->out[k]) rc = dsvg_lane_download(l, io->out[k], k ? p.dst2 : p.dst, io->out_bytes[k]);
    if (!rc) rc = dsvg_lane_sync(l);
    dsvg_lane_destroy(l);                               /* (waits for the stream; frees what the call allocated) */
    return rc;
}
