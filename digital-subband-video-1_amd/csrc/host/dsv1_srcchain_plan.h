/* dsv1_srcchain_plan.h -- private: what the source side of a session (dsv1_srcchain.c: convert -> levels -> deinterlace or inverse
 * telecine -> denoise -> orient -> reframe -> overlay) decides, in pure functions: whether a setter, a reset or a seek is taken and
 * with which text it is refused, the chain afterwards with its three geometries, the clips to allocate and to free, the histories to
 * forget, whether a lane remains; and for a call the upload, the ordered steps with their clips, and which clip comes out.  No device,
 * no chain struct, no allocation, no environment.  The chain commits and enqueues from the results; dsv1_srcchain_plan_set / _call
 * (include/dsv1_api.h) answer the same questions on plain structs.  Restated in tests/srcchain_plan.py.  The types are
 * include/dsv1_api.h's (Source chain plan).
 * EVERY RULE AND EVERY REFUSAL TEXT OF THE CHAIN IS HERE, ONCE.  Where several refusals apply the text is that of the first in this
 * order: the setting's validity, busy, exclusion by another pass (the code is DSVG_ERR_ARG for all of them). */
#ifndef DSV1_SRCCHAIN_PLAN_H
#define DSV1_SRCCHAIN_PLAN_H

#include <string.h>
#include "../../../include/dsv1_api.h"

#ifndef DSVG_OK         /* (include/dsvg.h's codes, for a program that includes this header alone) */
#define DSVG_OK        0
#define DSVG_ERR_ARG (-2)
#endif

/* the tightly packed planar frame */
static inline size_t dsv1_frame_bytes(int w, int h, int subsamp)
{
    const int hs = (subsamp >> 2) & 3, vs = subsamp & 3;
    return (size_t)w * h + 2 * (size_t)((w + (1 << hs) - 1) >> hs) * (size_t)((h + (1 << vs) - 1) >> vs);
}

/* THE REFUSAL TABLE.  The last seven rows: the setting is not one of its kind (levels have no such row: every table is a setting) */
enum { DSV1_SCT_NONE, DSV1_SCT_SOURCE, DSV1_SCT_FIELD_F, DSV1_SCT_IVTC_F, DSV1_SCT_BUSY, DSV1_SCT_NOT_SET,
       DSV1_SCT_DEINT_IVTC, DSV1_SCT_IVTC_DEINT, DSV1_SCT_REFRAME_FRONT, DSV1_SCT_REFRAME_ORIENT, DSV1_SCT_ORIENT_FRONT,
       DSV1_SCT_BAD_CONVERT, DSV1_SCT_BAD_DEINT, DSV1_SCT_BAD_IVTC, DSV1_SCT_BAD_DENOISE, DSV1_SCT_BAD_ORIENT, DSV1_SCT_BAD_REFRAME,
       DSV1_SCT_BAD_OVERLAY, DSV1_SCT_ROWS };
static inline const char *dsv1_scp_text(int row)
{
    static const char *const text[DSV1_SCT_ROWS] = {
        "",
        "no such source",
        "field rate needs an even frames_per_call",
        "inverse telecine needs a frames_per_call that is a multiple of 4",
        "not while calls are in flight or clips are staged",
        "the pass is not set",
        "a deinterlacer while an inverse telecine is set: clear it first",
        "an inverse telecine while a deinterlacer is set: clear it first",
        "a reframe while a source format, levels, a deinterlacer, an inverse telecine or a noise filter is set: clear them first, set them again after it",
        "a reframe while an orientation is set: clear it first, set it again after the reframe",
        "an orientation while a source format, levels, a deinterlacer, an inverse telecine or a noise filter is set: clear them first, set them again after it",
        "not a valid pixel or RGB format for the frames that come in",
        "not a deinterlacer (mode, field order)",
        "not an inverse telecine (field order, threshold)",
        "not a noise filter (strengths)",
        "not an orientation of this subsampling",
        "not a valid reframe onto the session's geometry",
        "not a valid list of overlays on the session's geometry",
    };
    return row >= 0 && row < DSV1_SCT_ROWS ? text[row] : NULL;
}

/* position of a kind in the chain (-1: no such kind): the deinterlacer and the inverse telecine share one */
static inline int dsv1_scp_pos(int kind)
{
    static const int pos[DSV1_SC_KINDS] = {-1, 0, 1, 2, 2, 3, 4, 5, 6};
    return kind > DSV1_SC_NONE && kind < DSV1_SC_KINDS ? pos[kind] : -1;
}
/* a request the plan answers: a pass's setter, a reset of a pass that keeps history or state, the seek of the overlays' counters */
static inline int dsv1_scp_req_ok(const dsv1_srcchain_req *q)
{
    const int k = q->kind;
    if (q->op == DSV1_SC_OP_SET) return dsv1_scp_pos(k) >= 0;
    if (q->op == DSV1_SC_OP_RESET) return k == DSV1_SC_DEINTERLACE || k == DSV1_SC_IVTC || k == DSV1_SC_DENOISE;
    return q->op == DSV1_SC_OP_SEEK && k == DSV1_SC_OVERLAY;
}
enum { DSV1_SCP_CONVERT, DSV1_SCP_LEVELS, DSV1_SCP_TEMPORAL, DSV1_SCP_DENOISE, DSV1_SCP_ORIENT, DSV1_SCP_REFRAME, DSV1_SCP_OVERLAY };

/* an orientation code of this subsampling: a transposed chroma plane is the output's only where both shifts are equal */
static inline int dsv1_scp_orient_ok(int code, int subsamp) { return code >= 0 && code < 8 && (!(code & 4) || ((subsamp >> 2) & 3) == (subsamp & 3)); }

/* THE THREE GEOMETRIES and what a call brings.  Canvas: the session's.  Oriented: the reframe's input, or the canvas.  Raw: the
 * oriented picture turned back by the inverse code, which transposes exactly when the code does. */
static inline dsv1_srcchain_geom dsv1_scp_geom(const dsv1_srcchain_state *s)
{
    dsv1_srcchain_geom g;
    const int ivtc = s->kind[DSV1_SCP_TEMPORAL] == DSV1_SC_IVTC, tr = s->kind[DSV1_SCP_ORIENT] && (s->orient & 4);
    int p;
    memset(&g, 0, sizeof(g));
    g.ow = s->ow; g.oh = s->oh;
    g.mw = s->kind[DSV1_SCP_REFRAME] ? s->in_w : s->ow; g.mh = s->kind[DSV1_SCP_REFRAME] ? s->in_h : s->oh;
    g.w = tr ? g.mh : g.mw; g.h = tr ? g.mw : g.mh;
    g.fb = dsv1_frame_bytes(g.w, g.h, s->subsamp); g.mfb = dsv1_frame_bytes(g.mw, g.mh, s->subsamp); g.ofb = dsv1_frame_bytes(g.ow, g.oh, s->subsamp);
    /* (never fewer than F in the converter's clips: a field-rate deinterlacer may be cleared behind a converter that stays) */
    g.conv_frames = ivtc ? s->F / 4 * 5 : s->F;
    g.frames_in = ivtc ? s->F / 4 * 5 : s->kind[DSV1_SCP_TEMPORAL] && s->deint_mode == DSV1_DEINT_FIELD ? s->F / 2 : s->F;
    g.frame_in_bytes = s->kind[DSV1_SCP_CONVERT] ? s->conv_fb : g.fb;
    g.bytes_in = g.frame_in_bytes * (size_t)s->nsrc * (size_t)g.frames_in;
    /* no pass, no lane: no stream, no device memory -- unless the session keeps it for its own uploads and scales */
    g.lane = s->keep_lane;
    for (p = 0; p < DSV1_SC_SLOTS; p++) g.lane |= s->kind[p] != DSV1_SC_NONE;
    return g;
}

/* bytes of each of the two clips (one per call parity) the pass at position p writes */
static inline size_t dsv1_scp_clip_bytes(const dsv1_srcchain_state *s, const dsv1_srcchain_geom *g, int p)
{
    const size_t fb = p >= DSV1_SCP_REFRAME ? g->ofb : p == DSV1_SCP_ORIENT ? g->mfb : g->fb;
    return fb * (size_t)s->nsrc * (size_t)(p <= DSV1_SCP_LEVELS ? g->conv_frames : s->F);
}

/* the first refusal that applies to a request (dsv1_scp_req_ok), in the stated order (0: it is taken) */
static inline int dsv1_scp_refusal(const dsv1_srcchain_state *s, const dsv1_srcchain_req *q)
{
    static const int bad[DSV1_SC_KINDS] = {0, DSV1_SCT_BAD_CONVERT, 0, DSV1_SCT_BAD_DEINT, DSV1_SCT_BAD_IVTC, DSV1_SCT_BAD_DENOISE, DSV1_SCT_BAD_ORIENT,
                                           DSV1_SCT_BAD_REFRAME, DSV1_SCT_BAD_OVERLAY};
    const int *K = s->kind, k = q->kind, p = dsv1_scp_pos(k);
    const int front = K[DSV1_SCP_CONVERT] || K[DSV1_SCP_LEVELS] || K[DSV1_SCP_TEMPORAL] || K[DSV1_SCP_DENOISE];
    if (q->op != DSV1_SC_OP_SET) {
        /* (a seek is taken in flight) */
        if (q->source < -1 || q->source >= s->nsrc) return DSV1_SCT_SOURCE;
        if (q->op == DSV1_SC_OP_RESET && q->busy) return DSV1_SCT_BUSY;
        return K[p] == k ? DSV1_SCT_NONE : DSV1_SCT_NOT_SET;
    }
    /* 1. validity of a setting given (the orientation's code is one even where 0 clears) */
    if (q->set && !q->valid && bad[k]) return bad[k];
    if (k == DSV1_SC_ORIENT && !dsv1_scp_orient_ok(q->mode, s->subsamp)) return bad[k];
    if (q->set && k == DSV1_SC_CONVERT && !q->frame_bytes) return bad[k];
    if (q->set && k == DSV1_SC_REFRAME && (q->out_w != s->ow || q->out_h != s->oh)) return bad[k];
    if (q->set && k == DSV1_SC_DEINTERLACE && q->mode == DSV1_DEINT_FIELD && (s->F & 1)) return DSV1_SCT_FIELD_F;
    if (q->set && k == DSV1_SC_IVTC && (s->F < 4 || s->F % 4)) return DSV1_SCT_IVTC_F;
    /* 2. busy */
    if (q->busy) return DSV1_SCT_BUSY;
    /* 3. exclusion.  The two occupants of one position exclude each other; the reframe changes the geometry every other pass but the
     * overlays resolves at, the orientation that of the passes in front of it: set, changed or CLEARED only while none of those is set */
    if (q->set && k == DSV1_SC_DEINTERLACE && K[p] == DSV1_SC_IVTC) return DSV1_SCT_DEINT_IVTC;
    if (q->set && k == DSV1_SC_IVTC && K[p] == DSV1_SC_DEINTERLACE) return DSV1_SCT_IVTC_DEINT;
    if (k == DSV1_SC_REFRAME && front) return DSV1_SCT_REFRAME_FRONT;
    if (k == DSV1_SC_REFRAME && K[DSV1_SCP_ORIENT]) return DSV1_SCT_REFRAME_ORIENT;
    if (k == DSV1_SC_ORIENT && front) return DSV1_SCT_ORIENT_FRONT;
    return DSV1_SCT_NONE;
}

/* ONE SETTER, RESET OR SEEK CALL */
static inline dsv1_srcchain_set_plan dsv1_scp_set(const dsv1_srcchain_state *s, const dsv1_srcchain_req *q)
{
    dsv1_srcchain_set_plan o;
    const int *K = s->kind, k = q->kind, p = dsv1_scp_pos(k), cf = dsv1_scp_geom(s).conv_frames;
    /* the identity of levels and reframe, and the orientation's code 0, clear the pass */
    const int set = k == DSV1_SC_ORIENT ? q->mode != 0 : q->set && !((k == DSV1_SC_LEVELS || k == DSV1_SC_REFRAME) && q->identity);
    int j;
    memset(&o, 0, sizeof(o));
    o.next = *s;
    o.g = dsv1_scp_geom(s);
    if ((o.text = dsv1_scp_refusal(s, q))) { o.rc = DSVG_ERR_ARG; return o; }
    if (q->op == DSV1_SC_OP_RESET) o.reset[p] = 1;      /* (of q->source) */
    if (q->op != DSV1_SC_OP_SET) return o;
    /* clearing the occupant that is not there while the other one is: taken, untouched */
    if (K[p] != DSV1_SC_NONE && K[p] != k) { o.noop = 1; return o; }
    if (!set && !K[p]) {
        o.noop = 1;
        /* KEPT ASYMMETRY (open): clearing a deinterlacer that is not set still forgets the noise filter's state; clearing
         * an inverse telecine that is not set does not.  Levels, as every other pass: none before, none now forgets nothing */
        if (k == DSV1_SC_DEINTERLACE && K[DSV1_SCP_DENOISE]) o.reset[DSV1_SCP_DENOISE] = 1;
        return o;
    }
    o.next.kind[p] = set ? k : DSV1_SC_NONE;
    if (k == DSV1_SC_CONVERT) { o.next.conv_rgb = set ? q->mode : 0; o.next.conv_fb = set ? q->frame_bytes : 0; }
    if (k == DSV1_SC_DEINTERLACE) o.next.deint_mode = set ? q->mode : 0;
    if (k == DSV1_SC_ORIENT) o.next.orient = q->mode;
    if (k == DSV1_SC_REFRAME) { o.next.in_w = set ? q->w : 0; o.next.in_h = set ? q->h : 0; }
    o.g = dsv1_scp_geom(&o.next);
    if (k == DSV1_SC_OVERLAY) {
        /* the pass works in place: its own clips come with the first call that needs them (dsv1_scp_call) and go with the list; a
         * new list starts every source's counter at 0 */
        o.reset[p] = set;
        for (j = 0; j < 2 && !set; j++) { o.free_[p] |= s->ov_clip[j]; o.next.ov_clip[j] = 0; }
        return o;
    }
    o.free_[p] = K[p] != DSV1_SC_NONE;
    o.alloc[p] = set ? dsv1_scp_clip_bytes(&o.next, &o.g, p) : 0;
    /* the inverse telecine changes what a call brings: the converter's and the levels' clips are allocated again in the same step */
    for (j = DSV1_SCP_CONVERT; k == DSV1_SC_IVTC && o.g.conv_frames != cf && j <= DSV1_SCP_LEVELS; j++)
        if (K[j]) { o.free_[j] = 1; o.alloc[j] = dsv1_scp_clip_bytes(&o.next, &o.g, j); }
    /* the pictures the passes behind see change meaning: behind the levels the deinterlacer's history, the inverse telecine's and the
     * noise filter's state go, behind the deinterlacer and the inverse telecine the noise filter's.  (The converter forgets nothing.) */
    if (k == DSV1_SC_LEVELS) o.reset[DSV1_SCP_TEMPORAL] = K[DSV1_SCP_TEMPORAL] != DSV1_SC_NONE;
    if (k == DSV1_SC_LEVELS || p == DSV1_SCP_TEMPORAL) o.reset[DSV1_SCP_DENOISE] = K[DSV1_SCP_DENOISE] != DSV1_SC_NONE;
    return o;
}

/* ONE CALL: a clip in `form` (0 host memory, else device memory) through the chain.  active: the overlays blend something in it */
static inline dsv1_srcchain_call_plan dsv1_scp_call(const dsv1_srcchain_state *s, int form, int active, int par)
{
    dsv1_srcchain_call_plan o;
    const dsv1_srcchain_geom g = dsv1_scp_geom(s);
    const int ov = s->kind[DSV1_SCP_OVERLAY] != DSV1_SC_NONE;
    int p, cur = DSV1_SC_CALLER, writes = 0;
    memset(&o, 0, sizeof(o));
    for (p = 0; p < DSV1_SCP_OVERLAY; p++) writes |= s->kind[p] != DSV1_SC_NONE;
    o.out = cur;
    if (!g.lane || par < 0 || par > 1) { o.rc = DSVG_ERR_ARG; return o; }
    o.advance = ov ? s->F : 0;                          /* the pictures count in every case */
    /* overlays alone at most, none active: no upload, no copy, no launch -- the clip goes on as it came (host memory stays host memory
     * unless the session keeps the lane: its scales read device memory) */
    if (!(ov && active) && !writes && (form || !s->keep_lane)) { o.bypass = 1; return o; }
    if (!form) { o.upload = g.bytes_in; cur = DSV1_SC_UPLOAD; }
    for (p = 0; p < DSV1_SCP_OVERLAY; p++) {
        dsv1_srcchain_step *st = &o.step[o.nsteps];
        if (!s->kind[p]) continue;
        st->kind = s->kind[p]; st->pos = p; st->src = cur; st->dst = cur = p;
        /* the frame-count argument: the converter and the levels take every frame of the call, the deinterlacer the frames per
         * source that come in (as the inverse telecine, which was told at its creation), the noise filter the pictures per source,
         * orientation and reframe every picture */
        st->nframes = p <= DSV1_SCP_LEVELS ? s->nsrc * g.frames_in : p == DSV1_SCP_TEMPORAL ? g.frames_in : p == DSV1_SCP_DENOISE ? s->F : s->nsrc * s->F;
        o.nsteps++;
    }
    if (ov && active) {
        dsv1_srcchain_step *st = &o.step[o.nsteps];
        if (cur == DSV1_SC_CALLER) {
            /* the caller's device memory is never written: a copy into a clip of the pass first, allocated by the first such call */
            st->kind = DSV1_SC_NONE; st->pos = DSV1_SCP_OVERLAY; st->src = cur; st->dst = cur = DSV1_SCP_OVERLAY;
            st->nframes = s->nsrc * s->F; st->bytes = dsv1_scp_clip_bytes(s, &g, DSV1_SCP_OVERLAY);
            st->alloc = s->ov_clip[par] ? 0 : st->bytes;
            o.nsteps++; st++;
        }
        st->kind = DSV1_SC_OVERLAY; st->pos = DSV1_SCP_OVERLAY; st->src = st->dst = cur; st->nframes = s->F;      /* in place */
        o.nsteps++;
    }
    o.out = cur;
    return o;
}

#endif
