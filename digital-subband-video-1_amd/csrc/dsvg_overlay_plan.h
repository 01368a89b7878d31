/* dsvg_overlay_plan.h -- private: what a call of the overlay pass (include/dsv1_api.h, Overlays; k_overlay.hip) does, decided in pure
 * functions: whether a placement is valid, the opacity of a picture, and the items of a call with their layers.  No device, no
 * allocation, no state; read by the C session layer and by the HIP plumbing, as dsvg_batch_plan.h is.  Stated in numpy in
 * tests/_overlay.py. */
#ifndef DSVG_OVERLAY_PLAN_H
#define DSVG_OVERLAY_PLAN_H

#include "../../include/dsv1_api.h"

static inline int dsvg_overlay_subsamp_known(int subsamp)
{
    return subsamp == DSV_SUBSAMP_444 || subsamp == DSV_SUBSAMP_422 || subsamp == DSV_SUBSAMP_420 || subsamp == DSV_SUBSAMP_411;
}

/* VALID: 1 / 0 for a placement on a canvas of W x H at `subsamp` in a session of S sources */
static inline int dsvg_overlay_valid(const dsv1_overlay *ov, int W, int H, int subsamp, int S)
{
    int hs, vs;
    if (!ov || !dsvg_overlay_subsamp_known(subsamp) || W < 1 || H < 1 || S < 1) return 0;
    hs = (subsamp >> 2) & 3; vs = subsamp & 3;
    if (!ov->planes || ov->reserved != 0) return 0;
    if (ov->w < 1 || ov->h < 1 || ov->x < 0 || ov->y < 0) return 0;
    if (ov->w > W || ov->x > W - ov->w || ov->h > H || ov->y > H - ov->h) return 0;
    if ((ov->x & ((1 << hs) - 1)) || (ov->y & ((1 << vs) - 1))) return 0;
    if (ov->opacity < 0 || ov->opacity > 256) return 0;
    if (ov->source < -1 || ov->source >= S) return 0;
    return 1;
}

/* the opacity of picture t, 0 .. 256: r(opacity a b / ((fade_in + 1) (fade_out + 1))), half up; every difference is taken where it
 * cannot wrap */
static inline int dsvg_overlay_opacity_at(const dsv1_overlay *ov, int64_t t)
{
    uint64_t d, a, b, den;
    if (t < ov->t0) return 0;
    d = (uint64_t)t - (uint64_t)ov->t0;                 /* pictures since the first: exact, t >= t0 */
    if (ov->dur && d >= ov->dur) return 0;
    a = (d < ov->fade_in ? d : ov->fade_in) + 1;
    b = (uint64_t)ov->fade_out + 1;
    if (ov->dur && ov->dur - d < b) b = ov->dur - d;
    den = ((uint64_t)ov->fade_in + 1) * ((uint64_t)ov->fade_out + 1);
    return (int)((2 * (uint64_t)ov->opacity * a * b + den) / (2 * den));
}

/* The items of a call: every (overlay, source, frame) with op > 0, in the order source, frame, overlay -- so the items of one picture
 * lie together in list order, which is the order they composite in.  layer = 1 + the largest layer of an earlier item of the same
 * picture whose luma rectangle intersects, 1 where there is none: items of one layer never touch the same byte (x, y are aligned to
 * the subsampling, so rectangles disjoint in luma are disjoint in chroma) and layer k reads what layers < k wrote.
 * counters[s] is the picture source s's first frame of the call is.  Returns the number of items; the first `room` of them are
 * written (items may be NULL with room 0: a count).  *nlayers: the largest layer among ALL of them when everything was written, else
 * untouched. */
static inline long long dsvg_overlay_plan(const dsv1_overlay *list, int n, int S, int F, const int64_t *counters, dsv1_overlay_item *items,
                                          long long room, int *nlayers)
{
    long long cnt = 0;
    int s, f, i, top = 0;
    for (s = 0; s < S; s++)
        for (f = 0; f < F; f++) {
            const long long first = cnt;
            const int64_t t = counters[s] + f;
            for (i = 0; i < n; i++) {
                const dsv1_overlay *o = &list[i];
                long long j;
                int op, layer = 1;
                if (o->source != -1 && o->source != s) continue;
                if (!(op = dsvg_overlay_opacity_at(o, t))) continue;
                if (cnt < room) {
                    for (j = first; j < cnt; j++) {
                        const dsv1_overlay *e = &list[items[j].overlay];
                        if (items[j].layer >= layer && e->x < o->x + o->w && o->x < e->x + e->w && e->y < o->y + o->h && o->y < e->y + e->h)
                            layer = items[j].layer + 1;
                    }
                    items[cnt].overlay = i; items[cnt].source = s; items[cnt].frame = f; items[cnt].op = op; items[cnt].layer = layer;
                    if (layer > top) top = layer;
                }
                cnt++;
            }
        }
    if (nlayers && cnt <= room) *nlayers = top;
    return cnt;
}

#endif
