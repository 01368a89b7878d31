/* dsvg_drawvec.h -- the line walk of the decoders' motion-vector overlay (drawvec dsv_decoder.c:147-182), for the host and the
 * device alike: k_drawinfo.hip walks it on the GPU, tools/drawvec_host.cpp on the CPU under a sanitizer.
 * A walk starts at the block's centre (cx, cy) and heads for (cx + mvx, cy + mvy), the vector taken raw, as pixels.  Every point from
 * the start up to, NOT including, the end point is visited; a zero vector visits the start alone.  The stepping rule is the
 * reference's: err = dx - dy, e2 = 2 err, two independent tests.  Each step moves at least one axis towards the end, so a walk takes
 * at most dx + dy <= 65 535 steps for any int16 vector, and every intermediate value fits an int.
 * dsvg_draw_vector is the whole walk of one block over a plane, with the rule that settles who wins a pixel (k_drawinfo.hip). */
#ifndef DSVG_DRAWVEC_H
#define DSVG_DRAWVEC_H
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSVG_HD __host__ __device__
#else
#define DSVG_HD
#endif

typedef struct { int x, y, x1, y1, dx, dy, sx, sy, err; } dsvg_drawvec;

DSVG_HD static inline void dsvg_drawvec_init(dsvg_drawvec *v, int cx, int cy, int mvx, int mvy)
{
    v->x = cx; v->y = cy;
    v->x1 = cx + mvx; v->y1 = cy + mvy;
    v->dx = mvx < 0 ? -mvx : mvx;
    v->dy = mvy < 0 ? -mvy : mvy;
    v->sx = cx < v->x1 ? 1 : -1;
    v->sy = cy < v->y1 ? 1 : -1;
    v->err = v->dx - v->dy;
}

/* 1: (v->x, v->y) is a point of the walk; 0: the end point is reached (it is not drawn) */
DSVG_HD static inline int dsvg_drawvec_more(const dsvg_drawvec *v) { return v->x != v->x1 || v->y != v->y1; }

DSVG_HD static inline void dsvg_drawvec_step(dsvg_drawvec *v)
{
    const int e2 = 2 * v->err;
    if (e2 > -v->dy) { v->err -= v->dy; v->x += v->sx; }
    if (e2 < v->dx) { v->err += v->dx; v->y += v->sy; }
}

/* 1: the walk is outside a w x h plane on a side it cannot come back from (it moves away from the plane on that axis, or does not move
 * on it at all), so nothing it visits from here on is inside */
DSVG_HD static inline int dsvg_drawvec_gone(const dsvg_drawvec *v, int w, int h)
{
    return (v->x < 0 && (v->sx < 0 || v->dx == 0)) || (v->x >= w && (v->sx > 0 || v->dx == 0)) ||
           (v->y < 0 && (v->sy < 0 || v->dy == 0)) || (v->y >= h && (v->sy > 0 || v->dy == 0));
}

#ifdef __cplusplus
/* the overlay's geometry: the luma plane and the blocks */
struct dsvg_drawgeo { int w, h, stride, bw, bh, nbh, nbv, mode; };

/* the four dot positions of a block at (x, y): sub-block bit k at (x + bw (1 + 2 (k & 1)) / 4, y + bh (1 + 2 (k >> 1)) / 4) */
DSVG_HD static inline int dsvg_dot_x(int x, int bw, int k) { return x + bw * ((k & 1) ? 3 : 1) / 4; }
DSVG_HD static inline int dsvg_dot_y(int y, int bh, int k) { return y + bh * ((k & 2) ? 3 : 1) / 4; }

/* does block (bi, bj) leave a 255 at (px, py)?  MV: x, y, mode (0 inter, 1 intra), submask; stable: bit 0 */
template <class MV> DSVG_HD static inline bool dsvg_marks_255(const dsvg_drawgeo &G, const MV *mv, const unsigned char *stable, int bi, int bj, int px, int py)
{
    const int b = bj * G.nbh + bi, x = bi * G.bw, y = bj * G.bh;
    if ((G.mode & 1) && (stable[b] & 1) && py == y + G.bh / 2) {
        const int k = px - (x + G.bw / 2);
        if (k >= -(G.bw / 4) && k <= G.bw / 4 && (k & 1)) return true;
    }
    if ((G.mode & 4) && mv[b].mode == 1) {
        const int sm = mv[b].submask;
        for (int k = 0; k < 4; k++)
            if (((sm >> k) & 1) && px == dsvg_dot_x(x, G.bw, k) && py == dsvg_dot_y(y, G.bh, k)) return true;
    }
    return false;
}

/* the vector of inter block b over the plane, behind the grid, dashes and dots of ALL blocks: 0 on every point of the walk inside the
 * plane, except where a LATER block (raster order) leaves a 255 -- that block draws after this one and wins.  The start is drawn even
 * by a zero vector; the end point never; at most dx + dy steps, fewer once the walk has left the plane for good. */
template <class MV> DSVG_HD static inline void dsvg_draw_vector(unsigned char *luma, const dsvg_drawgeo &G, const MV *mv, const unsigned char *stable, int b)
{
    dsvg_drawvec v;
    dsvg_drawvec_init(&v, (b % G.nbh) * G.bw + G.bw / 2, (b / G.nbh) * G.bh + G.bh / 2, mv[b].x, mv[b].y);
    for (int left = v.dx + v.dy;; left--) {
        if (v.x >= 0 && v.x < G.w && v.y >= 0 && v.y < G.h) {
            const int oi = v.x / G.bw, oj = v.y / G.bh;
            if (!(oj * G.nbh + oi > b && dsvg_marks_255(G, mv, stable, oi, oj, v.x, v.y))) luma[(size_t)v.y * G.stride + v.x] = 0;
        } else if (dsvg_drawvec_gone(&v, G.w, G.h)) break;
        if (left <= 0 || !dsvg_drawvec_more(&v)) break;
        dsvg_drawvec_step(&v);
        if (!dsvg_drawvec_more(&v)) break;
    }
}
#endif

#endif
