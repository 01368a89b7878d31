// k_drawinfo.hip -- the decoders' debug overlay (draw_info / drawvec dsv_decoder.c:147-243; stated in Python in tests/_drawinfo.py): the
// block grid, a dash in stable blocks, the motion vector of inter blocks and a dot per intra sub-block, drawn onto the luma planes of n
// pictures of one geometry in device memory -- reconstructions of a decoder context, or tightly packed planar frames.
//
// The reference walks the blocks in raster order and the last writer of a pixel wins.  Grid, dashes and dots of a block lie inside the
// block's own area (block sizes are 16 or more: the dash keeps bw/4 columns from the block's left edge, the dots a quarter) and never
// on one another, so they can be written in any order: k_draw_marks, a 64-lane workgroup per block.  The vectors (0) can cross the
// 255-pixels of any block: the odd pixels of a dash and the dots.  Such a pixel belongs to exactly one block, found from its
// coordinates, and whether that block draws a 255 there is read from the block's table entry.  A vector of block v loses against the
// 255 of block b exactly when b comes later in raster order (b > v; b == v is the block's own dash, drawn before its vector), so
// k_draw_vectors -- a thread per block, launched behind k_draw_marks -- leaves those pixels alone and writes 0 everywhere else it
// passes.  Several vectors over one pixel all write 0.  No scratch plane, no atomics.
//
// Every store is predicated on lying inside the plane; unlike the reference (whose dots are not bounds-checked) a dot outside the plane
// is not drawn.  The walk is dsvg_drawvec.h's: at most dx + dy <= 65 535 steps for any int16 vector, and a walk that has left the plane
// for good stops.
#include <algorithm>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"
#include "dsvg_drawvec.h"

#define DRAW_STABHQ 1                // DSV_DRAW_* dsv_decoder.h
#define DRAW_MOVECS 2
#define DRAW_IBLOCK 4

struct DrawGeo : dsvg_drawgeo {
    size_t pic_pitch;                // bytes from one picture's luma plane to the next one's
};

__global__ __launch_bounds__(64) void k_draw_marks(uint8_t *__restrict__ luma0, DrawGeo G, const DMV *__restrict__ mvs, const uint8_t *__restrict__ stable)
{
    const int nblk = G.nbh * G.nbv;
    const int pic = blockIdx.y, b = blockIdx.x;
    if (b >= nblk) return;
    const int bi = b % G.nbh, bj = b / G.nbh, x = bi * G.bw, y = bj * G.bh, t = threadIdx.x;
    uint8_t *luma = luma0 + (size_t)pic * G.pic_pitch;
    const DMV mv = mvs[(size_t)pic * nblk + b];
    const int st = stable[(size_t)pic * nblk + b];
    if (x >= G.w || y >= G.h) return;                               // (nbh = ceil(w / bw), nbv = ceil(h / bh): never)
    for (int i = x + t; i < x + G.bw && i < G.w; i += 64) luma[(size_t)y * G.stride + i] = 0;      // the block's part of grid row y
    for (int k = y + t; k < y + G.bh && k < G.h; k += 64) luma[(size_t)k * G.stride + x] = 0;      // grid column x
    if ((G.mode & DRAW_STABHQ) && (st & 1)) {
        const int a = x + G.bw / 2, r = y + G.bh / 2, q = G.bw / 4;
        for (int k = -q + t; k <= q; k += 64)
            if (r < G.h && a + k >= 0 && a + k < G.w) luma[(size_t)r * G.stride + a + k] = (uint8_t)((k & 1) * 255);
    }
    if ((G.mode & DRAW_IBLOCK) && mv.mode == 1 && t < 4 && ((mv.submask >> t) & 1)) {
        const int a = dsvg_dot_x(x, G.bw, t), r = dsvg_dot_y(y, G.bh, t);
        if (a < G.w && r < G.h) luma[(size_t)r * G.stride + a] = 255;
    }
}

__global__ __launch_bounds__(64) void k_draw_vectors(uint8_t *__restrict__ luma0, DrawGeo G, const DMV *__restrict__ mvs, const uint8_t *__restrict__ stable)
{
    const int nblk = G.nbh * G.nbv;
    const int pic = blockIdx.y, b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nblk) return;
    const DMV *mv = mvs + (size_t)pic * nblk;
    const uint8_t *stb = stable + (size_t)pic * nblk;
    if (mv[b].mode != 0) return;
    dsvg_draw_vector(luma0 + (size_t)pic * G.pic_pitch, G, mv, stb, b);
}

void launch_drawinfo(hipStream_t st, uint8_t *luma0, size_t pic_pitch, int w, int h, int stride, int bw, int bh, int mode,
                     const DMV *mvs, const uint8_t *stable, int n)
{
    DrawGeo G;
    G.w = w; G.h = h; G.stride = stride;
    G.bw = bw; G.bh = bh; G.nbh = (w + bw - 1) / bw; G.nbv = (h + bh - 1) / bh; G.mode = mode;
    G.pic_pitch = pic_pitch;
    const int nblk = G.nbh * G.nbv;
    for (int f0 = 0; f0 < n; f0 += 65535) {              // (gridDim.y)
        const int m = std::min(65535, n - f0);
        uint8_t *l0 = luma0 + (size_t)f0 * pic_pitch;
        const DMV *mv = mvs + (size_t)f0 * nblk;
        const uint8_t *sb = stable + (size_t)f0 * nblk;
        hipLaunchKernelGGL(k_draw_marks, dim3(nblk, m), dim3(64), 0, st, l0, G, mv, sb);
        if (mode & DRAW_MOVECS) hipLaunchKernelGGL(k_draw_vectors, dim3((nblk + 63) / 64, m), dim3(64), 0, st, l0, G, mv, sb);
    }
}

// n tightly packed planar frames, drawn in place: device pointers, or host memory staged on a lane of the call's own.  Synchronous.
extern "C" int dsvg_draw_info_planar(int device, void *clip, int w, int h, int subsamp, int n, int blk_w, int blk_h, const dsvg_mv *mvs,
                                     const unsigned char *stable, int mode, int on_device)
{
    if (!clip || !mvs || !stable || w < 1 || h < 1 || n < 1 || device < 0 || mode < 1 || mode > 7 || blk_w < 16 || blk_w > 64 || blk_h < 16 || blk_h > 64 ||
        (subsamp != 0x0 && subsamp != 0x4 && subsamp != 0x5 && subsamp != 0x8)) { dsvg_set_error("bad draw_info arguments"); return DSVG_ERR_ARG; }
    const size_t fb = (size_t)w * h + 2 * (size_t)rsu(w, fmt_hs(subsamp)) * rsu(h, fmt_vs(subsamp));
    const size_t nblk = (size_t)((w + blk_w - 1) / blk_w) * ((h + blk_h - 1) / blk_h);
    dsvg_lane *l = nullptr;
    int rc = dsvg_lane_create(&l, device);
    if (rc) return rc;
    void *d = clip, *mv_d = nullptr, *st_d = nullptr;
    if (!on_device) rc = dsvg_lane_upload(l, 0, clip, fb * n, &d);
    if (!rc) rc = dsvg_lane_alloc(l, &mv_d, nblk * n * sizeof(DMV));
    if (!rc) rc = dsvg_lane_alloc(l, &st_d, nblk * n);
    hipStream_t st = (hipStream_t)dsvg_lane_stream(l);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(mv_d, mvs, nblk * n * sizeof(DMV), hipMemcpyHostToDevice, st);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(st_d, stable, nblk * n, hipMemcpyHostToDevice, st);
    if (!rc && e == hipSuccess) {
        launch_drawinfo(st, (uint8_t *)d, fb, w, h, w, blk_w, blk_h, mode, (const DMV *)mv_d, (const uint8_t *)st_d, n);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { dsvg_set_error("the overlay could not be drawn: %s", hipGetErrorString(e)); rc = DSVG_ERR_HIP; }
    if (!rc && !on_device) rc = dsvg_lane_download(l, clip, d, fb * n);
    if (!rc) rc = dsvg_lane_sync(l);                     // (the tables are pageable: the copies above were staged inside the calls)
    dsvg_lane_destroy(l);
    return rc;
}
