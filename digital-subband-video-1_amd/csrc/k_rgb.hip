// k_rgb.hip -- RGB in and out (include/dsv1_api.h, RGB; stated in numpy in tests/_rgb.py).  Two pure streaming passes, exact integers.
//
// IMPORT (k_rgb_import): 8-bit RGB frames -> tightly packed planar 8-bit Y, Cb, Cr at 4:4:4, 4:2:2 or 4:2:0, in front of the scaler /
// the frame load (it is the pass of a dsvg_pixconv, k_pixfmt.hip).  The RGB frame is read once; Y and the SUBSAMPLED chroma are written
// -- no 4:4:4 chroma plane ever exists.  blockIdx.y = frame, an item is one STEP of 16 pixels of one row, or of a row PAIR at 4:2:0, so
// that it owns whole 2x2 cells: per row 16 pixels -> 16 Y bytes and 16 Cb / Cr values that are halved over column pairs in registers
// ((a + b + 1) >> 1, rounded to 8 bits), then over the two rows (ceil((a + b) / 2) byte for byte, as k_pixout.hip).
// EXPORT (k_rgb_export): decoded frames -> RGB frames, in the place of k_pixout (launch_pixout hands an RGB format over to
// launch_rgbout): blockIdx.y = frame (through the slot table of dsvg_export_recons), an item is 16 pixels of one output row.  It
// reads 16 Y and the chroma samples the step needs -- of one chroma row, or of two for linear vertical upsampling, the far row an edge
// select of the row pointer -- upsamples and applies the Q14 matrix in registers and writes only the bytes of pixels.
//
// Both passes work on the components in MEMORY order: the host permutes the matrix columns (import) / rows (export) by the order, so
// RGB24 and BGR24, RGBA and BGRA, PLANAR_RGB and PLANAR_GBR share a kernel; ARGB / ABGR differ from RGBA / BGRA by a shift of the
// pixel's dword.
// Loads and stores: a step is 48 bytes (3-byte orders: three 16-byte accesses, de-interleaved in registers), 64 bytes (4-byte orders)
// or 16 bytes of each plane, and 16 bytes of Y and 16 or 8 of each chroma plane on the planar side.  Each of the three streams of a
// pass (RGB, Y, chroma) takes 16-byte (8 for halved chroma) accesses when every one of its rows is aligned in every frame -- decided
// on the host per stream and launch from the pointers, offsets, pitches and frame strides: uniform, no per-lane test -- and the step
// is whole (its 16 pixels exist).  Else the byte path: loads clamp the column (and the row) to the last one, which IS the repeated
// last column / row of the halving and the edge clamp of the upsampling, and stores write exactly the bytes of the pixels that
// exist.  Nothing between a row's end and its pitch, behind the planes or between frames is ever read into a result or written.
#include <algorithm>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

#define RG_THREADS 256

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

enum { RGK_P3, RGK_P4, RGK_PLANAR };

static __device__ __forceinline__ u32x4 rg_ldnt(const uint8_t *p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p)); }
static __device__ __forceinline__ u32x4 rg_ld(const uint8_t *p) { return *reinterpret_cast<const u32x4 *>(p); }
static __device__ __forceinline__ void rg_st(uint8_t *p, u32x4 v) { *reinterpret_cast<u32x4 *>(p) = v; }
static __device__ __forceinline__ int rg_clamp(int v) { return min(max(v, 0), 255); }
// (a + b + 1) >> 1 of four byte pairs
static __device__ __forceinline__ unsigned rg_avg4(unsigned a, unsigned b) { return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu); }

// ------------------------------------------------------------------------------------------------ import
struct RgbInParams {
    long long sfb, dfb;                  // frame to frame: RGB, planar
    long long soff[3], spitch[3];        // the RGB planes (packed: [0])
    long long uoff, voff;                // the chroma planes of the planar frame (Y at 0, pitch w; chroma pitch cw)
    int w, h, cw, ch;
    int k[9];                            // Q16 rows Y, Cb, Cr over the components in memory order
    int ybias;                           // (oy << 16) + 32768
    int ash;                             // 4-byte orders: the pixel's dword >> ash has the components in bytes 0..2
    int cpr, groups;                     // steps per row; rows, or row pairs at 4:2:0
    int vec_i, vec_y, vec_c;             // 16-byte path of the RGB loads, the Y stores, the chroma stores
};

// 16 pixels of row y from column x0 as c0 | c1 << 8 | c2 << 16 (memory order; bits 24..31 are not looked at)
template <int KIND> static __device__ __forceinline__ void rg_load16(const RgbInParams &P, const uint8_t *frame, int y, int x0, bool vec, unsigned px[16])
{
    const uint8_t *r0 = frame + P.soff[0] + (long long)y * P.spitch[0];
    if (KIND == RGK_P3) {
        if (vec) {
            const uint8_t *p = r0 + 3 * (long long)x0;
            const u32x4 a = rg_ldnt(p), b = rg_ldnt(p + 16), c = rg_ldnt(p + 32);
            const unsigned d[13] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, 0};
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int o = 3 * i, j = o >> 2, s = (o & 3) * 8;
                px[i] = (unsigned)(((((unsigned long long)d[j + 1]) << 32) | d[j]) >> s);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint8_t *p = r0 + 3 * (long long)min(x0 + i, P.w - 1);
                px[i] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
            }
        }
    } else if (KIND == RGK_P4) {
        if (vec) {
            const uint8_t *p = r0 + 4 * (long long)x0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const u32x4 a = rg_ldnt(p + 16 * q);
                px[4 * q] = a.x >> P.ash; px[4 * q + 1] = a.y >> P.ash; px[4 * q + 2] = a.z >> P.ash; px[4 * q + 3] = a.w >> P.ash;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {               // (the A byte is not even read)
                const uint8_t *p = r0 + 4 * (long long)min(x0 + i, P.w - 1) + (P.ash >> 3);
                px[i] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
            }
        }
    } else {
        const uint8_t *r1 = frame + P.soff[1] + (long long)y * P.spitch[1], *r2 = frame + P.soff[2] + (long long)y * P.spitch[2];
        if (vec) {
            const u32x4 a = rg_ldnt(r0 + x0), b = rg_ldnt(r1 + x0), c = rg_ldnt(r2 + x0);
            const unsigned av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int s = 8 * (i & 3);
                px[i] = ((av[i >> 2] >> s) & 0xffu) | (((bv[i >> 2] >> s) & 0xffu) << 8) | (((cv[i >> 2] >> s) & 0xffu) << 16);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int x = min(x0 + i, P.w - 1);
                px[i] = (unsigned)r0[x] | ((unsigned)r1[x] << 8) | ((unsigned)r2[x] << 16);
            }
        }
    }
}

// 16 pixels -> 16 Y bytes in yy[0..3] and their Cb / Cr bytes: all 16 in cb / cr[0..3], or halved over column pairs in [0..1]
template <int HS> static __device__ __forceinline__ void rg_row(const RgbInParams &P, const unsigned px[16], unsigned yy[4], unsigned cb[4], unsigned cr[4])
{
    const int cbias = (128 << 16) + 32768;
#pragma unroll
    for (int j = 0; j < 4; j++) yy[j] = cb[j] = cr[j] = 0;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        int Y[2], B[2], R[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int c0 = px[i + e] & 0xff, c1 = (px[i + e] >> 8) & 0xff, c2 = (px[i + e] >> 16) & 0xff;
            Y[e] = rg_clamp((P.k[0] * c0 + P.k[1] * c1 + P.k[2] * c2 + P.ybias) >> 16);
            B[e] = rg_clamp((P.k[3] * c0 + P.k[4] * c1 + P.k[5] * c2 + cbias) >> 16);
            R[e] = rg_clamp((P.k[6] * c0 + P.k[7] * c1 + P.k[8] * c2 + cbias) >> 16);
        }
        yy[i >> 2] |= ((unsigned)Y[0] << (8 * (i & 3))) | ((unsigned)Y[1] << (8 * ((i + 1) & 3)));
        if (HS) {
            const int j = i >> 1;
            cb[j >> 2] |= (unsigned)((B[0] + B[1] + 1) >> 1) << (8 * (j & 3));
            cr[j >> 2] |= (unsigned)((R[0] + R[1] + 1) >> 1) << (8 * (j & 3));
        } else {
            cb[i >> 2] |= ((unsigned)B[0] << (8 * (i & 3))) | ((unsigned)B[1] << (8 * ((i + 1) & 3)));
            cr[i >> 2] |= ((unsigned)R[0] << (8 * (i & 3))) | ((unsigned)R[1] << (8 * ((i + 1) & 3)));
        }
    }
}

// N (16 or 8) bytes held in v[] to row + x0: one store, or the first n of them byte by byte
template <int N> static __device__ __forceinline__ void rg_put(uint8_t *row, int x0, int n, bool vec, const unsigned v[4])
{
    if (vec) {
        if (N == 16) { u32x4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3]; rg_st(row + x0, o); }
        else { u32x2 o; o.x = v[0]; o.y = v[1]; *reinterpret_cast<u32x2 *>(row + x0) = o; }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) if (i < n) row[x0 + i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
    }
}

template <int KIND, int HS, int VS>
__global__ __launch_bounds__(RG_THREADS) void k_rgb_import(const RgbInParams P, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst)
{
    const int item = blockIdx.x * RG_THREADS + (int)threadIdx.x;
    const int g = item / P.cpr, c = item - g * P.cpr;
    if (g >= P.groups) return;
    const int x0 = 16 * c, n = min(16, P.w - x0);
    const bool whole = n == 16;
    const uint8_t *frame = src + (long long)blockIdx.y * P.sfb;
    uint8_t *out = dst + (long long)blockIdx.y * P.dfb;
    const int y0 = g << VS;
    unsigned px[16], yy[4], cb[4], cr[4];
    rg_load16<KIND>(P, frame, y0, x0, P.vec_i && whole, px);
    rg_row<HS>(P, px, yy, cb, cr);
    rg_put<16>(out + (long long)y0 * P.w, x0, n, P.vec_y && whole, yy);
    if (VS) {
        // the second row of the cells; beyond the frame it is the first one again -- the repeated last row of the halving
        unsigned y2[4], cb2[4], cr2[4];
        rg_load16<KIND>(P, frame, min(y0 + 1, P.h - 1), x0, P.vec_i && whole, px);
        rg_row<HS>(P, px, y2, cb2, cr2);
        if (y0 + 1 < P.h) rg_put<16>(out + (long long)(y0 + 1) * P.w, x0, n, P.vec_y && whole, y2);
#pragma unroll
        for (int j = 0; j < 4; j++) { cb[j] = rg_avg4(cb[j], cb2[j]); cr[j] = rg_avg4(cr[j], cr2[j]); }
    }
    uint8_t *urow = out + P.uoff + (long long)g * P.cw, *vrow = out + P.voff + (long long)g * P.cw;
    if (HS) {
        const int nc = min(8, P.cw - 8 * c);
        rg_put<8>(urow, 8 * c, nc, P.vec_c && whole, cb);
        rg_put<8>(vrow, 8 * c, nc, P.vec_c && whole, cr);
    } else {
        rg_put<16>(urow, x0, n, P.vec_c && whole, cb);
        rg_put<16>(vrow, x0, n, P.vec_c && whole, cr);
    }
}

template <int KIND, int HS, int VS> static void rgi_launch(const RgbInParams &P, dim3 grid, hipStream_t st, const uint8_t *src, uint8_t *dst)
{
    hipLaunchKernelGGL((k_rgb_import<KIND, HS, VS>), grid, dim3(RG_THREADS), 0, st, P, src, dst);
}

static int rgb_kind(int nplanes, int bpp) { return nplanes == 3 ? RGK_PLANAR : bpp == 3 ? RGK_P3 : RGK_P4; }

extern "C" int dsvg_rgb_import_run(void *stream, const dsv1_rgb_layout *L, const void *src_dev, int nframes, void *dst_dev)
{
    if (!L || !src_dev || !dst_dev || nframes < 1) { dsvg_set_error("bad RGB import arguments"); return DSVG_ERR_ARG; }
    if (L->hs < L->vs || L->hs > 1 || L->vs < 0) { dsvg_set_error("RGB import: subsampling not offered"); return DSVG_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    RgbInParams P;
    memset(&P, 0, sizeof P);
    P.sfb = (long long)L->frame_bytes; P.dfb = (long long)L->yuv_frame_bytes;
    P.w = L->w; P.h = L->h; P.cw = L->cw; P.ch = L->ch;
    P.uoff = (long long)L->w * L->h; P.voff = P.uoff + (long long)L->cw * L->ch;
    for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) P.k[3 * r + k] = L->fwd[3 * r + L->comp[k]];
    P.ybias = (L->oy << 16) + 32768;
    P.ash = 8 * L->first;
    P.cpr = (L->w + 15) / 16;
    P.groups = L->vs ? L->ch : L->h;
    uintptr_t ai = (uintptr_t)src_dev | (uintptr_t)P.sfb;
    for (int p = 0; p < L->nplanes; p++) { P.soff[p] = (long long)L->off[p]; P.spitch[p] = (long long)L->pitch[p]; ai |= (uintptr_t)L->off[p] | (uintptr_t)L->pitch[p]; }
    P.vec_i = !(ai & 15);
    P.vec_y = !(((uintptr_t)dst_dev | (uintptr_t)P.dfb | (uintptr_t)P.w) & 15);
    P.vec_c = !(((uintptr_t)dst_dev | (uintptr_t)P.dfb | (uintptr_t)P.uoff | (uintptr_t)P.voff | (uintptr_t)P.cw) & (L->hs ? 7 : 15));
    const long long blocks = ((long long)P.cpr * P.groups + RG_THREADS - 1) / RG_THREADS;
    if (blocks > INT_MAX / 2) { dsvg_set_error("frame too large for the RGB import's grid"); return DSVG_ERR_UNSUPPORTED; }
    const int kind = rgb_kind(L->nplanes, L->bpp), sub = L->hs + L->vs;          // 0: 4:4:4, 1: 4:2:2, 2: 4:2:0
    for (int f0 = 0; f0 < nframes; f0 += 65535) {         // (gridDim.y; one launch for any call the batches make)
        const int n = std::min(65535, nframes - f0);
        const uint8_t *s = (const uint8_t *)src_dev + (size_t)f0 * L->frame_bytes;
        uint8_t *d = (uint8_t *)dst_dev + (size_t)f0 * L->yuv_frame_bytes;
        const dim3 grid((unsigned)blocks, n);
        switch (kind * 3 + sub) {
        case RGK_P3 * 3:         rgi_launch<RGK_P3, 0, 0>(P, grid, st, s, d); break;
        case RGK_P3 * 3 + 1:     rgi_launch<RGK_P3, 1, 0>(P, grid, st, s, d); break;
        case RGK_P3 * 3 + 2:     rgi_launch<RGK_P3, 1, 1>(P, grid, st, s, d); break;
        case RGK_P4 * 3:         rgi_launch<RGK_P4, 0, 0>(P, grid, st, s, d); break;
        case RGK_P4 * 3 + 1:     rgi_launch<RGK_P4, 1, 0>(P, grid, st, s, d); break;
        case RGK_P4 * 3 + 2:     rgi_launch<RGK_P4, 1, 1>(P, grid, st, s, d); break;
        case RGK_PLANAR * 3:     rgi_launch<RGK_PLANAR, 0, 0>(P, grid, st, s, d); break;
        case RGK_PLANAR * 3 + 1: rgi_launch<RGK_PLANAR, 1, 0>(P, grid, st, s, d); break;
        default:                 rgi_launch<RGK_PLANAR, 1, 1>(P, grid, st, s, d); break;
        }
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

// ------------------------------------------------------------------------------------------------ export
struct RgbOutParams {
    long long sfb, dfb;
    long long ioff[3], ipitch[3];        // Y, Cb, Cr inside a source frame
    long long ooff[3], opitch[3];        // the RGB planes inside an output frame (packed: [0])
    int w, h, cw, ch, vs;
    int iy, oy, ku[3], kv[3];            // component k in memory order: clamp((iy (Y - oy) + ku[k] u + kv[k] v + 8192) >> 14)
    int ash;                             // 4-byte orders: the dword is (components << ash) | amask
    unsigned amask;
    int cpr;
    int vec_y, vec_c, vec_o;             // 16-byte path of the Y loads, the chroma loads (8 bytes where halved), the RGB stores
};

// the chroma samples a step needs of one plane for output row y, the vertical step done.  HS: columns c0 - 1 .. c0 + 8, clamped, in
// cv[0..9] (the two outer ones only for LINEAR); else columns c0 .. c0 + 15 in cv[0..15]
template <int HS, bool LINEAR> static __device__ __forceinline__ void ro_chroma(const RgbOutParams &P, const uint8_t *plane, long long pitch, int y, int c0, bool vec, int *cv)
{
    constexpr int N = HS ? 8 : 16, B = HS ? 1 : 0;
    const int j = y >> P.vs;
    const bool vblend = LINEAR && P.vs;
    const uint8_t *rn = plane + (long long)j * pitch, *rf = rn;
    if (vblend) rf = plane + (long long)((y & 1) ? min(j + 1, P.ch - 1) : max(j - 1, 0)) * pitch;       // edge rows: a select of the pointer
    unsigned nd[4], fd[4];
    if (vec) {
        if (HS) {
            const u32x2 a = *reinterpret_cast<const u32x2 *>(rn + c0);
            nd[0] = a.x; nd[1] = a.y;
            if (vblend) { const u32x2 b = *reinterpret_cast<const u32x2 *>(rf + c0); fd[0] = b.x; fd[1] = b.y; }
        } else {
            const u32x4 a = rg_ld(rn + c0);
            nd[0] = a.x; nd[1] = a.y; nd[2] = a.z; nd[3] = a.w;
            if (vblend) { const u32x4 b = rg_ld(rf + c0); fd[0] = b.x; fd[1] = b.y; fd[2] = b.z; fd[3] = b.w; }
        }
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int a = (nd[i >> 2] >> (8 * (i & 3))) & 0xff;
            cv[B + i] = vblend ? (3 * a + (int)((fd[i >> 2] >> (8 * (i & 3))) & 0xff) + 2) >> 2 : a;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int x = min(c0 + i, P.cw - 1);
            cv[B + i] = vblend ? (3 * (int)rn[x] + (int)rf[x] + 2) >> 2 : (int)rn[x];
        }
    }
    if (HS && LINEAR) {
        const int xl = max(c0 - 1, 0), xr = min(c0 + 8, P.cw - 1);
        cv[0] = vblend ? (3 * (int)rn[xl] + (int)rf[xl] + 2) >> 2 : (int)rn[xl];
        cv[9] = vblend ? (3 * (int)rn[xr] + (int)rf[xr] + 2) >> 2 : (int)rn[xr];
    }
}

// tab: (source frame, output frame) per blockIdx.y -- the reconstruction slot and the caller's frame index -- or null: both blockIdx.y
template <int KIND, int HS, bool LINEAR>
__global__ __launch_bounds__(RG_THREADS) void k_rgb_export(const RgbOutParams P, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int *__restrict__ tab)
{
    const int item = blockIdx.x * RG_THREADS + (int)threadIdx.x;
    const int y = item / P.cpr, c = item - y * P.cpr;
    if (y >= P.h) return;
    const int x0 = 16 * c, n = min(16, P.w - x0);
    const bool whole = n == 16;
    const long long sf = tab ? tab[2 * blockIdx.y] : (int)blockIdx.y, df = tab ? tab[2 * blockIdx.y + 1] : (int)blockIdx.y;
    const uint8_t *frame = src + sf * P.sfb;
    uint8_t *oframe = dst + df * P.dfb;
    int Y[16];
    const uint8_t *yrow = frame + P.ioff[0] + (long long)y * P.ipitch[0];
    if (P.vec_y && whole) {
        const u32x4 a = rg_ld(yrow + x0);
        const unsigned av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int i = 0; i < 16; i++) Y[i] = (av[i >> 2] >> (8 * (i & 3))) & 0xff;
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) Y[i] = yrow[min(x0 + i, P.w - 1)];
    }
    constexpr int NC = HS ? 10 : 16;
    int cu[NC], cv[NC];
    const int c0 = x0 >> HS;
    ro_chroma<HS, LINEAR>(P, frame + P.ioff[1], P.ipitch[1], y, c0, P.vec_c && whole, cu);
    ro_chroma<HS, LINEAR>(P, frame + P.ioff[2], P.ipitch[2], y, c0, P.vec_c && whole, cv);
    unsigned px[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        int u, v;
        if (!HS) { u = cu[i]; v = cv[i]; }
        else {
            const int k = i >> 1;
            u = cu[1 + k]; v = cv[1 + k];
            if (LINEAR) {
                u = (3 * u + ((i & 1) ? cu[2 + k] : cu[k]) + 2) >> 2;
                v = (3 * v + ((i & 1) ? cv[2 + k] : cv[k]) + 2) >> 2;
            }
        }
        u -= 128; v -= 128;
        const int l = P.iy * (Y[i] - P.oy) + 8192;
        const int m0 = rg_clamp((l + P.ku[0] * u + P.kv[0] * v) >> 14), m1 = rg_clamp((l + P.ku[1] * u + P.kv[1] * v) >> 14),
                  m2 = rg_clamp((l + P.ku[2] * u + P.kv[2] * v) >> 14);
        px[i] = (unsigned)m0 | ((unsigned)m1 << 8) | ((unsigned)m2 << 16);
    }
    const bool ovec = P.vec_o && whole;
    uint8_t *o0 = oframe + P.ooff[0] + (long long)y * P.opitch[0];
    if (KIND == RGK_P3) {
        if (ovec) {
            unsigned d[13];
#pragma unroll
            for (int j = 0; j < 13; j++) d[j] = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int o = 3 * i, j = o >> 2, s = (o & 3) * 8;
                const unsigned long long q = (unsigned long long)px[i] << s;
                d[j] |= (unsigned)q; d[j + 1] |= (unsigned)(q >> 32);
            }
            uint8_t *p = o0 + 3 * (long long)x0;
            u32x4 a, b, e;
            a.x = d[0]; a.y = d[1]; a.z = d[2]; a.w = d[3]; b.x = d[4]; b.y = d[5]; b.z = d[6]; b.w = d[7]; e.x = d[8]; e.y = d[9]; e.z = d[10]; e.w = d[11];
            rg_st(p, a); rg_st(p + 16, b); rg_st(p + 32, e);
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) if (i < n) {
                uint8_t *p = o0 + 3 * (long long)(x0 + i);
                p[0] = (uint8_t)px[i]; p[1] = (uint8_t)(px[i] >> 8); p[2] = (uint8_t)(px[i] >> 16);
            }
        }
    } else if (KIND == RGK_P4) {
        if (ovec) {
            uint8_t *p = o0 + 4 * (long long)x0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                u32x4 a;
                a.x = (px[4 * q] << P.ash) | P.amask; a.y = (px[4 * q + 1] << P.ash) | P.amask;
                a.z = (px[4 * q + 2] << P.ash) | P.amask; a.w = (px[4 * q + 3] << P.ash) | P.amask;
                rg_st(p + 16 * q, a);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) if (i < n) {
                uint8_t *p = o0 + 4 * (long long)(x0 + i);
                const unsigned q = (px[i] << P.ash) | P.amask;
                p[0] = (uint8_t)q; p[1] = (uint8_t)(q >> 8); p[2] = (uint8_t)(q >> 16); p[3] = (uint8_t)(q >> 24);
            }
        }
    } else {
        uint8_t *o1 = oframe + P.ooff[1] + (long long)y * P.opitch[1], *o2 = oframe + P.ooff[2] + (long long)y * P.opitch[2];
        if (ovec) {
            unsigned a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int s = 8 * (i & 3);
                a[i >> 2] |= (px[i] & 0xffu) << s; b[i >> 2] |= ((px[i] >> 8) & 0xffu) << s; e[i >> 2] |= ((px[i] >> 16) & 0xffu) << s;
            }
            rg_put<16>(o0, x0, 16, true, a); rg_put<16>(o1, x0, 16, true, b); rg_put<16>(o2, x0, 16, true, e);
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) if (i < n) {
                o0[x0 + i] = (uint8_t)px[i]; o1[x0 + i] = (uint8_t)(px[i] >> 8); o2[x0 + i] = (uint8_t)(px[i] >> 16);
            }
        }
    }
}

template <int KIND, int HS, bool LINEAR> static void rgo_launch(const RgbOutParams &P, dim3 grid, hipStream_t st, const uint8_t *src, uint8_t *dst, const int *tab)
{
    hipLaunchKernelGGL((k_rgb_export<KIND, HS, LINEAR>), grid, dim3(RG_THREADS), 0, st, P, src, dst, tab);
}

// the format against the source's planes: kernel parameters, or DSVG_ERR_ARG for a format that does not fit them (every output byte
// the kernel can write lies inside planes_bytes <= frame_bytes <= dfb)
static int rgo_params(RgbOutParams &P, int &kind, const dsvg_pixout *F, const PoSource &S, long long dfb)
{
    // memory position -> component (0 R, 1 G, 2 B), as host/dsv1_rgb.c
    static const int comp_of[8][3] = {{0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {1, 2, 0}};
    if (!F || !F->rgb.on) return DSVG_ERR_ARG;
    const dsvg_rgbout &R = F->rgb;
    if (R.order < DSV1_RGB_RGB24 || R.order > DSV1_RGB_PLANAR_GBR || (R.linear & ~1) || R.hs < R.vs || R.hs > 1 || R.vs < 0 || (R.oy != 0 && R.oy != 16)) return DSVG_ERR_ARG;
    const int nplanes = R.order >= DSV1_RGB_PLANAR_RGB ? 3 : 1, bpp = nplanes == 3 ? 1 : R.order <= DSV1_RGB_BGR24 ? 3 : 4;
    if (F->nseg != nplanes || F->planes_bytes > F->frame_bytes || dfb < (long long)F->frame_bytes) return DSVG_ERR_ARG;
    const int w = S.w[0], h = S.h[0];
    if (w < 1 || h < 1 || S.w[1] != rsu(w, R.hs) || S.w[2] != S.w[1] || S.h[1] != rsu(h, R.vs) || S.h[2] != S.h[1]) return DSVG_ERR_ARG;
    memset(&P, 0, sizeof P);
    for (int p = 0; p < nplanes; p++) {
        const dsvg_pixout_seg &G = F->seg[p];
        const size_t rowb = (size_t)w * bpp;
        if (G.kind != DSVG_PIXOUT_RGB || G.rows != h || G.width != w) return DSVG_ERR_ARG;
        if (G.pitch < rowb || G.off + G.pitch * (size_t)(h - 1) + rowb > F->planes_bytes) return DSVG_ERR_ARG;
        P.ooff[p] = (long long)G.off; P.opitch[p] = (long long)G.pitch;
    }
    for (int p = 0; p < 3; p++) { P.ioff[p] = S.off[p]; P.ipitch[p] = S.pitch[p]; }
    P.sfb = S.fb; P.dfb = dfb;
    P.w = w; P.h = h; P.cw = S.w[1]; P.ch = S.h[1]; P.vs = R.vs;
    P.iy = R.inv[0]; P.oy = R.oy;
    const int ku[3] = {0, R.inv[2], R.inv[4]}, kv[3] = {R.inv[1], R.inv[3], 0};       // R, G, B
    for (int k = 0; k < 3; k++) { P.ku[k] = ku[comp_of[R.order][k]]; P.kv[k] = kv[comp_of[R.order][k]]; }
    const bool afirst = R.order == DSV1_RGB_ARGB || R.order == DSV1_RGB_ABGR;
    P.ash = afirst ? 8 : 0;
    P.amask = bpp == 4 ? (afirst ? 0x000000ffu : 0xff000000u) : 0;
    P.cpr = (w + 15) / 16;
    if (((long long)P.cpr * h + RG_THREADS - 1) / RG_THREADS > INT_MAX / 2) { dsvg_set_error("frame too large for the RGB output pass's grid"); return DSVG_ERR_UNSUPPORTED; }
    kind = rgb_kind(nplanes, bpp);
    return DSVG_OK;
}

int rgbout_check(const dsvg_pixout *F, const PoSource &S, size_t dfb)
{
    RgbOutParams P;
    int kind;
    return rgo_params(P, kind, F, S, (long long)dfb);
}

int launch_rgbout(hipStream_t st, const dsvg_pixout *F, const PoSource &S, const uint8_t *src, const int *tab_d, int n, uint8_t *dst, size_t dfb)
{
    RgbOutParams P;
    int kind = 0;
    const int rc = rgo_params(P, kind, F, S, (long long)dfb);
    if (rc) { if (rc == DSVG_ERR_ARG) dsvg_set_error("the RGB output format does not fit the frames"); return rc; }
    const int hs = F->rgb.hs;
    P.vec_y = !(((uintptr_t)src | (uintptr_t)P.sfb | (uintptr_t)P.ioff[0] | (uintptr_t)P.ipitch[0]) & 15);
    P.vec_c = !(((uintptr_t)src | (uintptr_t)P.sfb | (uintptr_t)P.ioff[1] | (uintptr_t)P.ioff[2] | (uintptr_t)P.ipitch[1] | (uintptr_t)P.ipitch[2]) & (hs ? 7 : 15));
    uintptr_t ao = (uintptr_t)dst | (uintptr_t)P.dfb;
    for (int p = 0; p < F->nseg; p++) ao |= (uintptr_t)P.ooff[p] | (uintptr_t)P.opitch[p];
    P.vec_o = !(ao & 15);
    const int nblocks = (int)(((long long)P.cpr * P.h + RG_THREADS - 1) / RG_THREADS);
    for (int f0 = 0; f0 < n; f0 += 65535) {               // (gridDim.y; one launch for any call the decoders make)
        const int m = std::min(65535, n - f0);
        const uint8_t *s = tab_d ? src : src + (size_t)f0 * (size_t)P.sfb;
        uint8_t *d = tab_d ? dst : dst + (size_t)f0 * dfb;
        const int *t = tab_d ? tab_d + 2 * (size_t)f0 : nullptr;
        const dim3 grid(nblocks, m);
        switch (kind * 4 + hs * 2 + (F->rgb.linear ? 1 : 0)) {
        case RGK_P3 * 4:         rgo_launch<RGK_P3, 0, false>(P, grid, st, s, d, t); break;
        case RGK_P3 * 4 + 1:     rgo_launch<RGK_P3, 0, true>(P, grid, st, s, d, t); break;
        case RGK_P3 * 4 + 2:     rgo_launch<RGK_P3, 1, false>(P, grid, st, s, d, t); break;
        case RGK_P3 * 4 + 3:     rgo_launch<RGK_P3, 1, true>(P, grid, st, s, d, t); break;
        case RGK_P4 * 4:         rgo_launch<RGK_P4, 0, false>(P, grid, st, s, d, t); break;
        case RGK_P4 * 4 + 1:     rgo_launch<RGK_P4, 0, true>(P, grid, st, s, d, t); break;
        case RGK_P4 * 4 + 2:     rgo_launch<RGK_P4, 1, false>(P, grid, st, s, d, t); break;
        case RGK_P4 * 4 + 3:     rgo_launch<RGK_P4, 1, true>(P, grid, st, s, d, t); break;
        case RGK_PLANAR * 4:     rgo_launch<RGK_PLANAR, 0, false>(P, grid, st, s, d, t); break;
        case RGK_PLANAR * 4 + 1: rgo_launch<RGK_PLANAR, 0, true>(P, grid, st, s, d, t); break;
        case RGK_PLANAR * 4 + 2: rgo_launch<RGK_PLANAR, 1, false>(P, grid, st, s, d, t); break;
        default:                 rgo_launch<RGK_PLANAR, 1, true>(P, grid, st, s, d, t); break;
        }
    }
    return DSVG_OK;
}
