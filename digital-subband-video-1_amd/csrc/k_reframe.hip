// k_reframe.hip -- the reframe pass and the line sums (include/dsv1_api.h, Reframe; stated in numpy in tests/_reframe.py): tightly
// packed planar 8-bit frames in, frames of another geometry out -- a window of the picture placed on a canvas, a fill colour
// elsewhere -- and, as a call of its own, the sums of every luma row and column of a clip.
//
// k_reframe: one launch covers every frame (blockIdx.y) and the three planes of a clip (blockIdx.x: the planes' blocks one after the
// other, so a block's plane is uniform).  An item is one 16-byte ALIGNED chunk of one output row: tight pitches with odd widths give
// every row its own alignment, so a row's chunks are counted from its address rounded down to 16, the first and the last of them
// may be partial, and cpr = (OW + 30) / 16 items cover any row.  A whole chunk is one 16-byte store of
//   the fill word                                  -- a row above or below the window, a chunk left or right of it;
//   16 source bytes, ONE unaligned 16-byte load    -- a chunk inside the window: the source is off the destination's alignment by
//                                                     (X0 - DX) plus the rows' pitch difference, any value mod 16, and the load
//                                                     names exactly the 16 window samples, so nothing outside the frames is read;
//   bytes picked one by one                        -- the at most two chunks of a row that hold a window edge.
// A partial chunk (a row's head and tail) stores its bytes one by one.  Every output byte is written exactly once and no byte
// outside the output frames is written; only window samples are loaded.
//
// k_line_sums: one read of the luma gives both sums.  A block is 32 rows of the picture, a wave 8 of them, over the whole width in
// strips of 256 columns (a lane: 4 columns, one unaligned dword).  A row's sum is accumulated per lane over the strips (v_sad_u8),
// reduced over the wave with DPP and stored once.  A lane keeps the sums of its 4 columns over the wave's 8 rows in registers; the
// block's four waves are combined through LDS and added with ONE integer atomicAdd per column and block into the zeroed array:
// integer sums are exact in any order, so the result does not depend on the grid or on the order the blocks arrive in.
#include <algorithm>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

#define RF_THREADS 256
#define LS_THREADS 256
#define LS_WAVE_ROWS 8
#define LS_BLOCK_ROWS (LS_WAVE_ROWS * LS_THREADS / 64)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4a1 __attribute__((ext_vector_type(4), aligned(1)));       // 16 bytes at any address
typedef unsigned u32a1 __attribute__((aligned(1)));

struct RfPlane {
    int OW, OH, cpr, block0;             // the canvas plane; chunks per row; first block of the plane in blockIdx.x
    int DX, DY, W, H;                    // the window on the canvas plane
    int X0, Y0, IW;                      // its top left in the input plane; the input plane's width
    unsigned fill;                       // the fill byte in all four bytes
    long long ioff, ooff;                // the plane inside an input / output frame
};
struct RfParams {
    RfPlane pl[3];
    long long ifb, ofb;                  // frame bytes in and out
};

__global__ __launch_bounds__(RF_THREADS) void k_reframe(const RfParams P, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst)
{
    const int bx = (int)blockIdx.x;
    const RfPlane &L = P.pl[bx >= P.pl[2].block0 ? 2 : bx >= P.pl[1].block0 ? 1 : 0];
    const int item = (bx - L.block0) * RF_THREADS + (int)threadIdx.x;
    const int Y = item / L.cpr;
    if (Y >= L.OH) return;
    uint8_t *row = dst + (long long)blockIdx.y * P.ofb + L.ooff + (long long)Y * L.OW;
    const int x0 = 16 * (item - Y * L.cpr) - (int)((uintptr_t)row & 15);
    if (x0 >= L.OW) return;
    const bool rowin = Y >= L.DY && Y < L.DY + L.H;
    // srow + x is the input sample of canvas column x, DX <= x < DX + W (read in a window row only)
    const uint8_t *srow = src + (long long)blockIdx.y * P.ifb + L.ioff + (long long)(Y - L.DY + L.Y0) * L.IW + (L.X0 - L.DX);
    const int wl = rowin ? L.DX : L.OW, wr = rowin ? L.DX + L.W : L.OW;     // the row's window columns [wl, wr)
    if (x0 >= 0 && x0 + 16 <= L.OW) {
        u32x4 v;
        if (x0 >= wr || x0 + 16 <= wl) {
            v = u32x4{L.fill, L.fill, L.fill, L.fill};
        } else if (x0 >= wl && x0 + 16 <= wr) {
            const u32x4a1 s = *reinterpret_cast<const u32x4a1 *>(srow + x0);
            v = u32x4{s.x, s.y, s.z, s.w};
        } else {
            unsigned d[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                d[k] = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int x = x0 + 4 * k + b;
                    const unsigned s = x >= wl && x < wr ? (unsigned)srow[x] : (L.fill & 0xffu);
                    d[k] |= s << (8 * b);
                }
            }
            v = u32x4{d[0], d[1], d[2], d[3]};
        }
        *reinterpret_cast<u32x4 *>(row + x0) = v;
    } else {
        for (int b = 0; b < 16; b++) {
            const int x = x0 + b;
            if (x >= 0 && x < L.OW) row[x] = x >= wl && x < wr ? srow[x] : (uint8_t)L.fill;
        }
    }
}

// the sum of v over the wave, in every lane: DPP inside the rows of 16 lanes, the four rows' sums read across
static __device__ __forceinline__ unsigned ls_wave_sum(unsigned v)
{
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, false);      // quad_perm [1, 0, 3, 2]
    x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, false);      // quad_perm [2, 3, 0, 1]
    x += __builtin_amdgcn_update_dpp(0, x, 0x124, 0xf, 0xf, false);     // row_ror:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, false);     // row_ror:8
    return (unsigned)(__builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) + __builtin_amdgcn_readlane(x, 32) +
                      __builtin_amdgcn_readlane(x, 48));
}

__global__ __launch_bounds__(LS_THREADS) void k_line_sums(const uint8_t *__restrict__ src, int W, int H, long long fb, unsigned *__restrict__ row_sum,
                                                          unsigned *__restrict__ col_sum)
{
    __shared__ unsigned part[LS_THREADS / 64][256];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint8_t *luma = src + (long long)blockIdx.y * fb;
    const int r0 = (int)blockIdx.x * LS_BLOCK_ROWS + wv * LS_WAVE_ROWS;
    unsigned racc[LS_WAVE_ROWS];
#pragma unroll
    for (int i = 0; i < LS_WAVE_ROWS; i++) racc[i] = 0;
    for (int c0 = 0; c0 < W; c0 += 256) {                // (uniform over the block)
        const int c = c0 + 4 * lane;
        unsigned cs[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < LS_WAVE_ROWS; i++) {
            const int r = r0 + i;
            if (r < H && c < W) {
                const uint8_t *p = luma + (long long)r * W + c;
                unsigned v;
                if (c + 4 <= W) {
                    v = *reinterpret_cast<const u32a1 *>(p);
                } else {                                 // the row's last columns: its own bytes only
                    v = p[0];
                    if (c + 1 < W) v |= (unsigned)p[1] << 8;
                    if (c + 2 < W) v |= (unsigned)p[2] << 16;
                }
                cs[0] += v & 0xffu; cs[1] += (v >> 8) & 0xffu; cs[2] += (v >> 16) & 0xffu; cs[3] += v >> 24;
                racc[i] = __builtin_amdgcn_sad_u8(v, 0u, racc[i]);
            }
        }
        *reinterpret_cast<u32x4 *>(&part[wv][4 * lane]) = u32x4{cs[0], cs[1], cs[2], cs[3]};
        __syncthreads();
        if (c0 + tid < W) {
            unsigned s = 0;
#pragma unroll
            for (int k = 0; k < LS_THREADS / 64; k++) s += part[k][tid];
            atomicAdd(&col_sum[(long long)blockIdx.y * W + c0 + tid], s);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < LS_WAVE_ROWS; i++) {
        const unsigned s = ls_wave_sum(racc[i]);
        if (lane == 0 && r0 + i < H) row_sum[(long long)blockIdx.y * H + r0 + i] = s;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct dsvg_reframe {
    int device = 0;
    RfParams P;
    int nblocks = 0;
};

extern "C" int dsv1_reframe_valid(const dsv1_reframe *rf, int subsamp);

extern "C" void dsvg_reframe_destroy(dsvg_reframe *r) { delete r; }

extern "C" int dsvg_reframe_create(dsvg_reframe **out, int device, const dsv1_reframe *rf, int subsamp)
{
    if (!out || !dsv1_reframe_valid(rf, subsamp)) { dsvg_set_error("bad reframe arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_reframe *r = new dsvg_reframe();
    r->device = device;
    memset(&r->P, 0, sizeof r->P);
    long long blocks = 0, ioff = 0, ooff = 0;
    for (int k = 0; k < 3; k++) {
        const int hs = k ? fmt_hs(subsamp) : 0, vs = k ? fmt_vs(subsamp) : 0;
        RfPlane &L = r->P.pl[k];
        L.OW = rsu(rf->out_w, hs); L.OH = rsu(rf->out_h, vs);
        L.cpr = (L.OW + 30) / 16;
        L.block0 = (int)blocks;
        L.DX = rf->dst_x >> hs; L.DY = rf->dst_y >> vs;
        L.W = rsu(rf->w, hs); L.H = rsu(rf->h, vs);
        L.X0 = rf->x >> hs; L.Y0 = rf->y >> vs;
        L.IW = rsu(rf->in_w, hs);
        L.fill = rf->fill[k] * 0x01010101u;
        L.ioff = ioff; L.ooff = ooff;
        ioff += (long long)L.IW * rsu(rf->in_h, vs);
        ooff += (long long)L.OW * L.OH;
        blocks += ((long long)L.OH * L.cpr + RF_THREADS - 1) / RF_THREADS;
        // (the kernel's item index, block * RF_THREADS + thread, is an int)
        if (blocks > INT_MAX / RF_THREADS) { delete r; dsvg_set_error("canvas too large for the reframe's grid"); return DSVG_ERR_UNSUPPORTED; }
    }
    r->nblocks = (int)blocks;
    r->P.ifb = ioff; r->P.ofb = ooff;
    *out = r;
    return DSVG_OK;
}

extern "C" int dsvg_reframe_run(dsvg_reframe *r, void *stream, const void *src_dev, int nframes, void *dst_dev)
{
    if (!r || !src_dev || !dst_dev || nframes < 1) { dsvg_set_error("bad reframe arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(r->device));
    for (int f0 = 0; f0 < nframes; f0 += 65535) {
        const int nf = std::min(65535, nframes - f0);
        hipLaunchKernelGGL(k_reframe, dim3(r->nblocks, nf), dim3(RF_THREADS), 0, (hipStream_t)stream, r->P,
                           (const uint8_t *)src_dev + (size_t)f0 * (size_t)r->P.ifb, (uint8_t *)dst_dev + (size_t)f0 * (size_t)r->P.ofb);
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

struct dsvg_linesums {
    int device = 0, w = 0, h = 0;
    size_t fb = 0;
};

extern "C" void dsvg_linesums_destroy(dsvg_linesums *s) { delete s; }

extern "C" int dsvg_linesums_create(dsvg_linesums **out, int device, int w, int h, int subsamp)
{
    if (!out || w < 1 || h < 1) { dsvg_set_error("bad line sums arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_linesums *s = new dsvg_linesums();
    s->device = device; s->w = w; s->h = h;
    s->fb = (size_t)w * h + 2 * (size_t)rsu(w, fmt_hs(subsamp)) * (size_t)rsu(h, fmt_vs(subsamp));
    *out = s;
    return DSVG_OK;
}

// nframes frames -> row_dev [nframes][h], col_dev [nframes][w] (uint32, device memory)
extern "C" int dsvg_linesums_run(dsvg_linesums *s, void *stream, const void *src_dev, int nframes, void *row_dev, void *col_dev)
{
    if (!s || !src_dev || !row_dev || !col_dev || nframes < 1) { dsvg_set_error("bad line sums arguments"); return DSVG_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemsetAsync(col_dev, 0, sizeof(unsigned) * (size_t)s->w * (size_t)nframes, st));
    for (int f0 = 0; f0 < nframes; f0 += 65535) {
        const int nf = std::min(65535, nframes - f0);
        hipLaunchKernelGGL(k_line_sums, dim3((s->h + LS_BLOCK_ROWS - 1) / LS_BLOCK_ROWS, nf), dim3(LS_THREADS), 0, st,
                           (const uint8_t *)src_dev + (size_t)f0 * s->fb, s->w, s->h, (long long)s->fb, (unsigned *)row_dev + (size_t)f0 * s->h,
                           (unsigned *)col_dev + (size_t)f0 * s->w);
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}
