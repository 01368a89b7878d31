// k_orient.hip -- the orientation pass (include/dsv1_api.h, Orientation; stated in numpy in tests/_orient.py): tightly packed planar
// 8-bit frames in, the same frames mirrored, rotated or transposed out, every plane on its own at its own dimensions.  The code is a
// bit set: bit 2 transposes first, bit 0 then mirrors the columns of the result, bit 1 its rows.  One launch covers every frame
// (blockIdx.y) and the three planes of a clip (blockIdx.x: the planes' blocks one after the other, so a block's plane is uniform).
//
// k_orient_rows (codes 1-3): rows stay rows.  The items are k_reframe's: one 16-byte ALIGNED chunk of one output row, counted from
// the row's address rounded down to 16, cpr = (OW + 30) / 16 items cover any row, the first and the last may be partial and store
// their bytes one by one.  A whole chunk is one 16-byte store of ONE unaligned 16-byte load: of the same columns of row IH-1-Y
// (VFLIP), or of columns IW-16-x0 .. IW-1-x0 -- exactly the 16 samples the chunk mirrors -- reversed in registers: the dwords in
// the opposite order, each with its bytes swapped by one v_perm_b32 (HFLIP, ROT180).
//
// k_orient_tr (codes 4-7): a block moves one tile of the INPUT plane, OR_TR = 128 rows of OR_TC = 64 columns, tiles counted from the
// plane's top left, through LDS.  Workgroups go to the 8 XCDs round robin, and each XCD has an L2 of its own: XCD x takes the x-th run
// of consecutive tiles of a plane, so that tiles that share input and output cache lines meet in one L2 (measured, with the tile's
// shape: profiles/orient_cost.txt, section "tile").
//   In:  thread t owns the 4 x 4 byte blocks (br, bc) and (br + 16, bc) of the tile, br = t >> 4, bc = t & 15: eight unaligned dword
//        loads, input rows 4 br .. 4 br + 3 and 64 + 4 br .. at column 4 bc (16 lanes read 64 consecutive bytes of a row), all issued
//        before the first use.  It transposes each block in registers -- 8 v_perm_b32, no byte loop -- into the four dwords "input
//        column 4 bc + j, input rows 4 br .. 4 br + 3" and stores them as dwords at row 4 bc + j, dword br (+ 16) of the TRANSPOSED
//        image img[64][OR_P], OR_P = 33 dwords.
//   Out: thread t owns 16 bytes (q = t & 7) of the image rows t >> 3 and 32 + (t >> 3): four dword reads, and one unaligned 16-byte
//        store along the output row (8 lanes write 128 consecutive bytes).
//   Mirrors: no second pass.  The tile lands at output rows 64 tj + r, or OH-1-(64 tj + r) under bit 1; its 16 bytes at columns
//        128 ti + 16 q .., or, under bit 0, at OW-16-(128 ti + 16 q) .. with the four dwords in the opposite order and the bytes of
//        each swapped (v_perm_b32 again).
//   Banks (64 x 4-byte banks; dword LDS stores and loads -- also as the ds_write2_b32 / ds_read2_b32 pairs the compiler forms, which
//        bank per dword -- are served per 32-lane half on address / 4 mod 32): a half of the writing wave holds bc = 0 .. 15 and
//        two neighbouring br, dword address (4 bc + j) * 33 + br = 4 bc + br + j mod 32: 4 bc takes 8 values twice over, br two
//        neighbours -- 16 banks with two lanes each, 2-way.  A half of the reading wave holds 4 consecutive rows r and q = 0 .. 7,
//        dword address 33 r + 4 q + k = r + 4 q + k mod 32: r in r0 .. r0 + 3 and 4 q in 0, 4 .. 28 -- 32 banks, conflict-free.
//        With OR_P = 32 every write would be 16-way and every read 4-way.
//   Edges: a 4 x 4 block that is not whole inside the plane loads the bytes that exist one by one (the rest are zero and never
//        stored); a 16-byte run of the image that is not whole stores the bytes that exist one by one.
// Both kernels write every output byte exactly once (the items / the tiles partition the output), nothing outside the output
// frames, and load only samples of the source frames.
#include <algorithm>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

#define OR_THREADS 256
#define OR_TR 128                        // the tile: input rows (the bytes of an output row) ...
#define OR_TC 64                         // ... and input columns (output rows)
#define OR_P 33                          // the LDS image's row pitch in dwords

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4a1 __attribute__((ext_vector_type(4), aligned(1)));       // 16 bytes at any address
typedef unsigned u32a1 __attribute__((aligned(1)));

struct OrPlane {
    int IW, IH, OW, OH;                  // the input and the output plane
    int cpr;                             // rows: chunks per output row
    int tiles_r;                         // tr: tiles along the input rows' direction (down the input = along the output rows)
    int block0, nblk;                    // first block of the plane in blockIdx.x; tr: the plane's blocks
    long long off;                       // the plane inside a frame (the same in and out: the planes keep their sizes)
};
struct OrParams {
    OrPlane pl[3];
    long long fb;                        // frame bytes, in and out
    int fx, fy;                          // mirror the columns / the rows (of the transposed picture, for codes 4-7)
};

static __device__ __forceinline__ unsigned or_bswap(unsigned v) { return __builtin_amdgcn_perm(0u, v, 0x00010203u); }

__global__ __launch_bounds__(OR_THREADS) void k_orient_rows(const OrParams P, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst)
{
    const int bx = (int)blockIdx.x;
    const OrPlane &L = P.pl[bx >= P.pl[2].block0 ? 2 : bx >= P.pl[1].block0 ? 1 : 0];
    const int item = (bx - L.block0) * OR_THREADS + (int)threadIdx.x;
    const int Y = item / L.cpr;
    if (Y >= L.OH) return;
    const long long base = (long long)blockIdx.y * P.fb + L.off;
    uint8_t *row = dst + base + (long long)Y * L.OW;
    const int x0 = 16 * (item - Y * L.cpr) - (int)((uintptr_t)row & 15);
    if (x0 >= L.OW) return;
    const uint8_t *srow = src + base + (long long)(P.fy ? L.IH - 1 - Y : Y) * L.IW;
    if (x0 >= 0 && x0 + 16 <= L.OW) {
        u32x4 v;
        if (P.fx) {
            const u32x4a1 s = *reinterpret_cast<const u32x4a1 *>(srow + (L.IW - 16 - x0));
            v = u32x4{or_bswap(s.w), or_bswap(s.z), or_bswap(s.y), or_bswap(s.x)};
        } else {
            const u32x4a1 s = *reinterpret_cast<const u32x4a1 *>(srow + x0);
            v = u32x4{s.x, s.y, s.z, s.w};
        }
        *reinterpret_cast<u32x4 *>(row + x0) = v;
    } else {
        for (int b = 0; b < 16; b++) {
            const int x = x0 + b;
            if (x >= 0 && x < L.OW) row[x] = srow[P.fx ? L.IW - 1 - x : x];
        }
    }
}

__global__ __launch_bounds__(OR_THREADS) void k_orient_tr(const OrParams P, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst)
{
    __shared__ unsigned img[OR_TC * OR_P];
    const int bx = (int)blockIdx.x, tid = (int)threadIdx.x;
    const OrPlane &L = P.pl[bx >= P.pl[2].block0 ? 2 : bx >= P.pl[1].block0 ? 1 : 0];
    // workgroups go to the 8 XCDs round robin, each with an L2 of its own: XCD x takes the x-th run of consecutive tiles, so that
    // tiles that share input and output cache lines meet in one L2 (a bijection of 0 .. nblk-1: XCD x gets q + (x < r) blocks)
    const int b = bx - L.block0, xcd = b & 7, q8 = L.nblk >> 3, r8 = L.nblk & 7;
    const int t = xcd * q8 + min(xcd, r8) + (b >> 3);
    const int tj = t / L.tiles_r, ti = t - tj * L.tiles_r;      // the tile: input rows 128 ti .., input columns 64 tj ..
    const long long base = (long long)blockIdx.y * P.fb + L.off;
    const int nr = min(OR_TR, L.IH - OR_TR * ti), nc = min(OR_TC, L.IW - OR_TC * tj);   // the tile's input rows and columns that exist
    {
        const int br = tid >> 4, bc = tid & 15;
        const uint8_t *p = src + base + (long long)(OR_TR * ti + 4 * br) * L.IW + (OR_TC * tj + 4 * bc);
        unsigned a[2][4];
#pragma unroll
        for (int h = 0; h < 2; h++) {                    // the block rows br and br + 16: all eight loads before the first use
            const int r0 = 4 * br + 64 * h;
            const uint8_t *ph = p + (long long)(64 * h) * L.IW;
            if (r0 + 4 <= nr && 4 * bc + 4 <= nc) {
#pragma unroll
                for (int i = 0; i < 4; i++) a[h][i] = *reinterpret_cast<const u32a1 *>(ph + (long long)i * L.IW);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    a[h][i] = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        if (r0 + i < nr && 4 * bc + b < nc) a[h][i] |= (unsigned)ph[(long long)i * L.IW + b] << (8 * b);
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            // 4 x 4 bytes transposed: byte j of a[0], a[1], a[2], a[3] is the dword of image row 4 bc + j
            const unsigned t0 = __builtin_amdgcn_perm(a[h][1], a[h][0], 0x05010400u), t1 = __builtin_amdgcn_perm(a[h][1], a[h][0], 0x07030602u);
            const unsigned u0 = __builtin_amdgcn_perm(a[h][3], a[h][2], 0x05010400u), u1 = __builtin_amdgcn_perm(a[h][3], a[h][2], 0x07030602u);
            unsigned *w = img + (4 * bc) * OR_P + br + 16 * h;
            w[0 * OR_P] = __builtin_amdgcn_perm(u0, t0, 0x05040100u);
            w[1 * OR_P] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
            w[2 * OR_P] = __builtin_amdgcn_perm(u1, t1, 0x05040100u);
            w[3 * OR_P] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
        }
    }
    __syncthreads();
    {
        const int q = tid & 7;                           // bytes 16 q .. of a row of the transposed image (input rows)
        if (16 * q >= nr) return;
        const int tx = OR_TR * ti + 16 * q;              // in the transposed plane
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int r = (tid >> 3) + 32 * h;           // the image row (input column)
            if (r >= nc) break;
            const unsigned *g = img + r * OR_P + 4 * q;
            const unsigned d[4] = {g[0], g[1], g[2], g[3]};
            const int ty = OR_TC * tj + r;
            uint8_t *row = dst + base + (long long)(P.fy ? L.OH - 1 - ty : ty) * L.OW;
            if (16 * q + 16 <= nr) {
                if (P.fx) *reinterpret_cast<u32x4a1 *>(row + (L.OW - 16 - tx)) = u32x4{or_bswap(d[3]), or_bswap(d[2]), or_bswap(d[1]), or_bswap(d[0])};
                else *reinterpret_cast<u32x4a1 *>(row + tx) = u32x4{d[0], d[1], d[2], d[3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const int c = 4 * k + b;
                        if (16 * q + c < nr) row[P.fx ? L.OW - 1 - (tx + c) : tx + c] = (uint8_t)(d[k] >> (8 * b));
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct dsvg_orient {
    int device = 0, orient = 0;
    OrParams P;
    int nblocks = 0;
};

extern "C" int dsv1_orient_valid(int orient, int subsamp);

extern "C" void dsvg_orient_destroy(dsvg_orient *o) { delete o; }

// w x h: the frames that come in
extern "C" int dsvg_orient_create(dsvg_orient **out, int device, int orient, int w, int h, int subsamp)
{
    if (!out || !dsv1_orient_valid(orient, subsamp) || w < 1 || h < 1) { dsvg_set_error("bad orientation arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_orient *o = new dsvg_orient();
    o->device = device; o->orient = orient;
    memset(&o->P, 0, sizeof o->P);
    o->P.fx = orient & 1; o->P.fy = (orient >> 1) & 1;
    long long blocks = 0, off = 0;
    for (int k = 0; k < 3; k++) {
        const int hs = k ? fmt_hs(subsamp) : 0, vs = k ? fmt_vs(subsamp) : 0;
        OrPlane &L = o->P.pl[k];
        L.IW = rsu(w, hs); L.IH = rsu(h, vs);
        L.OW = orient & 4 ? L.IH : L.IW; L.OH = orient & 4 ? L.IW : L.IH;
        L.cpr = (L.OW + 30) / 16;
        L.tiles_r = (L.IH + OR_TR - 1) / OR_TR;
        L.block0 = (int)blocks;
        L.off = off;
        off += (long long)L.IW * L.IH;
        const long long nb = orient & 4 ? (long long)L.tiles_r * ((L.IW + OR_TC - 1) / OR_TC) : ((long long)L.OH * L.cpr + OR_THREADS - 1) / OR_THREADS;
        blocks += nb;
        // (the row kernel's item index, block * OR_THREADS + thread, is an int; so is the block count of either)
        if (blocks > INT_MAX / OR_THREADS) { delete o; dsvg_set_error("picture too large for the orientation's grid"); return DSVG_ERR_UNSUPPORTED; }
    }
    for (int k = 0; k < 3; k++) o->P.pl[k].nblk = (k < 2 ? o->P.pl[k + 1].block0 : (int)blocks) - o->P.pl[k].block0;
    o->nblocks = (int)blocks;
    o->P.fb = off;
    *out = o;
    return DSVG_OK;
}

extern "C" int dsvg_orient_run(dsvg_orient *o, void *stream, const void *src_dev, int nframes, void *dst_dev)
{
    if (!o || !src_dev || !dst_dev || nframes < 1) { dsvg_set_error("bad orientation arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(o->device));
    if (!o->orient) {                                   // (the standalone call's code 0: a copy; a session sets no pass for it)
        HIPCHK(hipMemcpyAsync(dst_dev, src_dev, (size_t)o->P.fb * (size_t)nframes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return DSVG_OK;
    }
    for (int f0 = 0; f0 < nframes; f0 += 65535) {
        const int nf = std::min(65535, nframes - f0);
        const uint8_t *s = (const uint8_t *)src_dev + (size_t)f0 * (size_t)o->P.fb;
        uint8_t *d = (uint8_t *)dst_dev + (size_t)f0 * (size_t)o->P.fb;
        if (o->orient & 4) hipLaunchKernelGGL(k_orient_tr, dim3(o->nblocks, nf), dim3(OR_THREADS), 0, (hipStream_t)stream, o->P, s, d);
        else hipLaunchKernelGGL(k_orient_rows, dim3(o->nblocks, nf), dim3(OR_THREADS), 0, (hipStream_t)stream, o->P, s, d);
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}
