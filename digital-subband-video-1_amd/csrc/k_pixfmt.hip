// k_pixfmt.hip -- source pixel formats -> tightly packed planar 8-bit frames (include/dsv1_api.h dsv1_pix_format; stated in numpy in
// tests/_pixfmt.py).  A pure streaming pass in front of the scaler / the frame load.
//
// A source frame is one to three SEGMENTS (dsvg_pixfmt.h): a source plane and the output planes it feeds -- planar: Y, U, V, each one
// to one; semi-planar: Y one to one, the interleaved chroma plane to U and V; packed 4:2:2: the one plane to Y, U and V.  One launch
// converts every frame and segment of a clip: blockIdx.y = frame, blockIdx.x = 256 ITEMS of one segment (the segments' blocks one
// after the other, so a block's segment is uniform).  An item is one STEP of one row: 16 output bytes of each output plane (8 of U
// and V for the packed layouts), that is
//     8-bit plane             16 source bytes -> one 16-byte store
//     16-bit plane            32 source bytes -> one 16-byte store
//     8-bit interleaved UV    32 source bytes -> 16 U + 16 V
//     16-bit interleaved UV   64 source bytes -> 16 U + 16 V
//     YUYV / UYVY             32 source bytes -> 16 Y + 8 U + 8 V
// read with aligned 16-byte non-temporal loads (the source is read once), de-interleaved with v_perm_b32.
// Depth reduction (d > 8 bits, x the 16-bit word): v = msb_aligned ? x >> (16 - d) : x & (2^d - 1), out = min(255, (v + 2^(d-9)) >>
// (d - 8)).  With t = v >> (d - 9), the sample's 9 leading bits, (v + 2^(d-9)) >> (d - 8) = (t + 1) >> 1 (the bits below t cannot
// carry), and t = (x >> k) & 0x1ff with k = 7 (msb-aligned) or d - 9: the same for every depth, done on both 16-bit halves of a dword
// at once -- t + 1 <= 512 stays inside its half, the result is at most 256, and 256 becomes 255 by subtracting its own bit 8.
// The 16-byte path needs every row of the segment aligned, source and destination (16 bytes; 8 for the packed layouts' U and V):
// decided on the host per segment and launch from the pointers, offsets, pitches and frame strides -- uniform, no per-lane test.
// It takes the whole steps of a row; the row's tail, and every step of a segment that is not aligned, takes the byte path, which
// loads exactly the bytes of the samples it converts: nothing outside the frame is ever read, whatever the pitch or the width.
//
// Chroma halving (include/dsv1_api.h, chroma resampling; k_pixfmt_sub): a source at 4:4:4 or 4:2:2 into frames at 4:2:2 or 4:2:0 in the
// same launch.  The samples are reduced to 8 bits first and averaged second, with the carry-free byte arithmetic of k_pixout.hip:
// horizontally the even and the odd bytes of a dword are added in 16-bit halves, vertically ceil((a + b) / 2) = (a | b) - ((a ^ b) >>
// 1) byte for byte; horizontally first, rounded to 8 bits.  A step is still 16 bytes of each output plane: a planar chroma step reads
// 32 source samples of one or two rows, a semi-planar one 16 pairs of two rows; a packed item is a step of TWO source rows, which
// gives both luma rows and the one chroma row -- every source byte is loaded once.  The repeated last row is an edge select of the
// row pointer; the repeated last column takes the byte path, which clamps the index: no load past the last sample of a row.
#include <algorithm>
#include <vector>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

#define PX_THREADS 256

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct PixSeg {
    int kind, rows, width, cwidth;
    int cpr, block0, fast, nout;         // steps per row, first block of the segment in blockIdx.x, every row on the 16-byte path
    int dpitch[3], pad;
    long long doff[3];
    long long soff, spitch;
    int hd, vd, iw, ih;                  // k_pixfmt_sub: the segment's chroma is halved horizontally / vertically; source samples per row, rows
    int irows, pad2;                     // rows of items (packed, halved vertically: row pairs)
};
struct PixParams {
    PixSeg seg[3];
    long long sfb, dfb;
    int nseg, shift;
};

enum { PXL_PLANAR, PXL_SEMI, PXL_YUYV, PXL_UYVY };

// two 16-bit words -> their 8-bit values in bytes 0 and 2
static __device__ __forceinline__ unsigned px_reduce2(unsigned dw, int shift)
{
    unsigned t = (dw >> shift) & 0x01ff01ffu;
    t = ((t + 0x00010001u) >> 1) & 0x01ff01ffu;
    return t - ((t >> 8) & 0x00010001u);
}
// v_perm_b32: selector bytes 0..3 pick from lo, 4..7 from hi
static __device__ __forceinline__ unsigned px_perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#define PX_EVEN 0x06040200u              // lo.b0 lo.b2 hi.b0 hi.b2
#define PX_ODD  0x07050301u              // lo.b1 lo.b3 hi.b1 hi.b3
#define PX_ZIP  0x06020400u              // lo.b0 hi.b0 lo.b2 hi.b2
#define PX_LOW  0x05040100u              // lo.b0 lo.b1 hi.b0 hi.b1
#define PX_HIGH 0x07060302u              // lo.b2 lo.b3 hi.b2 hi.b3

static __device__ __forceinline__ u32x4 px_load(const uint8_t *p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p)); }
static __device__ __forceinline__ void px_store(uint8_t *p, u32x4 v) { *reinterpret_cast<u32x4 *>(p) = v; }

// byte path: sample i of a row
template <bool WIDE> static __device__ __forceinline__ unsigned px_sample(const uint8_t *row, long long i, int shift)
{
    if (!WIDE) return row[i];
    const unsigned x = (unsigned)row[2 * i] | ((unsigned)row[2 * i + 1] << 8);
    const unsigned t = (x >> shift) & 0x1ffu;
    return min(255u, (t + 1u) >> 1);
}

template <int LAYOUT, bool WIDE>
__global__ __launch_bounds__(PX_THREADS) void k_pixfmt(const PixParams P, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst)
{
    const int bx = blockIdx.x;
    const int si = (LAYOUT == PXL_PLANAR) ? (bx >= P.seg[2].block0 ? 2 : (bx >= P.seg[1].block0 ? 1 : 0))
                 : (LAYOUT == PXL_SEMI)   ? (bx >= P.seg[1].block0 ? 1 : 0) : 0;
    const PixSeg &S = P.seg[si];
    const int item = (bx - S.block0) * PX_THREADS + (int)threadIdx.x;
    const int cpr = S.cpr;
    const int y = item / cpr, c = item - y * cpr;
    if (y >= S.rows) return;
    const int shift = P.shift;
    const uint8_t *row = src + (long long)blockIdx.y * P.sfb + S.soff + (long long)y * S.spitch;
    uint8_t *frame = dst + (long long)blockIdx.y * P.dfb;
    uint8_t *o0 = frame + S.doff[0] + (long long)y * S.dpitch[0];
    const bool whole = S.fast && 16 * c + 16 <= S.width;
    if (LAYOUT == PXL_PLANAR || (LAYOUT == PXL_SEMI && si == 0)) {
        if (whole) {
            if (!WIDE) px_store(o0 + 16 * c, px_load(row + 16 * c));
            else {
                const u32x4 a = px_load(row + 32 * c), b = px_load(row + 32 * c + 16);
                u32x4 o;
                o.x = px_perm(px_reduce2(a.y, shift), px_reduce2(a.x, shift), PX_EVEN);
                o.y = px_perm(px_reduce2(a.w, shift), px_reduce2(a.z, shift), PX_EVEN);
                o.z = px_perm(px_reduce2(b.y, shift), px_reduce2(b.x, shift), PX_EVEN);
                o.w = px_perm(px_reduce2(b.w, shift), px_reduce2(b.z, shift), PX_EVEN);
                px_store(o0 + 16 * c, o);
            }
        } else {
            const int n = min(16, S.width - 16 * c);
            for (int i = 0; i < n; i++) o0[16 * c + i] = (uint8_t)px_sample<WIDE>(row, 16 * c + i, shift);
        }
    } else if (LAYOUT == PXL_SEMI) {
        uint8_t *o1 = frame + S.doff[1] + (long long)y * S.dpitch[1];
        if (whole) {
            u32x4 u, v;
            if (!WIDE) {
                const u32x4 a = px_load(row + 32 * c), b = px_load(row + 32 * c + 16);
                u.x = px_perm(a.y, a.x, PX_EVEN); u.y = px_perm(a.w, a.z, PX_EVEN); u.z = px_perm(b.y, b.x, PX_EVEN); u.w = px_perm(b.w, b.z, PX_EVEN);
                v.x = px_perm(a.y, a.x, PX_ODD);  v.y = px_perm(a.w, a.z, PX_ODD);  v.z = px_perm(b.y, b.x, PX_ODD);  v.w = px_perm(b.w, b.z, PX_ODD);
            } else {
                unsigned uo[4], vo[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {           // 16 source bytes = four (a, b) pairs -> four bytes of each plane
                    const u32x4 a = px_load(row + 64 * c + 16 * q);
                    const unsigned p0 = px_perm(px_reduce2(a.y, shift), px_reduce2(a.x, shift), PX_ZIP);     // a0 a1 b0 b1
                    const unsigned p1 = px_perm(px_reduce2(a.w, shift), px_reduce2(a.z, shift), PX_ZIP);     // a2 a3 b2 b3
                    uo[q] = px_perm(p1, p0, PX_LOW);
                    vo[q] = px_perm(p1, p0, PX_HIGH);
                }
                u.x = uo[0]; u.y = uo[1]; u.z = uo[2]; u.w = uo[3];
                v.x = vo[0]; v.y = vo[1]; v.z = vo[2]; v.w = vo[3];
            }
            px_store(o0 + 16 * c, u);
            px_store(o1 + 16 * c, v);
        } else {
            const int n = min(16, S.width - 16 * c);
            for (int i = 0; i < n; i++) {
                const long long x = 16 * c + i;
                o0[x] = (uint8_t)px_sample<WIDE>(row, 2 * x, shift);
                o1[x] = (uint8_t)px_sample<WIDE>(row, 2 * x + 1, shift);
            }
        }
    } else {
        // packed 4:2:2, 8 bits: a macro-pixel is Y0 U Y1 V (YUYV) or U Y0 V Y1 (UYVY)
        uint8_t *o1 = frame + S.doff[1] + (long long)y * S.dpitch[1];
        uint8_t *o2 = frame + S.doff[2] + (long long)y * S.dpitch[2];
        const unsigned ysel = LAYOUT == PXL_YUYV ? PX_EVEN : PX_ODD, csel = LAYOUT == PXL_YUYV ? PX_ODD : PX_EVEN;
        if (whole) {
            const u32x4 a = px_load(row + 32 * c), b = px_load(row + 32 * c + 16);
            u32x4 yy;
            yy.x = px_perm(a.y, a.x, ysel); yy.y = px_perm(a.w, a.z, ysel); yy.z = px_perm(b.y, b.x, ysel); yy.w = px_perm(b.w, b.z, ysel);
            const unsigned c0 = px_perm(a.y, a.x, csel), c1 = px_perm(a.w, a.z, csel), c2 = px_perm(b.y, b.x, csel), c3 = px_perm(b.w, b.z, csel);   // U V U V
            u32x2 u, v;
            u.x = px_perm(c1, c0, PX_EVEN); u.y = px_perm(c3, c2, PX_EVEN);
            v.x = px_perm(c1, c0, PX_ODD);  v.y = px_perm(c3, c2, PX_ODD);
            px_store(o0 + 16 * c, yy);
            *reinterpret_cast<u32x2 *>(o1 + 8 * c) = u;
            *reinterpret_cast<u32x2 *>(o2 + 8 * c) = v;
        } else {
            const int yo = LAYOUT == PXL_YUYV ? 0 : 1, uo = 1 - yo;
            const int n = min(16, S.width - 16 * c), m = min(8, S.cwidth - 8 * c);
            for (int i = 0; i < n; i++) o0[16 * c + i] = row[2 * (long long)(16 * c + i) + yo];
            for (int i = 0; i < m; i++) {
                o1[8 * c + i] = row[4 * (long long)(8 * c + i) + uo];
                o2[8 * c + i] = row[4 * (long long)(8 * c + i) + uo + 2];
            }
        }
    }
}

// ---- chroma halving on the way ----
// (a + b + 1) >> 1 of four byte pairs
static __device__ __forceinline__ unsigned px_avg4(unsigned a, unsigned b) { return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu); }
static __device__ __forceinline__ u32x4 px_avg16(u32x4 a, u32x4 b)
{
    u32x4 o;
    o.x = px_avg4(a.x, b.x); o.y = px_avg4(a.y, b.y); o.z = px_avg4(a.z, b.z); o.w = px_avg4(a.w, b.w);
    return o;
}
// (b0 + b1 + 1) >> 1 and (b2 + b3 + 1) >> 1 of a dword, in bytes 0 and 2
static __device__ __forceinline__ unsigned px_havg2(unsigned d) { return (((d & 0x00ff00ffu) + ((d >> 8) & 0x00ff00ffu) + 0x00010001u) >> 1) & 0x00ff00ffu; }
// 32 bytes -> the 16 averages of their pairs
static __device__ __forceinline__ u32x4 px_hhalf16(u32x4 a, u32x4 b)
{
    u32x4 o;
    o.x = px_perm(px_havg2(a.y), px_havg2(a.x), PX_EVEN); o.y = px_perm(px_havg2(a.w), px_havg2(a.z), PX_EVEN);
    o.z = px_perm(px_havg2(b.y), px_havg2(b.x), PX_EVEN); o.w = px_perm(px_havg2(b.w), px_havg2(b.z), PX_EVEN);
    return o;
}
// samples s0 .. s0 + 15 of a row as 8-bit values (s0 a multiple of 16, the row aligned)
template <bool WIDE> static __device__ __forceinline__ u32x4 px_get16(const uint8_t *row, long long s0, int shift)
{
    if (!WIDE) return px_load(row + s0);
    const u32x4 a = px_load(row + 2 * s0), b = px_load(row + 2 * s0 + 16);
    u32x4 o;
    o.x = px_perm(px_reduce2(a.y, shift), px_reduce2(a.x, shift), PX_EVEN);
    o.y = px_perm(px_reduce2(a.w, shift), px_reduce2(a.z, shift), PX_EVEN);
    o.z = px_perm(px_reduce2(b.y, shift), px_reduce2(b.x, shift), PX_EVEN);
    o.w = px_perm(px_reduce2(b.w, shift), px_reduce2(b.z, shift), PX_EVEN);
    return o;
}
// pairs p0 .. p0 + 15 of an interleaved row -> the 16 first and the 16 second samples
template <bool WIDE> static __device__ __forceinline__ void px_pair16(const uint8_t *row, long long p0, int shift, u32x4 &u, u32x4 &v)
{
    const u32x4 a = px_get16<WIDE>(row, 2 * p0, shift), b = px_get16<WIDE>(row, 2 * p0 + 16, shift);
    u.x = px_perm(a.y, a.x, PX_EVEN); u.y = px_perm(a.w, a.z, PX_EVEN); u.z = px_perm(b.y, b.x, PX_EVEN); u.w = px_perm(b.w, b.z, PX_EVEN);
    v.x = px_perm(a.y, a.x, PX_ODD);  v.y = px_perm(a.w, a.z, PX_ODD);  v.z = px_perm(b.y, b.x, PX_ODD);  v.w = px_perm(b.w, b.z, PX_ODD);
}
// byte path: output sample x of a plane whose rows r0 and r1 (the same at the last odd row) feed one output row; `step` source
// samples from one of the plane's to the next and `first` the plane's first (interleaved planes), iw samples of the plane per row
template <bool WIDE>
static __device__ __forceinline__ unsigned px_hsample(const uint8_t *r0, const uint8_t *r1, int x, int hd, int vd, int iw, int step, int first, int shift)
{
    const int x0 = hd ? 2 * x : x, x1 = hd ? min(x0 + 1, iw - 1) : x0;
    const long long i0 = (long long)x0 * step + first, i1 = (long long)x1 * step + first;
    unsigned v = hd ? (px_sample<WIDE>(r0, i0, shift) + px_sample<WIDE>(r0, i1, shift) + 1u) >> 1 : px_sample<WIDE>(r0, i0, shift);
    if (vd) {
        const unsigned u = hd ? (px_sample<WIDE>(r1, i0, shift) + px_sample<WIDE>(r1, i1, shift) + 1u) >> 1 : px_sample<WIDE>(r1, i0, shift);
        v = (v + u + 1u) >> 1;
    }
    return v;
}

template <int LAYOUT, bool WIDE>
__global__ __launch_bounds__(PX_THREADS) void k_pixfmt_sub(const PixParams P, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst)
{
    const int bx = blockIdx.x;
    const int si = (LAYOUT == PXL_PLANAR) ? (bx >= P.seg[2].block0 ? 2 : (bx >= P.seg[1].block0 ? 1 : 0))
                 : (LAYOUT == PXL_SEMI)   ? (bx >= P.seg[1].block0 ? 1 : 0) : 0;
    const PixSeg &S = P.seg[si];
    const int item = (bx - S.block0) * PX_THREADS + (int)threadIdx.x;
    const int cpr = S.cpr;
    const int y = item / cpr, c = item - y * cpr;
    if (y >= S.irows) return;
    const int shift = P.shift, hd = S.hd, vd = S.vd;
    const uint8_t *plane = src + (long long)blockIdx.y * P.sfb + S.soff;
    uint8_t *frame = dst + (long long)blockIdx.y * P.dfb;
    // the source rows of output (chroma) row y: the last one once more where there is no second
    const int y0 = vd ? 2 * y : y, y1 = min(y0 + 1, S.ih - 1);
    const uint8_t *r0 = plane + (long long)y0 * S.spitch, *r1 = plane + (long long)y1 * S.spitch;
    if (LAYOUT == PXL_PLANAR || (LAYOUT == PXL_SEMI && si == 0)) {
        uint8_t *o0 = frame + S.doff[0] + (long long)y * S.dpitch[0];
        if (S.fast && ((16 * c + 16) << hd) <= S.iw) {
            const long long s0 = (long long)(16 * c) << hd;
            u32x4 v = hd ? px_hhalf16(px_get16<WIDE>(r0, s0, shift), px_get16<WIDE>(r0, s0 + 16, shift)) : px_get16<WIDE>(r0, s0, shift);
            if (vd) v = px_avg16(v, hd ? px_hhalf16(px_get16<WIDE>(r1, s0, shift), px_get16<WIDE>(r1, s0 + 16, shift)) : px_get16<WIDE>(r1, s0, shift));
            px_store(o0 + 16 * c, v);
        } else {
            const int n = min(16, S.width - 16 * c);
            for (int i = 0; i < n; i++) o0[16 * c + i] = (uint8_t)px_hsample<WIDE>(r0, r1, 16 * c + i, hd, vd, S.iw, 1, 0, shift);
        }
    } else if (LAYOUT == PXL_SEMI) {
        // the interleaved plane of a 4:2:2 source: halved vertically only
        uint8_t *o0 = frame + S.doff[0] + (long long)y * S.dpitch[0], *o1 = frame + S.doff[1] + (long long)y * S.dpitch[1];
        if (S.fast && 16 * c + 16 <= S.width) {
            u32x4 u, v;
            px_pair16<WIDE>(r0, 16 * c, shift, u, v);
            if (vd) {
                u32x4 u1, v1;
                px_pair16<WIDE>(r1, 16 * c, shift, u1, v1);
                u = px_avg16(u, u1); v = px_avg16(v, v1);
            }
            px_store(o0 + 16 * c, u);
            px_store(o1 + 16 * c, v);
        } else {
            const int n = min(16, S.width - 16 * c);
            for (int i = 0; i < n; i++) {
                o0[16 * c + i] = (uint8_t)px_hsample<WIDE>(r0, r1, 16 * c + i, 0, vd, S.iw, 2, 0, shift);
                o1[16 * c + i] = (uint8_t)px_hsample<WIDE>(r0, r1, 16 * c + i, 0, vd, S.iw, 2, 1, shift);
            }
        }
    } else {
        // packed 4:2:2, 8 bits, halved vertically: item row y is source rows 2y and 2y + 1 -> two luma rows, one chroma row
        const bool two = y0 + 1 < S.rows;
        uint8_t *l0 = frame + S.doff[0] + (long long)y0 * S.dpitch[0], *l1 = l0 + S.dpitch[0];
        uint8_t *o1 = frame + S.doff[1] + (long long)y * S.dpitch[1], *o2 = frame + S.doff[2] + (long long)y * S.dpitch[2];
        const unsigned ysel = LAYOUT == PXL_YUYV ? PX_EVEN : PX_ODD, csel = LAYOUT == PXL_YUYV ? PX_ODD : PX_EVEN;
        if (S.fast && 16 * c + 16 <= S.width) {
            const u32x4 a = px_load(r0 + 32 * c), b = px_load(r0 + 32 * c + 16);
            u32x4 yy;
            yy.x = px_perm(a.y, a.x, ysel); yy.y = px_perm(a.w, a.z, ysel); yy.z = px_perm(b.y, b.x, ysel); yy.w = px_perm(b.w, b.z, ysel);
            px_store(l0 + 16 * c, yy);
            unsigned c0 = px_perm(a.y, a.x, csel), c1 = px_perm(a.w, a.z, csel), c2 = px_perm(b.y, b.x, csel), c3 = px_perm(b.w, b.z, csel);   // U V U V
            if (two) {
                const u32x4 d = px_load(r1 + 32 * c), e = px_load(r1 + 32 * c + 16);
                yy.x = px_perm(d.y, d.x, ysel); yy.y = px_perm(d.w, d.z, ysel); yy.z = px_perm(e.y, e.x, ysel); yy.w = px_perm(e.w, e.z, ysel);
                px_store(l1 + 16 * c, yy);
                c0 = px_avg4(c0, px_perm(d.y, d.x, csel)); c1 = px_avg4(c1, px_perm(d.w, d.z, csel));
                c2 = px_avg4(c2, px_perm(e.y, e.x, csel)); c3 = px_avg4(c3, px_perm(e.w, e.z, csel));
            }
            u32x2 u, v;
            u.x = px_perm(c1, c0, PX_EVEN); u.y = px_perm(c3, c2, PX_EVEN);
            v.x = px_perm(c1, c0, PX_ODD);  v.y = px_perm(c3, c2, PX_ODD);
            *reinterpret_cast<u32x2 *>(o1 + 8 * c) = u;
            *reinterpret_cast<u32x2 *>(o2 + 8 * c) = v;
        } else {
            const int yo = LAYOUT == PXL_YUYV ? 0 : 1, uo = 1 - yo;
            const int n = min(16, S.width - 16 * c), m = min(8, S.cwidth - 8 * c);
            for (int i = 0; i < n; i++) {
                l0[16 * c + i] = r0[2 * (long long)(16 * c + i) + yo];
                if (two) l1[16 * c + i] = r1[2 * (long long)(16 * c + i) + yo];
            }
            for (int i = 0; i < m; i++) {
                const long long k = 4 * (long long)(8 * c + i) + uo;
                o1[8 * c + i] = (uint8_t)(((unsigned)r0[k] + r1[k] + 1u) >> 1);
                o2[8 * c + i] = (uint8_t)(((unsigned)r0[k + 2] + r1[k + 2] + 1u) >> 1);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct dsvg_pixconv {
    int device = 0;
    int layout = 0;                      // PXL_*
    dsv1_pix_layout L;
    PixParams P;
    int nblocks = 0;
    bool rgb = false;                    // the pass is the RGB import (k_rgb.hip) of layout R; L, P and nblocks are not used
    dsv1_rgb_layout R;
    bool hdr = false;                    // the pass is the HDR import (k_hdr.hip) of layout H; L, P and nblocks are not used
    dsv1_hdr_layout H;
    dsvg_hdr_rows hdr_rows;              // the small tables: kernel arguments
    uint32_t *hdr_tab = nullptr;         // the lookup tables as the kernel stages them, device memory
    int hdr_upsample = 0, hdr_cus = 0;
};

extern "C" void dsvg_pixconv_destroy(dsvg_pixconv *c)
{
    if (!c) return;
    if (c->hdr_tab) { (void)hipSetDevice(c->device); (void)hipFree(c->hdr_tab); }
    delete c;
}

extern "C" int dsvg_pixconv_create(dsvg_pixconv **out, int device, const dsv1_pix_layout *L)
{
    if (!out || !L || L->nseg < 1 || L->nseg > 3) { dsvg_set_error("bad converter arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_pixconv *c = new dsvg_pixconv();
    c->device = device; c->L = *L;
    const int k0 = L->seg[0].kind;
    c->layout = k0 == DSV1_PIXSEG_YUYV ? PXL_YUYV : k0 == DSV1_PIXSEG_UYVY ? PXL_UYVY : L->nseg == 2 ? PXL_SEMI : PXL_PLANAR;
    memset(&c->P, 0, sizeof c->P);
    long long blocks = 0;
    for (int s = 0; s < 3; s++) {
        PixSeg &S = c->P.seg[s];
        if (s >= L->nseg) { S.block0 = INT_MAX; continue; }     // (never chosen)
        const dsv1_pix_seg &G = L->seg[s];
        S.kind = G.kind; S.rows = G.rows; S.width = G.width; S.cwidth = G.cwidth; S.nout = G.nout;
        S.cpr = (G.width + 15) / 16;
        S.block0 = (int)blocks;
        for (int o = 0; o < 3; o++) { S.dpitch[o] = G.dpitch[o]; S.doff[o] = (long long)G.doff[o]; }
        S.soff = (long long)G.soff; S.spitch = (long long)G.spitch;
        // chroma halving: the packed segment's rows are luma rows (an item is two of them), every other chroma segment's are halved
        const bool packed = c->layout == PXL_YUYV || c->layout == PXL_UYVY, chroma = packed || s > 0;
        S.hd = chroma ? L->hd : 0; S.vd = chroma ? L->vd : 0;
        if (packed && S.hd) { delete c; dsvg_set_error("bad converter arguments"); return DSVG_ERR_ARG; }
        S.iw = chroma && !packed ? L->scw : G.width; S.ih = chroma && !packed ? L->sch : G.rows;
        S.irows = packed && S.vd ? (G.rows + 1) / 2 : G.rows;
        blocks += ((long long)S.cpr * S.irows + PX_THREADS - 1) / PX_THREADS;
        if (blocks > INT_MAX / 2) { delete c; dsvg_set_error("frame too large for the converter's grid"); return DSVG_ERR_UNSUPPORTED; }
    }
    c->nblocks = (int)blocks;
    c->P.nseg = L->nseg; c->P.shift = L->shift;
    c->P.sfb = (long long)L->frame_bytes; c->P.dfb = (long long)L->out_frame_bytes;
    *out = c;
    return DSVG_OK;
}

// the converter of an RGB source: another pass behind the same entry points
extern "C" int dsvg_pixconv_create_rgb(dsvg_pixconv **out, int device, const dsv1_rgb_layout *R)
{
    if (!out || !R || R->w < 1 || R->h < 1 || (R->nplanes != 1 && R->nplanes != 3)) { dsvg_set_error("bad converter arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_pixconv *c = new dsvg_pixconv();
    c->device = device; c->rgb = true; c->R = *R;
    memset(&c->L, 0, sizeof c->L);
    memset(&c->P, 0, sizeof c->P);
    *out = c;
    return DSVG_OK;
}

// the converter of an HDR source: the third pass behind the same entry points.  The lookup tables' device copy is the converter's
// own, a plain device allocation as the levels pass's tables are (dsvg_mem_outstanding, which counts context memory, does not see
// it); it goes with the converter
extern "C" int dsvg_pixconv_create_hdr(dsvg_pixconv **out, int device, const dsv1_hdr_layout *H, const dsv1_hdr_tables *T, int upsample)
{
    if (!out || !H || !T || H->w < 1 || H->h < 1 || (upsample != DSV1_CHROMA_REPLICATE && upsample != DSV1_CHROMA_LINEAR) || !dsv1_hdr_tables_valid(T)) {
        dsvg_set_error("bad converter arguments"); return DSVG_ERR_ARG;
    }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_pixconv *c = new dsvg_pixconv();
    c->device = device; c->hdr = true; c->H = *H; c->hdr_upsample = upsample;
    dsvg_hdr_rows_of(T, &c->hdr_rows);
    memset(&c->L, 0, sizeof c->L);
    memset(&c->P, 0, sizeof c->P);
    memset(&c->R, 0, sizeof c->R);
    std::vector<uint32_t> words(DSVG_HDR_TAB_WORDS);
    dsvg_hdr_tab_pack(T, words.data());
    int cus = 0;
    if (hipSetDevice(device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1 ||
        hipMalloc((void **)&c->hdr_tab, words.size() * sizeof(uint32_t)) != hipSuccess) {
        c->hdr_tab = nullptr; dsvg_pixconv_destroy(c); (void)hipGetLastError();
        dsvg_set_error("no device memory for the HDR tables"); return DSVG_ERR_HIP;
    }
    if (hipMemcpy(c->hdr_tab, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
        dsvg_pixconv_destroy(c); (void)hipGetLastError();
        dsvg_set_error("HDR tables: upload failed"); return DSVG_ERR_HIP;
    }
    c->hdr_cus = cus;
    *out = c;
    return DSVG_OK;
}

template <int LAYOUT, bool WIDE> static void pix_launch(const PixParams &P, dim3 grid, hipStream_t st, const uint8_t *src, uint8_t *dst, bool sub)
{
    if (sub) hipLaunchKernelGGL((k_pixfmt_sub<LAYOUT, WIDE>), grid, dim3(PX_THREADS), 0, st, P, src, dst);
    else hipLaunchKernelGGL((k_pixfmt<LAYOUT, WIDE>), grid, dim3(PX_THREADS), 0, st, P, src, dst);
}

// the 16-byte path of a segment: every row of every frame aligned, source and destination
static int seg_fast(const PixParams &P, const PixSeg &S, const void *src, const void *dst)
{
    const bool packed = S.kind == DSV1_PIXSEG_YUYV || S.kind == DSV1_PIXSEG_UYVY;
    if ((((uintptr_t)src) | (uintptr_t)P.sfb | (uintptr_t)S.soff | (uintptr_t)S.spitch) & 15) return 0;
    for (int o = 0; o < S.nout; o++) {
        const uintptr_t m = packed && o > 0 ? 7 : 15;
        if ((((uintptr_t)dst) | (uintptr_t)P.dfb | (uintptr_t)S.doff[o] | (uintptr_t)S.dpitch[o]) & m) return 0;
    }
    return 1;
}

extern "C" int dsvg_pixconv_run(dsvg_pixconv *c, void *stream, const void *src_dev, int nframes, void *dst_dev)
{
    if (!c || !src_dev || !dst_dev || nframes < 1) { dsvg_set_error("bad convert arguments"); return DSVG_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    if (c->rgb) return dsvg_rgb_import_run(stream, &c->R, src_dev, nframes, dst_dev);
    if (c->hdr) return dsvg_hdr_import_run(stream, &c->H, &c->hdr_rows, c->hdr_tab, c->hdr_upsample, c->hdr_cus, src_dev, nframes, dst_dev);
    PixParams P = c->P;
    for (int s = 0; s < P.nseg; s++) P.seg[s].fast = seg_fast(P, P.seg[s], src_dev, dst_dev);
    const bool wide = c->L.wide != 0, sub = c->L.hd || c->L.vd;
    for (int f0 = 0; f0 < nframes; f0 += 65535) {        // (gridDim.y; one launch for any call the batches make)
        const int n = std::min(65535, nframes - f0);
        const uint8_t *s = (const uint8_t *)src_dev + (size_t)f0 * c->L.frame_bytes;
        uint8_t *d = (uint8_t *)dst_dev + (size_t)f0 * c->L.out_frame_bytes;
        const dim3 grid(c->nblocks, n);
        switch (c->layout * 2 + (wide ? 1 : 0)) {
        case PXL_PLANAR * 2:     pix_launch<PXL_PLANAR, false>(P, grid, st, s, d, sub); break;
        case PXL_PLANAR * 2 + 1: pix_launch<PXL_PLANAR, true>(P, grid, st, s, d, sub); break;
        case PXL_SEMI * 2:       pix_launch<PXL_SEMI, false>(P, grid, st, s, d, sub); break;
        case PXL_SEMI * 2 + 1:   pix_launch<PXL_SEMI, true>(P, grid, st, s, d, sub); break;
        case PXL_YUYV * 2:       pix_launch<PXL_YUYV, false>(P, grid, st, s, d, sub); break;
        case PXL_UYVY * 2:       pix_launch<PXL_UYVY, false>(P, grid, st, s, d, sub); break;
        default: dsvg_set_error("no converter kernel for this format"); return DSVG_ERR_UNSUPPORTED;
        }
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}
