// k_pixout.hip -- decoded frames -> the caller's pixel format (include/dsvg.h dsvg_pixout, include/dsv1_api.h decoder output formats;
// stated in numpy in tests/_pixout.py): k_pixfmt.hip read in reverse.  A pure streaming pass that takes the place of k_pack_n: it
// reads the planes of the decoded frames once -- the bordered reconstruction slots of a context, picked by a slot table, or tightly
// packed planar frames -- and writes NV12 / NV21 / NV16, P010 / P210, 10 / 12 / 16-bit planar, YUYV / UYVY or padded planar 8-bit,
// halving the chroma planes on the way where the output subsampling asks for it.  No intermediate plane is written.
//
// An output frame is one to three SEGMENTS: an output plane and the input planes that feed it -- planar: Y, U, V, each one to one;
// semi-planar: Y one to one, U and V to the interleaved plane; packed 4:2:2: Y, U and V to the one plane.  One launch writes every
// frame and segment of a call: blockIdx.y = frame, blockIdx.x = 256 ITEMS of one segment (the segments' blocks one after the other, so
// a block's segment is uniform).  An item is one STEP of one output row: 16 samples of each input plane as they arrive (8 of U and V
// for the packed layouts), that is
//     8-bit plane             one 16-byte store              16-bit plane             two
//     8-bit interleaved UV    two                            16-bit interleaved UV    four
//     YUYV / UYVY             two
// read with aligned 16-byte loads, interleaved and widened with v_perm_b32 (selector 0x0c is a zero byte: a sample lands in the low
// byte of its 16-bit word and the word is shifted as one, v << shift <= 0xff00).
// Chroma halving: 16 arriving samples are 32 input bytes of one row (horizontal), 16 bytes of two rows (vertical) or 32 bytes of two
// rows (both: horizontal first, rounded to 8 bits, then vertical -- the order of the reference's -out420p).  o = (a + b + 1) >> 1 on
// packed bytes never drops the carry: horizontally the even and the odd bytes of a dword are added in 16-bit halves (<= 511);
// vertically ceil((a + b) / 2) = (a | b) - ((a ^ b) >> 1) byte for byte.  The repeated last row is an edge select of the row pointer;
// the repeated last column takes the byte path.
// The 16-byte path needs every row of the segment aligned, inputs and output (16 bytes; 8 for a packed layout's U and V that are not
// halved): decided on the host per segment and launch from the pointers, offsets, pitches and frame strides -- uniform, no per-lane
// test.  It takes the steps whose input samples all exist; a row's tail, and every step of a segment that is not aligned, takes the
// byte path, which stores exactly the bytes of the samples it owns: nothing between a row's end and its pitch, behind the planes or
// between frames is ever written.  The one exception lies inside the frame: the second luma byte of the last macro-pixel of an
// odd-width packed row repeats the row's last luma sample.
//
// Chroma doubling (include/dsv1_api.h, chroma resampling; the UP instances of the kernel): a 4:2:0 or 4:2:2 stream written at 4:2:2 or
// 4:4:4, as k_rgb.hip brings chroma to the luma grid -- vertically first, o = (3 c + n + 2) >> 2 with n the row above (even output
// rows) or below (odd ones), clamped; then the same over columns on that 8-bit result; replication is the same arithmetic with n = c.
// A step's 16 samples come from 16 (vertical only) or 8 (horizontal) input samples of one or two rows plus, horizontally, the one
// neighbour on each side -- two clamped byte loads.  3 a + b + 2 <= 1022 is formed on the even and the odd bytes of a dword in 16-bit
// halves, so nothing carries.  The 16-byte path takes the steps whose 16 output samples exist (their inputs then exist too).
#include <algorithm>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

#define PO_THREADS 256

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct PoSeg {
    int kind, rows, width, cwidth;
    int cpr, block0, fast, nin;          // steps per row, first block of the segment in blockIdx.x, every row on the 16-byte path
    int hd, vd, iw, ih;                  // the chroma inputs: halved horizontally / vertically, their dims (the clamps)
    int hu, vu, lin, pad2;               // ... or doubled; centre-sited linear, else replicated
    int ipitch[3], pad;
    long long ioff[3];                   // input planes inside a source frame
    long long ooff, opitch;              // the output plane inside an output frame
};
struct PoParams {
    PoSeg seg[3];
    long long sfb, dfb;
    int nseg, shift;
};

enum { POL_PLANAR, POL_SEMI, POL_YUYV, POL_UYVY };

// v_perm_b32: selector bytes 0..3 pick from lo, 4..7 from hi, 0x0c is zero
static __device__ __forceinline__ unsigned po_perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#define PO_EVEN  0x06040200u             // lo.b0 lo.b2 hi.b0 hi.b2
#define PO_ZIP01 0x05010400u             // lo.b0 hi.b0 lo.b1 hi.b1
#define PO_ZIP23 0x07030602u             // lo.b2 hi.b2 lo.b3 hi.b3
#define PO_WORD0 0x0c040c00u             // lo.b0 0 hi.b0 0 (+ 0x00010001 * i: byte i of both)
#define PO_W01   0x0c010c00u             // lo.b0 0 lo.b1 0
#define PO_W23   0x0c030c02u             // lo.b2 0 lo.b3 0

static __device__ __forceinline__ u32x4 po_load(const uint8_t *p) { return *reinterpret_cast<const u32x4 *>(p); }
static __device__ __forceinline__ void po_store(uint8_t *p, u32x4 v) { *reinterpret_cast<u32x4 *>(p) = v; }

// (a + b + 1) >> 1 of four byte pairs
static __device__ __forceinline__ unsigned po_avg4(unsigned a, unsigned b) { return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu); }
static __device__ __forceinline__ u32x4 po_avg16(u32x4 a, u32x4 b)
{
    u32x4 o;
    o.x = po_avg4(a.x, b.x); o.y = po_avg4(a.y, b.y); o.z = po_avg4(a.z, b.z); o.w = po_avg4(a.w, b.w);
    return o;
}
// (b0 + b1 + 1) >> 1 and (b2 + b3 + 1) >> 1 of a dword, in bytes 0 and 2
static __device__ __forceinline__ unsigned po_havg2(unsigned d) { return (((d & 0x00ff00ffu) + ((d >> 8) & 0x00ff00ffu) + 0x00010001u) >> 1) & 0x00ff00ffu; }
static __device__ __forceinline__ u32x2 po_hhalf8(u32x4 a)
{
    u32x2 o;
    o.x = po_perm(po_havg2(a.y), po_havg2(a.x), PO_EVEN);
    o.y = po_perm(po_havg2(a.w), po_havg2(a.z), PO_EVEN);
    return o;
}
static __device__ __forceinline__ u32x4 po_hhalf16(u32x4 a, u32x4 b)
{
    const u32x2 l = po_hhalf8(a), h = po_hhalf8(b);
    u32x4 o;
    o.x = l.x; o.y = l.y; o.z = h.x; o.w = h.y;
    return o;
}

// 16 arriving samples of a plane: output row y, output columns x0 .. x0 + 15 (every input sample exists, every load is aligned)
static __device__ __forceinline__ u32x4 po_fetch16(const uint8_t *plane, long long pitch, int y, int x0, int hd, int vd, int ih)
{
    const int y0 = vd ? 2 * y : y;
    const uint8_t *r0 = plane + (long long)y0 * pitch + ((long long)x0 << hd);
    u32x4 v = hd ? po_hhalf16(po_load(r0), po_load(r0 + 16)) : po_load(r0);
    if (vd) {
        const uint8_t *r1 = y0 + 1 < ih ? r0 + pitch : r0;
        v = po_avg16(v, hd ? po_hhalf16(po_load(r1), po_load(r1 + 16)) : po_load(r1));
    }
    return v;
}
// 8 of them (the packed layouts' U and V)
static __device__ __forceinline__ u32x2 po_fetch8(const uint8_t *plane, long long pitch, int y, int x0, int hd, int vd, int ih)
{
    const int y0 = vd ? 2 * y : y;
    const uint8_t *r0 = plane + (long long)y0 * pitch + ((long long)x0 << hd);
    u32x2 v = hd ? po_hhalf8(po_load(r0)) : *reinterpret_cast<const u32x2 *>(r0);
    if (vd) {
        const uint8_t *r1 = y0 + 1 < ih ? r0 + pitch : r0;
        const u32x2 u = hd ? po_hhalf8(po_load(r1)) : *reinterpret_cast<const u32x2 *>(r1);
        v.x = po_avg4(v.x, u.x); v.y = po_avg4(v.y, u.y);
    }
    return v;
}
// byte path: arriving sample x of output row y
static __device__ __forceinline__ unsigned po_sample(const uint8_t *plane, long long pitch, int y, int x, int hd, int vd, int iw, int ih)
{
    const int y0 = vd ? 2 * y : y, x0 = hd ? 2 * x : x, x1 = hd ? min(x0 + 1, iw - 1) : x0;
    const uint8_t *r0 = plane + (long long)y0 * pitch;
    unsigned v = hd ? ((unsigned)r0[x0] + r0[x1] + 1u) >> 1 : r0[x0];
    if (vd) {
        const uint8_t *r1 = plane + (long long)min(y0 + 1, ih - 1) * pitch;
        const unsigned u = hd ? ((unsigned)r1[x0] + r1[x1] + 1u) >> 1 : r1[x0];
        v = (v + u + 1u) >> 1;
    }
    return v;
}
// ---- chroma doubling ----
// (3 a + b + 2) >> 2 of four byte pairs
static __device__ __forceinline__ unsigned po_lerp4(unsigned a, unsigned b)
{
    const unsigned e = ((3u * (a & 0x00ff00ffu) + (b & 0x00ff00ffu) + 0x00020002u) >> 2) & 0x00ff00ffu;
    const unsigned o = ((3u * ((a >> 8) & 0x00ff00ffu) + ((b >> 8) & 0x00ff00ffu) + 0x00020002u) >> 2) & 0x00ff00ffu;
    return e | (o << 8);
}
// the two input rows of output row y: the one it lies in and its vertical neighbour (the same row: none, or replication)
static __device__ __forceinline__ void po_up_rows(const uint8_t *plane, long long pitch, int y, int vu, int lin, int ih, const uint8_t *&r0, const uint8_t *&r1)
{
    const int j = vu ? y >> 1 : y;
    const int n = vu && lin ? ((y & 1) ? min(j + 1, ih - 1) : max(j - 1, 0)) : j;
    r0 = plane + (long long)j * pitch;
    r1 = plane + (long long)n * pitch;
}
// 16 arriving samples of a plane, doubled: output row y, output columns x0 .. x0 + 15 (all of them exist, every load is aligned)
static __device__ __forceinline__ u32x4 po_up16(const uint8_t *plane, long long pitch, int y, int x0, int hu, int vu, int lin, int iw, int ih)
{
    const uint8_t *r0, *r1;
    po_up_rows(plane, pitch, y, vu, lin, ih, r0, r1);
    if (!hu) {
        const u32x4 a = po_load(r0 + x0);
        if (!(vu && lin)) return a;                     // (luma, replicated rows)
        const u32x4 b = po_load(r1 + x0);
        u32x4 o;
        o.x = po_lerp4(a.x, b.x); o.y = po_lerp4(a.y, b.y); o.z = po_lerp4(a.z, b.z); o.w = po_lerp4(a.w, b.w);
        return o;
    }
    // input columns i0 .. i0 + 7 and their neighbours on both sides, vertically interpolated first
    const int i0 = x0 >> 1, il = max(i0 - 1, 0), ir = min(i0 + 8, iw - 1);
    const u32x2 a = *reinterpret_cast<const u32x2 *>(r0 + i0), b = *reinterpret_cast<const u32x2 *>(r1 + i0);
    const unsigned lo = po_lerp4(a.x, b.x), hi = po_lerp4(a.y, b.y);
    const unsigned l = (3u * r0[il] + r1[il] + 2u) >> 2, r = (3u * r0[ir] + r1[ir] + 2u) >> 2;
    const unsigned plo = lin ? (lo << 8) | l : lo, phi = lin ? (hi << 8) | (lo >> 24) : hi;           // the sample before each
    const unsigned nlo = lin ? (lo >> 8) | (hi << 24) : lo, nhi = lin ? (hi >> 8) | (r << 24) : hi;    // the sample after each
    const unsigned elo = po_lerp4(lo, plo), ehi = po_lerp4(hi, phi), olo = po_lerp4(lo, nlo), ohi = po_lerp4(hi, nhi);
    u32x4 o;
    o.x = po_perm(olo, elo, PO_ZIP01); o.y = po_perm(olo, elo, PO_ZIP23); o.z = po_perm(ohi, ehi, PO_ZIP01); o.w = po_perm(ohi, ehi, PO_ZIP23);
    return o;
}
// 8 of them (the packed layouts' U and V: 4:2:2 out, so only rows are doubled)
static __device__ __forceinline__ u32x2 po_up8(const uint8_t *plane, long long pitch, int y, int x0, int vu, int lin, int ih)
{
    const uint8_t *r0, *r1;
    po_up_rows(plane, pitch, y, vu, lin, ih, r0, r1);
    const u32x2 a = *reinterpret_cast<const u32x2 *>(r0 + x0);
    if (!(vu && lin)) return a;
    const u32x2 b = *reinterpret_cast<const u32x2 *>(r1 + x0);
    u32x2 o;
    o.x = po_lerp4(a.x, b.x); o.y = po_lerp4(a.y, b.y);
    return o;
}
// byte path: arriving sample x of output row y
static __device__ __forceinline__ unsigned po_upsample(const uint8_t *plane, long long pitch, int y, int x, int hu, int vu, int lin, int iw, int ih)
{
    const uint8_t *r0, *r1;
    po_up_rows(plane, pitch, y, vu, lin, ih, r0, r1);
    const int i = hu ? x >> 1 : x;
    const int n = hu && lin ? ((x & 1) ? min(i + 1, iw - 1) : max(i - 1, 0)) : i;
    const unsigned a = (3u * r0[i] + r1[i] + 2u) >> 2, b = (3u * r0[n] + r1[n] + 2u) >> 2;
    return (3u * a + b + 2u) >> 2;
}
// the kernel's three fetches, halving or (UP) doubling
template <bool UP> static __device__ __forceinline__ u32x4 po_in16(const PoSeg &S, const uint8_t *plane, long long pitch, int y, int x0)
{
    return UP ? po_up16(plane, pitch, y, x0, S.hu, S.vu, S.lin, S.iw, S.ih) : po_fetch16(plane, pitch, y, x0, S.hd, S.vd, S.ih);
}
template <bool UP> static __device__ __forceinline__ u32x2 po_in8(const PoSeg &S, const uint8_t *plane, long long pitch, int y, int x0)
{
    return UP ? po_up8(plane, pitch, y, x0, S.vu, S.lin, S.ih) : po_fetch8(plane, pitch, y, x0, S.hd, S.vd, S.ih);
}
template <bool UP> static __device__ __forceinline__ unsigned po_in1(const PoSeg &S, const uint8_t *plane, long long pitch, int y, int x)
{
    return UP ? po_upsample(plane, pitch, y, x, S.hu, S.vu, S.lin, S.iw, S.ih) : po_sample(plane, pitch, y, x, S.hd, S.vd, S.iw, S.ih);
}
template <bool WIDE> static __device__ __forceinline__ void po_put(uint8_t *row, long long i, unsigned v, int shift)
{
    if (!WIDE) row[i] = (uint8_t)v;
    else { const unsigned x = v << shift; row[2 * i] = (uint8_t)x; row[2 * i + 1] = (uint8_t)(x >> 8); }
}

// tab: (source frame, output frame) per blockIdx.y -- the reconstruction slot and the caller's frame index -- or null: both blockIdx.y
template <int LAYOUT, bool WIDE, bool UP>
__global__ __launch_bounds__(PO_THREADS) void k_pixout(const PoParams P, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int *__restrict__ tab)
{
    const int bx = blockIdx.x;
    const int si = (LAYOUT == POL_PLANAR) ? (bx >= P.seg[2].block0 ? 2 : (bx >= P.seg[1].block0 ? 1 : 0))
                 : (LAYOUT == POL_SEMI)   ? (bx >= P.seg[1].block0 ? 1 : 0) : 0;
    const PoSeg &S = P.seg[si];
    const int item = (bx - S.block0) * PO_THREADS + (int)threadIdx.x;
    const int cpr = S.cpr;
    const int y = item / cpr, c = item - y * cpr;
    if (y >= S.rows) return;
    const int shift = P.shift;
    const long long sf = tab ? tab[2 * blockIdx.y] : (int)blockIdx.y, df = tab ? tab[2 * blockIdx.y + 1] : (int)blockIdx.y;
    const uint8_t *frame = src + sf * P.sfb;
    const uint8_t *i0 = frame + S.ioff[0];
    uint8_t *orow = dst + df * P.dfb + S.ooff + (long long)y * S.opitch;
    const int hd = S.hd, vd = S.vd;
    if (LAYOUT == POL_PLANAR || (LAYOUT == POL_SEMI && si == 0)) {
        const bool whole = S.fast && (UP ? 16 * c + 16 <= S.width : ((16 * c + 16) << hd) <= S.iw);
        if (whole) {
            const u32x4 v = po_in16<UP>(S, i0, S.ipitch[0], y, 16 * c);
            if (!WIDE) po_store(orow + 16 * c, v);
            else {
                u32x4 a, b;
                a.x = po_perm(0, v.x, PO_W01) << shift; a.y = po_perm(0, v.x, PO_W23) << shift;
                a.z = po_perm(0, v.y, PO_W01) << shift; a.w = po_perm(0, v.y, PO_W23) << shift;
                b.x = po_perm(0, v.z, PO_W01) << shift; b.y = po_perm(0, v.z, PO_W23) << shift;
                b.z = po_perm(0, v.w, PO_W01) << shift; b.w = po_perm(0, v.w, PO_W23) << shift;
                po_store(orow + 32 * c, a);
                po_store(orow + 32 * c + 16, b);
            }
        } else {
            const int n = min(16, S.width - 16 * c);
            for (int i = 0; i < n; i++) po_put<WIDE>(orow, 16 * c + i, po_in1<UP>(S, i0, S.ipitch[0], y, 16 * c + i), shift);
        }
    } else if (LAYOUT == POL_SEMI) {
        const uint8_t *i1 = frame + S.ioff[1];
        const bool whole = S.fast && (UP ? 16 * c + 16 <= S.width : ((16 * c + 16) << hd) <= S.iw);
        if (whole) {
            const u32x4 a = po_in16<UP>(S, i0, S.ipitch[0], y, 16 * c), b = po_in16<UP>(S, i1, S.ipitch[1], y, 16 * c);
            const unsigned av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
            if (!WIDE) {
                u32x4 o, p;
                o.x = po_perm(bv[0], av[0], PO_ZIP01); o.y = po_perm(bv[0], av[0], PO_ZIP23); o.z = po_perm(bv[1], av[1], PO_ZIP01); o.w = po_perm(bv[1], av[1], PO_ZIP23);
                p.x = po_perm(bv[2], av[2], PO_ZIP01); p.y = po_perm(bv[2], av[2], PO_ZIP23); p.z = po_perm(bv[3], av[3], PO_ZIP01); p.w = po_perm(bv[3], av[3], PO_ZIP23);
                po_store(orow + 32 * c, o);
                po_store(orow + 32 * c + 16, p);
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) {           // four (a, b) pairs -> four dwords of two 16-bit words
                    u32x4 o;
                    o.x = po_perm(bv[q], av[q], PO_WORD0) << shift;
                    o.y = po_perm(bv[q], av[q], PO_WORD0 + 0x00010001u) << shift;
                    o.z = po_perm(bv[q], av[q], PO_WORD0 + 0x00020002u) << shift;
                    o.w = po_perm(bv[q], av[q], PO_WORD0 + 0x00030003u) << shift;
                    po_store(orow + 64 * c + 16 * q, o);
                }
            }
        } else {
            const int n = min(16, S.width - 16 * c);
            for (int i = 0; i < n; i++) {
                const long long x = 16 * c + i;
                po_put<WIDE>(orow, 2 * x, po_in1<UP>(S, i0, S.ipitch[0], y, (int)x), shift);
                po_put<WIDE>(orow, 2 * x + 1, po_in1<UP>(S, i1, S.ipitch[1], y, (int)x), shift);
            }
        }
    } else {
        // packed 4:2:2, 8 bits: a macro-pixel is Y0 U Y1 V (YUYV) or U Y0 V Y1 (UYVY); luma is never halved
        const uint8_t *i1 = frame + S.ioff[1], *i2 = frame + S.ioff[2];
        const uint8_t *yrow = i0 + (long long)y * S.ipitch[0];
        const bool whole = S.fast && 16 * c + 16 <= S.width;           // (then the chroma inputs of the step exist too)
        if (whole) {
            const u32x4 yv = po_load(yrow + 16 * c);
            const u32x2 u = po_in8<UP>(S, i1, S.ipitch[1], y, 8 * c), v = po_in8<UP>(S, i2, S.ipitch[2], y, 8 * c);
            const unsigned yy[4] = {yv.x, yv.y, yv.z, yv.w};
            const unsigned uv[4] = {po_perm(v.x, u.x, PO_ZIP01), po_perm(v.x, u.x, PO_ZIP23), po_perm(v.y, u.y, PO_ZIP01), po_perm(v.y, u.y, PO_ZIP23)};   // U V U V
            unsigned o[8];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned hi = LAYOUT == POL_YUYV ? uv[j] : yy[j], lo = LAYOUT == POL_YUYV ? yy[j] : uv[j];
                o[2 * j] = po_perm(hi, lo, PO_ZIP01);
                o[2 * j + 1] = po_perm(hi, lo, PO_ZIP23);
            }
            u32x4 a, b;
            a.x = o[0]; a.y = o[1]; a.z = o[2]; a.w = o[3]; b.x = o[4]; b.y = o[5]; b.z = o[6]; b.w = o[7];
            po_store(orow + 32 * c, a);
            po_store(orow + 32 * c + 16, b);
        } else {
            const int yo = LAYOUT == POL_YUYV ? 0 : 1, uo = 1 - yo;
            const int m1 = min(8 * c + 8, S.cwidth);
            for (int m = 8 * c; m < m1; m++) {
                uint8_t *mp = orow + 4 * (long long)m;
                mp[yo] = yrow[2 * m];
                mp[yo + 2] = yrow[min(2 * m + 1, S.width - 1)];        // (odd width: the row's last luma sample once more)
                mp[uo] = (uint8_t)po_in1<UP>(S, i1, S.ipitch[1], y, m);
                mp[uo + 2] = (uint8_t)po_in1<UP>(S, i2, S.ipitch[2], y, m);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// the format against the source's planes: kernel parameters, or DSVG_ERR_ARG for a format that does not fit them (every output
// byte the kernel can write lies inside planes_bytes <= frame_bytes <= dfb)
static int po_params(PoParams &P, int &layout, int &nblocks, const dsvg_pixout *F, const PoSource &S, long long dfb)
{
    if (!F || F->nseg < 1 || F->nseg > 3 || (F->hd & ~1) || (F->vd & ~1) || (F->wide & ~1) || F->shift < 0 || F->shift > 8 || (!F->wide && F->shift)) return DSVG_ERR_ARG;
    if ((F->hu & ~1) || (F->vu & ~1) || ((F->hu || F->vu) && (F->hd || F->vd))) return DSVG_ERR_ARG;
    if (F->planes_bytes > F->frame_bytes || dfb < (long long)F->frame_bytes) return DSVG_ERR_ARG;
    const int k0 = F->seg[0].kind;
    const bool packed = k0 == DSVG_PIXOUT_YUYV || k0 == DSVG_PIXOUT_UYVY;
    layout = packed ? (k0 == DSVG_PIXOUT_YUYV ? POL_YUYV : POL_UYVY) : F->nseg == 2 ? POL_SEMI : POL_PLANAR;
    if ((packed && (F->nseg != 1 || F->wide)) || (!packed && F->nseg == 1)) return DSVG_ERR_ARG;
    memset(&P, 0, sizeof P);
    long long blocks = 0;
    for (int s = 0; s < 3; s++) {
        PoSeg &D = P.seg[s];
        if (s >= F->nseg) { D.block0 = INT_MAX; continue; }     // (never chosen)
        const dsvg_pixout_seg &G = F->seg[s];
        const int want_kind = packed ? k0 : (layout == POL_SEMI && s == 1) ? DSVG_PIXOUT_PAIR : DSVG_PIXOUT_PLAIN;
        const int nin = packed ? 3 : want_kind == DSVG_PIXOUT_PAIR ? 2 : 1;
        if (G.kind != want_kind || G.nin != nin) return DSVG_ERR_ARG;
        for (int k = 0; k < nin; k++) if (G.in_plane[k] < 0 || G.in_plane[k] > 2) return DSVG_ERR_ARG;
        if (packed && (G.in_plane[0] != 0 || G.in_plane[1] == 0 || G.in_plane[2] == 0)) return DSVG_ERR_ARG;
        if (nin == 2 && (G.in_plane[0] == 0) != (G.in_plane[1] == 0)) return DSVG_ERR_ARG;
        // the chroma inputs of a segment share their dims; luma is never halved
        const int pc = G.in_plane[nin - 1];
        const bool chroma = pc != 0;
        const int hd = chroma ? F->hd : 0, vd = chroma ? F->vd : 0, hu = chroma ? F->hu : 0, vu = chroma ? F->vu : 0;
        // doubled chroma reaches the luma dims on that axis, so the plane must be their rshift_up by one
        if ((hu && S.w[pc] != (S.w[0] + 1) / 2) || (vu && S.h[pc] != (S.h[0] + 1) / 2) || (packed && hu)) return DSVG_ERR_ARG;
        const int ow = hu ? S.w[0] : (S.w[pc] + hd) >> hd, oh = vu ? S.h[0] : (S.h[pc] + vd) >> vd;
        if (packed) {
            if (G.width != S.w[0] || G.rows != S.h[0] || oh != S.h[0] || G.cwidth != ow || ow != (S.w[0] + 1) / 2) return DSVG_ERR_ARG;
        } else if (G.width != ow || G.rows != oh) return DSVG_ERR_ARG;
        const size_t rowb = packed ? 4 * (size_t)G.cwidth : (size_t)G.width * (F->wide ? 2 : 1) * (nin == 2 ? 2 : 1);
        if (G.pitch < rowb || G.off + G.pitch * (size_t)(G.rows - 1) + rowb > F->planes_bytes) return DSVG_ERR_ARG;
        D.kind = G.kind; D.rows = G.rows; D.width = G.width; D.cwidth = G.cwidth; D.nin = nin;
        D.hd = hd; D.vd = vd; D.iw = S.w[pc]; D.ih = S.h[pc];
        D.hu = hu; D.vu = vu; D.lin = F->linear != 0;
        for (int k = 0; k < nin; k++) { D.ipitch[k] = (int)S.pitch[G.in_plane[k]]; D.ioff[k] = S.off[G.in_plane[k]]; }
        D.ooff = (long long)G.off; D.opitch = (long long)G.pitch;
        D.cpr = (G.width + 15) / 16;
        D.block0 = (int)blocks;
        blocks += ((long long)D.cpr * D.rows + PO_THREADS - 1) / PO_THREADS;
        if (blocks > INT_MAX / 2) { dsvg_set_error("frame too large for the output pass's grid"); return DSVG_ERR_UNSUPPORTED; }
    }
    nblocks = (int)blocks;
    P.nseg = F->nseg; P.shift = F->shift;
    P.sfb = S.fb; P.dfb = dfb;
    return DSVG_OK;
}

// the 16-byte path of a segment: every row of every frame aligned, inputs and output
static int po_seg_fast(const PoParams &P, const PoSeg &S, const void *src, const void *dst)
{
    const bool packed = S.kind == DSVG_PIXOUT_YUYV || S.kind == DSVG_PIXOUT_UYVY;
    for (int k = 0; k < S.nin; k++) {
        const uintptr_t m = (packed && k > 0 && !S.hd) || S.hu ? 7 : 15;    // (8-byte loads)
        if ((((uintptr_t)src) | (uintptr_t)P.sfb | (uintptr_t)S.ioff[k] | (uintptr_t)S.ipitch[k]) & m) return 0;
    }
    return !((((uintptr_t)dst) | (uintptr_t)P.dfb | (uintptr_t)S.ooff | (uintptr_t)S.opitch) & 15);
}

template <int LAYOUT, bool WIDE> static void po_launch(const PoParams &P, dim3 grid, hipStream_t st, const uint8_t *src, uint8_t *dst, const int *tab, bool up)
{
    if (up) hipLaunchKernelGGL((k_pixout<LAYOUT, WIDE, true>), grid, dim3(PO_THREADS), 0, st, P, src, dst, tab);
    else hipLaunchKernelGGL((k_pixout<LAYOUT, WIDE, false>), grid, dim3(PO_THREADS), 0, st, P, src, dst, tab);
}

int pixout_check(const dsvg_pixout *F, const PoSource &S, size_t dfb)
{
    PoParams P;
    int layout, nblocks;
    if (F && F->rgb.on) return rgbout_check(F, S, dfb);
    return po_params(P, layout, nblocks, F, S, (long long)dfb);
}

int launch_pixout(hipStream_t st, const dsvg_pixout *F, const PoSource &S, const uint8_t *src, const int *tab_d, int n, uint8_t *dst, size_t dfb, Prof *pf)
{
    PoParams P;
    int layout = 0, nblocks = 0;
    if (F && F->rgb.on) return launch_rgbout(st, F, S, src, tab_d, n, dst, dfb);     // (k_rgb.hip; not bracketed by the profiler)
    const int rc = po_params(P, layout, nblocks, F, S, (long long)dfb);
    if (rc) { if (rc == DSVG_ERR_ARG) dsvg_set_error("the output format does not fit the frames"); return rc; }
    double bytes = 0;
    for (int s = 0; s < P.nseg; s++) {
        PoSeg &D = P.seg[s];
        D.fast = po_seg_fast(P, D, src, dst);
        const bool packed = D.kind == DSVG_PIXOUT_YUYV || D.kind == DSVG_PIXOUT_UYVY;
        const double in_c = (double)D.iw * D.ih, out_row = packed ? 4.0 * D.cwidth : (double)D.width * D.nin * (F->wide ? 2 : 1);
        bytes += (packed ? (double)D.width * D.rows + 2 * in_c : in_c * D.nin) + out_row * D.rows;
    }
    const bool up = F->hu || F->vu;
    const int kid = layout == POL_PLANAR ? (F->wide ? KID_PIXOUT_PLANAR16 : KID_PIXOUT_PLANAR) : layout == POL_SEMI ? (F->wide ? KID_PIXOUT_SEMI16 : KID_PIXOUT_SEMI)
                  : layout == POL_YUYV ? KID_PIXOUT_YUYV : KID_PIXOUT_UYVY;
    if (pf) pf->begin(st, kid, bytes * n);
    for (int f0 = 0; f0 < n; f0 += 65535) {               // (gridDim.y; one launch for any call the decoders make)
        const int m = std::min(65535, n - f0);
        const uint8_t *s = tab_d ? src : src + (size_t)f0 * (size_t)P.sfb;
        uint8_t *d = tab_d ? dst : dst + (size_t)f0 * dfb;
        const int *t = tab_d ? tab_d + 2 * (size_t)f0 : nullptr;
        const dim3 grid(nblocks, m);
        switch (layout * 2 + (F->wide ? 1 : 0)) {
        case POL_PLANAR * 2:     po_launch<POL_PLANAR, false>(P, grid, st, s, d, t, up); break;
        case POL_PLANAR * 2 + 1: po_launch<POL_PLANAR, true>(P, grid, st, s, d, t, up); break;
        case POL_SEMI * 2:       po_launch<POL_SEMI, false>(P, grid, st, s, d, t, up); break;
        case POL_SEMI * 2 + 1:   po_launch<POL_SEMI, true>(P, grid, st, s, d, t, up); break;
        case POL_YUYV * 2:       po_launch<POL_YUYV, false>(P, grid, st, s, d, t, up); break;
        default:                 po_launch<POL_UYVY, false>(P, grid, st, s, d, t, up); break;
        }
    }
    if (pf) pf->end(st);
    return DSVG_OK;
}

extern "C" int dsvg_export_planar(int device, const void *src, int w, int h, int subsamp, int n, void *dst, const dsvg_pixout *F, int on_device)
{
    if (!src || !dst || !F || w < 1 || h < 1 || n < 1 || device < 0) { dsvg_set_error("bad export arguments"); return DSVG_ERR_ARG; }
    PoSource S;
    const int cw = rsu(w, fmt_hs(subsamp)), ch = rsu(h, fmt_vs(subsamp));
    S.w[0] = w; S.h[0] = h; S.w[1] = S.w[2] = cw; S.h[1] = S.h[2] = ch;
    S.pitch[0] = w; S.pitch[1] = S.pitch[2] = cw;
    S.off[0] = 0; S.off[1] = (long long)w * h; S.off[2] = S.off[1] + (long long)cw * ch;
    S.fb = S.off[2] + (long long)cw * ch;
    if (pixout_check(F, S, F->frame_bytes)) { dsvg_set_error("the output format does not fit the frames"); return DSVG_ERR_ARG; }
    // on a lane of the call's own (dsvg_pixfmt.h).  Host frames: the destination goes up as well, so that what the pass does not
    // write comes back as it was
    const size_t sbytes = (size_t)S.fb * n, dbytes = F->frame_bytes * (size_t)(n - 1) + F->planes_bytes;   // (the last frame ends with its planes)
    dsvg_lane *l = nullptr;
    int rc = dsvg_lane_create(&l, device);
    if (rc) return rc;
    void *s = const_cast<void *>(src), *d = dst;
    if (!on_device && !(rc = dsvg_lane_upload(l, 0, src, sbytes, &s))) rc = dsvg_lane_upload(l, 1, dst, dbytes, &d);
    if (!rc) rc = launch_pixout((hipStream_t)dsvg_lane_stream(l), F, S, (const uint8_t *)s, nullptr, n, (uint8_t *)d, F->frame_bytes, nullptr);
    const hipError_t e = rc ? hipSuccess : hipGetLastError();
    if (e != hipSuccess) { dsvg_set_error("the output pass could not be launched: %s", hipGetErrorString(e)); rc = DSVG_ERR_HIP; }
    if (!rc && !on_device) rc = dsvg_lane_download(l, dst, d, dbytes);
    if (!rc) rc = dsvg_lane_sync(l);
    dsvg_lane_destroy(l);                               // (waits for the stream; frees the uploads)
    return rc;
}
