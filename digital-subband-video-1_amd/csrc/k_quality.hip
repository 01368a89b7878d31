// k_quality.hip -- opt-in quality measurement of the encoder (dsvg_ctx_sse_enable): per picture and plane the sum of squared
// errors between the source and the reconstruction over the picture area (borders excluded),
//     SSE[p] = sum over the w[p] x h[p] samples of (src - recon)^2,
// an exact 64-bit integer.  DSV1 is closed-loop, so the reconstruction is what a decoder shows; PSNR follows on the host.
// The SSIM of the same pictures (dsvg_ctx_ssim_enable, k_ssim) is further down.
//
// One launch per frame step and coding stream, right behind the step's reconstruction (dsvg_pipe.hip, code_batch_impl): in
// stream order the reconstruction is complete, an in-place one has not yet been overwritten by the next step, and the source
// slot has not yet been refilled by the next batch's analysis.  The source is read where the forward transform read it
// (JobDev.srcp / srcs: the bordered source slot, or the caller's clip for planes loaded in place); the reconstruction where
// the inverse transform wrote it -- the kept slot, or for a picture nobody predicts from the job's work frame (JobDev.xf,
// `recon ? recon : xf` as in every inverse kernel).
//
// Work mapping: a workgroup of 4 waves takes 16 rows of one plane of one job, a wave 4 of them, two at a time; lane i reads the
// 16-byte chunks i, i + 64, ... of a row (coalesced 16-byte loads).  Per 4 samples: the bytes of source and reconstruction
// unpacked to 16-bit pairs (v_perm_b32), one v_pk_sub_i16, one v_dot2_i32_i16 into the lane's sum -- about 2 VALU instructions
// per sample against 2 bytes of HBM traffic, far below the VALU rate.  A lane adds at most 4 rows x ceil(w / 1024) x 16
// samples of at most 255^2: below 2^31 for any w below 500 000.  The lanes' sums are added up in 64 bits across the wave
// (shuffles) and the workgroup (LDS), then ONE 64-bit atomic add per workgroup into sse[out slot][plane].  Integer sums do
// not depend on the order of the adds: the result is deterministic.
//
// The out slot of a job is not in its record: JobDev.psum points at psum[3 * out_slot] in the encoder (code_batch_impl), so
// (jb.psum - psum0) is 3 * out_slot.
#include <algorithm>
#include <cstdlib>
#include "dsvg_kernels.hpp"
#include "dsvg_host.hpp"

#define SSE_WAVES 4
#define SSE_ROWS_PER_WAVE 4
#define SSE_ROWS (SSE_WAVES * SSE_ROWS_PER_WAVE)      // rows per workgroup

typedef short dsvg_s16x2 __attribute__((ext_vector_type(2)));

// (a - b)^2 of the 4 byte pairs of two dwords added to acc
static __device__ __forceinline__ int sse_dword(unsigned a, unsigned b, int acc)
{
    const dsvg_s16x2 dl = __builtin_bit_cast(dsvg_s16x2, __builtin_amdgcn_perm(0u, a, 0x0c020c00u)) -
                          __builtin_bit_cast(dsvg_s16x2, __builtin_amdgcn_perm(0u, b, 0x0c020c00u));   // bytes 0, 2
    const dsvg_s16x2 dh = __builtin_bit_cast(dsvg_s16x2, __builtin_amdgcn_perm(0u, a, 0x0c030c01u)) -
                          __builtin_bit_cast(dsvg_s16x2, __builtin_amdgcn_perm(0u, b, 0x0c030c01u));   // bytes 1, 3
    acc = __builtin_amdgcn_sdot2(dl, dl, acc, false);
    return __builtin_amdgcn_sdot2(dh, dh, acc, false);
}
static __device__ __forceinline__ int sse_chunk(uint4 a, uint4 b, int acc)
{
    acc = sse_dword(a.x, b.x, acc);
    acc = sse_dword(a.y, b.y, acc);
    acc = sse_dword(a.z, b.z, acc);
    return sse_dword(a.w, b.w, acc);
}
// the 16 bytes of row p from column x: one 16-byte load where the row is 16-byte aligned and the chunk lies inside the picture;
// else byte by byte, bytes at or beyond column w read as 0 (in both images: they add nothing)
static __device__ __forceinline__ uint4 sse_load(const DSVG_GLOBAL uint8_t *p, int x, int w, bool al)
{
    if (al && x + 16 <= w) return dsvg_ld4(p + x);
    unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++)
        if (x + i < w) v[i >> 2] |= (unsigned)p[x + i] << (8 * (i & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

__global__ __launch_bounds__(64 * SSE_WAVES) void k_sse(const JobDev *__restrict__ jobs, FrameLayout L, int nb0, int nb1,
                                                       const HzPlaneSum *psum0, unsigned long long *__restrict__ sse)
{
    __shared__ unsigned long long part[SSE_WAVES];
    const int bx = (int)blockIdx.x;
    const int p = bx < nb0 ? 0 : 1 + (bx - nb0) / nb1;                  // workgroups [0, nb0) luma, then nb1 per chroma plane
    const int rg = bx < nb0 ? bx : (bx - nb0) % nb1;
    const JobDev &jb = jobs[blockIdx.y];
    const int w = L.w[p], h = L.h[p];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const auto src = dsvg_global(jb.srcp[p]);
    const size_t ss = (size_t)jb.srcs[p], rs = (size_t)L.stride[p];
    const auto rec = dsvg_global(static_cast<const uint8_t *>((jb.recon ? jb.recon : jb.xf) + L.off[p]));
    int acc = 0;
    const int y0 = rg * SSE_ROWS + wave * SSE_ROWS_PER_WAVE;
#pragma unroll
    for (int r = 0; r < SSE_ROWS_PER_WAVE; r += 2) {
        const int y = y0 + r;
        if (y >= h) break;
        const bool two = y + 1 < h;
        const auto sa = src + (size_t)y * ss, ra = rec + (size_t)y * rs;
        const auto sb = sa + ss, rb = ra + rs;
        const bool ala = (((uintptr_t)sa | (uintptr_t)ra) & 15) == 0, alb = (((uintptr_t)sb | (uintptr_t)rb) & 15) == 0;
        for (int x = 16 * lane; x < w; x += 16 * 64) {
            // both rows' loads first: four 16-byte loads in flight per lane
            const uint4 a0 = sse_load(sa, x, w, ala), b0 = sse_load(ra, x, w, ala);
            uint4 a1 = make_uint4(0u, 0u, 0u, 0u), b1 = a1;
            if (two) { a1 = sse_load(sb, x, w, alb); b1 = sse_load(rb, x, w, alb); }
            acc = sse_chunk(a0, b0, acc);
            acc = sse_chunk(a1, b1, acc);
        }
    }
    unsigned long long v = (unsigned)acc;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int i = 0; i < SSE_WAVES; i++) t += part[i];
        if (t) atomicAdd(sse + (jb.psum - psum0) + p, t);
    }
}

void launch_sse(hipStream_t st, const JobDev *jobs, int njobs, const FrameLayout &L, const HzPlaneSum *psum0, unsigned long long *sse)
{
    if (njobs <= 0) return;
    const int nb0 = (L.h[0] + SSE_ROWS - 1) / SSE_ROWS, nb1 = (L.h[1] + SSE_ROWS - 1) / SSE_ROWS;
    hipLaunchKernelGGL(k_sse, dim3(nb0 + 2 * nb1, njobs), dim3(64 * SSE_WAVES), 0, st, jobs, L, nb0, nb1, psum0, sse);
}

// ---- SSIM (dsvg_ctx_ssim_enable) -------------------------------------------------------------------------------------------
// Per picture and plane the sum over the 8x8 windows at stride 4 (top-left (4i, 4j), 0 <= 4i <= w - 8, 0 <= 4j <= h - 8) of
//     q = rint(2^32 s),  s = ((P1 + c1) (P2 + c2)) / ((Q1 + c1) (Q2 + c2))   in binary64, this order, no contraction,
// with the window's int32 sums Sa = sum a, Sb = sum b, Sq = sum (a^2 + b^2), Sab = sum ab and P1 = 2 Sa Sb, Q1 = Sa^2 + Sb^2,
// P2 = 2 (64 Sab - Sa Sb), Q2 = 64 Sq - Sa^2 - Sb^2 (each at most 532 684 800 in magnitude); c1 = (0.01 255)^2 64^2,
// c2 = (0.03 255)^2 64^2.  SSIM_FX = sum q, an exact int64 (mean SSIM = SSIM_FX / (2^32 nwin)), added into ssim[3 * out slot + p].
// The definition is stated in numpy by tests/_ssim.py; the two agree to the integer.
//
// Work mapping: a wave takes one strip of 1008 columns (63 lanes x 16; lane 63 reads the next strip's first 16 columns and owns
// nothing) and SSIM_SEG block rows of 4 pixel rows.  Per block row a lane loads 4 rows x 16 bytes of source and reconstruction
// and sums its four 4x4 blocks with v_dot4_u32_u8 (5 per 4 samples: Sa, Sb, a.a + b.b, a.b).  The horizontal window pairs block
// i with i + 1 -- for the lane's last block, the right-hand lane's first (one shuffle per sum); the vertical window adds the
// previous block row's pairs, kept in registers, so a wave reads one block row below its segment (the next wave's first).
// The per-window formula is evaluated on every lane and selected by the window's validity; the lane adds the integer-valued
// q in binary64 (exact: |sum| < 2^53) and converts once.  One 64-bit atomic per workgroup, signed sums as two's complement.
//
// With SSE requested as well (sse != nullptr) the same pass adds, per lane and block it owns, Sq - 2 Sab = sum (a - b)^2 over
// every sample of its segment -- windows or not: bytes beyond the picture read as 0 in both images -- into sse[3 * out slot + p],
// the exact sums k_sse makes.
#define SSIM_WAVES 4
#define SSIM_SEG 8                                    // block rows whose windows (and SSE) a wave owns
#define SSIM_LANES 63                                 // lanes that own columns; the last one only lends its first block
#define SSIM_STRIP (16 * SSIM_LANES)                  // columns per strip

static __device__ __forceinline__ double ssim_q(int sa, int sb, int sq, int sab)
{
#pragma clang fp contract(off)
    const int p1 = 2 * sa * sb, q1 = sa * sa + sb * sb;
    const int p2 = 2 * (64 * sab - sa * sb), q2 = 64 * sq - sa * sa - sb * sb;
    const double c1 = 26634.24, c2 = 239708.16;
    const double s = (((double)p1 + c1) * ((double)p2 + c2)) / (((double)q1 + c1) * ((double)q2 + c2));
    return __builtin_rint(s * 4294967296.0);
}

__global__ __launch_bounds__(64 * SSIM_WAVES) void k_ssim(const JobDev *__restrict__ jobs, FrameLayout L, int nb0, int nb1,
                                                         int ns0, int ns1, const HzPlaneSum *psum0,
                                                         unsigned long long *__restrict__ ssim, unsigned long long *__restrict__ sse)
{
    __shared__ long long part[2][SSIM_WAVES];
    const int bx = (int)blockIdx.x;
    const int p = bx < nb0 ? 0 : 1 + (bx - nb0) / nb1;                  // workgroups [0, nb0) luma, then nb1 per chroma plane
    const int rem = bx < nb0 ? bx : (bx - nb0) % nb1, ns = p ? ns1 : ns0;
    const int strip = rem % ns, rg = rem / ns;
    const JobDev &jb = jobs[blockIdx.y];
    const int w = L.w[p], h = L.h[p];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const auto src = dsvg_global(jb.srcp[p]);
    const size_t ss = (size_t)jb.srcs[p], rs = (size_t)L.stride[p];
    const auto rec = dsvg_global(static_cast<const uint8_t *>((jb.recon ? jb.recon : jb.xf) + L.off[p]));
    const int x = strip * SSIM_STRIP + 16 * lane;
    const int nbr = (h + 3) >> 2, nbyf = h >> 2, nbxf = w >> 2;      // block rows (the last one maybe partial), whole ones, whole columns
    const int cb = x >> 2;                                             // the lane's first block column
    const bool own = lane < SSIM_LANES;
    const int r0 = (rg * SSIM_WAVES + wave) * SSIM_SEG;
    unsigned pa[4] = {0u, 0u, 0u, 0u}, pb[4] = {0u, 0u, 0u, 0u}, pq[4] = {0u, 0u, 0u, 0u}, pab[4] = {0u, 0u, 0u, 0u};   // previous block row's pairs
    double qsum = 0.0;
    unsigned esum = 0u;
    for (int jr = 0; jr <= SSIM_SEG; jr++) {
        const int br = r0 + jr;
        if (br >= (jr < SSIM_SEG ? nbr : nbyf)) break;                 // (the row below the segment: for windows only)
        unsigned sa[4] = {0u, 0u, 0u, 0u}, sb[4] = {0u, 0u, 0u, 0u}, sq[4] = {0u, 0u, 0u, 0u}, sab[4] = {0u, 0u, 0u, 0u};
        uint4 a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {                                  // all loads first: eight 16-byte loads in flight per lane
            const int y = 4 * br + r;
            a[r] = b[r] = make_uint4(0u, 0u, 0u, 0u);
            if (y < h && x < w) {
                const auto sy = src + (size_t)y * ss, ry = rec + (size_t)y * rs;
                const bool al = (((uintptr_t)sy | (uintptr_t)ry) & 15) == 0;
                a[r] = sse_load(sy, x, w, al);
                b[r] = sse_load(ry, x, w, al);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const unsigned av[4] = {a[r].x, a[r].y, a[r].z, a[r].w}, bv[4] = {b[r].x, b[r].y, b[r].z, b[r].w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                sa[i] = __builtin_amdgcn_udot4(av[i], 0x01010101u, sa[i], false);
                sb[i] = __builtin_amdgcn_udot4(bv[i], 0x01010101u, sb[i], false);
                sq[i] = __builtin_amdgcn_udot4(bv[i], bv[i], __builtin_amdgcn_udot4(av[i], av[i], sq[i], false), false);
                sab[i] = __builtin_amdgcn_udot4(av[i], bv[i], sab[i], false);
            }
        }
        if (sse && own && jr < SSIM_SEG) {
#pragma unroll
            for (int i = 0; i < 4; i++) esum += sq[i] - 2u * sab[i];
        }
        // horizontal pairs (block i, block i + 1): the last one with the right-hand lane's first block
        const unsigned na = __shfl_down(sa[0], 1, 64), nb = __shfl_down(sb[0], 1, 64);
        const unsigned nq = __shfl_down(sq[0], 1, 64), nab = __shfl_down(sab[0], 1, 64);
        unsigned ha[4], hb[4], hq[4], hab[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            ha[i] = sa[i] + (i < 3 ? sa[i + 1] : na);
            hb[i] = sb[i] + (i < 3 ? sb[i + 1] : nb);
            hq[i] = sq[i] + (i < 3 ? sq[i + 1] : nq);
            hab[i] = sab[i] + (i < 3 ? sab[i + 1] : nab);
        }
        if (jr > 0 && br < nbyf) {                                     // windows with top block row br - 1 (both rows whole)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const double q = ssim_q((int)(pa[i] + ha[i]), (int)(pb[i] + hb[i]), (int)(pq[i] + hq[i]), (int)(pab[i] + hab[i]));
                qsum += (own && cb + i + 1 < nbxf) ? q : 0.0;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { pa[i] = ha[i]; pb[i] = hb[i]; pq[i] = hq[i]; pab[i] = hab[i]; }
    }
    long long v = (long long)qsum, e = (long long)esum;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { v += __shfl_xor(v, o, 64); e += __shfl_xor(e, o, 64); }
    if (lane == 0) { part[0][wave] = v; part[1][wave] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0, te = 0;
#pragma unroll
        for (int i = 0; i < SSIM_WAVES; i++) { t += part[0][i]; te += part[1][i]; }
        if (t) atomicAdd(ssim + (jb.psum - psum0) + p, (unsigned long long)t);
        if (sse && te) atomicAdd(sse + (jb.psum - psum0) + p, (unsigned long long)te);
    }
}

void launch_ssim(hipStream_t st, const JobDev *jobs, int njobs, const FrameLayout &L, const HzPlaneSum *psum0, unsigned long long *ssim,
                 unsigned long long *sse)
{
    if (njobs <= 0) return;
    const int rows = 4 * SSIM_SEG * SSIM_WAVES;                        // pixel rows per workgroup
    const int ns0 = (L.w[0] + SSIM_STRIP - 1) / SSIM_STRIP, ns1 = (L.w[1] + SSIM_STRIP - 1) / SSIM_STRIP;
    const int nb0 = ns0 * ((L.h[0] + rows - 1) / rows), nb1 = ns1 * ((L.h[1] + rows - 1) / rows);
    hipLaunchKernelGGL(k_ssim, dim3(nb0 + 2 * nb1, njobs), dim3(64 * SSIM_WAVES), 0, st, jobs, L, nb0, nb1, ns0, ns1, psum0, ssim, sse);
}

// ---- source-resolution quality (dsvg_ctx_xres_enable) -----------------------------------------------------------------------
// Per job and plane, the reconstruction (L.w[p] x L.h[p]) upscaled to the REFERENCE plane dims (dw x dh, a resolution ladder's
// source) by the tables of dsv1_resample_weights -- integer arithmetic of k_scale, to the byte what dsv1_resample_clip makes:
//     H = sum_t qh[t] R[y][clamp(sx + t)],  Hs = (H + 128) >> 8,  V = sum_t qv[t] Hs[clamp(sy + t)][x],  U = clamp((V + 2^19) >> 20)
// -- and compared with the reference frame of the job's out slot (xref[out slot], a packed planar frame; nullptr: not measured):
//     SSE[p] = sum (ref - U)^2 over dw x dh samples, and SSIM_FX[p] over the 8x8 windows at stride 4 of dw x dh (k_ssim's formula,
// ssim_q), both exact integers added into xsse / xssim[3 * out slot + p].  Same stream and place as k_sse / k_ssim (code_batch_impl):
// the reconstruction is complete and not yet overwritten.  Upscale or identity only (dw >= sw, dh >= sh): the host refuses less.
// Bounds: the tables' sum |q| < 2 * 16384 is checked on the host for every row (xres_geo_build), so |H| < 2^23, |Hs| < 2^15,
// |V| < 2^30 as in k_scale.
//
// Work mapping: a workgroup of 256 threads owns a 64 x 32 tile of the reference plane (blockIdx.x, the planes' tiles one after the
// other; blockIdx.y = job) and produces U for the tile plus a 4-sample halo right and below (68 x 36: the windows whose origin
// lies in the tile reach 4 samples beyond it):
//   0. the tile's weights into LDS;
//   1. stages the reconstruction rows and columns the tile needs (clamped), and the reference tile, with aligned 16-byte loads
//      (a load is issued only for an aligned chunk that holds a needed byte: it never leaves the 16-byte block of a sample that
//      exists);
//   2. horizontal pass into int32 LDS (rows x 68), vertical pass into bytes (36 x 68);
//   3. 4x4 block sums Sa, Sb, Sa^2 + Sb^2 (Sq), SaSb (Sab) of the 17 x 9 blocks (samples beyond the plane read as 0 in both);
//   4. a thread per owned block (128): its SSE Sq - 2 Sab and the window with that block as its top-left corner, if valid;
//   5. one 64-bit atomic per sum per workgroup.
// LDS (bounded exactly on the host from the tables, xres_geo_build): about 22 KB for 720p -> 1080p or the identity, cubic, so 7
// workgroups per CU of gfx950's 160 KB.  66 VGPRs (occupancy 7 waves per SIMD), no scratch.
#define XR_TW 64
#define XR_TH 32
#define XR_UW (XR_TW + 4)
#define XR_UH (XR_TH + 4)
#define XR_BW (XR_UW / 4)
#define XR_BH (XR_UH / 4)
#define XR_THREADS 256
#define XR_LDS_MAX (64 * 1024)

// rows r0 .. r0 + nrows - 1 (clamped to [0, h - 1]) of a plane, columns lo .. hi, into dst[i * dstride + (x - lo)]
static __device__ __forceinline__ void xr_stage(uint8_t *dst, int dstride, const uint8_t *plane, size_t pstride, int r0, int nrows, int h,
                                                int lo, int hi)
{
    const int span = hi - lo + 1, nch = (span + 15) / 16 + 1;
    for (int it = (int)threadIdx.x; it < nrows * nch; it += XR_THREADS) {
        const int i = it / nch, k = it - i * nch;
        const int sr = min(max(r0 + i, 0), h - 1);
        const uint8_t *row = plane + (size_t)sr * pstride;
        const uintptr_t a = (((uintptr_t)(row + lo)) & ~(uintptr_t)15) + 16u * (uintptr_t)k;
        if (a <= (uintptr_t)(row + hi)) {
            const int4 v = *(const int4 *)a;
            const uint32_t wd[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
            const long long pos0 = (long long)(a - (uintptr_t)(row + lo));
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const long long pos = pos0 + b;
                if (pos >= 0 && pos < span) dst[i * dstride + (int)pos] = (uint8_t)(wd[b >> 2] >> (8 * (b & 3)));
            }
        }
    }
}

__global__ __launch_bounds__(XR_THREADS) void k_xres_quality(const JobDev *__restrict__ jobs, FrameLayout L, const XresPlane *__restrict__ planes,
                                                             const uint8_t *const *__restrict__ xref, const HzPlaneSum *psum0,
                                                             unsigned long long *__restrict__ xsse, unsigned long long *__restrict__ xssim,
                                                             int rows_cap, int th_cap, int tv_cap, int span_cap)
{
    extern __shared__ int4 xr_lds[];
    __shared__ long long part[2][XR_THREADS / 64];
    int *Hs = (int *)xr_lds;                                           // [rows_cap][XR_UW]
    unsigned *bs = (unsigned *)(Hs + (size_t)rows_cap * XR_UW);        // [4][XR_BH * XR_BW]
    short *qh = (short *)(bs + 4 * XR_BH * XR_BW);                     // [XR_UW * th_cap]
    short *qv = qh + XR_UW * th_cap;                                   // [XR_UH * tv_cap] (rounded up to 8)
    uint8_t *stage = (uint8_t *)(qv + ((XR_UH * tv_cap + 7) & ~7));    // [rows_cap][span_cap]
    uint8_t *U = stage + (size_t)rows_cap * span_cap;                  // [XR_UH][XR_UW] upscaled reconstruction
    uint8_t *Rf = U + XR_UH * XR_UW;                                   // [XR_UH][XR_UW] reference
    const JobDev &jb = jobs[blockIdx.y];
    const size_t o3 = (size_t)(jb.psum - psum0);                       // 3 * out slot
    const uint8_t *ref = xref[o3 / 3];
    if (!ref) return;                                                  // (the whole workgroup: this picture is not measured)
    const int tile = blockIdx.x;
    const int p = tile < planes[1].tile0 ? 0 : (tile < planes[2].tile0 ? 1 : 2);
    const XresPlane &P = planes[p];
    const int sw = P.sw, sh = P.sh, dw = P.dw, dh = P.dh, th = P.th, tv = P.tv;
    const int t = tile - P.tile0;
    const int x0 = (t % P.tx) * XR_TW, y0 = (t / P.tx) * XR_TH;
    const int nx = min(XR_UW, dw - x0), ny = min(XR_UH, dh - y0);
    const int r0 = P.vs[y0], nrows = P.vs[y0 + ny - 1] + tv - r0;
    const int lo = max(P.hs[x0], 0), hi = min(P.hs[x0 + nx - 1] + th - 1, sw - 1);
    const uint8_t *rec = (jb.recon ? jb.recon : jb.xf) + L.off[p];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < nx * th; i += XR_THREADS) qh[i] = P.hq[(size_t)x0 * th + i];
    for (int i = tid; i < ny * tv; i += XR_THREADS) qv[i] = P.vq[(size_t)y0 * tv + i];
    xr_stage(stage, span_cap, rec, (size_t)L.stride[p], r0, nrows, sh, lo, hi);
    xr_stage(Rf, XR_UW, ref + P.doff, (size_t)dw, y0, ny, dh, x0, x0 + nx - 1);
    __syncthreads();
    for (int it = tid; it < nrows * nx; it += XR_THREADS) {
        const int i = it / nx, x = it - i * nx;
        const short *w = qh + x * th;
        const uint8_t *srow = stage + i * span_cap - lo;
        const int sx = P.hs[x0 + x];
        int H = 0;
        for (int k = 0; k < th; k++) H += (int)w[k] * (int)srow[min(max(sx + k, 0), sw - 1)];
        Hs[i * XR_UW + x] = (H + 128) >> 8;
    }
    __syncthreads();
    for (int it = tid; it < ny * nx; it += XR_THREADS) {
        const int yy = it / nx, x = it - yy * nx;
        const short *w = qv + yy * tv;
        const int *hc = Hs + (P.vs[y0 + yy] - r0) * XR_UW + x;
        int V = 0;
        for (int k = 0; k < tv; k++) V += (int)w[k] * hc[k * XR_UW];
        U[yy * XR_UW + x] = (uint8_t)min(max((V + (1 << 19)) >> 20, 0), 255);
    }
    __syncthreads();
    for (int b = tid; b < XR_BH * XR_BW; b += XR_THREADS) {
        const int bj = b / XR_BW, bi = b - bj * XR_BW;
        unsigned sa = 0u, sb = 0u, sq = 0u, sab = 0u;
        for (int r = 0; r < 4; r++) {
            const int y = 4 * bj + r;
            for (int c = 0; c < 4; c++) {
                const int x = 4 * bi + c;
                const bool in = y < ny && x < nx;
                const unsigned a = in ? Rf[y * XR_UW + x] : 0u, u = in ? U[y * XR_UW + x] : 0u;
                sa += a; sb += u; sq += a * a + u * u; sab += a * u;
            }
        }
        bs[b] = sa; bs[XR_BH * XR_BW + b] = sb; bs[2 * XR_BH * XR_BW + b] = sq; bs[3 * XR_BH * XR_BW + b] = sab;
    }
    __syncthreads();
    double qsum = 0.0;
    unsigned esum = 0u;
    if (tid < (XR_TW / 4) * (XR_TH / 4)) {
        const int bi = tid % (XR_TW / 4), bj = tid / (XR_TW / 4);
        const int b = bj * XR_BW + bi;
        esum = bs[2 * XR_BH * XR_BW + b] - 2u * bs[3 * XR_BH * XR_BW + b];
        const int gbx = (x0 >> 2) + bi, gby = (y0 >> 2) + bj;
        if (gbx + 1 < (dw >> 2) && gby + 1 < (dh >> 2)) {
            int s[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned *v = bs + k * XR_BH * XR_BW + b;
                s[k] = (int)(v[0] + v[1] + v[XR_BW] + v[XR_BW + 1]);
            }
            qsum = ssim_q(s[0], s[1], s[2], s[3]);
        }
    }
    long long v = (long long)qsum, e = (long long)esum;
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { v += __shfl_xor(v, o, 64); e += __shfl_xor(e, o, 64); }
    if (lane == 0) { part[0][wave] = v; part[1][wave] = e; }
    __syncthreads();
    if (tid == 0) {
        long long tq = 0, te = 0;
#pragma unroll
        for (int i = 0; i < XR_THREADS / 64; i++) { tq += part[0][i]; te += part[1][i]; }
        if (xssim && tq) atomicAdd(xssim + o3 + p, (unsigned long long)tq);
        if (xsse && te) atomicAdd(xsse + o3 + p, (unsigned long long)te);
    }
}

// ------------------------------------------------------------------------------------------------ host side
extern "C" int dsv1_resample_taps(int S, int D, int filter);
extern "C" int dsv1_resample_weights(int S, int D, int filter, int32_t *start, int16_t *q, int T);

static size_t xr_align16(size_t v) { return (v + 15) & ~(size_t)15; }

void xres_geo_free(XresGeo &G)
{
    if (G.planes_d) (void)hipFree(G.planes_d);
    G = XresGeo();
}

// tables of the reconstruction's planes (L) -> the reference's (rw x rh, the same format): [3] XresPlane, then per plane hs int[dw],
// hq short[dw th], vs int[dh], vq short[dh tv]; the LDS of a workgroup, exactly from the tables
int xres_geo_build(XresGeo &G, const FrameLayout &L, int rw, int rh, int filter)
{
    const int RW[3] = {rw, rsu(rw, L.hs), rsu(rw, L.hs)}, RH[3] = {rh, rsu(rh, L.vs), rsu(rh, L.vs)};
    XresPlane pl[3];
    std::vector<std::vector<int32_t>> hs(3), vs(3);
    std::vector<std::vector<int16_t>> hq(3), vq(3);
    size_t off = xr_align16(3 * sizeof(XresPlane)), offs[3][4];
    int tile0 = 0, th_cap = 1, tv_cap = 1, rows_cap = 1, span_cap = 16;
    long long dof = 0;
    for (int p = 0; p < 3; p++) {
        const int sw = L.w[p], sh = L.h[p];
        if (RW[p] < sw || RH[p] < sh) { dsvg_set_error("source-resolution quality: reference plane %d (%dx%d) smaller than the picture's (%dx%d)", p, RW[p], RH[p], sw, sh); return DSVG_ERR_ARG; }
        const int th = dsv1_resample_taps(sw, RW[p], filter), tv = dsv1_resample_taps(sh, RH[p], filter);
        if (th < 0 || tv < 0) { dsvg_set_error("source-resolution quality: %dx%d -> %dx%d is outside the resampler's limits", sw, sh, RW[p], RH[p]); return DSVG_ERR_ARG; }
        hs[p].resize(RW[p]); hq[p].resize((size_t)RW[p] * th); vs[p].resize(RH[p]); vq[p].resize((size_t)RH[p] * tv);
        if (dsv1_resample_weights(sw, RW[p], filter, hs[p].data(), hq[p].data(), th) ||
            dsv1_resample_weights(sh, RH[p], filter, vs[p].data(), vq[p].data(), tv)) { dsvg_set_error("weight tables"); return DSVG_ERR_ARG; }
        // the kernel's int32 bounds (|H| < 2^23, |Hs| < 2^15, |V| < 2^30) and its row / column ranges (starts never decrease)
        for (int tb = 0; tb < 2; tb++) {
            const std::vector<int16_t> &q = tb ? vq[p] : hq[p];
            const std::vector<int32_t> &st = tb ? vs[p] : hs[p];
            const int T = tb ? tv : th;
            for (size_t i = 0; i < st.size(); i++) {
                int a = 0;
                for (int k = 0; k < T; k++) a += std::abs((int)q[i * T + k]);
                if (a >= 2 * 16384 || (i && st[i] < st[i - 1])) { dsvg_set_error("weight table row %zu outside the kernel's bounds", i); return DSVG_ERR_ARG; }
            }
        }
        pl[p].sw = sw; pl[p].sh = sh; pl[p].dw = RW[p]; pl[p].dh = RH[p]; pl[p].th = th; pl[p].tv = tv;
        pl[p].doff = dof;
        dof += (long long)RW[p] * RH[p];
        th_cap = std::max(th_cap, th); tv_cap = std::max(tv_cap, tv);
        for (int x0 = 0; x0 < RW[p]; x0 += XR_TW) {
            const int nx = std::min(XR_UW, RW[p] - x0);
            span_cap = std::max(span_cap, std::min(hs[p][x0 + nx - 1] + th - 1, sw - 1) - std::max(hs[p][x0], 0) + 1);
        }
        for (int y0 = 0; y0 < RH[p]; y0 += XR_TH) {
            const int ny = std::min(XR_UH, RH[p] - y0);
            rows_cap = std::max(rows_cap, vs[p][y0 + ny - 1] + tv - vs[p][y0]);
        }
        pl[p].tx = (RW[p] + XR_TW - 1) / XR_TW;
        pl[p].tile0 = tile0;
        tile0 += pl[p].tx * ((RH[p] + XR_TH - 1) / XR_TH);
        offs[p][0] = off; off = xr_align16(off + sizeof(int32_t) * RW[p]);
        offs[p][1] = off; off = xr_align16(off + sizeof(int16_t) * RW[p] * th);
        offs[p][2] = off; off = xr_align16(off + sizeof(int32_t) * RH[p]);
        offs[p][3] = off; off = xr_align16(off + sizeof(int16_t) * RH[p] * tv);
    }
    span_cap = (int)xr_align16((size_t)span_cap);
    const size_t lds = sizeof(int) * ((size_t)rows_cap * XR_UW + 4 * XR_BH * XR_BW) +
                       sizeof(short) * ((size_t)XR_UW * th_cap + (((size_t)XR_UH * tv_cap + 7) & ~(size_t)7)) +
                       (size_t)rows_cap * span_cap + 2 * XR_UH * XR_UW;
    if (lds > XR_LDS_MAX) { dsvg_set_error("source-resolution quality: a tile needs %zu bytes of LDS", lds); return DSVG_ERR_UNSUPPORTED; }
    XresGeo N;
    N.ntiles = tile0; N.lds = lds; N.rows_cap = rows_cap; N.th_cap = th_cap; N.tv_cap = tv_cap; N.span_cap = span_cap;
    N.rfb = (size_t)dof; N.rw = rw; N.rh = rh; N.filter = filter;
    HIPCHK(hipMalloc((void **)&N.planes_d, off));
    uint8_t *base = (uint8_t *)N.planes_d;
    std::vector<uint8_t> h(off, 0);
    for (int p = 0; p < 3; p++) {
        pl[p].hs = (const int *)(base + offs[p][0]); pl[p].hq = (const short *)(base + offs[p][1]);
        pl[p].vs = (const int *)(base + offs[p][2]); pl[p].vq = (const short *)(base + offs[p][3]);
        memcpy(&h[offs[p][0]], hs[p].data(), sizeof(int32_t) * hs[p].size());
        memcpy(&h[offs[p][1]], hq[p].data(), sizeof(int16_t) * hq[p].size());
        memcpy(&h[offs[p][2]], vs[p].data(), sizeof(int32_t) * vs[p].size());
        memcpy(&h[offs[p][3]], vq[p].data(), sizeof(int16_t) * vq[p].size());
    }
    memcpy(h.data(), pl, sizeof pl);
    const hipError_t e = hipMemcpy(N.planes_d, h.data(), off, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(N.planes_d); (void)hipGetLastError(); dsvg_set_error("table upload failed"); return DSVG_ERR_HIP; }
    xres_geo_free(G);
    G = N;
    return DSVG_OK;
}

void launch_xres(hipStream_t st, const JobDev *jobs, int njobs, const FrameLayout &L, const XresGeo &G, const uint8_t *const *xref,
                 const HzPlaneSum *psum0, unsigned long long *xsse, unsigned long long *xssim)
{
    if (njobs <= 0 || (!xsse && !xssim)) return;
    hipLaunchKernelGGL(k_xres_quality, dim3(G.ntiles, njobs), dim3(XR_THREADS), G.lds, st, jobs, L, (const XresPlane *)G.planes_d, xref, psum0,
                       xsse, xssim, G.rows_cap, G.th_cap, G.tv_cap, G.span_cap);
}
