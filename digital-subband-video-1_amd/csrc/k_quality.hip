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
