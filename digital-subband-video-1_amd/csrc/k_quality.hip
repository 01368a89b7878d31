// k_quality.hip -- opt-in quality measurement of the encoder (dsvg_ctx_sse_enable): per picture and plane the sum of squared
// errors between the source and the reconstruction over the picture area (borders excluded),
//     SSE[p] = sum over the w[p] x h[p] samples of (src - recon)^2,
// an exact 64-bit integer.  DSV1 is closed-loop, so the reconstruction is what a decoder shows; PSNR follows on the host.
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
