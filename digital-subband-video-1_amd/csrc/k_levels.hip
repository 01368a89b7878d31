// k_levels.hip -- the levels pass and the per-plane histogram (include/dsv1_api.h, Levels; stated in numpy in tests/_levels.py): tightly
// packed planar 8-bit frames in, out_p[i] = lut[p][in_p[i]] out, and hist[t][p][v] = the samples of plane p of frame t with value v.
//
// k_levels: the clip is one flat byte array, one launch covers it.  The items are 16-byte chunks ALIGNED in the destination, counted
// from the destination's address rounded down to 16 (head = dst & 15 bytes in front of the clip belong to chunk 0 and are never
// touched).  A block takes LV_CHUNKS * LV_THREADS consecutive chunks (64 KiB), thread t the chunks t, t + 256, ...: a wave's loads and
// stores are 1 KiB runs.  A chunk that lies whole inside one plane of one frame is ONE unaligned 16-byte load (aligned too where the
// source has the destination's alignment, and always when dst == src), sixteen table lookups and ONE aligned 16-byte store; the
// first and the last chunk of the clip, and every chunk a plane or frame boundary falls into, choose the table and store per byte.
// The offset inside the frame is a 64-bit remainder once per block and a 32-bit one per chunk.  Every byte of the clip is read and
// written by exactly one thread, the read first, so dst == src is fine; nothing outside the clip is loaded or stored.
//   Tables: the three tables come as 256 dwords, entry v = lut[0][v] | lut[1][v] << 8 | lut[2][v] << 16 (device memory of the pass).
//        Staged in LDS once per block, REP times over: dword v * REP + (lane % REP).  A lookup is a byte read (ds_read_u8) at byte
//        p of the lane's own copy of entry v.
//   Banks (byte and dword LDS reads are served per 32-lane half on dword address mod 32): with REP = 32 the dword address is
//        32 v + lane % 32, bank lane % 32 whatever the sample -- conflict-free for every picture, 2 LDS cycles per wave-instruction,
//        32 per chunk and wave; 32 KiB of LDS, five blocks per CU.  With REP = 1 the bank is v mod 32: a flat picture broadcasts, a
//        noise picture meets ~3.5 lanes per busiest bank.  Both are built; dsvg_levels_set_replicas chooses (default 32), and
//        tools/levels_cost.py times them side by side (profiles/levels_cost.txt).
//        Staging: thread v loads entry v and writes its 32 copies, copy (k + v) mod 32 in step k: the lanes of a half-wave write 32
//        different banks in every step.
//
// k_histogram: a block is within ONE frame (blockIdx.y), HG_CHUNKS * HG_THREADS chunks of it (128 KiB), aligned in the SOURCE frame
// (the frame's own head), so a 16-byte load is aligned; whole one-plane chunks count sixteen samples, the others per byte.  Counts are
// privatised per WAVE in LDS ([4][3][256] dwords, LDS integer atomics), summed over the waves at the end and merged into the output
// with one global integer atomicAdd per non-zero bin and block (the output is zeroed on the stream first).
//   Flat pictures: 64 lanes adding to one LDS address serialise.  Where every active lane of the wave holds the same 16 bytes of the
//        same plane -- one compare against the first lane's and a ballot -- ONE lane adds the lane count sixteen times instead.  A
//        flat picture, black bars and clipped skies take this path; the count is the same either way.
//   Exact: a bin holds at most a plane's sample count < 2^31.
#include <algorithm>
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

#define LV_THREADS 256
#define LV_CHUNKS 16                     // chunks per thread and block
#define LV_REP 32                        // copies of the table in LDS: one per bank
#define HG_THREADS 256
#define HG_CHUNKS 32

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4a1 __attribute__((ext_vector_type(4), aligned(1)));       // 16 bytes at any address

struct LvParams {
    unsigned e0, e1, fb;                 // a frame: luma in [0, e0), U in [e0, e1), V in [e1, fb)
    unsigned head;                       // dst & 15
    long long nbytes;                    // the clip
};

static __device__ __forceinline__ int lv_plane(unsigned r, const LvParams &P) { return r < P.e0 ? 0 : r < P.e1 ? 1 : 2; }
// the plane a 16-byte run at frame offset r lies whole in, or -1
static __device__ __forceinline__ int lv_plane16(unsigned r, const LvParams &P)
{
    if (r + 16 <= P.e0) return 0;
    if (r >= P.e0 && r + 16 <= P.e1) return 1;
    if (r >= P.e1 && r + 16 <= P.fb) return 2;
    return -1;
}

template <int REP>
__global__ __launch_bounds__(LV_THREADS) void k_levels(const LvParams P, const unsigned *__restrict__ tab, const uint8_t *src, uint8_t *dst)
{
    __shared__ unsigned lut[256 * REP];
    const int tid = (int)threadIdx.x;
    {
        const unsigned e = tab[tid];                     // thread v writes the REP copies of entry v, copy (k + v) mod REP in step k
#pragma unroll 8
        for (int k = 0; k < REP; k++) lut[tid * REP + ((k + tid) & (REP - 1))] = e;
    }
    __syncthreads();
    const uint8_t *lb = reinterpret_cast<const uint8_t *>(lut) + 4 * (tid & (REP - 1));
    const long long q0 = (long long)blockIdx.x * (16LL * LV_CHUNKS * LV_THREADS);       // the block's first chunk, from dst - head
    const unsigned rb = (unsigned)((q0 + 16LL * P.fb - P.head) % (long long)P.fb);      // ... and its offset inside its frame
#pragma unroll 4
    for (int k = 0; k < LV_CHUNKS; k++) {
        const unsigned t16 = 16u * (unsigned)(k * LV_THREADS + tid);
        const long long o = q0 - P.head + t16;           // the chunk inside the clip (chunk 0: -head)
        if (o >= P.nbytes) break;
        const unsigned r = (rb + t16) % P.fb;            // (rb < fb < 2^31 - 2^16, t16 < 2^16)
        const int p = o >= 0 && o + 16 <= P.nbytes ? lv_plane16(r, P) : -1;
        if (p >= 0) {
            const u32x4a1 s = *reinterpret_cast<const u32x4a1 *>(src + o);
            const uint8_t *lp = lb + p;
            u32x4 v;
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const unsigned w = s[d];
                v[d] = (unsigned)lp[(w & 255u) * (4 * REP)] | (unsigned)lp[((w >> 8) & 255u) * (4 * REP)] << 8 |
                       (unsigned)lp[((w >> 16) & 255u) * (4 * REP)] << 16 | (unsigned)lp[(w >> 24) * (4 * REP)] << 24;
            }
            *reinterpret_cast<u32x4 *>(dst + o) = v;
        } else {
            for (int b = 0; b < 16; b++) {
                const long long ob = o + b;
                if (ob < 0 || ob >= P.nbytes) continue;
                unsigned rr = r + (unsigned)b;
                if (rr >= P.fb) rr %= P.fb;
                dst[ob] = lb[(unsigned)src[ob] * (4 * REP) + lv_plane(rr, P)];
            }
        }
    }
}

__global__ __launch_bounds__(HG_THREADS) void k_histogram(const LvParams P, const uint8_t *__restrict__ src, unsigned *__restrict__ hist)
{
    __shared__ unsigned cnt[HG_THREADS / 64][768];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < (HG_THREADS / 64) * 768; i += HG_THREADS) (&cnt[0][0])[i] = 0;
    __syncthreads();
    unsigned *c = cnt[tid >> 6];
    const uint8_t *fr = src + (long long)blockIdx.y * P.fb;
    const int head = (int)((uintptr_t)fr & 15);
    const int fb = (int)P.fb;
    for (int k = 0; k < HG_CHUNKS; k++) {
        // (fb + 30 < 2^31: the chunk's offset inside the frame is an int)
        const long long q = (((long long)blockIdx.x * HG_CHUNKS + k) * HG_THREADS + tid) * 16;
        if (q - head >= fb) break;
        const int r = (int)(q - head);
        const int p = r >= 0 && r + 16 <= fb ? lv_plane16((unsigned)r, P) : -1;
        if (p >= 0) {
            const u32x4 s = *reinterpret_cast<const u32x4 *>(fr + r);
            const unsigned x0 = __builtin_amdgcn_readfirstlane(s.x), y0 = __builtin_amdgcn_readfirstlane(s.y);
            const unsigned z0 = __builtin_amdgcn_readfirstlane(s.z), w0 = __builtin_amdgcn_readfirstlane(s.w);
            const int p0 = __builtin_amdgcn_readfirstlane(p);
            const unsigned long long act = __ballot(1);
            const unsigned long long same = __ballot(s.x == x0 && s.y == y0 && s.z == z0 && s.w == w0 && p == p0);
            if (same == act) {
                if ((tid & 63) == __ffsll((long long)act) - 1) {
                    const unsigned nl = (unsigned)__popcll(act);
#pragma unroll
                    for (int d = 0; d < 4; d++)
#pragma unroll
                        for (int b = 0; b < 4; b++) atomicAdd(&c[p * 256 + ((s[d] >> (8 * b)) & 255u)], nl);
                }
            } else {
#pragma unroll
                for (int d = 0; d < 4; d++)
#pragma unroll
                    for (int b = 0; b < 4; b++) atomicAdd(&c[p * 256 + ((s[d] >> (8 * b)) & 255u)], 1u);
            }
        } else {
            for (int b = 0; b < 16; b++) {
                const int rr = r + b;
                if (rr >= 0 && rr < fb) atomicAdd(&c[lv_plane((unsigned)rr, P) * 256 + fr[rr]], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < 768; i += HG_THREADS) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < HG_THREADS / 64; w++) s += cnt[w][i];
        if (s) atomicAdd(&hist[(size_t)blockIdx.y * 768 + i], s);
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct dsvg_levels {
    int device = 0, rep = LV_REP;
    LvParams P;
    unsigned *tab = nullptr;             // 256 packed entries, device memory
};

static int lv_geometry(LvParams *P, int w, int h, int subsamp)
{
    if (w < 1 || h < 1 || (subsamp != DSV_SUBSAMP_444 && subsamp != DSV_SUBSAMP_422 && subsamp != DSV_SUBSAMP_420 && subsamp != DSV_SUBSAMP_411)) return DSVG_ERR_ARG;
    const long long y = (long long)w * h, c = (long long)rsu(w, fmt_hs(subsamp)) * rsu(h, fmt_vs(subsamp));
    // (the kernels keep offsets inside a frame, plus a block's span, in 32 bits)
    if (y + 2 * c > INT_MAX - (1 << 17)) return DSVG_ERR_UNSUPPORTED;
    memset(P, 0, sizeof *P);
    P->e0 = (unsigned)y; P->e1 = (unsigned)(y + c); P->fb = (unsigned)(y + 2 * c);
    return DSVG_OK;
}

extern "C" void dsvg_levels_destroy(dsvg_levels *l)
{
    if (!l) return;
    if (l->tab) { (void)hipSetDevice(l->device); (void)hipFree(l->tab); }
    delete l;
}

extern "C" int dsvg_levels_create(dsvg_levels **out, int device, const dsv1_levels *lv, int w, int h, int subsamp)
{
    LvParams P;
    int rc;
    if (!out || !lv) { dsvg_set_error("bad levels arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if ((rc = lv_geometry(&P, w, h, subsamp))) { dsvg_set_error(rc == DSVG_ERR_ARG ? "bad levels arguments" : "picture too large for the levels pass"); return rc; }
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    unsigned packed[256];
    for (int v = 0; v < 256; v++) packed[v] = (unsigned)lv->lut[0][v] | (unsigned)lv->lut[1][v] << 8 | (unsigned)lv->lut[2][v] << 16;
    dsvg_levels *l = new dsvg_levels();
    l->device = device; l->P = P;
    if (hipSetDevice(device) != hipSuccess || hipMalloc((void **)&l->tab, sizeof packed) != hipSuccess) {
        l->tab = nullptr; dsvg_levels_destroy(l); (void)hipGetLastError();
        dsvg_set_error("no device memory for the levels tables"); return DSVG_ERR_HIP;
    }
    if (hipMemcpy(l->tab, packed, sizeof packed, hipMemcpyHostToDevice) != hipSuccess) {
        dsvg_levels_destroy(l); (void)hipGetLastError();
        dsvg_set_error("levels tables: upload failed"); return DSVG_ERR_HIP;
    }
    *out = l;
    return DSVG_OK;
}

// measurements (tools/levels_cost.py): the copies of the table a block keeps in LDS, 32 (one per bank, the default) or 1
extern "C" int dsvg_levels_set_replicas(dsvg_levels *l, int rep)
{
    if (!l || (rep != 1 && rep != LV_REP)) return DSVG_ERR_ARG;
    l->rep = rep;
    return DSVG_OK;
}

extern "C" int dsvg_levels_run(dsvg_levels *l, void *stream, const void *src_dev, int nframes, void *dst_dev)
{
    if (!l || !src_dev || !dst_dev || nframes < 1) { dsvg_set_error("bad levels arguments"); return DSVG_ERR_ARG; }
    HIPCHK(hipSetDevice(l->device));
    LvParams P = l->P;
    P.head = (unsigned)((uintptr_t)dst_dev & 15);
    P.nbytes = (long long)P.fb * nframes;
    const long long nchunks = (P.head + P.nbytes + 15) / 16, per = (long long)LV_CHUNKS * LV_THREADS;
    const long long blocks = (nchunks + per - 1) / per;
    if (blocks > INT_MAX) { dsvg_set_error("clip too large for the levels pass's grid"); return DSVG_ERR_UNSUPPORTED; }
    if (l->rep == 1) hipLaunchKernelGGL(k_levels<1>, dim3((unsigned)blocks), dim3(LV_THREADS), 0, (hipStream_t)stream, P, l->tab, (const uint8_t *)src_dev, (uint8_t *)dst_dev);
    else hipLaunchKernelGGL(k_levels<LV_REP>, dim3((unsigned)blocks), dim3(LV_THREADS), 0, (hipStream_t)stream, P, l->tab, (const uint8_t *)src_dev, (uint8_t *)dst_dev);
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

struct dsvg_histogram {
    int device = 0;
    LvParams P;
};

extern "C" void dsvg_histogram_destroy(dsvg_histogram *g) { delete g; }

extern "C" int dsvg_histogram_create(dsvg_histogram **out, int device, int w, int h, int subsamp)
{
    LvParams P;
    int rc;
    if (!out) { dsvg_set_error("bad histogram arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if ((rc = lv_geometry(&P, w, h, subsamp))) { dsvg_set_error(rc == DSVG_ERR_ARG ? "bad histogram arguments" : "picture too large for the histogram"); return rc; }
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_histogram *g = new dsvg_histogram();
    g->device = device; g->P = P;
    *out = g;
    return DSVG_OK;
}

// nframes frames -> hist_dev [nframes][3][256] (uint32, device memory)
extern "C" int dsvg_histogram_run(dsvg_histogram *g, void *stream, const void *src_dev, int nframes, void *hist_dev)
{
    if (!g || !src_dev || !hist_dev || nframes < 1) { dsvg_set_error("bad histogram arguments"); return DSVG_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(g->device));
    HIPCHK(hipMemsetAsync(hist_dev, 0, sizeof(unsigned) * 768 * (size_t)nframes, st));
    const long long nchunks = ((long long)g->P.fb + 30) / 16, per = (long long)HG_CHUNKS * HG_THREADS;
    const unsigned blocks = (unsigned)((nchunks + per - 1) / per);
    for (int f0 = 0; f0 < nframes; f0 += 65535) {
        const int nf = std::min(65535, nframes - f0);
        hipLaunchKernelGGL(k_histogram, dim3(blocks, nf), dim3(HG_THREADS), 0, st, g->P, (const uint8_t *)src_dev + (size_t)f0 * g->P.fb,
                           (unsigned *)hist_dev + (size_t)f0 * 768);
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}
