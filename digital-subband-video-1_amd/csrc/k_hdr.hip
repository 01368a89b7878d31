// k_hdr.hip -- the HDR import (include/dsv1_api.h, HDR sources; stated in numpy in tests/_hdr.py): frames of a deep pixel format with a
// PQ or HLG transfer -> tightly packed planar 8-bit SDR Y, Cb, Cr at 4:4:4, 4:2:2 or 4:2:0.  It is the pass of a dsvg_pixconv
// (k_pixfmt.hip), beside the re-packing converter and the RGB import.  Exact integers: every transcendental lives in the host-built
// tables (host/dsv1_hdr.c); the pixel path is the one function of (tables, layout, upsample) the header states, steps a to i.
//
// Shape, after k_rgb_import: an item is one STEP of 16 pixels of one row, or of a row PAIR where the output's chroma is halved
// vertically (a source halved vertically is never written at full height), so that it owns whole 2x2 cells: per row 16 luma samples
// and the chroma samples the step needs -- of one chroma row, or of two for linear vertical upsampling, the far row an edge select of
// the row index -- brought to the luma grid at 10 bits in registers, 16 pixels through steps c to h, 16 Y bytes and 16 Cb / Cr values
// halved over column pairs ((a + b + 1) >> 1, rounded to 8 bits), then over the two rows.  No 4:4:4 plane ever exists in memory.
// Loads and stores: 16 samples are 32 bytes.  Each of the four streams (luma and chroma words in, Y and chroma bytes out) takes 16-byte
// accesses (8 for halved chroma bytes) when every one of its rows is aligned in every frame -- decided on the host per stream and
// launch from the pointers, offsets, pitches and frame strides: uniform, no per-lane test -- and the step is whole.  Else the byte
// path: loads clamp the column (and the row) to the last one, which IS the edge clamp of the upsampling, and stores write exactly
// the bytes of the pixels that exist; the repeated last column of the halving repeats the last pixel's result.  Nothing between a
// row's end and its pitch, behind the planes or between frames is ever read into a result or written.
// Tables: eotf, gain and oetf (36 360 bytes: dsvg_hdr_tab_pack) are staged in LDS once per workgroup; the grid is sized by CUs, not
// by pixels (the workgroups resident at once: hd_launch), and a workgroup walks items across all frames of the call -- one workgroup per 256 items would fetch more table bytes
// per 1080p frame than the frame holds.  (The same kernel with the three tables read through cached global loads took 1.33 times
// as long at 1080p, 96 pictures: profiles/hdr_cost.txt.  It is not built.)  The 64-bit products of steps e and f are plain C++:
// v_mad_i64_i32 / v_mad_u64_u32.
#include <algorithm>
#include <atomic>
#define DSV1_HDR_FN static __host__ __device__ __forceinline__
#include "dsvg_host.hpp"
#include "dsvg_pixfmt.h"

#define HD_THREADS 256

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct HdrParams {
    long long sfb, dfb;                  // frame to frame: source, planar
    long long soff[3], spitch[3];        // Y, Cb, Cr source planes (interleaved: [1] == [2])
    long long uoff, voff;                // the chroma planes of the planar frame (Y at 0, pitch w; chroma pitch ocw)
    long long total;                     // items of the call
    int w, h, scw, sch, ocw;
    int cstep, cfirst[2];                // words from one chroma sample of a plane to the next; the first of Cb, of Cr
    int vshift, vmask, rs, rnd;          // sample: min(1023, ((word >> vshift & vmask) + rnd) >> rs)
    int linear;
    int ycc[5], in_oy, in_oc, gamut[9], fwd[9], ybias, cbias;
    int cpr, per;                        // steps per row; items per frame
    int vec_sy, vec_sc, vec_y, vec_c;    // 16-byte path of the luma loads, the chroma loads, the Y stores, the chroma stores
};

static __device__ __forceinline__ int hd_clamp(int v, int hi) { return min(max(v, 0), hi); }
// (a + b + 1) >> 1 of four byte pairs
static __device__ __forceinline__ unsigned hd_avg4(unsigned a, unsigned b) { return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu); }
static __device__ __forceinline__ u32x4 hd_ld(const uint8_t *p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p)); }

// N samples i0 .. i0 + N - 1 of a plane's row (sample i: word i * step + first) at 10 bits.  vec: the words lie in aligned 16-byte
// runs and all exist; else word by word (two byte loads: a pitch may be odd), the index clamped to `last`
template <int N> static __device__ __forceinline__ void hd_get(const HdrParams &P, const uint8_t *row, int i0, int last, int step, int first, bool vec, int s[N])
{
    unsigned x[N];
    if (vec) {
        if (step == 1) {
            unsigned d[N / 2];
#pragma unroll
            for (int q = 0; q < N / 8; q++) { const u32x4 a = hd_ld(row + 2 * (long long)i0 + 16 * q); d[4 * q] = a.x; d[4 * q + 1] = a.y; d[4 * q + 2] = a.z; d[4 * q + 3] = a.w; }
#pragma unroll
            for (int i = 0; i < N; i++) x[i] = (d[i >> 1] >> (16 * (i & 1))) & 0xffffu;
        } else {
            unsigned d[N];
#pragma unroll
            for (int q = 0; q < N / 4; q++) { const u32x4 a = hd_ld(row + 4 * (long long)i0 + 16 * q); d[4 * q] = a.x; d[4 * q + 1] = a.y; d[4 * q + 2] = a.z; d[4 * q + 3] = a.w; }
#pragma unroll
            for (int i = 0; i < N; i++) x[i] = (d[i] >> (16 * first)) & 0xffffu;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) {
            const uint8_t *p = row + 2 * ((long long)min(i0 + i, last) * step + first);
            x[i] = (unsigned)p[0] | ((unsigned)p[1] << 8);
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) s[i] = min(1023, (int)((((x[i] >> P.vshift) & (unsigned)P.vmask) + (unsigned)P.rnd) >> P.rs));
}

// one sample, the index already inside the row
static __device__ __forceinline__ int hd_get1(const HdrParams &P, const uint8_t *row, int i, int step, int first)
{
    const uint8_t *p = row + 2 * ((long long)i * step + first);
    const unsigned x = (unsigned)p[0] | ((unsigned)p[1] << 8);
    return min(1023, (int)((((x >> P.vshift) & (unsigned)P.vmask) + (unsigned)P.rnd) >> P.rs));
}

// step b: one chroma plane on the luma grid for the 16 pixels from x0 of luma row y (the RGB output pass's rule, on 10-bit samples)
template <int SHS, int SVS> static __device__ __forceinline__ void hd_chroma(const HdrParams &P, const uint8_t *plane, long long pitch, int first, int y, int x0, bool vec, int out[16])
{
    constexpr int N = SHS ? 8 : 16, B = SHS ? 1 : 0;
    const int j = y >> SVS, c0 = x0 >> SHS;
    const bool vblend = SVS && P.linear, hblend = SHS && P.linear;
    const uint8_t *rn = plane + (long long)j * pitch, *rf = rn;
    if (vblend) rf = plane + (long long)((y & 1) ? min(j + 1, P.sch - 1) : max(j - 1, 0)) * pitch;        // edge rows: a select of the index
    int cv[N + 2 * B], nr[N];
    hd_get<N>(P, rn, c0, P.scw - 1, P.cstep, first, vec, nr);
    if (vblend) {
        int fr[N];
        hd_get<N>(P, rf, c0, P.scw - 1, P.cstep, first, vec, fr);
#pragma unroll
        for (int i = 0; i < N; i++) nr[i] = (3 * nr[i] + fr[i] + 2) >> 2;
    }
#pragma unroll
    for (int i = 0; i < N; i++) cv[B + i] = nr[i];
    if (SHS) {
        cv[0] = cv[1]; cv[N + 1] = cv[N];
        if (hblend) {
            const int xl = max(c0 - 1, 0), xr = min(c0 + 8, P.scw - 1);
            const int a = hd_get1(P, rn, xl, P.cstep, first), b = hd_get1(P, rn, xr, P.cstep, first);
            cv[0] = vblend ? (3 * a + hd_get1(P, rf, xl, P.cstep, first) + 2) >> 2 : a;
            cv[N + 1] = vblend ? (3 * b + hd_get1(P, rf, xr, P.cstep, first) + 2) >> 2 : b;
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (!SHS) out[i] = cv[i];
        else {
            const int k = i >> 1;
            out[i] = hblend ? (3 * cv[1 + k] + ((i & 1) ? cv[2 + k] : cv[k]) + 2) >> 2 : cv[1 + k];
        }
    }
}

// steps c to h of one pixel.  T: the lookup tables in LDS, eotf at 0, gain at 4096, oetf (16-bit entries) at 4096 + DSV1_HDR_NBUCKETS
static __device__ __forceinline__ void hd_pixel(const HdrParams &P, const unsigned *T, int Y, int U, int V, int &oy, int &ob, int &orr)
{
    const unsigned *gain = T + 4096;
    const unsigned short *oetf = reinterpret_cast<const unsigned short *>(T + 4096 + DSV1_HDR_NBUCKETS);
    const int y = Y - P.in_oy, u = U - P.in_oc, v = V - P.in_oc;
    const int l = P.ycc[0] * y + 8192;
    const long long lr = T[hd_clamp((l + P.ycc[1] * v) >> 14, 4095)];
    const long long lg = T[hd_clamp((l + P.ycc[2] * u + P.ycc[3] * v) >> 14, 4095)];
    const long long lb = T[hd_clamp((l + P.ycc[4] * u) >> 14, 4095)];
    const long long one = (long long)DSV1_HDR_ONE;
    const long long r = min(max((P.gamut[0] * lr + P.gamut[1] * lg + P.gamut[2] * lb + 8192) >> 14, 0LL), one);
    const long long g = min(max((P.gamut[3] * lr + P.gamut[4] * lg + P.gamut[5] * lb + 8192) >> 14, 0LL), one);
    const long long b = min(max((P.gamut[6] * lr + P.gamut[7] * lg + P.gamut[8] * lb + 8192) >> 14, 0LL), one);
    const unsigned m = (unsigned)max(r, max(g, b));
    const unsigned long long k = gain[dsv1_hdr_cidx(m)];
    const unsigned tr = (unsigned)min(((unsigned long long)r * k + 32768u) >> 16, (unsigned long long)one);
    const unsigned tg = (unsigned)min(((unsigned long long)g * k + 32768u) >> 16, (unsigned long long)one);
    const unsigned tb = (unsigned)min(((unsigned long long)b * k + 32768u) >> 16, (unsigned long long)one);
    const int er = oetf[dsv1_hdr_cidx(tr)], eg = oetf[dsv1_hdr_cidx(tg)], eb = oetf[dsv1_hdr_cidx(tb)];
    // clamp(x >> 20, 0, 255), the clamp done on x: written the other way round the compiler pairs the results up with
    // v_ashr_pk_u8_i32, whose upper half it gets wrong on gfx950 (the ISA check in the Makefile)
    const int top = (256 << 20) - 1;
    oy = hd_clamp(P.fwd[0] * er + P.fwd[1] * eg + P.fwd[2] * eb + P.ybias, top) >> 20;
    ob = hd_clamp(P.fwd[3] * er + P.fwd[4] * eg + P.fwd[5] * eb + P.cbias, top) >> 20;
    orr = hd_clamp(P.fwd[6] * er + P.fwd[7] * eg + P.fwd[8] * eb + P.cbias, top) >> 20;
}

// N (16 or 8) bytes held in v[] to row + x0: one store, or the first n of them byte by byte
template <int N> static __device__ __forceinline__ void hd_put(uint8_t *row, int x0, int n, bool vec, const unsigned v[4])
{
    if (vec) {
        if (N == 16) { u32x4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3]; *reinterpret_cast<u32x4 *>(row + x0) = o; }
        else { u32x2 o; o.x = v[0]; o.y = v[1]; *reinterpret_cast<u32x2 *>(row + x0) = o; }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) if (i < n) row[x0 + i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
    }
}

// the 16 pixels from x0 of luma row y (n of them exist) -> 16 Y bytes in yy[0..3] and their Cb / Cr bytes: all 16 in cb / cr[0..3], or
// halved over column pairs in [0..1]
template <int SHS, int SVS, int DHS>
static __device__ __forceinline__ void hd_row(const HdrParams &P, const unsigned *lt, const uint8_t *frame, int y, int x0, int n, bool whole,
                                              unsigned yy[4], unsigned cb[4], unsigned cr[4])
{
    int Y[16], U[16], V[16];
    hd_get<16>(P, frame + P.soff[0] + (long long)y * P.spitch[0], x0, P.w - 1, 1, 0, P.vec_sy && whole, Y);
    hd_chroma<SHS, SVS>(P, frame + P.soff[1], P.spitch[1], P.cfirst[0], y, x0, P.vec_sc && whole, U);
    hd_chroma<SHS, SVS>(P, frame + P.soff[2], P.spitch[2], P.cfirst[1], y, x0, P.vec_sc && whole, V);
#pragma unroll
    for (int j = 0; j < 4; j++) yy[j] = cb[j] = cr[j] = 0;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        int L[2], B[2], R[2];
        hd_pixel(P, lt, Y[i], U[i], V[i], L[0], B[0], R[0]);
        hd_pixel(P, lt, Y[i + 1], U[i + 1], V[i + 1], L[1], B[1], R[1]);
        yy[i >> 2] |= ((unsigned)L[0] << (8 * (i & 3))) | ((unsigned)L[1] << (8 * ((i + 1) & 3)));
        if (DHS) {
            const int j = i >> 1;
            if (i + 1 >= n) { B[1] = B[0]; R[1] = R[0]; }          // the repeated last column of the halving
            cb[j >> 2] |= (unsigned)((B[0] + B[1] + 1) >> 1) << (8 * (j & 3));
            cr[j >> 2] |= (unsigned)((R[0] + R[1] + 1) >> 1) << (8 * (j & 3));
        } else {
            cb[i >> 2] |= ((unsigned)B[0] << (8 * (i & 3))) | ((unsigned)B[1] << (8 * ((i + 1) & 3)));
            cr[i >> 2] |= ((unsigned)R[0] << (8 * (i & 3))) | ((unsigned)R[1] << (8 * ((i + 1) & 3)));
        }
    }
}

template <int SHS, int SVS, int DHS, int DVS>
__global__ __launch_bounds__(HD_THREADS) void k_hdr_import(const HdrParams P, const unsigned *__restrict__ tab, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst)
{
    __shared__ unsigned lt[DSVG_HDR_TAB_WORDS];
    for (int i = (int)threadIdx.x; i < DSVG_HDR_TAB_WORDS; i += HD_THREADS) lt[i] = tab[i];
    __syncthreads();
    for (long long item = (long long)blockIdx.x * HD_THREADS + (int)threadIdx.x; item < P.total; item += (long long)gridDim.x * HD_THREADS) {
        const long long f = item / P.per;
        const int rem = (int)(item - f * P.per);
        const int g = rem / P.cpr, c = rem - g * P.cpr;
        const int x0 = 16 * c, n = min(16, P.w - x0);
        const bool whole = n == 16;
        const uint8_t *frame = src + f * P.sfb;
        uint8_t *out = dst + f * P.dfb;
        const int y0 = g << DVS;
        unsigned cbs[4], crs[4];
#pragma unroll 1
        for (int r = 0; r <= DVS; r++) {
            // the second row of the cells; beyond the frame it is the first one again -- the repeated last row of the halving
            unsigned yy[4], cb[4], cr[4];
            hd_row<SHS, SVS, DHS>(P, lt, frame, min(y0 + r, P.h - 1), x0, n, whole, yy, cb, cr);
            if (y0 + r < P.h) hd_put<16>(out + (long long)(y0 + r) * P.w, x0, n, P.vec_y && whole, yy);
#pragma unroll
            for (int j = 0; j < 4; j++) { cbs[j] = r ? hd_avg4(cbs[j], cb[j]) : cb[j]; crs[j] = r ? hd_avg4(crs[j], cr[j]) : cr[j]; }
        }
        uint8_t *urow = out + P.uoff + (long long)g * P.ocw, *vrow = out + P.voff + (long long)g * P.ocw;
        if (DHS) {
            const int nc = min(8, P.ocw - 8 * c);
            hd_put<8>(urow, 8 * c, nc, P.vec_c && whole, cbs);
            hd_put<8>(vrow, 8 * c, nc, P.vec_c && whole, crs);
        } else {
            hd_put<16>(urow, x0, n, P.vec_c && whole, cbs);
            hd_put<16>(vrow, x0, n, P.vec_c && whole, crs);
        }
    }
}

// The grid: the workgroups that are resident at once, no more -- a workgroup that waits for a place would stage the tables again.
// How many fit on a CU is the runtime's answer for the kernel (LDS allows four; the registers of the row-pair kernels allow fewer),
// asked once per kernel and process: the answer is not kept per device, so on a machine with GPUs of different kinds the first
// device's answer serves all of them -- a grid that is then too large or too small is slower, never wrong.
template <int SHS, int SVS, int DHS, int DVS> static int hd_launch(const HdrParams &P, int cus, hipStream_t st, const unsigned *tab, const uint8_t *src, uint8_t *dst)
{
    static std::atomic<int> per_cu{0};
    int n = per_cu.load();
    if (!n) {
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_hdr_import<SHS, SVS, DHS, DVS>, HD_THREADS, 0));
        if (n < 1) { dsvg_set_error("HDR import: the kernel does not fit on a CU"); return DSVG_ERR_HIP; }
        per_cu.store(n);
    }
    const unsigned grid = (unsigned)std::min<long long>((P.total + HD_THREADS - 1) / HD_THREADS, (long long)n * cus);
    hipLaunchKernelGGL((k_hdr_import<SHS, SVS, DHS, DVS>), dim3(grid), dim3(HD_THREADS), 0, st, P, tab, src, dst);
    return DSVG_OK;
}

// eotf, gain, then oetf two entries to a dword: what the kernel stages
extern "C" void dsvg_hdr_tab_pack(const dsv1_hdr_tables *t, uint32_t *words)
{
    memcpy(words, t->eotf, sizeof t->eotf);
    memcpy(words + 4096, t->gain, sizeof t->gain);
    words[DSVG_HDR_TAB_WORDS - 1] = 0;
    memcpy(words + 4096 + DSV1_HDR_NBUCKETS, t->oetf, sizeof t->oetf);
}

extern "C" void dsvg_hdr_rows_of(const dsv1_hdr_tables *t, dsvg_hdr_rows *r)
{
    memcpy(r->ycc, t->ycc, sizeof r->ycc); memcpy(r->gamut, t->gamut, sizeof r->gamut); memcpy(r->fwd, t->fwd, sizeof r->fwd);
    r->in_oy = t->in_oy; r->in_oc = t->in_oc; r->ybias = t->ybias; r->cbias = t->cbias;
}

extern "C" int dsvg_hdr_import_run(void *stream, const dsv1_hdr_layout *L, const dsvg_hdr_rows *t, const uint32_t *tab_dev, int upsample, int cus,
                                   const void *src_dev, int nframes, void *dst_dev)
{
    if (!L || !t || !tab_dev || !src_dev || !dst_dev || nframes < 1 || cus < 1) { dsvg_set_error("bad HDR import arguments"); return DSVG_ERR_ARG; }
    if (upsample != DSV1_CHROMA_REPLICATE && upsample != DSV1_CHROMA_LINEAR) { dsvg_set_error("HDR import: unknown upsampling mode"); return DSVG_ERR_ARG; }
    if (L->shs < L->svs || L->shs > 1 || L->svs < 0 || L->dhs < L->dvs || L->dhs > 1 || L->dhs < L->shs || L->dvs < L->svs || L->w < 1 || L->h < 1 ||
        L->semi < 0 || L->semi > 2 || (L->semi && !L->shs)) {
        dsvg_set_error("HDR import: subsampling not offered"); return DSVG_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    HdrParams P;
    memset(&P, 0, sizeof P);
    P.sfb = (long long)L->frame_bytes; P.dfb = (long long)L->out_frame_bytes;
    P.w = L->w; P.h = L->h; P.scw = L->scw; P.sch = L->sch; P.ocw = L->ocw;
    P.uoff = (long long)L->w * L->h; P.voff = P.uoff + (long long)L->ocw * L->och;
    for (int p = 0; p < 3; p++) { P.soff[p] = (long long)L->off[p]; P.spitch[p] = (long long)L->pitch[p]; }
    P.cstep = L->semi ? 2 : 1;
    P.cfirst[0] = L->semi == 2 ? 1 : 0; P.cfirst[1] = L->semi == 1 ? 1 : 0;
    P.vshift = L->vshift; P.vmask = L->vmask; P.rs = L->rs; P.rnd = L->rnd;
    P.linear = upsample == DSV1_CHROMA_LINEAR;
    memcpy(P.ycc, t->ycc, sizeof P.ycc); memcpy(P.gamut, t->gamut, sizeof P.gamut); memcpy(P.fwd, t->fwd, sizeof P.fwd);
    P.in_oy = t->in_oy; P.in_oc = t->in_oc; P.ybias = t->ybias; P.cbias = t->cbias;
    P.cpr = (L->w + 15) / 16;
    const long long per = (long long)P.cpr * (L->dvs ? L->och : L->h);
    if (per > INT_MAX / 2) { dsvg_set_error("frame too large for the HDR import's grid"); return DSVG_ERR_UNSUPPORTED; }
    P.per = (int)per;
    P.total = per * nframes;
    P.vec_sy = !(((uintptr_t)src_dev | (uintptr_t)P.sfb | (uintptr_t)P.soff[0] | (uintptr_t)P.spitch[0]) & 15);
    P.vec_sc = !(((uintptr_t)src_dev | (uintptr_t)P.sfb | (uintptr_t)P.soff[1] | (uintptr_t)P.soff[2] | (uintptr_t)P.spitch[1] | (uintptr_t)P.spitch[2]) & 15);
    P.vec_y = !(((uintptr_t)dst_dev | (uintptr_t)P.dfb | (uintptr_t)P.w) & 15);
    P.vec_c = !(((uintptr_t)dst_dev | (uintptr_t)P.dfb | (uintptr_t)P.uoff | (uintptr_t)P.voff | (uintptr_t)P.ocw) & (L->dhs ? 7 : 15));
    const uint8_t *s = (const uint8_t *)src_dev;
    uint8_t *d = (uint8_t *)dst_dev;
    int rc;
    switch (L->shs + L->svs + 3 * (L->dhs + L->dvs)) {      // source 0: 4:4:4, 1: 4:2:2, 2: 4:2:0; three times the output's
    case 0:  rc = hd_launch<0, 0, 0, 0>(P, cus, st, tab_dev, s, d); break;
    case 3:  rc = hd_launch<0, 0, 1, 0>(P, cus, st, tab_dev, s, d); break;
    case 4:  rc = hd_launch<1, 0, 1, 0>(P, cus, st, tab_dev, s, d); break;
    case 6:  rc = hd_launch<0, 0, 1, 1>(P, cus, st, tab_dev, s, d); break;
    case 7:  rc = hd_launch<1, 0, 1, 1>(P, cus, st, tab_dev, s, d); break;
    case 8:  rc = hd_launch<1, 1, 1, 1>(P, cus, st, tab_dev, s, d); break;
    default: dsvg_set_error("HDR import: subsampling not offered"); return DSVG_ERR_ARG;
    }
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}
