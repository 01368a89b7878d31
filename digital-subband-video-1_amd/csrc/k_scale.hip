// k_scale.hip -- the resampler of resolution ladders (include/dsv1_api.h dsv1_scale_*; stated in numpy in tests/_scale.py).
//
// Per plane and axis a weight table from the host (dsv1_scale_weights, csrc/host/dsv1_scale.c): output sample i reads the T source
// samples start[i] .. start[i] + T - 1, clamped to [0, S - 1], with int16 weights that sum to 16384.  Horizontal pass first:
//     H  = sum_t qh[t] P[y][clamp(sx + t)]          |H| <= 255 * sum |qh| < 255 * 2 * 16384 < 2^23: int32
//     Hs = (H + 128) >> 8                          |Hs| < 2^15 (a row's weights sum to 16384, its negative ones to less than 16384 / 2)
//     V  = sum_t qv[t] Hs[clamp(sy + t)][x]        |V| <= 2^15 * sum |qv| < 2^15 * 2^15 = 2^30: int32
//     out = clamp((V + 2^19) >> 20, 0, 255)
// (tests/test_scale_host.py checks the tighter bound of the worst cubic row: sum |q| of every table generated is far below 2 * 16384;
// scaler_geo asserts sum |q| < 2 * 16384 for every row it builds.)  The same kernel upscales (dsv1_resample_clip: tables of
// dsv1_resample_weights, S < D on an axis): a tile then needs at most TH + T rows and 64 + T columns, the bounds hold unchanged
// (tests/test_resample_host.py), and scaler_geo's exact LDS bound and tile-height choice read the tables whichever way they go.
//
// One launch scales every frame and all three planes of a call: blockIdx.y = frame, blockIdx.x = an output tile of 64 x TH samples
// of one plane (the planes' tiles one after the other).  TH is 64, 32 or 16: the tallest whose LDS fits 64 KB, chosen per geometry
// on the host (the source rows a tile needs grow with TH x S / D).  A workgroup of 256 threads:
//   0. copies its columns' horizontal and its rows' vertical weights into LDS;
//   1. walks the source rows its tile needs (start[y0] .. start[y1] + Tv - 1, clamped) in groups of SC_RG: stages each row's
//      columns start[x0] .. start[x1] + Th - 1 (clamped) into LDS with aligned 16-byte loads, then runs the horizontal pass of the
//      group into an int32 LDS array of rows x 64 (a thread keeps one column);
//   2. runs the vertical pass from LDS: a thread takes 4 adjacent outputs of one row at a time and writes them as one packed 32-bit
//      word where the row's alignment allows it, as bytes at the edges.
// LDS = rows x 256 + 2 (64 Th + TH Tv) + 32 x span bytes, bounded exactly on the host from the tables (scaler_geo): 31 KB for
// 1080p -> 720p (TH 64, 102 rows), 42 KB for 1080p -> 540p, 62 KB at the worst ratio (8, cubic; TH 16): 2 to 5 workgroups per CU
// of gfx950's 160 KB.  74 VGPRs, no scratch.
// The tile body (scale_tile) has two entries.  k_scale reads tightly packed planar frames: rows of a plane are the plane's width apart,
// frame blockIdx.y at src + y * sfb, written to dst + y * dfb.  k_scale_slots reads bordered reconstruction slots for the decoders'
// output pass (output_pass, dsvg_pipe.hip): a plane's pixel (0, 0) at soff and its rows spitch apart (FrameLayout::off / stride), and
// entry i of a (slot, output frame) table names the slot at slab + slot * sfb and the output frame at dst + frame * dfb.  It clamps
// source indices exactly as the packed entry does and never reads a border sample for its value: a border is written only as far as
// its readers reach.  gfx950, both entries: 74 VGPRs, 62 SGPRs, no scratch, no static LDS (the dynamic LDS above), 6 waves per SIMD by
// registers.
// A 16-byte load is issued only for an aligned chunk that holds at least one byte of the row's needed columns: it never leaves the
// 16-byte block of a sample that exists.
#include <algorithm>
#include <cstdlib>
#include "dsvg_host.hpp"

#define SC_TW 64
#define SC_RG 32
#define SC_THREADS 256
#define SC_LDS_MAX (64 * 1024)   // a tile height is chosen per geometry so that a workgroup needs at most this much LDS

struct ScalePlane {              // one plane's geometry and tables (device memory; read with uniform loads)
    int sw, sh, dw, dh;
    int th, tv, tx, tile0;       // taps per axis, tiles across, first tile of the plane in blockIdx.x
    long long soff, doff;        // plane offsets inside a packed frame
    const int *hs;
    const short *hq;
    const int *vs;
    const short *vq;
    long long spitch;            // k_scale_slots: distance of the source plane's rows (k_scale: the plane's width)
};

// LDS of a workgroup (sizes from the host): Hs int[rows_cap][SC_TW] | qh short[SC_TW * th_cap] | qv short[TH * tv_cap] | stage
// byte[SC_RG][span_cap]
// sframe / dframe: the source and the destination frame of this workgroup; SLOTS: source rows are P.spitch apart, not P.sw
template <bool SLOTS>
__device__ __forceinline__ void scale_tile(const ScalePlane *__restrict__ planes, const uint8_t *__restrict__ sframe, uint8_t *__restrict__ dframe,
                                           int TH, int rows_cap, int th_cap, int tv_cap, int span_cap)
{
    extern __shared__ int4 sc_lds[];
    int *Hs = (int *)sc_lds;
    short *qh = (short *)(Hs + (size_t)rows_cap * SC_TW);
    short *qv = qh + SC_TW * th_cap;
    uint8_t *stage = (uint8_t *)(qv + ((TH * tv_cap + 7) & ~7));
    const int tile = blockIdx.x;
    const int p = tile < planes[1].tile0 ? 0 : (tile < planes[2].tile0 ? 1 : 2);
    const ScalePlane &P = planes[p];
    const int sw = P.sw, sh = P.sh, dw = P.dw, dh = P.dh, th = P.th, tv = P.tv;
    const int t = tile - P.tile0;
    const int x0 = (t % P.tx) * SC_TW, y0 = (t / P.tx) * TH;
    const int nx = min(SC_TW, dw - x0), ny = min(TH, dh - y0);
    const int r0 = P.vs[y0], nrows = P.vs[y0 + ny - 1] + tv - r0;
    const int c0 = P.hs[x0], c1 = P.hs[x0 + nx - 1] + th - 1;
    const int lo = max(c0, 0), hi = min(c1, sw - 1);
    const int span = hi - lo + 1;
    const uint8_t *plane = sframe + P.soff;
    const long long spitch = SLOTS ? P.spitch : (long long)sw;
    const int nch = (span + 15) / 16 + 1;                          // 16-byte chunks a row segment can touch
    const int tid = threadIdx.x;
    // the tile's weights, once: its columns' horizontal and its rows' vertical taps
    for (int i = tid; i < nx * th; i += SC_THREADS) qh[i] = P.hq[(size_t)x0 * th + i];
    for (int i = tid; i < ny * tv; i += SC_THREADS) qv[i] = P.vq[(size_t)y0 * tv + i];
    // a thread's column in the horizontal pass is fixed (SC_THREADS is a multiple of SC_TW)
    const int hx = tid % SC_TW, hrow = tid / SC_TW;
    const int hsx = hx < nx ? P.hs[x0 + hx] : 0;
    for (int g = 0; g < nrows; g += SC_RG) {
        const int ng = min(SC_RG, nrows - g);
        for (int it = tid; it < ng * nch; it += SC_THREADS) {
            const int i = it / nch, k = it - i * nch;
            const int sr = min(max(r0 + g + i, 0), sh - 1);
            const uint8_t *row = plane + (long long)sr * spitch;
            const uintptr_t a0 = ((uintptr_t)(row + lo)) & ~(uintptr_t)15, a = a0 + 16u * (uintptr_t)k;
            if (a <= (uintptr_t)(row + hi)) {
                const int4 v = *(const int4 *)a;
                const uint32_t wd[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
                const long long pos0 = (long long)(a - (uintptr_t)(row + lo));
#pragma unroll
                for (int b = 0; b < 16; b++) {
                    const long long pos = pos0 + b;
                    if (pos >= 0 && pos < span) stage[i * span_cap + (int)pos] = (uint8_t)(wd[b >> 2] >> (8 * (b & 3)));
                }
            }
        }
        __syncthreads();
        if (hx < nx) {
            const short *w = qh + hx * th;
            for (int i = hrow; i < ng; i += SC_THREADS / SC_TW) {
                const uint8_t *srow = stage + i * span_cap - lo;
                int H = 0;
                for (int k = 0; k < th; k++) H += (int)w[k] * (int)srow[min(max(hsx + k, 0), sw - 1)];
                Hs[(g + i) * SC_TW + hx] = (H + 128) >> 8;
            }
        }
        __syncthreads();
    }
    for (int o = tid; o < TH * (SC_TW / 4); o += SC_THREADS) {
        const int yy = o / (SC_TW / 4), xq = (o % (SC_TW / 4)) * 4;
        if (yy >= ny || xq >= nx) continue;
        const int base = P.vs[y0 + yy] - r0;
        const short *w = qv + yy * tv;
        int V[4] = {0, 0, 0, 0};
        for (int k = 0; k < tv; k++) {
            const int *hr = Hs + (base + k) * SC_TW + xq;
            const int q = w[k];
#pragma unroll
            for (int j = 0; j < 4; j++) V[j] += q * hr[j];
        }
        uint32_t o4[4];
#pragma unroll
        for (int j = 0; j < 4; j++) o4[j] = (uint32_t)min(max((V[j] + (1 << 19)) >> 20, 0), 255);
        uint8_t *d = dframe + P.doff + (long long)(y0 + yy) * dw + x0 + xq;
        if (xq + 4 <= nx && ((uintptr_t)d & 3) == 0) *(uint32_t *)d = o4[0] | (o4[1] << 8) | (o4[2] << 16) | (o4[3] << 24);
        else
            for (int j = 0; j < 4 && xq + j < nx; j++) d[j] = (uint8_t)o4[j];
    }
}

__global__ __launch_bounds__(SC_THREADS) void k_scale(const ScalePlane *__restrict__ planes, const uint8_t *__restrict__ src,
                                                      uint8_t *__restrict__ dst, long long sfb, long long dfb, int TH, int rows_cap,
                                                      int th_cap, int tv_cap, int span_cap)
{
    scale_tile<false>(planes, src + (long long)blockIdx.y * sfb, dst + (long long)blockIdx.y * dfb, TH, rows_cap, th_cap, tv_cap, span_cap);
}

// tab: (slot, output frame) pairs, entry blockIdx.y
__global__ __launch_bounds__(SC_THREADS) void k_scale_slots(const ScalePlane *__restrict__ planes, const uint8_t *__restrict__ slab,
                                                            const int *__restrict__ tab, uint8_t *__restrict__ dst, long long sfb,
                                                            long long dfb, int TH, int rows_cap, int th_cap, int tv_cap, int span_cap)
{
    const int slot = tab[2 * blockIdx.y], frame = tab[2 * blockIdx.y + 1];
    scale_tile<true>(planes, slab + (long long)slot * sfb, dst + (long long)frame * dfb, TH, rows_cap, th_cap, tv_cap, span_cap);
}

// ------------------------------------------------------------------------------------------------ host side
extern "C" int dsv1_resample_taps(int S, int D, int filter);
extern "C" int dsv1_resample_weights(int S, int D, int filter, int32_t *start, int16_t *q, int T);

struct dsvg_scaler {
    int device = 0, sw = 0, sh = 0, fmt = 0, filter = 0;
    size_t sfb = 0;
    std::vector<ScaleGeo> geo;
};

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// tables of one geometry: [3] ScalePlane, then per plane hs int[dw], hq short[dw th], vs int[dh], vq short[dh tv].  The source is
// packed planar frames of sw x sh at subsampling fmt, or (L != nullptr) the bordered frames of that layout: its planes' dims, offsets
// and strides (k_scale_slots)
static int scaler_geo(int sw, int sh, int fmt, int filter, const FrameLayout *L, int dw, int dh, ScaleGeo &G)
{
    const int hsh = fmt_hs(fmt), vsh = fmt_vs(fmt);
    const int SW[3] = {L ? L->w[0] : sw, L ? L->w[1] : rsu(sw, hsh), L ? L->w[2] : rsu(sw, hsh)};
    const int SH[3] = {L ? L->h[0] : sh, L ? L->h[1] : rsu(sh, vsh), L ? L->h[2] : rsu(sh, vsh)};
    const int DW[3] = {dw, rsu(dw, hsh), rsu(dw, hsh)}, DH[3] = {dh, rsu(dh, vsh), rsu(dh, vsh)};
    ScalePlane pl[3];
    std::vector<std::vector<int32_t>> hs(3), vs(3);
    std::vector<std::vector<int16_t>> hq(3), vq(3);
    size_t off = align16(3 * sizeof(ScalePlane)), offs[3][4];
    int tile0 = 0, th_cap = 1, tv_cap = 1;
    long long so = 0, dof = 0;
    for (int p = 0; p < 3; p++) {
        // (dsv1_resample_*: for a downscale the tables are dsv1_scale_weights'; the callers have checked the direction they allow)
        const int th = dsv1_resample_taps(SW[p], DW[p], filter), tv = dsv1_resample_taps(SH[p], DH[p], filter);
        if (th < 0 || tv < 0) { dsvg_set_error("scale %dx%d -> %dx%d: ratio outside 1/8..8", SW[p], SH[p], DW[p], DH[p]); return DSVG_ERR_ARG; }
        hs[p].resize(DW[p]); hq[p].resize((size_t)DW[p] * th); vs[p].resize(DH[p]); vq[p].resize((size_t)DH[p] * tv);
        if (dsv1_resample_weights(SW[p], DW[p], filter, hs[p].data(), hq[p].data(), th) ||
            dsv1_resample_weights(SH[p], DH[p], filter, vs[p].data(), vq[p].data(), tv)) { dsvg_set_error("weight tables"); return DSVG_ERR_ARG; }
        // (the kernel's row and column ranges need starts that never decrease; its int32 bounds need sum |q| < 2 * 16384 in every row,
        // which Catmull-Rom's negative lobes keep in both directions -- asserted for every table built)
        for (int i = 1; i < DW[p]; i++) if (hs[p][i] < hs[p][i - 1]) { dsvg_set_error("weight table starts decrease"); return DSVG_ERR_ARG; }
        for (int i = 1; i < DH[p]; i++) if (vs[p][i] < vs[p][i - 1]) { dsvg_set_error("weight table starts decrease"); return DSVG_ERR_ARG; }
        for (int tb = 0; tb < 2; tb++) {
            const std::vector<int16_t> &q = tb ? vq[p] : hq[p];
            const int T = tb ? tv : th;
            for (size_t i = 0; i < q.size(); i += (size_t)T) {
                int a = 0;
                for (int k = 0; k < T; k++) a += std::abs((int)q[i + k]);
                if (a >= 2 * 16384) { dsvg_set_error("weight table row outside the kernel's int32 bounds"); return DSVG_ERR_ARG; }
            }
        }
        pl[p].sw = SW[p]; pl[p].sh = SH[p]; pl[p].dw = DW[p]; pl[p].dh = DH[p]; pl[p].th = th; pl[p].tv = tv;
        pl[p].soff = L ? (long long)L->off[p] : so; pl[p].doff = dof;
        pl[p].spitch = L ? (long long)L->stride[p] : (long long)SW[p];
        so += (long long)SW[p] * SH[p]; dof += (long long)DW[p] * DH[p];
        th_cap = std::max(th_cap, th); tv_cap = std::max(tv_cap, tv);
        offs[p][0] = off; off = align16(off + sizeof(int32_t) * DW[p]);
        offs[p][1] = off; off = align16(off + sizeof(int16_t) * DW[p] * th);
        offs[p][2] = off; off = align16(off + sizeof(int32_t) * DH[p]);
        offs[p][3] = off; off = align16(off + sizeof(int16_t) * DH[p] * tv);
    }
    // the tallest tile (64, 32 or 16 output rows) whose LDS fits SC_LDS_MAX, sized exactly from the tables: the source rows and
    // columns any tile of any plane needs
    int span_cap = 16;
    for (int p = 0; p < 3; p++)
        for (int x0 = 0; x0 < DW[p]; x0 += SC_TW) {
            const int c0 = hs[p][x0], c1 = hs[p][std::min(x0 + SC_TW, DW[p]) - 1] + pl[p].th - 1;
            span_cap = std::max(span_cap, std::min(c1, SW[p] - 1) - std::max(c0, 0) + 1);
        }
    span_cap = (int)align16((size_t)span_cap);
    for (int TH = 64; TH >= 16; TH /= 2) {
        int rows_cap = 1;
        for (int p = 0; p < 3; p++)
            for (int y0 = 0; y0 < DH[p]; y0 += TH)
                rows_cap = std::max(rows_cap, vs[p][std::min(y0 + TH, DH[p]) - 1] + pl[p].tv - vs[p][y0]);
        G.lds = sizeof(int) * (size_t)rows_cap * SC_TW + sizeof(short) * ((size_t)SC_TW * th_cap + (((size_t)TH * tv_cap + 7) & ~(size_t)7)) +
                (size_t)SC_RG * span_cap;
        G.th_tile = TH; G.rows_cap = rows_cap;
        if (G.lds <= SC_LDS_MAX) break;
    }
    if (G.lds > 160 * 1024 - 1024) { dsvg_set_error("scale tile needs %zu bytes of LDS", G.lds); return DSVG_ERR_UNSUPPORTED; }
    for (int p = 0; p < 3; p++) {
        pl[p].tx = (DW[p] + SC_TW - 1) / SC_TW;
        pl[p].tile0 = tile0;
        tile0 += pl[p].tx * ((DH[p] + G.th_tile - 1) / G.th_tile);
    }
    G.th_cap = th_cap; G.tv_cap = tv_cap; G.span_cap = span_cap;
    G.ntiles = tile0;
    G.dfb = (size_t)dof;
    G.sbytes = (size_t)so;
    HIPCHK(hipMalloc((void **)&G.planes_d, off));
    uint8_t *base = (uint8_t *)G.planes_d;
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
    HIPCHK(hipMemcpy(G.planes_d, h.data(), off, hipMemcpyHostToDevice));
    return DSVG_OK;
}

extern "C" void dsvg_scaler_destroy(dsvg_scaler *s)
{
    if (!s) return;
    if (hipSetDevice(s->device) == hipSuccess)
        for (auto &G : s->geo) if (G.planes_d) (void)hipFree(G.planes_d);
    (void)hipGetLastError();
    delete s;
}

static int scaler_create_impl(dsvg_scaler *s, int ngeom, const int *dw, const int *dh)
{
    HIPCHK(hipSetDevice(s->device));
    s->geo.resize((size_t)ngeom);
    for (int g = 0; g < ngeom; g++) {
        const int rc = scaler_geo(s->sw, s->sh, s->fmt, s->filter, nullptr, dw[g], dh[g], s->geo[(size_t)g]);
        if (rc) return rc;
    }
    return DSVG_OK;
}

extern "C" int dsvg_scaler_create(dsvg_scaler **out, int device, int sw, int sh, int subsamp, int ngeom, const int *dw, const int *dh, int filter)
{
    if (!out || sw < 1 || sh < 1 || ngeom < 0 || (ngeom && (!dw || !dh))) { dsvg_set_error("bad scaler arguments"); return DSVG_ERR_ARG; }
    *out = nullptr;
    if (dsvg_device_count() <= device || device < 0) { dsvg_set_error("HIP device %d not present", device); (void)hipGetLastError(); return DSVG_ERR_NODEVICE; }
    dsvg_scaler *s = new dsvg_scaler();
    s->device = device; s->sw = sw; s->sh = sh; s->fmt = subsamp; s->filter = filter;
    s->sfb = (size_t)sw * sh + 2 * (size_t)rsu(sw, fmt_hs(subsamp)) * rsu(sh, fmt_vs(subsamp));
    const int rc = scaler_create_impl(s, ngeom, dw, dh);
    if (rc) { dsvg_scaler_destroy(s); return rc; }      // (no pending HIP error left behind)
    *out = s;
    return DSVG_OK;
}

extern "C" int dsvg_scaler_run(dsvg_scaler *s, void *stream, int g, const void *src_dev, int nframes, void *dst_dev)
{
    if (!s || g < 0 || g >= (int)s->geo.size() || !src_dev || !dst_dev || nframes < 1) { dsvg_set_error("bad scale arguments"); return DSVG_ERR_ARG; }
    const ScaleGeo &G = s->geo[(size_t)g];
    HIPCHK(hipSetDevice(s->device));
    for (int f0 = 0; f0 < nframes; f0 += 65535) {        // (gridDim.y; one launch for any call the ladders make)
        const int n = std::min(65535, nframes - f0);
        hipLaunchKernelGGL(k_scale, dim3(G.ntiles, n), dim3(SC_THREADS), G.lds, (hipStream_t)stream, G.planes_d,
                           (const uint8_t *)src_dev + (size_t)f0 * s->sfb, (uint8_t *)dst_dev + (size_t)f0 * G.dfb,
                           (long long)s->sfb, (long long)G.dfb, G.th_tile, G.rows_cap, G.th_cap, G.tv_cap, G.span_cap);
    }
    HIPCHK(hipGetLastError());
    return DSVG_OK;
}

// ------------------------------------------------------------------------------------------------ the decoders' output pass
void scale_geo_free(ScaleGeo &G)
{
    if (G.planes_d) (void)hipFree(G.planes_d);
    G = ScaleGeo();
}

int scale_geo_build(ScaleGeo &G, const FrameLayout &L, int fmt, int dw, int dh, int filter)
{
    ScaleGeo N;
    const int rc = scaler_geo(L.w[0], L.h[0], fmt, filter, &L, dw, dh, N);
    if (rc) { scale_geo_free(N); return rc; }
    scale_geo_free(G);
    G = N;
    return DSVG_OK;
}

void launch_scale_slots(hipStream_t st, const ScaleGeo &G, const uint8_t *slab, size_t sfb, const int *tab_d, int n, uint8_t *dst, size_t dfb, Prof *pf)
{
    if (pf) pf->begin(st, KID_SCALE_SLOTS, (double)n * ((double)G.sbytes + (double)G.dfb));
    for (int f0 = 0; f0 < n; f0 += 65535)                 // (gridDim.y; one launch for any call the decoders make)
        hipLaunchKernelGGL(k_scale_slots, dim3(G.ntiles, std::min(65535, n - f0)), dim3(SC_THREADS), G.lds, st, G.planes_d, slab, tab_d + 2 * (size_t)f0,
                           dst, (long long)sfb, (long long)dfb, G.th_tile, G.rows_cap, G.th_cap, G.tv_cap, G.span_cap);
    if (pf) pf->end(st);
}
